#!/usr/bin/env python3
"""Time a validation pass: ``evaluate`` (detections to the host batch by batch, matching and metrics in numpy, ADD / ADD-S through a
second upload) against ``DeviceEvaluator`` (one hep_score_detections_device launch per batch, one copy per evaluation).

Set-up: 256 uint8 frames of 256 x 256, phi 0, size 256, batch 16, fp32, seeded weights, a 1500-point model, one annotation per
frame; IoU threshold 0 so that every frame with a candidate of the label is matched and every metric is computed (a trained model
matches most frames; the seeded one would match almost none at 0.5).

  evaluate          the frames in host memory behind the ``LinemodFolder`` interface (``evaluate`` uploads them itself)
  evaluate_device   the same in-memory folder through ``evaluate_device`` (the upload is in the window as well)
  DeviceEvaluator   frames, camera rows and the ground-truth table preloaded on the device: ``add`` x 16, then ``result``

Host clock around calls that end in a synchronise (``result`` and ``evaluate`` both end in a device-to-host copy).  One warm-up pass
of every path, then the paths alternate, ``--repeats`` times each; the spread of a path is max - min over its repeats.
Device-to-host copies (each one waits for the device) by construction: ``evaluate`` copies 6 tensors per IMAGE (post_filter) and
ends with the 5 uploads, 2 downloads, allocation and release of hep_pose_errors - 6 n + 2; ``DeviceEvaluator`` makes one, in ``result``.

    python tools/eval_time.py [--frames 256] [--batch 16] [--repeats 3] [--json FILE]

``--scene`` times the multi-object pass instead (hep_score_scene_device): the same frames with THREE annotations per frame, one per
label, a seeded 3-class model, inputs preloaded on the device, IoU threshold 0:

  scene3      ``SceneEvaluator`` over three labels: one forward and one scoring launch per batch
  device3x    three ``DeviceEvaluator`` passes, one per label, each with its own forward of every batch (what there was before)
  scene1      ``SceneEvaluator`` with one label and one annotation per frame, 1-class model
  device1     ``DeviceEvaluator`` on the same frames and model

Every measurement runs in a child process of its own (``--scene-child NAME``: one warm-up pass, then ``--passes`` timed passes), the
four alternating, ``--repeats`` rounds; this process never opens the GPU.

    python tools/eval_time.py --scene [--frames 256] [--batch 16] [--repeats 3] [--passes 3] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class MemoryFolder:
    """What ``evaluate`` reads of a ``LinemodFolder``, held in memory."""

    def __init__(self, n, size, seed=0):
        from hmd_ego_pose_amd.evaluate import LinemodFolder
        rng = np.random.Generator(np.random.PCG64(seed))
        self.points = (rng.standard_normal((1500, 3)) * np.array([40.0, 25.0, 60.0])).astype(np.float32)
        self.diameter = 180.0
        self.frames = rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)
        self.annotations, self.camera = [], []
        for _ in range(n):
            x0, y0 = rng.integers(5, 100, 2)
            w, h = rng.integers(30, 120, 2)
            rot = rng.standard_normal(3)
            self.annotations.append(dict(bbox=np.array([x0, y0, x0 + w, y0 + h], np.float32), rotation=rot,
                                         translation=np.array([rng.normal(0, 40), rng.normal(0, 40), 500 + rng.normal(0, 50)]),
                                         drill_tip=np.array([10.0, -20.0, 30.0, 1.0]), coords_3d=rng.standard_normal((21, 3)) * 0.05))
            self.camera.append(np.array([[480.0, 0, 128.0], [0, 480.0, 128.0], [0, 0, 1.0]]))
        self.camera_input = lambda i, scale, norm=1000.0: LinemodFolder.camera_input(self, i, scale, norm)

    def __len__(self):
        return len(self.frames)

    def load_image(self, i):
        return self.frames[i]


SCENE_PATHS = ("scene3", "device3x", "scene1", "device1")


def scene_child(name, frames, batch, passes):
    """One measurement of ``--scene`` in this process: build, preload, one warm-up pass, ``passes`` timed passes.  Prints one JSON line."""
    import torch
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    size, dev = 256, torch.device("cuda", 0)
    labels = 3 if name.endswith(("3", "3x")) else 1
    sets = [MemoryFolder(frames, size, seed=l) for l in range(labels)]          # set l: the annotations and the cloud of label l; the frames are set 0's
    ds = sets[0]
    m = HMDEgoPose({"iter": 0}, num_classes=labels, compound_coef=0, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(0, 0, num_classes=labels), strict=True)
    model = TrainModelWithLoss(m.to(dev).eval()).eval()
    u8 = torch.from_numpy(ds.frames).to(dev)
    cam = torch.from_numpy(np.stack([ds.camera_input(i, 1.0) for i in range(frames)])).to(dev)
    kw = dict(score_threshold=0.5, max_detections=10, iou_threshold=0.0)
    if name.startswith("scene"):
        anns = [[dict(sets[l].annotations[i], label=l) for l in range(labels)] for i in range(frames)]
        gt = torch.from_numpy(E.gt_scene_table(anns, ds.camera, 1.0, labels)).to(dev)
        ev = E.SceneEvaluator(model, [(s_.points, s_.diameter, False) for s_ in sets], size, frames, labels, device=dev, **kw)

        def one_pass():
            ev.reset()
            for o in range(0, frames, batch):
                ev.add(u8[o:o + batch], cam[o:o + batch], gt[o:o + batch])
            r = ev.result()
            return [r["labels"][l]["num_matched"] for l in range(labels)]
    else:
        gts = [torch.from_numpy(E.gt_table(s_.annotations, ds.camera, 1.0)).to(dev) for s_ in sets]
        evs = [E.DeviceEvaluator(model, s_.points, s_.diameter, size, frames, label=l, device=dev, **kw) for l, s_ in enumerate(sets)]

        def one_pass():
            matched = []
            for ev, gt in zip(evs, gts):                                        # one whole pass, forwards included, per label
                ev.reset()
                for o in range(0, frames, batch):
                    ev.add(u8[o:o + batch], cam[o:o + batch], gt[o:o + batch])
                matched.append(ev.result()["num_matched"])
            return matched
    matched = one_pass()
    ms = []
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_pass()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"path": name, "ms": ms, "num_matched": matched}))


def scene_main(a):
    """The parent of ``--scene``: children in turn, alternating over the four paths; never touches the GPU itself."""
    import subprocess
    runs = {k: [] for k in SCENE_PATHS}
    matched = {}
    for _ in range(a.repeats):
        for k in SCENE_PATHS:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--scene-child", k, "--frames", str(a.frames), "--batch", str(a.batch),
                                  "--passes", str(a.passes)], check=True, capture_output=True, text=True, timeout=600).stdout
            rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            runs[k] += rec["ms"]
            matched[k] = rec["num_matched"]
            print(f"{k:>9s}: {['%.1f' % v for v in rec['ms']]} ms, matched {rec['num_matched']}", flush=True)
    n_batches = (a.frames + a.batch - 1) // a.batch
    out = {"frames": a.frames, "batch": a.batch, "children_per_path": a.repeats, "passes_per_child": a.passes, "num_matched": matched,
           "ms": {k: dict(min=min(v), median=float(np.median(v)), max=max(v)) for k, v in runs.items()},
           "forwards": {"scene3": n_batches, "device3x": 3 * n_batches, "scene1": n_batches, "device1": n_batches},
           "scoring_launches": {"scene3": n_batches, "device3x": 3 * n_batches, "scene1": n_batches, "device1": n_batches},
           "device_to_host_copies": {"scene3": 1, "device3x": 3, "scene1": 1, "device1": 1}}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--scene", action="store_true", help="time the multi-object pass (SceneEvaluator) against one DeviceEvaluator pass per label")
    ap.add_argument("--scene-child", default=None, choices=SCENE_PATHS, help="one measurement of --scene, in this process")
    ap.add_argument("--passes", type=int, default=3, help="timed passes per child process of --scene")
    a = ap.parse_args(argv)
    if a.scene_child:
        return scene_child(a.scene_child, a.frames, a.batch, a.passes)
    if a.scene:
        return scene_main(a)
    import torch
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    size, dev = 256, torch.device("cuda", 0)
    ds = MemoryFolder(a.frames, size)
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(0, 0), strict=True)
    model = TrainModelWithLoss(m.to(dev).eval()).eval()
    kw = dict(score_threshold=0.5, max_detections=10, iou_threshold=0.0, batch_size=a.batch)
    # the preloaded inputs of the DeviceEvaluator path
    u8 = torch.from_numpy(ds.frames).to(dev)
    cam = torch.from_numpy(np.stack([ds.camera_input(i, 1.0) for i in range(len(ds))])).to(dev)
    gt = torch.from_numpy(E.gt_table(ds.annotations, ds.camera, 1.0)).to(dev)
    ev = E.DeviceEvaluator(model, ds.points, ds.diameter, size, len(ds), kw["score_threshold"], kw["max_detections"], kw["iou_threshold"], device=dev)

    def device_pass():
        ev.reset()
        for o in range(0, len(ds), a.batch):
            ev.add(u8[o:o + a.batch], cam[o:o + a.batch], gt[o:o + a.batch])
        return ev.result()

    paths = {"evaluate": lambda: E.evaluate(ds, model, size, device=dev, **kw),
             "evaluate_device": lambda: E.evaluate_device(ds, model, size, device=dev, **kw),
             "DeviceEvaluator": device_pass}
    res = {k: f() for k, f in paths.items()}                            # warm-up: every shape, every code object
    times = {k: [] for k in paths}
    for _ in range(a.repeats):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    n_batches = (len(ds) + a.batch - 1) // a.batch
    out = {"frames": len(ds), "batch": a.batch, "num_matched": res["evaluate"]["num_matched"],
           "same_counts": all(res[k][q] == res["evaluate"][q] for k in paths for q in ("num_matched", "AP", "ADD", "ADD-S", "5cm_5deg", "2D_projection")),
           "ms": {k: dict(min=min(v), median=float(np.median(v)), max=max(v)) for k, v in times.items()},
           "device_to_host_copies": {"evaluate": 6 * len(ds) + 2, "evaluate_device": 1, "DeviceEvaluator": 1},
           "launches_of_the_score_kernel": n_batches}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
