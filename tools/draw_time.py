#!/usr/bin/env python3
"""Time the pose overlays (hep_draw_poses_device, hmd_ego_pose_amd/draw.py) on the MI355X.

  call      the draw call alone by device events: 256 x 256 frames, batch 16, thickness 2, every layer on; ``light`` = one annotation and one
            detection per image, ``heavy`` = 16 annotations and 10 detections per image; 5 warm-up calls, 50 timed ones
  pass      a 256-frame validation pass of ``DeviceEvaluator`` (phi 0, size 256, batch 16, fp32, seeded weights, frames, camera rows and
            table preloaded: the set-up of tools/eval_time.py) without and with ``draw_into`` (the frames themselves), nothing saved;
            host clock around ``add`` x 16 + ``result``, the two alternating
  save      the same pass with the drawn batches saved, one synchronise per batch: forward + scoring + draw, the copy of the drawn batch to
            the host and the PNG encoding with PIL (to memory), host clock, each summed over the pass; the draw's own share is the
            difference of the two ``pass`` figures

    python tools/draw_time.py [--frames 256] [--batch 16] [--repeats 5] [--json FILE]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(v):
    return dict(min=float(min(v)), median=float(np.median(v)), max=float(max(v)))


def call_inputs(rng, B, size, anns, dets, dev):
    """Ground-truth table [B,anns,88], detection rows [B,dets,...] and three cuboids: poses in front of the camera, on the frame."""
    import torch
    cam = np.array([480.0, 480.0, size / 2, size / 2, 1.0])
    gt = np.zeros((B, anns, 88))
    gt[..., 0] = 1.0
    gt[..., 1:5] = rng.uniform(5, size - 5, (B, anns, 4))
    gt[..., 5:8] = rng.standard_normal((B, anns, 3))
    gt[..., 8:11] = np.stack([rng.normal(0, 60, (B, anns)), rng.normal(0, 60, (B, anns)), 600 + rng.normal(0, 50, (B, anns))], axis=-1)
    gt[..., 14:19] = cam
    gt[..., 19] = 1.0
    gt[..., 20:83] = (np.array([0.0, 0.0, 0.5]) + rng.standard_normal((B, anns, 21, 3)) * 0.04).reshape(B, anns, 63)
    gt[..., 83] = rng.integers(0, 3, (B, anns))
    det = dict(boxes=rng.uniform(5, size - 5, (B, dets, 4)).astype(np.float32), scores=rng.uniform(0.6, 0.99, (B, dets)).astype(np.float32),
               labels=rng.integers(0, 3, (B, dets)).astype(np.int32), rotation=rng.uniform(-1, 1, (B, dets, 3)).astype(np.float32),
               translation=gt[:, np.arange(dets) % anns, 8:11].astype(np.float32),
               hand=(np.array([0.0, 0.0, 0.5]) + rng.standard_normal((B, dets, 21, 3)) * 0.04).reshape(B, dets, 63).astype(np.float32))
    cub = np.stack([np.array([[x, y, z] for z in (-50 - 5 * l, 50 + 5 * l) for x, y in ((-40, -30), (40, -30), (40, 30), (-40, 30))], np.float32) for l in range(3)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return up(gt), {k: up(v) for k, v in det.items()}, up(cub)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    import torch
    from PIL import Image
    from eval_time import MemoryFolder
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd import draw as DR
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    size, dev = 256, torch.device("cuda", 0)
    ALL = _capi.DRAW_BOX2D | _capi.DRAW_CUBOID | _capi.DRAW_HAND
    rng = np.random.Generator(np.random.PCG64(5))
    out = {"frames": a.frames, "batch": a.batch, "size": size}

    # ---- the call alone
    clean = torch.from_numpy(rng.integers(0, 256, (a.batch, size, size, 3), dtype=np.uint8)).to(dev)
    out["call_us"] = {}
    for name, anns, dets in (("light", 1, 1), ("heavy", 16, 10)):
        gt, det, cub = call_inputs(rng, a.batch, size, anns, dets, dev)
        frames = clean.clone()
        kw = dict(cuboids=cub, gt=gt, detections=det, score_threshold=0.5, max_detections=dets, ann_layers=ALL, det_layers=ALL, thickness=2)
        for _ in range(5):
            DR.draw_poses(frames, **kw)
        us = []
        for _ in range(50):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            DR.draw_poses(frames, **kw)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        out["call_us"][name] = dict(stats(us), annotations=anns, detections=dets, drawn_pixels_per_image=int((frames != clean).any(dim=3).sum()) // a.batch)

    # ---- the validation pass
    ds = MemoryFolder(a.frames, size)
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(0, 0), strict=True)
    model = TrainModelWithLoss(m.to(dev).eval()).eval()
    u8 = torch.from_numpy(ds.frames).to(dev)
    cam = torch.from_numpy(np.stack([ds.camera_input(i, 1.0) for i in range(len(ds))])).to(dev)
    gt = torch.from_numpy(E.gt_table(ds.annotations, ds.camera, 1.0)).to(dev)
    cuboid = DR.cuboid_corners([-100.0, -80.0, -150.0], [200.0, 160.0, 300.0])
    ev = E.DeviceEvaluator(model, ds.points, ds.diameter, size, len(ds), 0.5, 10, 0.0, device=dev, cuboid=cuboid, draw_layers=_capi.DRAW_CUBOID | _capi.DRAW_HAND)
    canvas = u8.clone()

    def one_pass(draw):
        ev.reset()
        for o in range(0, len(ds), a.batch):
            ev.add(u8[o:o + a.batch], cam[o:o + a.batch], gt[o:o + a.batch], draw_into=canvas[o:o + a.batch] if draw else None)
        return ev.result()

    res = {k: one_pass(k) for k in (False, True)}
    assert res[False] == res[True] or all(np.array([res[False][k]]).tobytes() == np.array([res[True][k]]).tobytes() for k in res[False])
    times = {False: [], True: []}
    for _ in range(a.repeats):
        for k in (False, True):
            canvas.copy_(u8)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one_pass(k)
            times[k].append((time.perf_counter() - t0) * 1e3)
    out["pass_ms"] = {"plain": stats(times[False]), "draw_into": stats(times[True])}
    out["num_matched"] = res[True]["num_matched"]

    # ---- the pass with the frames saved, split
    split = {"forward_score_draw_ms": [], "copy_ms": [], "png_ms": [], "total_ms": []}
    for _ in range(a.repeats):
        canvas.copy_(u8)
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        ev.reset()
        work = copy = png = 0.0
        for o in range(0, len(ds), a.batch):
            c = canvas[o:o + a.batch]
            t0 = time.perf_counter()
            ev.add(u8[o:o + a.batch], cam[o:o + a.batch], gt[o:o + a.batch], draw_into=c)
            torch.cuda.synchronize()
            work += (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            host = c.cpu().numpy()
            copy += (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            for img in host:
                Image.fromarray(img).save(io.BytesIO(), format="PNG")
            png += (time.perf_counter() - t0) * 1e3
        ev.result()
        split["total_ms"].append((time.perf_counter() - t_all) * 1e3)
        split["forward_score_draw_ms"].append(work); split["copy_ms"].append(copy); split["png_ms"].append(png)
    out["save_pass"] = {k: stats(v) for k, v in split.items()}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
