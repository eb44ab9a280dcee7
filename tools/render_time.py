#!/usr/bin/env python3
"""Time the model renderer (hep_render_models_device, hmd_ego_pose_amd/render.py) on the MI355X.

  one       16 frames of 256 x 256, ONE pose each of an icosphere with 20480 faces (10242 vertices, built here), mask + depth + blend;
            device events around ``render_models``, 5 warm-up calls, 50 timed ones
  sixteen   the same with 16 poses per frame
  pass      a 256-frame validation pass of ``DeviceEvaluator`` (phi 0, size 256, batch 16, fp32, seeded weights, everything preloaded: the
            set-up of tools/draw_time.py) with ``draw_into`` and without / with ``meshes`` (the icosphere), host clock around
            ``add`` x 16 + ``result``, the two alternating

Every workload runs in a child process of its own under its own time limit; the parent prints one JSON line with min / median / max.

    python tools/render_time.py [--repeats 5] [--json FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMITS = {"one": 120, "sixteen": 180, "pass": 300}       # seconds per child


def stats(v):
    return dict(min=float(min(v)), median=float(np.median(v)), max=float(max(v)))


def icosphere(level=5, radius=1.0):
    """(vertices float32 [10 * 4^level + 2, 3], faces int32 [20 * 4^level, 3]) of a subdivided icosahedron."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def child_call(pmax):
    import torch
    from hmd_ego_pose_amd import render as RN
    from scipy.spatial.transform import Rotation
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    dev, B, size = torch.device("cuda", 0), 16, 256
    rng = np.random.Generator(np.random.PCG64(9))
    mesh = RN.MeshSet([icosphere(5, 0.05)], device=dev)
    poses = np.zeros((B, pmax, 16))
    poses[..., 0], poses[..., 2] = 1.0, 1.0 + np.arange(pmax)
    poses[..., 4:13] = Rotation.from_rotvec(rng.standard_normal((B * pmax, 3))).as_matrix().reshape(B, pmax, 9)
    poses[..., 13:16] = np.stack([rng.normal(0, 0.06, (B, pmax)), rng.normal(0, 0.06, (B, pmax)), 0.45 + rng.normal(0, 0.05, (B, pmax))], axis=-1)
    d_poses = torch.from_numpy(poses).to(dev)
    cam = torch.from_numpy(np.tile(np.array([480.0, 480.0, size / 2, size / 2, 1.0]), (B, 1))).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (B, size, size, 3), dtype=np.uint8)).to(dev)
    run = lambda: RN.render_models(d_poses, cam, mesh, size, size, mask=True, depth=True, blend_into=frames)
    for _ in range(5):
        out = run()
    us = []
    for _ in range(50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return dict(stats(us), poses_per_frame=pmax, faces=mesh.num_faces, vertices=mesh.num_vertices, covered_pixels_per_image=int((out["mask"] > 0).sum()) // B)


def child_pass(repeats, n_frames=256, batch=16):
    import torch
    from eval_time import MemoryFolder
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import draw as DR
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd import render as RN
    from hmd_ego_pose_amd.weights import seeded_state_dict
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    size, dev = 256, torch.device("cuda", 0)
    ds = MemoryFolder(n_frames, size)
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(0, 0), strict=True)
    model = TrainModelWithLoss(m.to(dev).eval()).eval()
    u8 = torch.from_numpy(ds.frames).to(dev)
    cam = torch.from_numpy(np.stack([ds.camera_input(i, 1.0) for i in range(len(ds))])).to(dev)
    gt = torch.from_numpy(E.gt_table(ds.annotations, ds.camera, 1.0)).to(dev)
    cuboid = DR.cuboid_corners([-100.0, -80.0, -150.0], [200.0, 160.0, 300.0])
    ev = E.DeviceEvaluator(model, ds.points, ds.diameter, size, len(ds), 0.5, 10, 0.0, device=dev, cuboid=cuboid)
    mesh = RN.MeshSet([icosphere(5, 80.0)], device=dev)
    canvas = u8.clone()

    def one_pass(with_model):
        ev.reset()
        for o in range(0, len(ds), batch):
            ev.add(u8[o:o + batch], cam[o:o + batch], gt[o:o + batch], draw_into=canvas[o:o + batch], meshes=mesh if with_model else None)
        return ev.result()

    res = {k: one_pass(k) for k in (False, True)}
    assert all(np.array([res[False][k]]).tobytes() == np.array([res[True][k]]).tobytes() for k in res[False])
    times = {False: [], True: []}
    for _ in range(repeats):
        for k in (False, True):
            canvas.copy_(u8)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one_pass(k)
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {"frames": n_frames, "batch": batch, "draw_ms": stats(times[False]), "draw_model_ms": stats(times[True])}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None, choices=list(LIMITS))
    a = ap.parse_args(argv)
    if a.child:
        res = child_pass(a.repeats) if a.child == "pass" else child_call(1 if a.child == "one" else 16)
        print("RESULT " + json.dumps(res))
        return res
    out = {}
    for name, limit in LIMITS.items():
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out[name] = {"error": f"no result within {limit} s"}
            break                                  # nothing more is started on the device after a child that did not end
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            out[name] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-400:]}
            break
        out[name] = json.loads(lines[-1][7:])
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
