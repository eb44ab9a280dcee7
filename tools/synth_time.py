#!/usr/bin/env python3
"""Time the synthetic-frame generator (hep_synth_frames_device, hmd_ego_pose_amd/synth.py) next to the model renderer on the MI355X.

  one       16 frames of 256 x 256, ONE pose each of an icosphere with 20480 faces (10242 vertices, tools/render_time.py builds it) with
            random vertex colours; device events around ``synth_frames`` (mask, depth, visible, annotations) and around ``render_models``
            (mask + depth + blend) on the SAME pose table, 5 warm-up calls and 50 timed ones each
  sixteen   the same with 16 poses per frame

Every workload runs in a child process of its own under its own time limit; the parent prints one JSON line with min / median / max in
microseconds.  ``--lib FILE`` times another build of the library; ``--render-only`` leaves ``synth_frames`` out, for a build without it
(the A/B of ``render_models`` across two commits: alternate the two libraries in one job).

    python tools/synth_time.py [--lib FILE] [--render-only] [--json FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMITS = {"one": 120, "sixteen": 180}       # seconds per child


def timed(run, warm=5, calls=50):
    import torch
    from render_time import stats
    for _ in range(warm):
        run()
    us = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return stats(us)


def child_call(pmax, lib, render_only):
    import torch
    from hmd_ego_pose_amd import _capi
    if lib:
        have = ctypes.CDLL(lib)
        _capi.LIB_PATH = lib
        _capi.SYMBOLS = {k: v for k, v in _capi.SYMBOLS.items() if hasattr(have, k)}      # an older build: what it lacks stays unbound
    from hmd_ego_pose_amd import render as RN
    from hmd_ego_pose_amd import synth as SY
    from render_time import icosphere
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    dev, B, size = torch.device("cuda", 0), 16, 256
    rng = np.random.Generator(np.random.PCG64(9))
    v, f = icosphere(5, 0.05)
    mesh = SY.ShadedMeshSet([(v, f, rng.integers(0, 256, (len(v), 3), dtype=np.uint8))], device=dev)
    tvec = np.stack([rng.normal(0, 0.06, (B, pmax)), rng.normal(0, 0.06, (B, pmax)), 0.45 + rng.normal(0, 0.05, (B, pmax))], axis=-1)
    ann = dict(labels=np.zeros((B, pmax), np.int32), mask_values=np.tile(1 + np.arange(pmax, dtype=np.int32), (B, 1)), rvec=rng.standard_normal((B, pmax, 3)).astype(np.float32),
               tvec=tvec.astype(np.float32), extra=np.zeros((B, pmax, 2), np.float32), num_gt=np.full(B, pmax, np.int32))
    ann = {k: torch.from_numpy(a).to(dev) for k, a in ann.items()}
    poses = RN.poses_from_annotations(ann)
    cam = torch.from_numpy(np.tile(np.array([480.0, 480.0, size / 2, size / 2, 1.0]), (B, 1))).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (B, size, size, 3), dtype=np.uint8)).to(dev)
    lights = torch.from_numpy(SY.draw_lights(rng, B)).to(dev)
    out = RN.render_models(poses, cam, mesh, size, size, mask=True, depth=True, blend_into=frames)
    res = dict(poses_per_frame=pmax, faces=mesh.num_faces, vertices=mesh.num_vertices, covered_pixels_per_image=int((out["mask"] > 0).sum()) // B,
               library=os.path.basename(_capi.LIB_PATH))
    res["render_models_us"] = timed(lambda: RN.render_models(poses, cam, mesh, size, size, mask=True, depth=True, blend_into=frames))
    if not render_only:
        res["synth_frames_us"] = timed(lambda: SY.synth_frames(frames, ann, cam, mesh, lights, alpha=256, min_pixels=16, mask=True, depth=True))
        res["kept_objects_per_image"] = float(SY.synth_frames(frames, ann, cam, mesh, lights, mask=True, depth=True)["annotations"]["num_gt"].float().mean())
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=None, help="another build of libhep.so")
    ap.add_argument("--render-only", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None, choices=list(LIMITS))
    a = ap.parse_args(argv)
    if a.child:
        res = child_call(1 if a.child == "one" else 16, a.lib, a.render_only)
        print("RESULT " + json.dumps(res))
        return res
    out = {}
    for name, limit in LIMITS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name] + (["--lib", os.path.abspath(a.lib)] if a.lib else []) + (["--render-only"] if a.render_only else [])
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
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
