#!/usr/bin/env python3
"""Time the BOP pose errors (hmd_ego_pose_amd/bop.py: hep_bop_point_errors_device, hep_bop_vsd_device behind two renders) on the MI355X.

  pairs16    ``bop_errors`` for 16 matched pairs at 256 x 256 with an icosphere of 20480 faces (10242 vertices, tools/render_time.py), ten
             taus, no test image: device events around the whole call and around its parts - the two renders (ground truth, estimate),
             the point errors, VSD - 5 warm-up calls, 30 timed ones
  pairs256   the same for 256 pairs (four chunks of 64)
  pass       a 256-frame validation pass of ``SceneEvaluator`` (phi 0, size 256, batch 16, fp32, seeded weights, one annotation per frame,
             everything preloaded, a detection planted on every annotation so that every frame has a matched pair) without and with
             ``bop=``, the two alternating; host clock around ``add`` x 16 + ``result``
  parent     with ``--parent ROOT`` (a built tree of the parent commit): the same pass without ``bop=`` run from that tree

Every workload runs in a child process of its own under its own time limit; the parent prints one JSON line with min / median / max.

    python tools/bop_time.py [--repeats 5] [--parent ROOT] [--json FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIMITS = {"pairs16": 120, "pairs256": 180, "pass": 300, "parent": 300}       # seconds per child


def stats(v):
    return dict(min=float(min(v)), median=float(np.median(v)), max=float(max(v)))


def timed(run, warm, n):
    import torch
    for _ in range(warm):
        run()
    us = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return stats(us)


def child_pairs(n):
    import torch
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd import bop as BP
    from hmd_ego_pose_amd import render as RN
    from render_time import icosphere
    from scipy.spatial.transform import Rotation
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    dev, size, chunk = torch.device("cuda", 0), 256, 64
    rng = np.random.Generator(np.random.PCG64(9))
    mesh = RN.MeshSet([icosphere(5, 80.0)], device=dev)
    syms = BP.SymmetrySet([None], device=dev)
    pairs = np.zeros((n, 32))
    pairs[:, 0] = 1.0
    pairs[:, 2] = np.arange(n)
    Rg = Rotation.from_rotvec(rng.standard_normal((n, 3)))
    pairs[:, 4:13] = Rg.as_matrix().reshape(n, 9)
    pairs[:, 13:16] = np.stack([rng.normal(0, 40, n), rng.normal(0, 40, n), 500 + rng.normal(0, 50, n)], axis=-1)
    pairs[:, 16:25] = (Rotation.from_rotvec(rng.standard_normal((n, 3)) * 0.05) * Rg).as_matrix().reshape(n, 9)
    pairs[:, 25:28] = pairs[:, 13:16] + rng.standard_normal((n, 3)) * np.array([2.0, 2.0, 10.0])
    pairs[:, 28:32] = (480.0, 480.0, size / 2, size / 2)
    p = torch.from_numpy(pairs).to(dev)
    tau = np.ascontiguousarray(np.array(BP.TAU_FRACTIONS) * 160.0)
    out = BP.bop_errors(p, mesh, syms, size, size, taus=tau, chunk=chunk)
    res = dict(pairs=n, faces=mesh.num_faces, vertices=mesh.num_vertices, taus=len(tau), chunk=chunk,
               union_pixels_per_pair=int(out["counts"][:, 0].sum()) // n, mean_mssd=float(out["mssd"].mean()), mean_vsd=float(out["vsd"].mean()))
    res["bop_errors_us"] = timed(lambda: BP.bop_errors(p, mesh, syms, size, size, taus=tau, chunk=chunk), 5, 30)
    # the parts, on the first chunk's shapes repeated for every chunk
    lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    cam = torch.ones((n, 5), dtype=torch.float64, device=dev)
    cam[:, :4] = p[:, 28:32]
    tables = []
    for o in (4, 16):
        poses = torch.zeros((n, 1, 16), dtype=torch.float64, device=dev)
        poses[:, 0, 0], poses[:, 0, 2] = 1.0, 1.0
        poses[:, 0, 4:16] = p[:, o:o + 12]
        tables.append(poses)

    def renders():
        return [[RN.render_models(t[c:c + chunk], cam[c:c + chunk], mesh, size, size, mask=False, depth=True)["depth"] for t in tables] for c in range(0, n, chunk)]
    res["two_renders_us"] = timed(renders, 5, 30)
    errors = torch.empty((n, 2), dtype=torch.float64, device=dev)
    as_i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    res["point_errors_us"] = timed(lambda: _capi.check(lib.hep_bop_point_errors_device(
        p.data_ptr(), n, mesh.vertices.data_ptr(), mesh.num_vertices, as_i32(mesh.vertex_start), syms.table.data_ptr(), syms.num_symmetries, as_i32(syms.start), 1,
        errors.data_ptr(), stream)), 5, 30)
    depth = renders()
    vsd, counts = torch.empty((n, len(tau)), dtype=torch.float64, device=dev), torch.empty((n, 2 + len(tau)), dtype=torch.int32, device=dev)
    m = min(n, chunk)
    ws = torch.empty((_capi.check(lib.hep_bop_workspace_bytes(m, len(tau))),), dtype=torch.uint8, device=dev)

    def all_vsd():
        for k, c in enumerate(range(0, n, chunk)):
            _capi.check(lib.hep_bop_vsd_device(p[c:c + chunk].data_ptr(), m, 1, depth[k][0].data_ptr(), depth[k][1].data_ptr(), None, 0, size, size, 15.0,
                                               tau.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(tau), vsd[c:].data_ptr(), counts[c:].data_ptr(),
                                               ws.data_ptr(), ws.numel(), stream))
    res["vsd_us"] = timed(all_vsd, 5, 30)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), out["counts"].cpu().numpy())
    return res


class Planted:
    """The model with one detection planted on every frame's annotation (row 0: its box, its pose moved a little)."""

    def __init__(self, inner, boxes, rotation, translation):
        self.inner, self.model, self.rows, self.at = inner, inner.model, (boxes, rotation, translation), 0

    def detect(self, x, camera):
        det = {k: v.clone() for k, v in self.inner.detect(x, camera).items()}
        B = det["scores"].shape[0]
        boxes, rot, trn = (t[self.at:self.at + B] for t in self.rows)
        det["scores"][:, 0], det["labels"][:, 0] = 0.99, 0
        det["boxes"][:, 0], det["rotation"][:, 0], det["translation"][:, 0] = boxes, rot, trn
        self.at += B
        return det


def child_pass(repeats, with_bop, n_frames=256, batch=16):
    import torch
    from eval_time import MemoryFolder
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from render_time import icosphere
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    size, dev = 256, torch.device("cuda", 0)
    ds = MemoryFolder(n_frames, size)
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(0, 0), strict=True)
    inner = TrainModelWithLoss(m.to(dev).eval()).eval()
    u8 = torch.from_numpy(ds.frames).to(dev)
    cam = torch.from_numpy(np.stack([ds.camera_input(i, 1.0) for i in range(len(ds))])).to(dev)
    anns = [[dict(a, label=0)] for a in ds.annotations]
    gt = torch.from_numpy(E.gt_scene_table(anns, ds.camera, 1.0, 1)).to(dev)
    rng = np.random.Generator(np.random.PCG64(4))
    model = Planted(inner, gt[:, 0, 1:5].float(), ((gt[:, 0, 5:8] + 0.02) / np.pi).float(),
                    (gt[:, 0, 8:11] + torch.from_numpy(rng.standard_normal((n_frames, 3)) * np.array([2.0, 2.0, 10.0])).to(dev)).float())
    ev = E.SceneEvaluator(model, [(ds.points, ds.diameter, False)], size, len(ds), 1, 0.5, 10, 0.5, device=dev)
    settings = None
    if with_bop:
        from hmd_ego_pose_amd import bop as BP
        from hmd_ego_pose_amd import render as RN
        settings = BP.BopSettings(RN.MeshSet([icosphere(5, 80.0)], device=dev), BP.SymmetrySet([None], device=dev))

    def one_pass(bop):
        ev.reset()
        model.at = 0
        for o in range(0, len(ds), batch):
            if bop is None:
                ev.add(u8[o:o + batch], cam[o:o + batch], gt[o:o + batch])
            else:
                ev.add(u8[o:o + batch], cam[o:o + batch], gt[o:o + batch], bop=bop)
        return ev.result()

    kinds = [None, settings] if with_bop else [None]
    res = [one_pass(k) for k in kinds]
    out = {"frames": n_frames, "batch": batch, "matched": res[0]["mean"]["num_matched"]}
    if with_bop:
        assert repr({k: res[1][k] for k in res[0]}) == repr(res[0])
        out["AR"] = res[1]["bop"]["mean"]
    times = [[] for _ in kinds]
    for _ in range(repeats):
        for i, k in enumerate(kinds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one_pass(k)
            times[i].append((time.perf_counter() - t0) * 1e3)
    out["plain_ms"] = stats(times[0])
    if with_bop:
        out["bop_ms"] = stats(times[1])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: its SceneEvaluator pass is timed next to this tree's")
    ap.add_argument("--child", default=None, choices=list(LIMITS))
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        sys.path.insert(0, HERE)
        sys.path.insert(0, a.root)                                  # the package of the tree under test; the helpers of tools/ are this tree's
        res = child_pass(a.repeats, a.child == "pass") if a.child in ("pass", "parent") else child_pairs(16 if a.child == "pairs16" else 256)
        print("RESULT " + json.dumps(res))
        return res
    out = {}
    for name, limit in LIMITS.items():
        if name == "parent" and a.parent is None:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats)] + (["--root", os.path.abspath(a.parent)] if name == "parent" else [])
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
