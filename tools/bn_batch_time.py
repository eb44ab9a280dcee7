#!/usr/bin/env python3
"""Time forward + backward of the three trainable parts with running-statistics and with batch-statistics BatchNorm on the GPU
(device events, warm-up first; the timing approach of tools/heads_grad_time.py: the two ABI calls back to back, the workspace
from torch's caching allocator, median of --reps after --warmup), and print the workspace size of both modes.

Shape: phi 0 @ 256 batch 16, seed-0 weights, the seeded inputs and cotangents of the gradient tests.  HEP_BN_RUNNING runs the
launches of hep_{part}_{forward,backward}_device; HEP_BN_BATCH adds per BatchNorm three launches to the forward (statistics,
finish, apply) and two to the backward (the gamma / beta reduce ahead of the products, the d z correction).

    python tools/bn_batch_time.py [--reps 20] [--warmup 5] [--json FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmd_ego_pose_amd import _capi, seeded_state_dict  # noqa: E402
from hmd_ego_pose_amd import backbone as BK  # noqa: E402
from hmd_ego_pose_amd import heads as HD  # noqa: E402
from hmd_ego_pose_amd import neck as NK  # noqa: E402
from tests import _bn_batch as BB  # noqa: E402
from tools.heads_grad_time import timed  # noqa: E402


def one_part(part, phi, size, batch, reps, warmup):
    case = (phi, size, batch, 0, 1 if part == "heads" else None, None)
    sd = seeded_state_dict(phi, 0)
    m = {"heads": lambda: HD.TrainableHeads(phi, 1), "neck": lambda: NK.TrainableNeck(phi), "backbone": lambda: BK.TrainableBackbone(phi)}[part]()
    m.load_state_dict(sd, strict=False)
    flat = m.cuda().flat_parameters().detach()
    x_np, cots_np = BB.inputs(part, case)
    xs = [torch.from_numpy(a).cuda() for a in x_np]
    cots = [torch.from_numpy(a).cuda() for a in cots_np]
    shapes = [tuple(a.shape) for a in xs]
    stats = torch.empty_like(flat)
    l = _capi.lib()
    cfg = (phi, 1, size, batch) if part == "heads" else (phi, size, batch)
    out = {"part": part, "phi": phi, "size": size, "batch": batch, "rows_ms": {}, "workspace_bytes": {}}
    for name, mode in (("running", 0), ("batch", 1)):
        if part == "heads":
            fwd = lambda: HD.heads_forward(flat, xs, phi, 1, size, mode, stats=stats if mode else None)
            bwd = lambda ws: HD.heads_backward(flat, cots, ws, phi, 1, size, shapes, mode)
        elif part == "neck":
            fwd = lambda: NK.neck_forward(flat, xs, phi, size, mode, stats=stats if mode else None)
            bwd = lambda ws: NK.neck_backward(flat, cots, ws, phi, size, shapes, mode)
        else:
            fwd = lambda: BK.backbone_forward(flat, xs[0], phi, None, mode, stats=stats if mode else None)
            bwd = lambda ws: BK.backbone_backward(flat, cots, ws, phi, size, None, True, mode)
        _o, ws = fwd()
        out["rows_ms"][f"{name} fwd"] = timed(fwd, reps, warmup)
        out["rows_ms"][f"{name} bwd"] = timed(lambda: bwd(ws), reps, warmup)
        out["rows_ms"][f"{name} fwd+bwd"] = timed(lambda: bwd(fwd()[1]), reps, warmup)
        out["workspace_bytes"][name] = int(getattr(l, f"hep_{part}_workspace_bytes_bn")(*cfg, mode))
        del ws
    print(f"{part} phi {phi} @ {size} batch {batch}: workspace {out['workspace_bytes']['running'] / 2 ** 20:.1f} MiB running, "
          f"{out['workspace_bytes']['batch'] / 2 ** 20:.1f} MiB batch")
    for k, (med, lo, hi) in out["rows_ms"].items():
        print(f"  {k:18s} {med:9.3f} ms   (min {lo:.3f}, max {hi:.3f})")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = [one_part(part, 0, 256, 16, args.reps, args.warmup) for part in BB.PARTS]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
