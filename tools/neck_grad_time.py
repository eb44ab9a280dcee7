#!/usr/bin/env python3
"""Time the trainable neck's HIP forward + backward on the GPU next to stock PyTorch-ROCm autograd of the same function.

Shapes: phi 0 @ 256 batch 16 and phi 3 @ 512 batch 8, seed-0 weights, the seeded taps and cotangents of tests/_neck_grad.py.
Device events around each repetition after a warm-up, the two paths ALTERNATING in one run; rows in milliseconds (median,
min, max of --reps):
  hip fwd+bwd      neck.neck_forward + neck.neck_backward (the two ABI calls, parameter and tap gradients)
  hip autograd     TrainableNeck(taps) + backward through autograd (adds the flat-parameter cat and its split)
  torch fwd+bwd    autograd through oracle.efficientpose_ref.bifpn_cell on the same device and inputs, float32: the baseline

    python tools/neck_grad_time.py [--reps 50] [--warmup 5] [--json FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmd_ego_pose_amd import get_arch, seeded_state_dict  # noqa: E402
from hmd_ego_pose_amd import neck as NK  # noqa: E402
from tests import _neck_grad as N  # noqa: E402


def one_shape(phi, size, batch, reps, warmup):
    sd = seeded_state_dict(phi, 0)
    neck = NK.TrainableNeck(phi)
    neck.load_state_dict(sd, strict=False)
    neck = neck.cuda()
    taps_np, cots_np = N.seeded_inputs(phi, size, batch)
    taps = [torch.from_numpy(a).cuda() for a in taps_np]
    cots = [torch.from_numpy(a).cuda() for a in cots_np]
    flat = neck.flat_parameters().detach()
    shapes = [tuple(t.shape) for t in taps]
    tg = [t.clone().requires_grad_(True) for t in taps]
    sd_dev = {k: sd[k].cuda().requires_grad_(N.trainable(k)) for k, _ in N.neck_keys(phi)}

    def hip_abi():
        _f, ws = NK.neck_forward(flat, taps, phi, size)
        NK.neck_backward(flat, cots, ws, phi, size, shapes)

    def hip_autograd():
        neck.zero_grad(set_to_none=True)
        for t in tg:
            t.grad = None
        torch.autograd.backward(neck(tg), cots)

    def torch_fb():
        for v in sd_dev.values():
            v.grad = None
        for t in tg:
            t.grad = None
        torch.autograd.backward(N.oracle_neck(sd_dev, tg, phi), cots)

    fns = {"hip fwd+bwd": hip_abi, "hip autograd": hip_autograd, "torch fwd+bwd": torch_fb}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():                    # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    nbytes = NK._capi.lib().hep_neck_workspace_bytes(phi, size, batch)
    cells = get_arch(phi).fpn_cells
    print(f"phi {phi} @ {size} batch {batch}: width {get_arch(phi).fpn_w}, {cells} cells, workspace {nbytes / 2 ** 20:.0f} MiB; "
          f"launches: forward {17 + 24 * cells}, backward {48 * cells + 29}")
    rows = {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}
    for k, (med, lo, hi) in rows.items():
        print(f"  {k:16s} {med:9.3f} ms   (min {lo:.3f}, max {hi:.3f})")
    return {"phi": phi, "size": size, "batch": batch, "workspace_bytes": int(nbytes), "rows_ms": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = [one_shape(0, 256, 16, args.reps, args.warmup), one_shape(3, 512, 8, args.reps, args.warmup)]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
