#!/usr/bin/env python3
"""Time the trainable heads' HIP forward and backward on the GPU (device events, warm-up first).

Shapes: phi 0 @ 256 batch 16 and phi 3 @ 512 batch 8 (the benchmarked inference shapes), seed-0 weights, unit-normal maps
and cotangents.  Rows (milliseconds, median of --reps timed repetitions after --warmup):
  hip fwd            heads.heads_forward (hep_heads_forward_device; the workspace is allocated by torch's caching allocator)
  hip bwd            heads.heads_backward on that workspace (hep_heads_backward_device, parameter and map gradients)
  hip fwd+bwd        the two back to back (the row tools/neck_grad_time.py and tools/backbone_grad_time.py call the same)
  hip fwd+bwd (autograd)  TrainableHeads(feats) + backward through autograd (adds the flat-parameter cat of 363 tensors and its
                     split; at phi 0 the row is 2 .. 4 ms around 1 ms of kernels, so presumably bound by that host work)
  torch fwd / fwd+bwd  stock PyTorch-ROCm autograd through oracle.efficientpose_ref.head on the same device and inputs:
                     the baseline (the same function as ~1000 small launches), not the code under test
and the launch counts of the two HIP entry points.

    python tools/heads_grad_time.py [--reps 20] [--warmup 5] [--json FILE]
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
from hmd_ego_pose_amd import heads as HD  # noqa: E402
from tests import _head_grad as H  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def one_shape(phi, size, batch, reps, warmup):
    classes = 1
    sd = seeded_state_dict(phi, 0, num_classes=classes)
    h = HD.TrainableHeads(phi, classes)
    h.load_state_dict(sd, strict=False)
    h = h.cuda()
    feats = [torch.from_numpy(a).cuda() for a in H.seeded_maps(phi, size, batch, 1)]
    cots = [torch.from_numpy(a).cuda() for a in H.seeded_cotangents(classes, size, batch, 2)]
    flat = h.flat_parameters().detach()
    shapes = [tuple(f.shape) for f in feats]
    outs, ws = HD.heads_forward(flat, feats, phi, classes, size)

    fg = [f.clone().requires_grad_(True) for f in feats]

    def hip_abi():
        _o, w = HD.heads_forward(flat, feats, phi, classes, size)
        HD.heads_backward(flat, cots, w, phi, classes, size, shapes)

    def hip_fb():
        h.zero_grad(set_to_none=True)
        for f in fg:
            f.grad = None
        o = h(fg)
        torch.autograd.backward(o, cots)

    sd_dev = {k: v.cuda().requires_grad_(H.trainable(k)) for k, v in sd.items() if k.split(".", 1)[0] in H.HEAD_NAMES and v.dtype == torch.float32}

    def torch_f():
        with torch.no_grad():
            return H.oracle_heads(sd_dev, feats, phi, classes)

    def torch_fb():
        for v in sd_dev.values():
            v.grad = None
        for f in fg:
            f.grad = None
        torch.autograd.backward(H.oracle_heads(sd_dev, fg, phi, classes), cots)

    d = get_arch(phi).head_depth
    rows = {
        "hip fwd": timed(lambda: HD.heads_forward(flat, feats, phi, classes, size), reps, warmup),
        "hip bwd": timed(lambda: HD.heads_backward(flat, cots, ws, phi, classes, size, shapes), reps, warmup),
        "hip fwd+bwd": timed(hip_abi, reps, warmup),
        "hip fwd+bwd (autograd)": timed(hip_fb, reps, warmup),
        "torch fwd": timed(torch_f, reps, warmup),
        "torch fwd+bwd (autograd)": timed(torch_fb, reps, warmup),
    }
    print(f"phi {phi} @ {size} batch {batch}: width {get_arch(phi).fpn_w}, depth {d}, {batch * sum(s * s for s in HD.level_sizes(size))} pixels per net and layer, "
          f"workspace {ws.numel() / 2 ** 20:.0f} MiB; launches: forward {3 + 2 * d}, backward {6 + 4 * d}")
    for k, (med, lo, hi) in rows.items():
        print(f"  {k:28s} {med:9.3f} ms   (min {lo:.3f}, max {hi:.3f})")
    return {"phi": phi, "size": size, "batch": batch, "rows_ms": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
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
