#!/usr/bin/env python3
"""Time the trainable backbone's HIP forward + backward on the GPU next to stock PyTorch-ROCm autograd of the same function.

Shapes: phi 0 @ 256 batch 16 and phi 3 @ 512 batch 8, seed-0 weights, the seeded image and cotangents of
tests/_backbone_grad.py.  Device events around each repetition after a warm-up, the paths ALTERNATING in one run; rows in
milliseconds (median, min, max of --reps):
  hip fwd+bwd      backbone.backbone_forward + backbone.backbone_backward (the two ABI calls, parameter gradients only)
  hip autograd     TrainableBackbone(image) + backward through autograd (adds the flat-parameter cat and its split)
  torch fwd+bwd    autograd through oracle.efficientpose_ref.backbone on the same device and inputs, float32: the baseline
Every shape runs in a child process of its own under a time limit (--limit seconds); a shape that fails ends the run.

    python tools/backbone_grad_time.py [--reps 50] [--warmup 5] [--json FILE] [--limit 240]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmd_ego_pose_amd import get_arch, seeded_state_dict  # noqa: E402
from hmd_ego_pose_amd import backbone as BB  # noqa: E402
from tests import _backbone_grad as G  # noqa: E402

SHAPES = [(0, 256, 16), (3, 512, 8)]


def launches(phi):
    """(forward, backward without the image gradient) kernel launches of hep_backbone_*_device."""
    blocks = get_arch(phi).blocks
    fwd = 3 + sum(6 if b.expand else 5 for b in blocks) + 3        # pack, image copy, stem; per block; the three taps
    bwd = sum(15 if b.expand else 11 for b in blocks) + 3
    return fwd, bwd


def one_shape(phi, size, batch, reps, warmup):
    sd = seeded_state_dict(phi, 0)
    bb = BB.TrainableBackbone(phi)
    bb.load_state_dict(sd, strict=False)
    bb = bb.cuda()
    image_np, cots_np = G.seeded_inputs(phi, size, batch)
    image = torch.from_numpy(image_np).cuda()
    cots = [torch.from_numpy(a).cuda() for a in cots_np]
    flat = bb.flat_parameters().detach()
    sd_dev = {k: sd[k].cuda().requires_grad_(G.trainable(k)) for k, _ in G.backbone_keys(phi)}

    def hip_abi():
        _t, ws = BB.backbone_forward(flat, image, phi)
        BB.backbone_backward(flat, cots, ws, phi, size)

    def hip_autograd():
        bb.zero_grad(set_to_none=True)
        torch.autograd.backward(bb(image), cots)

    def torch_fb():
        for v in sd_dev.values():
            v.grad = None
        torch.autograd.backward(G.oracle_backbone(sd_dev, image, phi), cots)

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
    nbytes = BB._capi.lib().hep_backbone_workspace_bytes(phi, size, batch)
    fwd, bwd = launches(phi)
    print(f"phi {phi} @ {size} batch {batch}: {len(get_arch(phi).blocks)} blocks, workspace {nbytes / 2 ** 20:.0f} MiB "
          f"({nbytes / 2 ** 20 / batch:.0f} MiB per image); launches: forward {fwd}, backward {bwd}")
    rows = {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}
    for k, (med, lo, hi) in rows.items():
        print(f"  {k:16s} {med:9.3f} ms   (min {lo:.3f}, max {hi:.3f})")
    return {"phi": phi, "size": size, "batch": batch, "workspace_bytes": int(nbytes), "launches": [fwd, bwd], "rows_ms": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the table to this file")
    ap.add_argument("--limit", type=int, default=240, help="seconds one shape may take")
    ap.add_argument("--shape", default=None, help="phi,size,batch: run this one shape in this process and print its JSON row last")
    args = ap.parse_args()
    if args.shape:
        assert torch.cuda.is_available(), "needs the MI355X"
        phi, size, batch = (int(v) for v in args.shape.split(","))
        print("JSON " + json.dumps(one_shape(phi, size, batch, args.reps, args.warmup)))
        return 0
    res, status = [], 0
    for phi, size, batch in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{phi},{size},{batch}", "--reps", str(args.reps), "--warmup", str(args.warmup)]
        try:
            done = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)     # a fresh child per shape, under its own limit
        except subprocess.TimeoutExpired:
            print(f"phi {phi} @ {size} batch {batch}: over its limit of {args.limit} s; stopping")
            status = 1
            break
        sys.stdout.write("".join(l + "\n" for l in done.stdout.splitlines() if not l.startswith("JSON ")))
        if done.returncode != 0:
            print(f"phi {phi} @ {size} batch {batch}: exit status {done.returncode}; stopping")
            status = 1
            break
        res.extend(json.loads(l[5:]) for l in done.stdout.splitlines() if l.startswith("JSON "))
    if args.json:                                    # the shapes that finished, also after a failure
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return status


if __name__ == "__main__":
    sys.exit(main())
