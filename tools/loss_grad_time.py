#!/usr/bin/env python3
"""Time the training losses' forward + backward on the GPU (device events, warm-up first).

Shape: B 16, N 12276 anchors, K 1, H 63, P 500 model points, about 40 object anchors per image, half of them symmetric.
Rows printed (milliseconds, median of --reps timed repetitions after --warmup):
  hip fwd            training.losses without grad (hep_losses_device; includes its stream synchronise)
  hip bwd            training.losses_backward alone (hep_losses_backward_device: three launches)
  hip fwd+bwd        losses() with requires_grad + backward of the train.py weighting
  f64 restatement    tests/_loss_grad.py forward + autograd backward (float64 torch on the GPU; its symmetric
                     nearest-point search runs in numpy on the host)
  per-image loop     the reference's shape of the computation in float32 torch on the GPU: a Python loop over the
                     batch, index gathers and a dense P x P torch.norm for the symmetric objects, autograd backward
and the backward's byte floor: the bytes it must move (every gradient element written, the state columns read, the
object rows read) over the HBM peak of 8 TB/s (6.3 TB/s measured copy rate in brackets).

    python tools/loss_grad_time.py [--reps 20] [--warmup 5]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmd_ego_pose_amd.training import _loss_inputs, losses, losses_backward  # noqa: E402
from tests._loss_grad import TRAIN_WEIGHTS, batch_losses  # noqa: E402
from tests.test_gpu_loss_grad import make_case  # noqa: E402


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


def per_image_loop(d, pts, R=3):
    """The reference's batch_iterate structure (a loop over the images, gathers, dense symmetric distances), float32."""
    B = d["classification"].shape[0]
    out = [[] for _ in range(5)]
    for j in range(B):
        gc, pc = d["gt_classification"][j], d["classification"][j]
        keep = gc[:, -1] != -1
        lab, p = gc[keep, :-1], torch.clamp(pc, 1e-4, 1 - 1e-4)[keep]
        af = torch.where(lab == 1, 0.25, 0.75)
        fw = af * torch.pow(torch.where(lab == 1, 1 - p, p), 1.5)
        bce = -(lab * torch.log(p) + (1 - lab) * torch.log(1 - p))
        out[0].append(torch.where(lab != -1, fw * bce, 0).sum() / max(1.0, float((gc[:, -1] == 1).sum())))

        def sl1(gt, pred):
            o = gt[:, -1] == 1
            dd = (pred[o] - gt[o, :-1]).abs()
            return torch.where(dd <= 1 / 9, 4.5 * dd * dd, dd - 0.5 / 9).sum() / max(1.0, float(o.sum()))
        out[1].append(sl1(d["gt_regression"][j], d["regression"][j]))
        out[4].append(sl1(d["gt_hand"][j], d["hand"][j]))
        gt, pt = d["gt_transformation"][j], d["transformation"][j]
        o = torch.round(gt[:, -1]) == 1
        g, p = gt[o], pt[o]
        mp = pts[torch.round(g[:, -2]).long()]

        def rot(v):
            v = v * math.pi
            ang = v.norm(dim=-1, keepdim=True)[:, None]
            ax = (v / ang.squeeze(1))[:, None]
            return mp * torch.cos(ang) + torch.cross(ax.expand_as(mp), mp, dim=-1) * torch.sin(ang) + ax * (ax * mp).sum(-1, keepdim=True) * (1 - torch.cos(ang))
        op, ot = rot(p[:, :R]), rot(g[:, :R])
        sym = torch.round(g[:, -3]) == 1
        ds = torch.min(torch.norm(op[sym][:, :, None] - ot[sym][:, None], dim=-1), dim=-1)[0].mean(-1)
        da = torch.norm(op[~sym] - ot[~sym], dim=-1).mean(-1)
        r = torch.cat([ds, da]).mean()
        out[2].append(torch.where(torch.isnan(r), torch.zeros_like(r), r))
        out[3].append(torch.nn.functional.smooth_l1_loss(p[:, R:], g[:, R:R + 3]))
    return [torch.stack(x).mean() * (50 if k == 1 else 1) for k, x in enumerate(out)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    B, N, K, H, P = 16, 12276, 1, 63, 500
    c = make_case(B, N, K, P, 40, 2024)
    d = {k: torch.from_numpy(v).cuda() for k, v in c.items() if k != "model_points"}
    pts = torch.from_numpy(c["model_points"]).cuda()
    w = torch.tensor(TRAIN_WEIGHTS, device="cuda")
    args_l = lambda dd: (dd["gt_classification"], dd["classification"], dd["gt_regression"], dd["regression"], dd["gt_transformation"],
                         dd["transformation"], dd["gt_hand"], dd["hand"], c["model_points"], 3)
    preds = ("classification", "regression", "transformation", "hand")
    dg = dict(d)
    for k in preds:
        dg[k] = d[k].clone().requires_grad_(True)
    t, sizes = _loss_inputs(*args_l(d))
    u = torch.zeros((B, 5), device="cuda") + (w * torch.tensor([1.0, 50.0, 1.0, 1.0, 1.0], device="cuda") / B)[None]

    def hip_fb():
        for k in preds:
            dg[k].grad = None
        out, _ = losses(*args_l(dg))
        (out * w).sum().backward()

    d64 = {k: v.double() for k, v in d.items()}
    p64 = {k: d64[k].clone().requires_grad_(True) for k in preds}

    def f64_fb():
        for k in preds:
            p64[k].grad = None
        out, _ = batch_losses(d64["gt_classification"], p64["classification"], d64["gt_regression"], p64["regression"], d64["gt_transformation"],
                              p64["transformation"], d64["gt_hand"], p64["hand"], c["model_points"], 3)
        (out * w.double()).sum().backward()

    def loop_fb():
        for k in preds:
            dg[k].grad = None
        res = per_image_loop(dg, pts)
        sum(wt * r for wt, r in zip(TRAIN_WEIGHTS, res)).backward()

    rows = {
        "hip fwd": timed(lambda: losses(*args_l(d)), args.reps, args.warmup),
        "hip bwd": timed(lambda: losses_backward(t, sizes, u), args.reps, args.warmup),
        "hip fwd+bwd": timed(hip_fb, args.reps, args.warmup),
        "f64 restatement fwd+bwd": timed(f64_fb, max(3, args.reps // 4), 1),
        "per-image loop fp32 fwd+bwd": timed(loop_fb, max(3, args.reps // 4), 1),
    }
    nobj = int((np.round(c["gt_transformation"][..., -1]) == 1).sum())
    write = 4 * B * N * (K + 4 + 6 + H)                                 # every gradient element, zeros included
    read = (4 * B * N * ((2 * K + 1) + 1 + 2 + 1)                       # labels + scores + state; the other states (transformation twice)
            + 4 * nobj * ((4 + 4) + (6 + 6) + (H + H))                  # the object rows: prediction + target
            + 4 * B * 5 + 4 * B * (N + 4) * 2)                          # upstream gradient, workspace written and read
    floor_ms = (write + read) / 8e12 * 1e3
    print(f"shape B {B} N {N} K {K} H {H} P {P}: {nobj} object anchors, {int((c['gt_transformation'][..., -3] == 1)[np.round(c['gt_transformation'][..., -1]) == 1].sum())} symmetric")
    for k, (med, lo, hi) in rows.items():
        print(f"{k:30s} {med:9.3f} ms   (min {lo:.3f}, max {hi:.3f})")
    print(f"backward bytes: {write / 1e6:.1f} MB written + {read / 1e6:.1f} MB read -> floor {floor_ms * 1e3:.1f} us at 8 TB/s "
          f"({(write + read) / 6.3e12 * 1e6:.1f} us at 6.3 TB/s); measured bwd {rows['hip bwd'][0] * 1e3:.1f} us")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows_ms": rows, "bytes_written": write, "bytes_read": read, "floor_us_8TBs": floor_ms * 1e3}, f, indent=1)

if __name__ == "__main__":
    main()
