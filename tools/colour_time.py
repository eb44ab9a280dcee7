#!/usr/bin/env python3
"""Time the colour augmentation on the GPU (device events, warm-up first, median of --reps repetitions): hep_colour_augment_device
(augment.colour_augment's ABI call on buffers allocated once) for every operation alone in slot 0 and for a three-operation chain
through the fused statistics (Equalize -> EnhanceContrast -> Autocontrast), at the frame shapes tools/augment_time.py times:

    256 x 256, batch 16        256 x 256, batch 8

Every image of the batch carries the same table row.  A call is always a memset of the counters and four launches (stats0, apply0,
apply1, apply2); the workgroups of a launch whose slot is empty, or whose image needs no statistics, exit at once.  Printed per row:
the whole call, the number of launches that do work (n, plus stats0 when slot 0 needs statistics), the whole call divided by that
number (the per-launch figure: it includes the share of the idle launches), the bytes the working launches must move (n reads and
writes of B * H * W * 3, plus one frame read for stats0) and the rate that gives over the whole call.  The yardstick is
hep_augment_6dof_device at the same shape (every image augmented, no resize), measured the same way in the same process.

    python tools/colour_time.py [--reps 50] [--warmup 5] [--json FILE]

The measurement runs in a child process under its own time limit.
"""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("256x256, batch 16", 16, 256, 256), ("256x256, batch 8", 8, 256, 256))
CHAIN = (2, 7, 1)
NEEDS_STATS = (1, 2, 7)


def child(args):
    import numpy as np
    import torch

    from hmd_ego_pose_amd import _capi, augment
    assert torch.cuda.is_available(), "needs the MI355X"

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    def table(B, H, W, ids):
        ops = np.zeros((B, 3, 8), np.int32)
        ops[:, :, 0] = -1
        arg = np.zeros((B, 3, 2), np.float32)
        for k, op in enumerate(ids):
            i0, i1, i2, i3, seed, f = augment.colour_parameters(op, 14, H, W, 1, (0.5, 0.5), 0x1234567 + k)
            ops[:, k, :5] = (op, i0, i1, i2, i3)
            ops[:, k, 5] = seed
            arg[:, k, 0] = f
        return augment.check_colour_table(ops, arg, B, H, W)

    def yardstick(B, H, W, d_frames):
        """hep_augment_6dof_device on the same frames: three objects per image, every image augmented, size = H (no resize launch)."""
        kmax, S = 3, max(H, W)
        rng = np.random.Generator(np.random.PCG64(20))
        masks = np.zeros((B, H, W), np.uint8)
        boxes = np.zeros((B, kmax, 4), np.float64)
        for k, (x0, y0) in enumerate(((60, 70), (130, 90), (100, 150))):
            masks[:, y0:y0 + 40, x0:x0 + 50] = 21 * (k + 1)
            boxes[:, k] = (x0, y0, x0 + 49, y0 + 39)
        axis = rng.standard_normal((B, kmax, 3)); axis /= np.linalg.norm(axis, axis=2, keepdims=True)
        host = dict(boxes=boxes, labels=rng.integers(0, 8, (B, kmax)).astype(np.int32), mask_values=np.tile(np.array([21, 42, 63], np.int32), (B, 1)),
                    rvec=(axis * rng.uniform(0.4, 2.4, (B, kmax, 1))).astype(np.float32), tvec=rng.uniform(-200, 900, (B, kmax, 3)).astype(np.float32),
                    extra=np.zeros((B, kmax, 2), np.float32))
        ann = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        num_gt = torch.full((B,), kmax, dtype=torch.int32, device="cuda")
        cam = np.tile(np.array([572.4, 573.6, W / 2.0, H / 2.0], np.float32), (B, 1))
        ang, sc, ap = augment.draw_6dof(random.Random(1), B, chance_no_augmentation=0.0)
        xform = np.empty((B, 9), np.float64)
        xform[:, :6] = augment.rotation_matrices(ang, sc, cam[:, 2:4])
        xform[:, 6], xform[:, 7], xform[:, 8] = ang / 180.0 * np.pi, sc, ap
        d_masks, d_xform, d_cam = (torch.from_numpy(v).cuda() for v in (masks, xform, cam))
        ws = torch.empty((_capi.check(l.hep_augment_workspace_bytes(B, H, W, S, kmax)),), dtype=torch.uint8, device="cuda")
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
        out = {"image": f32(B, 3, S, S), "mask": torch.empty((B, H, W), dtype=torch.uint8, device="cuda"), "camera": f32(B, 6),
               "gt_boxes": torch.empty((B, kmax, 4), dtype=torch.float64, device="cuda"), "gt_labels": i32(B, kmax), "gt_transform": f32(B, kmax, 8),
               "gt_num": i32(B), "applied": i32(B)}
        t = timed(lambda: augment._run(l, d_frames, d_masks, d_xform, d_cam, ann, num_gt, B, H, W, S, kmax, 1000.0, out, ws, d_frames.device))
        assert out["applied"].sum().item() == B, "every image of the timed batch is meant to be augmented"
        return t, B * H * W * (3 + 1 + 1) + B * 3 * S * S * 4

    l = _capi.lib()
    result = []
    for name, B, H, W in SHAPES:
        frames = np.random.Generator(np.random.PCG64(21)).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        d_frames = torch.from_numpy(frames).cuda()
        out = torch.empty_like(d_frames)
        ws = torch.empty((_capi.check(l.hep_colour_workspace_bytes(B, H, W)),), dtype=torch.uint8, device="cuda")
        frame_bytes = B * H * W * 3
        rows = []
        for label, ids in [("no operation (copy)", ())] + [(augment.COLOUR_OPS[op], (op,)) for op in range(len(augment.COLOUR_OPS))] + \
                          [(" -> ".join(augment.COLOUR_OPS[op] for op in CHAIN), CHAIN)]:
            ops, arg = table(B, H, W, ids)
            d_ops, d_arg = torch.from_numpy(ops).cuda(), torch.from_numpy(arg).cuda()
            t = timed(lambda: augment._run_colour(l, d_frames, d_ops, d_arg, B, H, W, out, ws, d_frames.device))
            stats0 = bool(ids) and ids[0] in NEEDS_STATS
            working = max(len(ids), 1) + stats0
            nbytes = 2 * max(len(ids), 1) * frame_bytes + stats0 * frame_bytes
            rows.append(dict(operations=label, call_ms=t, working_launches=working, ms_per_working_launch=t[0] / working, bytes=nbytes,
                             GBps=nbytes / (t[0] * 1e-3) / 1e9))
        t6, b6 = yardstick(B, H, W, d_frames)
        result.append(dict(shape=name, rows=rows, augment_6dof_ms=t6, augment_6dof_bytes=b6, augment_6dof_GBps=b6 / (t6[0] * 1e-3) / 1e9))
    for r in result:
        print(f"{r['shape']}: augment_6dof (3 launches) {r['augment_6dof_ms'][0]:.4f} ms (min {r['augment_6dof_ms'][1]:.4f}, max {r['augment_6dof_ms'][2]:.4f}), "
              f"{r['augment_6dof_bytes'] / 1e6:.1f} MB -> {r['augment_6dof_GBps']:.0f} GB/s effective")
        for row in r["rows"]:
            print(f"  {row['operations']:<52} call {row['call_ms'][0]:.4f} ms (min {row['call_ms'][1]:.4f}, max {row['call_ms'][2]:.4f}), {row['working_launches']} working "
                  f"launch(es): {row['ms_per_working_launch']:.4f} ms each; {row['bytes'] / 1e6:.1f} MB -> {row['GBps']:.0f} GB/s effective")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the table to this file")
    ap.add_argument("--timeout", type=int, default=240, help="time limit of the measuring child process, seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--warmup", str(args.warmup)] + (["--json", args.json] if args.json else [])
    sys.exit(subprocess.run(cmd, timeout=args.timeout).returncode)


if __name__ == "__main__":
    main()
