#!/usr/bin/env python3
"""Time the training input path on the GPU (device events, warm-up first, median of --reps repetitions): the three or four
launches of hep_augment_6dof_device (augment.augment_6dof's ABI call on buffers allocated once) and training.anchor_targets_device
on its outputs, at the two shapes whose training-step times NOTEBOOK section 14 records:

    256 x 256 -> 256, batch 16, phi 0   (step 11.06 ms)     fused path, three launches
    256 x 256 -> 512, batch 8,  phi 3   (step 34.27 ms)     with the resize launch

Every image is augmented (apply = 1, scale and angle drawn with draw_6dof's defaults), three objects per image.  Also printed:
the bytes the call must move (frames and masks read, warped mask and float32 planes written; with a resize the uint8 frame once
more each way) and the rate that gives over the measured time.  The measurement runs in a child process under its own time limit.

    python tools/augment_time.py [--reps 50] [--warmup 5] [--json FILE]

Pinning the restated OpenCV conventions: where cv2 is installed, compare tests/_augment.py's warp_nearest / warp_bilinear with
cv2.warpAffine(..., flags=cv2.INTER_NEAREST / INTER_LINEAR) on the cases of tests/_augment.py:make_case, and forward_matrix with
cv2.getRotationMatrix2D; cv2 is not available where this project is built, so that comparison has not been made.
"""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("256x256 -> 256, batch 16", 16, 256, 256, 256, 11.06), ("256x256 -> 512, batch 8", 8, 256, 256, 512, 34.27))


def child(args):
    import numpy as np
    import torch

    from hmd_ego_pose_amd import _capi, augment
    from hmd_ego_pose_amd.training import anchor_targets_device
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

    l = _capi.lib()
    rows = []
    for name, B, H, W, S, step_ms in SHAPES:
        rng = np.random.Generator(np.random.PCG64(20))
        kmax = 3
        frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        masks = np.zeros((B, H, W), np.uint8)
        boxes = np.zeros((B, kmax, 4), np.float64)
        for b in range(B):
            for k, (x0, y0) in enumerate(((60, 70), (130, 90), (100, 150))):      # three objects near the centre: every warp keeps them
                masks[b, y0:y0 + 40, x0:x0 + 50] = 21 * (k + 1)
                boxes[b, k] = (x0, y0, x0 + 49, y0 + 39)
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
        d_frames, d_masks, d_xform, d_cam = (torch.from_numpy(v).cuda() for v in (frames, masks, xform, cam))
        need = _capi.check(l.hep_augment_workspace_bytes(B, H, W, S, kmax))
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
        out = {"image": f32(B, 3, S, S), "mask": torch.empty((B, H, W), dtype=torch.uint8, device="cuda"), "camera": f32(B, 6),
               "gt_boxes": torch.empty((B, kmax, 4), dtype=torch.float64, device="cuda"), "gt_labels": i32(B, kmax), "gt_transform": f32(B, kmax, 8),
               "gt_num": i32(B), "applied": i32(B)}
        n = _capi.check(l.hep_anchors(S, None, None))
        an = np.empty((n, 4), np.float32); ta = np.empty((n, 3), np.float32)
        _capi.check(l.hep_anchors(S, an.ctypes.data, ta.ctypes.data))
        anchors = torch.from_numpy(an).cuda()
        hw = torch.tensor([[S, S]] * B, dtype=torch.int32, device="cuda")

        def aug():
            augment._run(l, d_frames, d_masks, d_xform, d_cam, ann, num_gt, B, H, W, S, kmax, 1000.0, out, ws, d_frames.device)

        def targets():
            return anchor_targets_device(anchors, out["gt_boxes"], out["gt_labels"], out["gt_transform"], None, out["gt_num"], hw, num_classes=8)

        def both():
            aug()
            targets()

        t_aug, t_tgt, t_both = timed(aug), timed(targets), timed(both)
        assert out["applied"].sum().item() == B, "every image of the timed batch is meant to be augmented"
        resize = max(H, W) != S
        nbytes = B * H * W * (3 + 1 + 1) + B * 3 * S * S * 4 + (2 * B * H * W * 3 if resize else 0)
        rows.append(dict(shape=name, launches=4 if resize else 3, augment_ms=t_aug, anchor_targets_ms=t_tgt, both_ms=t_both, bytes=nbytes,
                         augment_GBps=nbytes / (t_aug[0] * 1e-3) / 1e9, training_step_ms=step_ms, share_of_step=t_both[0] / step_ms, anchors=n))
    for r in rows:
        print(f"{r['shape']}: augment ({r['launches']} launches) {r['augment_ms'][0]:.3f} ms (min {r['augment_ms'][1]:.3f}, max {r['augment_ms'][2]:.3f}), "
              f"anchor_targets_device ({r['anchors']} anchors) {r['anchor_targets_ms'][0]:.3f} ms, both {r['both_ms'][0]:.3f} ms = {100 * r['share_of_step']:.1f} % of the "
              f"{r['training_step_ms']} ms training step; {r['bytes'] / 1e6:.1f} MB -> {r['augment_GBps']:.0f} GB/s effective")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


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
