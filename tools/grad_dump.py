#!/usr/bin/env python3
"""Dump every result of the three trainable parts' HIP forward and backward to one .npz, and compare two dumps byte for byte.

Under whichever library HEP_LIB selects, for the heads, the neck and the backbone: every forward output, every parameter
gradient (the flat gradient buffer split into its tensors) and every input gradient, on the seeded inputs of
tests/_head_grad.py, tests/_neck_grad.py and tests/_backbone_grad.py with seed-0 weights, at
  phi 0 @ 128 batch 2   one split-K slab in the heads, row counts that are no multiples of the 64-row tile
  phi 3 @ 128 batch 1   width 160: the column tiles are edge-masked
  phi 0 @ 256 batch 2   several split-K slabs in the heads and the neck
  heads also with num_classes 3; backbone also with the drop-connect table of tests/golden/backbone_grads.npz.
A change that must not move a bit (a refactor of the kernels, a new compiler) is checked by dumping once with the old
library and once with the new one, each in a process of its own:

    HEP_LIB=old/libhep.so python tools/grad_dump.py old.npz
    python tools/grad_dump.py new.npz --against old.npz        # exit status 1 and the list of arrays that differ
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmd_ego_pose_amd import seeded_state_dict  # noqa: E402
from hmd_ego_pose_amd import backbone as BB, heads as HD, neck as NK  # noqa: E402
from tests import _backbone_grad as GB, _head_grad as GH, _neck_grad as GN  # noqa: E402

SHAPES = [(0, 128, 2), (3, 128, 1), (0, 256, 2)]
GOLDEN_BACKBONE = os.path.join(ROOT, "tests", "golden", "backbone_grads.npz")


def _dev(arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


def _flat(module, sd):
    module.load_state_dict(sd, strict=False)
    return module.cuda().flat_parameters().detach()


def _put(out, tag, keys, outs, g_flat, g_in):
    """outs / g_in: name -> tensor; g_flat: the flat gradient buffer, split by ``keys`` [(key, shape)]."""
    for group in (outs, g_in):
        for n, t in group.items():
            out[f"{tag}/{n}"] = t.cpu().numpy()
    g, at = g_flat.cpu().numpy(), 0
    for k, shape in keys:
        n = int(np.prod(shape, dtype=np.int64))
        out[f"{tag}/param.{k}"] = g[at:at + n].reshape(shape)
        at += n
    assert at == g.size, (tag, at, g.size)


def dump_heads(out, phi, size, batch, classes):
    flat = _flat(HD.TrainableHeads(phi, classes), seeded_state_dict(phi, 0, num_classes=classes))
    feats, cots = _dev(GH.seeded_maps(phi, size, batch, 1)), _dev(GH.seeded_cotangents(classes, size, batch, 2))
    outs, ws = HD.heads_forward(flat, feats, phi, classes, size)
    g_flat, g_feats = HD.heads_backward(flat, cots, ws, phi, classes, size, [tuple(f.shape) for f in feats])
    _put(out, f"heads_phi{phi}_s{size}_b{batch}_k{classes}", HD.flat_keys(phi, classes), {f"out.{n}": o for n, o in zip(GH.OUT_NAMES, outs)},
         g_flat, {f"feat.{l}": g for l, g in enumerate(g_feats)})


def dump_neck(out, phi, size, batch):
    flat = _flat(NK.TrainableNeck(phi), seeded_state_dict(phi, 0))
    taps, cots = (_dev(a) for a in GN.seeded_inputs(phi, size, batch))
    feats, ws = NK.neck_forward(flat, taps, phi, size)
    g_flat, g_taps = NK.neck_backward(flat, cots, ws, phi, size, [tuple(t.shape) for t in taps])
    _put(out, f"neck_phi{phi}_s{size}_b{batch}", NK.flat_keys(phi), {f"map.{l}": f for l, f in enumerate(feats)}, g_flat,
         {f"tap.{t}": g for t, g in enumerate(g_taps)})


def dump_backbone(out, phi, size, batch, scales=None):
    flat = _flat(BB.TrainableBackbone(phi), seeded_state_dict(phi, 0))
    image, cots = GB.seeded_inputs(phi, size, batch)
    image, cots = torch.from_numpy(image).cuda(), _dev(cots)
    taps, ws = BB.backbone_forward(flat, image, phi, scales)
    g_flat, g_img = BB.backbone_backward(flat, cots, ws, phi, size, scales, want_image=True)
    _put(out, f"backbone_phi{phi}_s{size}_b{batch}" + ("" if scales is None else "_dropconnect"), BB.flat_keys(phi),
         {f"tap.{t}": f for t, f in enumerate(taps)}, g_flat, {"image": g_img})


def compare(new, old):
    """Names of the arrays that differ byte for byte (or exist on one side only), each with the count of differing elements
    and the largest distance in units of the last place."""
    bad = [f"{n}: only in one dump" for n in sorted(set(new) ^ set(old.files))]
    for n in sorted(set(new) & set(old.files)):
        a, b = np.ascontiguousarray(new[n]), np.ascontiguousarray(old[n])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f"{n}: {a.dtype}{a.shape} against {b.dtype}{b.shape}")
        elif a.tobytes() != b.tobytes():
            ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
            bad.append(f"{n}: {int((ia != ib).sum())} of {a.size} elements differ, up to {int(np.abs(ia - ib).max())} ulp")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", help="the .npz to write")
    ap.add_argument("--against", default=None, help="an earlier dump: compare byte for byte, exit status 1 when an array differs")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    out = {}
    for phi, size, batch in SHAPES:
        dump_heads(out, phi, size, batch, 1)
        dump_neck(out, phi, size, batch)
        dump_backbone(out, phi, size, batch)
    dump_heads(out, 0, 128, 2, 3)
    tag, (phi, size, batch, _seed) = GB.DROP_TAG, GB.DROP_CASE
    dump_backbone(out, phi, size, batch, torch.from_numpy(np.load(GOLDEN_BACKBONE)[f"{tag}/scales"]).float().cuda().contiguous())
    torch.cuda.synchronize()
    np.savez(args.out, **out)
    print(f"{args.out}: {len(out)} arrays, {sum(a.nbytes for a in out.values()) / 2 ** 20:.1f} MiB, library {os.environ.get('HEP_LIB', 'default')}")
    if args.against:
        bad = compare(out, np.load(args.against))
        for line in bad:
            print("DIFFERS " + line)
        print(f"against {args.against}: {len(bad)} differing arrays of {len(out)}")
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
