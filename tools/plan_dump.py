#!/usr/bin/env python3
"""Dump the launch plan and every result of the inference sessions that reach each planner branch to one .npz, and compare
two dumps byte for byte.

Under whichever library HEP_LIB selects, with seed-0 weights and a seeded input, for each session: the launch list of
Session.kernels (name, device function, bytes, flops), the five feature maps, the five head outputs, the decoded boxes and
translations and, with FLAG_KEEP_INTERMEDIATES, every stage tensor hep_debug_tensor_info names.  The sessions:
  phi 0 @ 256 batch 2, fp32 and bf16, with and without the keep flag
  phi 3 @ 512 batch 1, fp32 and bf16   width 160: cooperative towers, streamed chain weights, multi-pass fronts
  phi 0 @ 256 batch 3, HEP_LANES=2     uneven lanes
  phi 0 @ 256 batch 2 under each plan knob of KNOBS (set before the session is created: knobs are read at hep_create)
Knobs already in the environment stay set for every session (the alternative library's kernels are selected that way).
A change that must not move a bit (a refactor of the planner, a new compiler) is checked by dumping once with the old
library and once with the new one, each in a process of its own:

    HEP_LIB=old/libhep.so python tools/plan_dump.py old.npz
    python tools/plan_dump.py new.npz --against old.npz        # exit status 1 and the list of arrays that differ
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmd_ego_pose_amd import _capi, seeded_state_dict  # noqa: E402
from hmd_ego_pose_amd.model import Session  # noqa: E402

KNOBS = [{"HEP_MBF_MP": "force"}, {"HEP_SE_MAXMB": "0"}, {"HEP_SE_MAXMB": "1000"}, {"HEP_XBF_GENERIC": "1"}, {"HEP_MBF_GENERIC": "1"}, {"HEP_STEM_MFMA": "1"},
         {"HEP_PW_FRAG": "0"}, {"HEP_SEP_WLDS": "0"}, {"HEP_CHAIN_STREAM": "1"}, {"HEP_CHAIN_STREAM": "2"}, {"HEP_TOWER_COOP": "0"},
         {"HEP_TOWER_COOP": "1"}]
KEEP = _capi.FLAG_KEEP_INTERMEDIATES
# (phi, size, batch, precision, flags, knobs)
SESSIONS = ([(0, 256, 2, prec, flags, {}) for prec in ("fp32", "bf16") for flags in (0, KEEP)] +
            [(3, 512, 1, prec, 0, {}) for prec in ("fp32", "bf16")] +
            [(0, 256, 3, prec, 0, {"HEP_LANES": "2"}) for prec in ("fp32", "bf16")] +
            [(0, 256, 2, prec, 0, k) for k in KNOBS for prec in ("fp32", "bf16")])


def stage_names(s):
    l, names = _capi.lib(), []
    for i in range(l.hep_debug_tensor_count(s.handle)):
        nm = ctypes.c_char_p(); dims = (ctypes.c_int64 * 4)()
        l.hep_debug_tensor_info(s.handle, i, ctypes.byref(nm), dims)
        names.append(nm.value.decode())
    return names


def dump_session(out, sd, phi, size, batch, prec, flags, knobs):
    tag = f"phi{phi}_s{size}_b{batch}_{prec}" + ("_keep" if flags else "") + "".join(f"_{k}={v}" for k, v in knobs.items())
    saved = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        s = Session(sd, phi, size, batch, prec, flags=flags)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    rng = np.random.Generator(np.random.PCG64(7 + phi))
    x = torch.from_numpy(rng.standard_normal((batch, 3, size, size)).astype(np.float32)).cuda()
    feats, reg, cls, rot, trn, hand = s.forward(x)
    cam = torch.tensor([[480, 480, 128, 128, 1000, 1.0]] * batch).cuda()
    boxes, trans = s.decode(reg, trn, cam)
    torch.cuda.synchronize()
    ks = s.kernels(batch)
    out[f"{tag}/launch.names"] = np.array([f"{n} | {sym}" for n, _, _, sym in ks])
    out[f"{tag}/launch.bytes_flops"] = np.array([[b, f] for _, b, f, _ in ks], dtype=np.float64)
    for l, f in enumerate(feats):
        out[f"{tag}/feat.{l}"] = f.cpu().numpy()
    for n, t in zip(("regression", "classification", "rotation", "translation_raw", "hand", "boxes", "translation"), (reg, cls, rot, trn, hand, boxes, trans)):
        out[f"{tag}/out.{n}"] = t.cpu().numpy()
    if flags & KEEP:
        for n in stage_names(s):
            out[f"{tag}/stage.{n}"] = s.stage(n, batch).numpy()
    s.close()
    return len(ks)


def compare(new, old):
    """Names of the arrays that differ byte for byte (or exist on one side only); launch lists entry by entry."""
    bad = [f"{n}: only in one dump" for n in sorted(set(new) ^ set(old.files))]
    for n in sorted(set(new) & set(old.files)):
        a, b = np.ascontiguousarray(new[n]), np.ascontiguousarray(old[n])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f"{n}: {a.dtype}{a.shape} against {b.dtype}{b.shape}")
        elif a.tobytes() != b.tobytes():
            if a.dtype.kind == "U":
                bad.append(f"{n}: " + "; ".join(f"launch {i}: {x} against {y}" for i, (x, y) in enumerate(zip(a, b)) if x != y))
            else:
                bad.append(f"{n}: {int((a.view(np.uint8) != b.view(np.uint8)).reshape(a.size, -1).any(axis=1).sum())} of {a.size} elements differ")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", help="the .npz to write")
    ap.add_argument("--against", default=None, help="an earlier dump: compare byte for byte, exit status 1 when an array differs")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    out, launches, sds = {}, 0, {}
    for phi, size, batch, prec, flags, knobs in SESSIONS:
        if phi not in sds:
            sds[phi] = seeded_state_dict(phi, 0)
        launches += dump_session(out, sds[phi], phi, size, batch, prec, flags, knobs)
    np.savez(args.out, **out)
    print(f"{args.out}: {len(SESSIONS)} sessions, {launches} launch-list entries, {len(out)} arrays, {sum(a.nbytes for a in out.values()) / 2 ** 20:.1f} MiB, "
          f"library {os.environ.get('HEP_LIB', 'default')} ({_capi.lib().hep_build_info().decode()})")
    if args.against:
        bad = compare(out, np.load(args.against))
        for line in bad:
            print("DIFFERS " + line)
        print(f"against {args.against}: {len(bad)} differing arrays of {len(out)}")
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
