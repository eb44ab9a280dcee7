#!/usr/bin/env python3
"""Time one whole training step: the loop of INTEGRATION.md section 1 with a stock optimiser (TrainableBackbone / TrainableNeck /
TrainableHeads, training.format_translation, training.losses, torch.optim.Adam with zero_grad(set_to_none=True)) against
``Trainer.step``, same weights, inputs and targets, batch-statistics BatchNorm in both.

Shapes: phi 0 @ 256 batch 16 and phi 3 @ 512 batch 8.  Every measurement is a child process of its own under its own time limit,
in the order parent, new, parent, new; in it one device-event pair per step, ``--warmup`` steps first, then ``--reps``; the median,
minimum and maximum in ms.  The rule of NOTEBOOK.md section 15: the new path's slower process may not be slower than the parent
loop's slower process by more than the parent's own spread (its two processes against each other).

Also: ``--launches`` counts the kernel launches of one step of either path (torch.profiler, one child each), ``--rate`` times
hep_optim_update_device alone and prints its effective rate at 29 bytes per element.

    python tools/train_step_time.py [--reps 30] [--warmup 5] [--launches] [--rate] [--json FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(0, 256, 16), (3, 512, 8)]
CHILD_LIMIT_S = 240
LR = 1e-4


def problem(phi, size, batch):
    """Seed-0 weights, a seeded image batch, one or two boxes per image -> training.anchor_targets, model points, cameras."""
    import numpy as np
    import torch
    from hmd_ego_pose_amd import _capi, seeded_state_dict, training
    from tests._util import CAMS, seeded_input
    sd = seeded_state_dict(phi, 0)
    x = torch.from_numpy(seeded_input((batch, 3, size, size), 31)).cuda()
    n = _capi.check(_capi.lib().hep_anchors(size, None, None))
    anchors = np.empty((n, 4), np.float32); t_anchors = np.empty((n, 3), np.float32)
    _capi.check(_capi.lib().hep_anchors(size, anchors.ctypes.data, t_anchors.ctypes.data))
    rng = np.random.Generator(np.random.PCG64(8))
    k = size / 256.0
    two = [np.array([[48., 48., 176., 176.]]) * k, np.array([[16., 16., 80., 80.], [112., 112., 240., 240.]]) * k]
    boxes = [two[i % 2] + (i // 2) * k for i in range(batch)]
    labels = [np.zeros((len(b),), np.int32) for b in boxes]
    tr = [np.concatenate([rng.uniform(-1, 1, (len(b), 3)), rng.standard_normal((len(b), 3)) * 100 + [0, 0, 600], np.zeros((len(b), 2))], 1).astype(np.float32) for b in boxes]
    co = [rng.standard_normal((len(b), 63)).astype(np.float32) * 50 for b in boxes]
    lab, reg_t, tra_t, crd_t = training.anchor_targets(torch.from_numpy(anchors).cuda(), boxes, labels, tr, co, [(size, size)] * batch, 1)
    pts = torch.from_numpy((rng.standard_normal((1, 300, 3)) * 30).astype(np.float32)).cuda()
    cam = torch.from_numpy(np.stack([CAMS[i % 2] for i in range(batch)])).cuda()
    return sd, dict(image=x, camera=cam, lab=lab, reg_t=reg_t, tra_t=tra_t, crd_t=crd_t, pts=pts, size=size)


def make_step(path, phi, sd, pr):
    """A callable that runs one training step of ``path`` ("parent" or "new") and returns the weighted total (device tensor)."""
    import torch
    from hmd_ego_pose_amd import Trainer, TrainableBackbone, TrainableHeads, TrainableNeck, training
    if path == "new":
        tr = Trainer(sd, phi, 1, "cuda", optimizer="adam", lr=LR, batch_norm="batch")
        return lambda: tr.step(pr["image"], pr["camera"], pr["lab"], pr["reg_t"], pr["tra_t"], pr["crd_t"], pr["pts"])[5]
    mods = [TrainableBackbone(phi, batch_norm="batch"), TrainableNeck(phi, batch_norm="batch"), TrainableHeads(phi, 1, batch_norm="batch")]
    for m in mods:
        m.load_state_dict(sd, strict=False)
        m.cuda().train()
    bb, neck, heads = mods
    opt = torch.optim.Adam([p for m in mods for p in m.parameters()], lr=LR)
    weights = torch.tensor([1.0, 1.0, 100.0, 0.1, 1.0], device="cuda")

    def step():
        opt.zero_grad(set_to_none=True)
        reg, cls, rot, raw, hand = heads(neck(bb(pr["image"])))
        trn = training.format_translation(raw, pr["camera"], pr["size"])
        out, _per = training.losses(pr["lab"], cls, pr["reg_t"], reg, pr["tra_t"], torch.cat((rot, trn), 2), pr["crd_t"], hand, pr["pts"], 3)
        total = (out * weights).sum()
        total.backward()
        opt.step()
        return total.detach()
    return step


def child_time(path, phi, size, batch, reps, warmup):
    import torch
    sd, pr = problem(phi, size, batch)
    step = make_step(path, phi, sd, pr)
    for _ in range(warmup):
        last = step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        last = step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(path=path, phi=phi, size=size, batch=batch, median=statistics.median(ms), min=min(ms), max=max(ms), last_total=float(last),
                allocated_mib=torch.cuda.max_memory_allocated() / 2 ** 20)


def child_launches(path, phi, size, batch):
    import torch
    from torch.profiler import ProfilerActivity, profile
    sd, pr = problem(phi, size, batch)
    step = make_step(path, phi, sd, pr)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    copies = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and ("memcpy" in e.name.lower() or "memset" in e.name.lower())]
    return dict(path=path, phi=phi, size=size, batch=batch, kernel_launches=len(kernels), copies=len(copies))


def child_rate(n, reps):
    """hep_optim_update_device alone on n trainable elements (Adam): median ms and the effective rate at 29 bytes per element."""
    import torch
    from hmd_ego_pose_amd import _capi
    l = _capi.lib()
    p, g, m, v = (torch.randn(n, device="cuda") for _ in range(4))
    v.abs_()
    kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
    state = torch.zeros(32, dtype=torch.uint8, device="cuda")
    ws = torch.empty(_capi.check(l.hep_optim_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    norm = lambda: _capi.check(l.hep_optim_grad_norm_device(g.data_ptr(), kind.data_ptr(), n, 0, 0.9, 0.999, 0.0, state.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    upd = lambda: _capi.check(l.hep_optim_update_device(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, kind.data_ptr(), n, 0, 1e-4, 0.9, 0.999,
                                                        1e-8, state.data_ptr(), stream))
    out = {}
    for name, fn, nbytes in (("update", upd, 29 * n), ("norm", norm, 5 * n)):
        norm()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ms.append(a.elapsed_time(b))
        med = statistics.median(ms)
        out[name] = dict(median_ms=med, min_ms=min(ms), gb_per_s=nbytes / med / 1e6)
    return dict(n=n, **out)


def run_child(args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"child {args} ran into its limit of {CHILD_LIMIT_S} s: nothing more is started")
    if r.returncode != 0:
        raise SystemExit(f"child {args} ended with {r.returncode}: nothing more is started\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--rate", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, rest = args.child[0], args.child[1:]
        if kind == "time":
            res = child_time(rest[0], int(rest[1]), int(rest[2]), int(rest[3]), int(rest[4]), int(rest[5]))
        elif kind == "launches":
            res = child_launches(rest[0], int(rest[1]), int(rest[2]), int(rest[3]))
        else:
            res = child_rate(int(rest[0]), int(rest[1]))
        print(json.dumps(res))
        return
    out = dict(shapes=[], launches=[], rate=[])
    for phi, size, batch in SHAPES:
        runs = [run_child(["time", path, phi, size, batch, args.reps, args.warmup]) for path in ("parent", "new", "parent", "new")]
        for r in runs:
            print(f"phi {phi} @ {size} batch {batch} {r['path']:6s}: median {r['median']:.3f} ms (min {r['min']:.3f}, max {r['max']:.3f}), "
                  f"total after the last step {r['last_total']:.6g}, peak {r['allocated_mib']:.0f} MiB")
        parent, new = [r["median"] for r in runs if r["path"] == "parent"], [r["median"] for r in runs if r["path"] == "new"]
        spread = abs(parent[0] - parent[1])
        ok = max(new) <= max(parent) + spread
        print(f"  parent spread {spread:.3f} ms; slower new {max(new):.3f} against slower parent {max(parent):.3f}: {'within the rule' if ok else 'SLOWER'}; "
              f"medians' ratio {statistics.mean(parent) / statistics.mean(new):.3f} x")
        out["shapes"].append(dict(phi=phi, size=size, batch=batch, runs=runs, parent_spread=spread, within_rule=ok))
        if args.launches:
            for path in ("parent", "new"):
                r = run_child(["launches", path, phi, size, batch])
                print(f"  {path}: {r['kernel_launches']} kernel launches and {r['copies']} copies / fills per step")
                out["launches"].append(r)
    if args.rate:
        for n in (4_000_000, 12_000_000, 64_000_000):
            r = run_child(["rate", n, 50])
            print(f"update kernel alone, n = {n}: {r['update']['median_ms'] * 1e3:.1f} us, {r['update']['gb_per_s']:.0f} GB/s at 29 B per element; "
                  f"norm {r['norm']['median_ms'] * 1e3:.1f} us, {r['norm']['gb_per_s']:.0f} GB/s at 5 B")
            out["rate"].append(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
