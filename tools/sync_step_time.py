#!/usr/bin/env python3
"""Time ``Trainer.step`` with synchronised BatchNorm on one device: what the seam between the replicas costs before any second
replica exists.  phi 0 @ 256 batch 16 (tools/train_step_time.py's problem) in three configurations:

    batch       ``batch_norm="batch"``: the untouched path
    sync        ``batch_norm="sync"`` with no group (``sync.LOCAL``): the exchange block, the extra passes and the identity hook (a ctypes callback)
    sync-rccl   ``batch_norm="sync"`` with an RCCL group of world size 1 and ``SumHook.force``: every hook call is a real
                ``dist.all_reduce`` on a view of the workspace (in a group of one the hook would otherwise do nothing); the one
                collective over the flat gradient and the one over the losses stay skipped, as in every group of one

Every measurement is a child process of its own under its own time limit, the configurations alternating (batch, sync, sync-rccl,
twice); in it one device-event pair per step, ``--warmup`` steps first, then ``--reps``; the median, minimum and maximum in ms and
the hook calls per step.  Real multi-GPU step times need a box with more than one GPU; this tool does not measure them.

    python tools/sync_step_time.py [--reps 30] [--warmup 5] [--configs batch,sync,sync-rccl] [--json FILE]
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHI, SIZE, BATCH = 0, 256, 16
CONFIGS = ("batch", "sync", "sync-rccl")
CHILD_LIMIT_S = 240
LR = 1e-4


def child_time(config, reps, warmup):
    import torch
    from hmd_ego_pose_amd import Trainer, sync
    from tools.train_step_time import problem
    group = None if config == "batch" else sync.LOCAL
    if config == "sync-rccl":
        import datetime
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, timeout=datetime.timedelta(seconds=120))
        group = dist.group.WORLD
    sd, pr = problem(PHI, SIZE, BATCH)
    tr = Trainer(sd, PHI, 1, "cuda", optimizer="adam", lr=LR, batch_norm="batch" if config == "batch" else "sync", process_group=group)
    if config == "sync-rccl":
        tr._hook.force = True
    step = lambda: tr.step(pr["image"], pr["camera"], pr["lab"], pr["reg_t"], pr["tra_t"], pr["crd_t"], pr["pts"])[5]
    for _ in range(warmup):
        last = step()
    torch.cuda.synchronize()
    calls0 = tr._hook.calls if tr._hook is not None else 0
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        last = step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    calls = ((tr._hook.calls - calls0) // reps) if tr._hook is not None else 0
    res = dict(config=config, phi=PHI, size=SIZE, batch=BATCH, median=statistics.median(ms), min=min(ms), max=max(ms), last_total=float(last),
               hook_calls_per_step=calls, world=tr.world, allocated_mib=torch.cuda.max_memory_allocated() / 2 ** 20)
    if config == "sync-rccl":
        import torch.distributed as dist
        dist.destroy_process_group()
    return res


def run_child(config, reps, warmup):
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", config, str(reps), str(warmup)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S, cwd=ROOT, env=env)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"child {config} ran into its limit of {CHILD_LIMIT_S} s: nothing more is started")
    if r.returncode != 0:
        raise SystemExit(f"child {config} ended with {r.returncode}: nothing more is started\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child_time(args.child[0], int(args.child[1]), int(args.child[2]))))
        return
    configs = [c for c in args.configs.split(",") if c]
    if any(c not in CONFIGS for c in configs):
        raise SystemExit(f"--configs: a comma-separated subset of {CONFIGS}")
    runs = []
    for _ in range(2):
        for c in configs:
            r = run_child(c, args.reps, args.warmup)
            runs.append(r)
            print(f"phi {PHI} @ {SIZE} batch {BATCH} {c:9s}: median {r['median']:.3f} ms (min {r['min']:.3f}, max {r['max']:.3f}), {r['hook_calls_per_step']} hook calls "
                  f"per step, total after the last step {r['last_total']:.6g}, peak {r['allocated_mib']:.0f} MiB", flush=True)
    for c in configs:
        med = [r["median"] for r in runs if r["config"] == c]
        print(f"  {c:9s}: medians {', '.join(f'{m:.3f}' for m in med)} ms; slower process {max(med):.3f}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
