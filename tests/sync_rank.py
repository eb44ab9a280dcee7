"""One rank of the two-rank synchronised-BatchNorm run of tests/test_gpu_sync_bn.py (a fresh child process per rank, started by
that file's fixture; never collected by pytest).

    python tests/sync_rank.py BACKEND OUT_DIR        with RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT in the environment

BACKEND "gloo": both ranks on device 0 (RCCL refuses two ranks on one device; the hook stages through the host);
"nccl": rank r on device r.  The rank runs its shard of every case and leaves ``rank{r}.npz`` in OUT_DIR:

  parts     heads and neck at tests/_bn_batch.py's phi0_s128_b8 split 5 + 3, the backbone at phi0_s128_b2 split 1 + 1
            (``dist.shard_range``): outputs, input gradients, this rank's parameter gradients, the running statistics after
            the forward, the neck's max-pool argmax; heads and neck also N2_CASE split 1 + 1, forward only (ONE local row at P7)
  trainer   phi 0 @ 128, global batch 4 split 3 + 1, hand targets, SGD at lr 1.95e-6, ``batch_norm="sync"``: two steps, then
            a step with a NaN in rank 1's image
"""
import datetime
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _bn_batch as BB  # noqa: E402
from tests import _neck_grad as N  # noqa: E402
from tests._util import seeded_state_dict_once as seeded_state_dict  # noqa: E402

PART_CASES = [("heads", "phi0_s128_b8", (5, 3)), ("neck", "phi0_s128_b8", (5, 3)), ("backbone", "phi0_s128_b2", None)]
TRAINER_SPLIT, TRAINER_BATCH, TRAINER_LR = (3, 1), 4, float(np.float32(1e-3 / 512))
TIMEOUT_S = 120


def shard(total, rank, world, split):
    """[lo, hi) of this rank: an explicit split, or ``dist.shard_range``."""
    from hmd_ego_pose_amd.dist import shard_range
    if split is None:
        return shard_range(total, rank, world)
    assert sum(split) == total and len(split) == world
    return sum(split[:rank]), sum(split[:rank + 1])


def neck_case(case):
    return case[:3] + (4, None, None)


def module(part, case, group):
    from hmd_ego_pose_amd import TrainableHeads
    from hmd_ego_pose_amd.backbone import TrainableBackbone
    from hmd_ego_pose_amd.neck import TrainableNeck
    phi, _size, _batch, seed, classes, _drop = case
    kw = dict(batch_norm="sync", process_group=group)
    m = TrainableHeads(phi, classes, **kw) if part == "heads" else TrainableNeck(phi, **kw) if part == "neck" else TrainableBackbone(phi, **kw)
    m.load_state_dict(seeded_state_dict(phi, seed, num_classes=classes or 1), strict=False)
    return m.cuda().train()


def run_part(part, case, lo, hi, group, out, tag, backward=True):
    """This rank's rows [lo, hi) of the case through the module's autograd path."""
    from hmd_ego_pose_amd import neck as NK
    x_np, cots_np = BB.inputs(part, case)
    m = module(part, case, group)
    xs = [torch.from_numpy(a[lo:hi].copy()).cuda().requires_grad_(backward) for a in x_np]
    outs = m(xs[0]) if part == "backbone" else m(xs)
    if part == "neck":
        views = NK.stage_views(outs[0].grad_fn.saved_tensors[1], case[0], case[1], hi - lo)
        for i, name in enumerate(N.pool_names(case[0])):
            out[f"{tag}/argmax{i}"] = N.first_argmax(views[name].permute(0, 3, 1, 2)).cpu().numpy()
    for i, o in enumerate(outs):
        out[f"{tag}/out{i}"] = o.detach().cpu().numpy()
    if backward:
        sum((o * torch.from_numpy(c[lo:hi].copy()).cuda()).sum() for o, c in zip(outs, cots_np)).backward()
        for k, p in m.named_parameters():
            out[f"{tag}/grad/{k}"] = p.grad.detach().cpu().numpy()
        for i, a in enumerate(xs):
            out[f"{tag}/gin{i}"] = a.grad.cpu().numpy()
    torch.cuda.synchronize()
    for k, b in m.named_buffers():
        if k.endswith(("running_mean", "running_var")):
            out[f"{tag}/stat/{k}"] = b.detach().cpu().numpy()
    out[f"{tag}/hook_calls"] = np.int64(m._hook.calls)


def run_trainer(rank, world, group, out):
    from hmd_ego_pose_amd import Trainer
    from tests import test_gpu_trainer as TT
    pr = TT._problem(batch=TRAINER_BATCH)
    lo, hi = shard(TRAINER_BATCH, rank, world, TRAINER_SPLIT)
    tr = Trainer(seeded_state_dict(TT.PHI, 0), TT.PHI, 1, "cuda", optimizer="sgd", lr=TRAINER_LR, batch_norm="sync", process_group=group)
    args = lambda image: (image, pr["camera"][lo:hi].contiguous(), pr["lab"][lo:hi].contiguous(), pr["reg_t"][lo:hi].contiguous(),
                          pr["tra_t"][lo:hi].contiguous(), pr["crd_t"][lo:hi].contiguous(), pr["pts"])
    image = pr["image"][lo:hi].contiguous()
    for s in (1, 2):
        losses = tr.step(*args(image), global_batch=TRAINER_BATCH).clone()
        torch.cuda.synchronize()
        out[f"trainer/step{s}/losses"] = losses.cpu().numpy()
        out[f"trainer/step{s}/params"] = tr.params.cpu().numpy()
        out[f"trainer/step{s}/m"] = tr.m.cpu().numpy()
        out[f"trainer/step{s}/state"] = tr.state.cpu().numpy()
        out[f"trainer/step{s}/counts"] = np.array([tr.steps_taken, tr.steps_skipped], np.int64)
        if s == 1:
            out["trainer/step1/grad"] = tr.grad.cpu().numpy()
            out["trainer/step1/stats"] = tr.stats.cpu().numpy()
    out["trainer/hook_calls_per_step"] = np.int64(tr._hook.calls // 2)
    bad = image.clone()
    if rank == 1:
        bad[0, 1, 5, 7] = float("nan")
    tr.step(*args(bad), global_batch=TRAINER_BATCH)
    torch.cuda.synchronize()
    out["trainer/nan/params"] = tr.params.cpu().numpy()
    out["trainer/nan/counts"] = np.array([tr.steps_taken, tr.steps_skipped], np.int64)


def main():
    backend, out_dir = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(rank if backend == "nccl" else 0)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=TIMEOUT_S))
    group = dist.group.WORLD
    out = {}
    for part, tag, split in PART_CASES:
        case = BB.CASES[part][tag]
        lo, hi = shard(case[2], rank, world, split)
        run_part(part, case, lo, hi, group, out, f"{part}.{tag}")
    for part in ("heads", "neck"):
        case = BB.N2_CASE if part == "heads" else neck_case(BB.N2_CASE)
        lo, hi = shard(case[2], rank, world, None)
        assert hi - lo == 1
        run_part(part, case, lo, hi, group, out, f"{part}.n2", backward=False)      # (with a graph: the neck's argmax is read from its workspace)
    run_trainer(rank, world, group, out)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()
    print(f"rank {rank}: {len(out)} arrays")


if __name__ == "__main__":
    main()
