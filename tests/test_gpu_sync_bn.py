"""GPU (MI355X): synchronised BatchNorm - ``batch_norm="sync"`` of TrainableHeads / TrainableNeck / TrainableBackbone and of
``Trainer`` over hep_{heads,neck,backbone}_*_device_sync (csrc/grad_dev.h: the exchange block and the passes around it).

One process.  With no group the hook is the identity and "sync" must be "batch" BIT FOR BIT: outputs, updated running
statistics, every parameter gradient, the input gradients; then the ``Trainer`` step (losses, flat gradient, statistics,
parameters).  A hook that fails ends the call with a negative code that names the hook, and nothing reaches ``stats_out``.

Two ranks.  tests/sync_rank.py runs once per rank in a fresh child process (both on ONE device over gloo: RCCL refuses two ranks
on one device; on two devices over RCCL where the box has them) and leaves its arrays in an .npz.  The parts are compared with
tests/_bn_batch.py's patched float64 oracle of the FULL case - concatenated outputs and input gradients, the rank-SUM of the
parameter gradients, the running statistics - under the bounds of tests/test_gpu_bn_batch.py (4 x the float32 one-thread CPU
oracle, floor 2e-6; the zero set the same way); the neck's oracle is routed by the ranks' concatenated argmax.  heads and neck
split 5 + 3 (uneven on purpose: the row counts travel in the exchange block; ``dist.shard_range`` would give 4 + 4), the backbone
1 + 1, N2_CASE 1 + 1 (one local row at P7, which batch mode refuses).  The ``Trainer`` (phi 0 @ 128, global batch 4 split 3 + 1)
is compared with a single-process ``Trainer(batch_norm="batch")`` on the four images under the composed-oracle bound computed as
tests/test_gpu_bn_batch.py::test_one_composed_training_step_matches_the_composed_oracle computes its own.

The tests print what they reach (device | float32 torch on the CPU | bound); NOTEBOOK.md section 30 records the values.  Measured
on MI355X over gloo (two ranks | CPU float32 | bound): heads outputs 6.0e-7 | 6.7e-7 | 2.7e-6, gradients 1.95e-6 | 2.01e-6 | 8.0e-6; neck
2.5e-6 | 3.0e-6 | 1.2e-5 and 5.55e-6 | 3.29e-6 | 1.3e-5; backbone 6.1e-6 | 5.8e-6 | 2.3e-5 and 1.65e-5 | 1.53e-5 | 6.1e-5; trainer bound
1.17e-4, rank-summed gradients within 1.6e-6, parameters within 1.2e-7 of the single process (allowed 3.7e-7 in the neck).  The RCCL pair
skipped: the box has one GPU.
"""
import ctypes
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _backbone_grad as G
from tests import _bn_batch as BB
from tests import _head_grad as H
from tests import _neck_grad as N
from tests import sync_rank as SR
from tests import test_gpu_bn_batch as TB
from tests import test_gpu_trainer as TT
from tests._util import seeded_state_dict_once as seeded_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = [("heads", "phi0_s128_b8"), ("neck", "phi0_s128_b8"), ("backbone", "phi0_s128_b2")]
CHILD_TIMEOUT_S = 600


# ---- one process: the identity hook ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sync_run(part, tag):
    case = BB.CASES[part][tag]
    m = TB._module(part, case, "sync").train()
    res = TB._run(part, m, case)
    return m, res, TB._buffers(m)


@pytest.mark.parametrize("part,tag", IDENTITY, ids=[p for p, _ in IDENTITY])
def test_sync_without_a_group_is_batch_mode_bit_for_bit(part, tag):
    batch = TB._case(part, tag)                                  # the batch-mode module's forward and backward, cached across the files
    m, res, after = _sync_run(part, tag)
    assert m.batch_norm == "sync" and m._hook.world == 1 and m._hook.calls > 0 and m._hook.error is None
    print(f"{part} {tag}: {m._hook.calls} hook calls in one forward and backward")
    assert all(torch.equal(a, b) for a, b in zip(res["outs"], batch["dev"]["outs"]))
    assert all(torch.equal(a, b) for a, b in zip(res["gin"], batch["dev"]["gin"]))
    assert set(res["grads"]) == set(batch["dev"]["grads"])
    assert all(torch.equal(res["grads"][k], v) for k, v in batch["dev"]["grads"].items()), [k for k, v in batch["dev"]["grads"].items() if not torch.equal(res["grads"][k], v)][:5]
    assert set(after) == set(batch["after"]) and all(torch.equal(after[k], v) for k, v in batch["after"].items())
    assert any(not torch.equal(after[k], batch["before"][k]) for k in after if k.endswith("running_var"))


@pytest.mark.parametrize("part,tag", IDENTITY, ids=[p for p, _ in IDENTITY])
def test_two_identical_sync_runs_are_bit_equal_and_eval_is_the_running_function(part, tag):
    case = BB.CASES[part][tag]
    _m, first, _after = _sync_run(part, tag)
    again = TB._run(part, TB._module(part, case, "sync").train(), case)
    assert all(torch.equal(a, b) for a, b in zip(again["outs"], first["outs"]))
    assert all(torch.equal(a, b) for a, b in zip(again["gin"], first["gin"]))
    assert all(torch.equal(again["grads"][k], v) for k, v in first["grads"].items())
    ev = TB._module(part, case, "sync").eval()
    b0 = TB._buffers(ev)
    got, want = TB._run(part, ev, case), TB._run(part, TB._module(part, case, None).eval(), case)
    assert ev._hook.calls == 0 and all(torch.equal(v, b0[k]) for k, v in TB._buffers(ev).items())
    assert all(torch.equal(a, b) for a, b in zip(got["outs"], want["outs"])) and all(torch.equal(got["grads"][k], v) for k, v in want["grads"].items())


def test_one_local_row_is_accepted_by_the_abi_and_refused_by_a_lone_module():
    """phi 0 @ 128 batch 1: P7 has one row.  A module with no group knows that the global count is 1 and refuses as batch mode
    does; the ABI accepts the replica (tests/test_sync_bn_cpu.py) - its two-rank run is the N2 case below."""
    for part in ("heads", "neck"):
        one = BB.N1_CASE if part == "heads" else BB.N1_CASE[:3] + (4, None, None)
        m = TB._module(part, one, "sync").train()
        with pytest.raises(ValueError):
            TB._run(part, m, one, backward=False)


def _abi_sync(part, case, hook_ref, stats):
    """Forward, then (with a backward hook) backward through the sync entry points on fresh buffers; returns (rc forward, rc
    backward, errors).  The backward only ever follows a forward that succeeded."""
    from hmd_ego_pose_amd import _capi
    l = _capi.lib()
    phi, size, batch, _seed, classes, _drop = case
    flat = TB._module(part, case).flat_parameters().detach()
    x_np, cots_np = BB.inputs(part, case)
    xs = [torch.from_numpy(a).cuda() for a in x_np]
    cots = [torch.from_numpy(a).cuda() for a in cots_np]
    outs = [torch.zeros_like(c) for c in cots]
    g_flat, g_in = torch.zeros_like(flat), [torch.zeros_like(a) for a in xs]
    cfg = (phi, classes, size, batch) if part == "heads" else (phi, size, batch)
    nbytes = _capi.check(getattr(l, f"hep_{part}_workspace_bytes_sync")(*cfg))
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    P = _capi.ptr_array
    fwd_ref, bwd_ref = hook_ref
    if bwd_ref is None:
        fwd_only = {"heads": lambda: l.hep_heads_forward_device_sync(flat.data_ptr(), P(xs), phi, classes, size, batch, P(outs), ws.data_ptr(), nbytes, BB.MOMENTUM,
                                                                     stats.data_ptr(), fwd_ref, stream),
                    "neck": lambda: l.hep_neck_forward_device_sync(flat.data_ptr(), P(xs), phi, size, batch, P(outs), ws.data_ptr(), nbytes, BB.MOMENTUM,
                                                                   stats.data_ptr(), fwd_ref, stream),
                    "backbone": lambda: l.hep_backbone_forward_device_sync(flat.data_ptr(), xs[0].data_ptr(), None, phi, size, batch, P(outs), ws.data_ptr(), nbytes,
                                                                           BB.MOMENTUM, stats.data_ptr(), fwd_ref, stream)}
        rc1 = fwd_only[part]()
        e1 = l.hep_last_error()
        torch.cuda.synchronize()
        return rc1, None, e1, None
    if part == "heads":
        rc1 = l.hep_heads_forward_device_sync(flat.data_ptr(), P(xs), phi, classes, size, batch, P(outs), ws.data_ptr(), nbytes, BB.MOMENTUM, stats.data_ptr(), fwd_ref, stream)
        e1 = l.hep_last_error()
        assert rc1 == 0, e1
        rc2 = l.hep_heads_backward_device_sync(flat.data_ptr(), P(cots), phi, classes, size, batch, g_flat.data_ptr(), P(g_in), ws.data_ptr(), nbytes, bwd_ref, stream)
    elif part == "neck":
        rc1 = l.hep_neck_forward_device_sync(flat.data_ptr(), P(xs), phi, size, batch, P(outs), ws.data_ptr(), nbytes, BB.MOMENTUM, stats.data_ptr(), fwd_ref, stream)
        e1 = l.hep_last_error()
        assert rc1 == 0, e1
        rc2 = l.hep_neck_backward_device_sync(flat.data_ptr(), P(cots), phi, size, batch, g_flat.data_ptr(), P(g_in), ws.data_ptr(), nbytes, bwd_ref, stream)
    else:
        rc1 = l.hep_backbone_forward_device_sync(flat.data_ptr(), xs[0].data_ptr(), None, phi, size, batch, P(outs), ws.data_ptr(), nbytes, BB.MOMENTUM, stats.data_ptr(), fwd_ref, stream)
        e1 = l.hep_last_error()
        assert rc1 == 0, e1
        rc2 = l.hep_backbone_backward_device_sync(flat.data_ptr(), P(cots), None, phi, size, batch, g_flat.data_ptr(), g_in[0].data_ptr(), ws.data_ptr(), nbytes, bwd_ref, stream)
    e2 = l.hep_last_error()
    torch.cuda.synchronize()
    return rc1, rc2, e1, e2


@pytest.mark.parametrize("part,tag", IDENTITY, ids=[p for p, _ in IDENTITY])
def test_a_failing_hook_ends_the_call_with_a_negative_code_and_writes_no_statistics(part, tag):
    from hmd_ego_pose_amd import sync
    case = BB.CASES[part][tag]
    n = TB._module(part, case).flat_parameters().numel()
    calls = {"good": 0, "bad": 0}

    def good(ctx, data, count, is_double, stream):
        calls["good"] += 1
        return 0

    def bad(ctx, data, count, is_double, stream):
        calls["bad"] += 1
        return 1

    cb_good, cb_bad = sync.SUM_FN(good), sync.SUM_FN(bad)
    s_good, s_bad = sync.HepSync(cb_good, None), sync.HepSync(cb_bad, None)
    # forward fails at its first exchange: nothing in stats_out
    stats = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    rc1, _rc2, e1, _e2 = _abi_sync(part, case, (ctypes.byref(s_bad), None), stats)
    assert rc1 < 0 and b"hook" in e1, (rc1, e1)
    assert bool(torch.isnan(stats).all())
    assert calls["bad"] == 1                                     # one call, nothing further was launched
    # a good forward, then the backward fails at its first exchange
    stats = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    calls["bad"] = 0
    rc1, rc2, e1, e2 = _abi_sync(part, case, (ctypes.byref(s_good), ctypes.byref(s_bad)), stats)
    assert rc1 == 0, e1
    assert rc2 < 0 and b"hook" in e2, (rc2, e2)
    assert calls["bad"] == 1 and calls["good"] > 0 and not bool(torch.isnan(stats).all())
    print(f"{part} {tag}: {calls['good']} hook calls in a forward; failing hook: rc {rc2}, {e2.decode()!r}")


def test_trainer_sync_without_a_group_is_the_batch_trainer_bit_for_bit():
    from hmd_ego_pose_amd import sync
    pr = TT._problem(batch=2)
    sd = seeded_state_dict(TT.PHI, 0)
    res = {}
    for mode in ("batch", "sync"):
        tr = TT._trainer(sd, optimizer="adam", lr=TT.LR, batch_norm=mode, **({"process_group": sync.LOCAL} if mode == "sync" else {}))
        losses = TT._step(tr, pr).clone()
        torch.cuda.synchronize()
        res[mode] = (losses, tr.grad.clone(), tr.stats.clone(), tr.params.clone(), tr.steps_taken, tr.steps_skipped)
        if mode == "sync":
            print(f"trainer phi 0 @ 128 batch 2: {tr._hook.calls} hook calls per step")
            assert tr._hook.calls > 0 and tr.world == 1
    for a, b, name in zip(res["sync"][:4], res["batch"][:4], ("losses", "grad", "stats", "params")):
        assert torch.equal(a, b), name
    assert res["sync"][4:] == res["batch"][4:] == (1, 0)
    one = TT._problem(batch=1)
    with pytest.raises(ValueError):                              # one image at 128: P7 has one global row
        TT._step(TT._trainer(sd, batch_norm="sync", process_group=sync.LOCAL), one)


# ---- two ranks ---------------------------------------------------------------------------------------------------------------------------
def _run_pair(backend, out_dir):
    """Two fresh child processes, one per rank, each under a timeout; if one exits non-zero the other is killed."""
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "sync_rank.py"), backend, str(out_dir)], env=env,
                                      stdout=open(os.path.join(out_dir, f"rank{rank}.out"), "w"),
                                      stderr=open(os.path.join(out_dir, f"rank{rank}.err"), "w")))
    import time
    deadline = time.monotonic() + CHILD_TIMEOUT_S
    failed = None
    while any(p.poll() is None for p in procs):
        if any(p.poll() not in (None, 0) for p in procs):
            failed = "a rank exited non-zero"
        elif time.monotonic() > deadline:
            failed = f"no result after {CHILD_TIMEOUT_S} s"
        if failed:
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        try:
            next(p for p in procs if p.poll() is None).wait(timeout=1.0)
        except subprocess.TimeoutExpired:
            pass
    for p in procs:
        p.wait()
    codes = [p.returncode for p in procs]
    tails = [open(os.path.join(out_dir, f"rank{r}.err")).read()[-1500:] for r in range(2)]
    assert failed is None and codes == [0, 0], (failed, codes, tails)
    return [dict(np.load(os.path.join(out_dir, f"rank{r}.npz"))) for r in range(2)]


@pytest.fixture(scope="module")
def gloo_pair(tmp_path_factory):
    return _run_pair("gloo", tmp_path_factory.mktemp("sync_gloo"))


@pytest.fixture(scope="module")
def rccl_pair(tmp_path_factory):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    return _run_pair("nccl", tmp_path_factory.mktemp("sync_rccl"))


def _gathered(ranks, part, tag, case, backward=True):
    """The two ranks' arrays as one result in the layout of BB.oracle: outputs and input gradients concatenated, parameter
    gradients summed (float64), rank 0's statistics, the concatenated argmax."""
    pre = f"{part}.{tag}/"
    cat = lambda name: torch.from_numpy(np.concatenate([r[pre + name] for r in ranks], 0))
    nouts = sum(1 for k in ranks[0] if k.startswith(pre + "out"))
    res = dict(outs=[cat(f"out{i}") for i in range(nouts)])
    res["argmax"] = [cat(f"argmax{i}") for i in range(len(N.pool_names(case[0])))] if part == "neck" else None
    if backward:
        nin = sum(1 for k in ranks[0] if k.startswith(pre + "gin"))
        res["gin"] = [cat(f"gin{i}") for i in range(nin)]
        keys = [k[len(pre + "grad/"):] for k in ranks[0] if k.startswith(pre + "grad/")]
        res["grads"] = {k: torch.from_numpy(sum(r[pre + "grad/" + k].astype(np.float64) for r in ranks)) for k in keys}
    res["stats"] = [{k[len(pre + "stat/"):]: torch.from_numpy(r[k]) for k in r if k.startswith(pre + "stat/")} for r in ranks]
    return res


def _check_parts(ranks, label):
    bad = {}
    for part, tag, split in SR.PART_CASES:
        case = BB.CASES[part][tag]
        sd = seeded_state_dict(case[0], case[3], num_classes=case[4] or 1)
        got = _gathered(ranks, part, tag, case)
        assert sum(r[f"{part}.{tag}/out0"].shape[0] for r in ranks) == case[2]
        if split is not None:
            assert tuple(r[f"{part}.{tag}/out0"].shape[0] for r in ranks) == split
        r64 = BB.oracle(part, sd, case, torch.float64, got["argmax"])
        r32 = BB.one_thread(BB.oracle, part, sd, case, torch.float32, got["argmax"])
        zeros = BB.zero_set(r64["grads"])
        assert set(got["grads"]) == set(r64["grads"])
        e32, e = BB.group_errors(r32, r64, zeros), BB.group_errors(got, r64, zeros)
        for grp in ("outputs", "gradients", "fusion"):
            if grp not in e:
                continue
            bound = BB.bound(e32[grp])
            print(f"{label} {part} {tag} {grp}: two ranks {e[grp]:.3e} | float32 torch on the CPU {e32[grp]:.3e} | bound {bound:.3e}"
                  + (f" (worst: {e['worst_gradient']})" if grp == "gradients" else ""))
            if not e[grp] <= bound:
                bad[(part, grp)] = (e[grp], bound)
        zbound = BB.BOUND_FACTOR * e32["zeros"]
        print(f"{label} {part} {tag} zeros: {len(zeros)} tensors, rank-sum max |g| {e['zeros']:.3e} | float32 torch on the CPU {e32['zeros']:.3e} | bound {zbound:.3e}")
        if not e["zeros"] <= zbound:
            bad[(part, "zeros")] = (e["zeros"], zbound)
        # the parameter gradients are LOCAL contributions: one rank's alone is not the gradient (d gamma of the first BatchNorm found)
        k = next(k for k in r64["grads"] if k.endswith(".weight") and BB.is_bn_bias(k[:-6] + "bias"))
        assert H.rel_err(ranks[0][f"{part}.{tag}/grad/{k}"].astype(np.float64), r64["grads"][k].numpy()) > 1e-3, k
        s0, s1 = got["stats"]
        assert set(s0) == set(r64["stats"]) and all(torch.equal(s0[k], s1[k]) for k in s0), "the running statistics differ between the ranks"
        s32, se = BB.stat_errors(r32["stats"], r64["stats"]), BB.stat_errors(s0, r64["stats"])
        for kind, v in se.items():
            sbound = BB.BOUND_FACTOR * s32[kind]
            print(f"{label} {part} {tag} {kind}: two ranks {v:.3e} | float32 torch on the CPU {s32[kind]:.3e} | bound {sbound:.3e}")
            if not v <= sbound:
                bad[(part, kind)] = (v, sbound)
        print(f"{label} {part} {tag}: {int(ranks[0][f'{part}.{tag}/hook_calls'])} hook calls per rank in one forward and backward")
    assert not bad, bad


def _check_n2(ranks, label):
    for part in ("heads", "neck"):
        case = BB.N2_CASE if part == "heads" else SR.neck_case(BB.N2_CASE)
        sd = seeded_state_dict(case[0], case[3], num_classes=case[4] or 1)
        got = _gathered(ranks, part, "n2", case, backward=False)
        assert [r[f"{part}.n2/out0"].shape[0] for r in ranks] == [1, 1]
        r64 = BB.oracle(part, sd, case, torch.float64, got["argmax"])
        r32 = BB.one_thread(BB.oracle, part, sd, case, torch.float32, got["argmax"])
        assert all(bool(torch.isfinite(o).all()) for o in got["outs"])
        e = max(H.rel_err(a.numpy(), b.numpy()) for a, b in zip(got["outs"], r64["outs"]))
        e32 = max(H.rel_err(a.numpy(), b.numpy()) for a, b in zip(r32["outs"], r64["outs"]))
        print(f"{label} {part} phi0_s128_b2 split 1 + 1 (one local, two global rows at P7) outputs: two ranks {e:.3e} | float32 torch on the CPU {e32:.3e} | "
              f"bound {BB.bound(e32):.3e}")
        assert e <= BB.bound(e32), (part, e, BB.bound(e32))
        s0, s1 = got["stats"]
        assert all(torch.equal(s0[k], s1[k]) and bool(torch.isfinite(s0[k]).all()) for k in s0)


@functools.lru_cache(maxsize=None)
def _trainer_reference():
    """The single-process ``Trainer(batch_norm="batch")`` on the four images, one step; and the composed-oracle gradient bound of
    this model and batch, computed as tests/test_gpu_bn_batch.py's composed-step case computes its own: the composed float32 CPU
    oracle (one thread) against the float64 one, max-pools routed as the device routed them, x 4, floor 2e-6."""
    from hmd_ego_pose_amd import neck as NK
    phi, size, batch = TT.PHI, TT.SIZE, SR.TRAINER_BATCH
    sd = seeded_state_dict(phi, 0)
    pr = TT._problem(batch=batch)
    tr = TT._trainer(sd, optimizer="sgd", lr=SR.TRAINER_LR, batch_norm="batch")
    losses = TT._step(tr, pr).clone()
    torch.cuda.synchronize()
    ref = dict(losses=losses.cpu().numpy(), grad=tr.grad.cpu().numpy(), stats=tr.stats.cpu().numpy(), params=tr.params.cpu().numpy(),
               parts=dict(tr.parts), kind=tr.kind.cpu().numpy())
    mods = TT._modules(sd, "batch")
    maps = mods[1](mods[0](pr["image"]))
    views = NK.stage_views(maps[0].grad_fn.saved_tensors[1], phi, size, batch)
    argmax = [N.first_argmax(views[name].permute(0, 3, 1, 2)).cpu() for name in N.pool_names(phi)]
    picks = ("backbone_net.model._conv_stem.conv.weight", "bifpn.1.conv4_down.pointwise_conv.conv.weight", "regressor.header.pointwise_conv.conv.weight")
    cots = H.seeded_cotangents(1, size, batch, 2)
    image = pr["image"].cpu().numpy()

    def composed(dtype):
        t = lambda a: (torch.from_numpy(a) if isinstance(a, np.ndarray) else a.detach().cpu()).to(dtype)
        p = {k: t(v).clone() for k, v in sd.items() if v.dtype == torch.float32}
        for k in picks:
            p[k].requires_grad_(True)
        with BB.batch_statistics():
            taps = G.oracle_backbone(p, t(image), phi)
            o = H.oracle_heads(p, N.oracle_neck(p, taps, phi, N.RoutedPool(argmax)), phi, 1)
            sum((a * t(c)).sum() for a, c in zip(o, cots)).backward()
        return {k: p[k].grad for k in picks}

    g64 = composed(torch.float64)
    g32 = BB.one_thread(composed, torch.float32)
    e32 = max(H.rel_err(g32[k].numpy(), g64[k].numpy()) for k in picks)
    print(f"composed oracle (phi 0 @ 128 batch {batch}): float32 torch on the CPU, gradients {e32:.3e} -> bound {BB.bound(e32):.3e}")
    ref["bound"] = BB.bound(e32)
    return ref


def _check_trainer(ranks, label):
    ref = _trainer_reference()
    bound, lr = ref["bound"], SR.TRAINER_LR
    r0, r1 = ranks
    bad = []
    # step 1 against the single process
    for i, name in enumerate(("classification", "regression", "rotation", "translation", "hand", "total")):
        got, want = float(r0["trainer/step1/losses"][i]), float(ref["losses"][i])
        e = abs(got - want) / max(abs(want), 1e-30)
        print(f"{label} trainer step 1 loss {name}: two ranks {got:.8g} | one process {want:.8g} | rel {e:.3e} | bound {bound:.3e}")
        if not e <= bound:
            bad.append((name, e, bound))
    assert float(r0["trainer/step1/losses"][4]) > 0              # the hand loss is on
    trainable = ref["kind"] == 0
    for name, (o, n) in ref["parts"].items():
        sl = slice(o, o + n)
        g = ref["grad"][sl]
        eg = H.rel_err(r0["trainer/step1/grad"][sl].astype(np.float64), g.astype(np.float64))
        es = H.rel_err(r0["trainer/step1/stats"][sl].astype(np.float64), ref["stats"][sl].astype(np.float64))
        k = trainable[sl]
        dp = float(np.abs(r0["trainer/step1/params"][sl][k].astype(np.float64) - ref["params"][sl][k].astype(np.float64)).max())
        allowed = lr * bound * float(np.abs(g).max())
        print(f"{label} trainer step 1 {name}: rank-summed gradient rel {eg:.3e} | statistics rel {es:.3e} | bound {bound:.3e}; "
              f"max |p - p_one| {dp:.3e} | allowed lr x bound x max |g| = {allowed:.3e} (max |g| {float(np.abs(g).max()):.3e})")
        if not eg <= bound:
            bad.append((name, "gradient", eg, bound))
        if not es <= bound:
            bad.append((name, "statistics", es, bound))
        if not dp <= allowed:
            bad.append((name, "parameters", dp, allowed))
    # every rank holds the same bits, after step 1 and after step 2
    for s in (1, 2):
        for what in ("losses", "params", "m", "state"):
            assert np.array_equal(r0[f"trainer/step{s}/{what}"], r1[f"trainer/step{s}/{what}"], equal_nan=False), (s, what)
        assert np.isfinite(r0[f"trainer/step{s}/losses"]).all()
    assert np.array_equal(r0["trainer/step1/grad"], r1["trainer/step1/grad"]) and np.array_equal(r0["trainer/step1/stats"], r1["trainer/step1/stats"])
    assert r0["trainer/step2/counts"].tolist() == r1["trainer/step2/counts"].tolist() == [2, 0]
    assert not np.array_equal(r0["trainer/step2/params"], r0["trainer/step1/params"])
    # a NaN in rank 1's image: both ranks skip, both parameter buffers stay
    for r in ranks:
        assert r["trainer/nan/counts"].tolist() == [2, 1]
        assert np.array_equal(r["trainer/nan/params"], r["trainer/step2/params"])
    print(f"{label} trainer: {int(r0['trainer/hook_calls_per_step'])} hook calls per step and rank")
    assert not bad, bad


def test_two_ranks_on_one_device_the_parts_equal_the_oracle_of_the_full_batch(gloo_pair):
    _check_parts(gloo_pair, "gloo")


def test_two_ranks_on_one_device_one_local_row_at_p7_is_two_global_rows(gloo_pair):
    _check_n2(gloo_pair, "gloo")


def test_two_ranks_on_one_device_the_trainer_step_equals_the_single_process_step(gloo_pair):
    _check_trainer(gloo_pair, "gloo")


def test_two_ranks_over_rccl(rccl_pair):
    _check_parts(rccl_pair, "rccl")
    _check_n2(rccl_pair, "rccl")
    _check_trainer(rccl_pair, "rccl")
