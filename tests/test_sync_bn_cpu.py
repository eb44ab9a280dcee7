"""CPU side of synchronised BatchNorm (``batch_norm="sync"``, hep_{heads,neck,backbone}_*_device_sync): the ABI surface and its
argument checks (all before any HIP call: no device here), the exchange arithmetic (tests/_sync_bn.py) against
``F.batch_norm(training=True)`` and its autograd on the concatenated batch in float64, the module and ``Trainer`` argument rules
and the sum hook's behaviour without a group.  The device side: tests/test_gpu_sync_bn.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hmd_ego_pose_amd import _capi, sync
from tests import _sync_bn as SB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4
PARTS = ("heads", "neck", "backbone")
NINE = [f"hep_{part}_{what}_sync" for part in PARTS for what in ("workspace_bytes", "forward_device", "backward_device")]


def _cfg(part, phi, size, batch):
    return (phi, 1, size, batch) if part == "heads" else (phi, size, batch)


def test_the_nine_symbols_are_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(REPO, "include", "hep.h")).read()
    declared = set(re.findall(r"\b(hep_[a-z_0-9]+)\s*\(", header))
    l = _capi.lib()
    for name in NINE:
        assert name in declared and name in _capi.SYMBOLS and hasattr(l, name), name
    assert "hep_sum_fn" not in declared and "hep_sync" not in declared      # the typedefs are no exports
    assert l.hep_abi_version() == 1


def test_the_sync_workspace_is_at_least_the_batch_mode_one_and_takes_one_local_row():
    l = _capi.lib()
    for phi, size, batch in [(0, 128, 2), (0, 256, 16), (3, 128, 8), (5, 256, 1)]:
        for part in PARTS:
            cfg = _cfg(part, phi, size, batch)
            bat, syn = getattr(l, f"hep_{part}_workspace_bytes_bn")(*cfg, 1), getattr(l, f"hep_{part}_workspace_bytes_sync")(*cfg)
            assert bat > 0 and syn >= bat and syn % 16 == 0, (part, cfg, bat, syn)
            print(f"{part} phi {phi} @ {size} b{batch}: workspace {bat} bytes (batch), {syn} (sync)")
    # phi 0, size 128, batch 1: one local row at P7 - batch mode refuses, a replica of a larger global batch must not
    assert l.hep_heads_workspace_bytes_bn(0, 1, 128, 1, 1) == UNSUPPORTED and l.hep_neck_workspace_bytes_bn(0, 128, 1, 1) == UNSUPPORTED
    for part in PARTS:
        assert getattr(l, f"hep_{part}_workspace_bytes_sync")(*_cfg(part, 0, 128, 1)) > 0, part
        assert getattr(l, f"hep_{part}_workspace_bytes_sync")(*_cfg(part, 0, 200, 2)) == UNSUPPORTED, part
        assert getattr(l, f"hep_{part}_workspace_bytes_sync")(*_cfg(part, 0, 128, 0)) < 0, part
    assert l.hep_neck_workspace_bytes_sync(6, 128, 2) == UNSUPPORTED


def test_the_argument_checks_come_before_any_hip_call():
    """On a machine without a device.  The hook given here must never be called."""
    l = _capi.lib()
    called = []
    cb = sync.SUM_FN(lambda ctx, data, count, is_double, stream: called.append(count) or 0)
    good, no_sum = sync.HepSync(cb, None), sync.HepSync(sync.SUM_FN(0), None)
    buf = np.zeros(64, np.float32)
    a = (buf.ctypes.data + 15) // 16 * 16                       # a non-NULL, 16-byte aligned host address: never dereferenced
    five, three = (ctypes.c_void_p * 5)(*([a] * 5)), (ctypes.c_void_p * 3)(*([a] * 3))
    big = 1 << 40
    calls = {
        "heads_fwd": lambda sy, size=128, batch=2, mom=0.01, ws=a, n=big: l.hep_heads_forward_device_sync(a, five, 0, 1, size, batch, five, ws, n, mom, None, sy, None),
        "heads_bwd": lambda sy, size=128, batch=2, mom=0.01, ws=a, n=big: l.hep_heads_backward_device_sync(a, five, 0, 1, size, batch, a, None, ws, n, sy, None),
        "neck_fwd": lambda sy, size=128, batch=2, mom=0.01, ws=a, n=big: l.hep_neck_forward_device_sync(a, three, 0, size, batch, five, ws, n, mom, None, sy, None),
        "neck_bwd": lambda sy, size=128, batch=2, mom=0.01, ws=a, n=big: l.hep_neck_backward_device_sync(a, five, 0, size, batch, a, None, ws, n, sy, None),
        "backbone_fwd": lambda sy, size=128, batch=2, mom=0.01, ws=a, n=big: l.hep_backbone_forward_device_sync(a, a, None, 0, size, batch, three, ws, n, mom, None, sy, None),
        "backbone_bwd": lambda sy, size=128, batch=2, mom=0.01, ws=a, n=big: l.hep_backbone_backward_device_sync(a, three, None, 0, size, batch, a, None, ws, n, sy, None),
    }
    ok = ctypes.byref(good)
    for name, f in calls.items():
        part = name.split("_")[0]
        assert f(None) == INVALID and b"sync" in l.hep_last_error(), name
        assert f(ctypes.byref(no_sum)) == INVALID and b"sync" in l.hep_last_error(), name
        assert f(ok, size=200) == UNSUPPORTED, name
        assert f(ok, batch=0) < 0, name
        if name.endswith("fwd"):
            assert f(ok, mom=1.5) == INVALID and b"momentum" in l.hep_last_error(), name
            assert f(ok, mom=-0.1) == INVALID and b"momentum" in l.hep_last_error(), name
            assert f(ok, mom=float("nan")) == INVALID and b"momentum" in l.hep_last_error(), name
        need = getattr(l, f"hep_{part}_workspace_bytes_sync")(*_cfg(part, 0, 128, 2))
        assert f(ok, n=need - 16) == INVALID and b"workspace" in l.hep_last_error(), name
        assert f(ok, ws=a + 4) == INVALID and b"aligned" in l.hep_last_error(), name
        assert f(ok, ws=None) == INVALID, name
        # a workspace of the batch-mode size is too small: the exchange block is sync's own
        assert f(ok, n=getattr(l, f"hep_{part}_workspace_bytes_bn")(*_cfg(part, 0, 128, 2), 1)) == INVALID and b"workspace" in l.hep_last_error(), name
    assert l.hep_neck_forward_device_sync(a, three, 6, 128, 2, five, a, big, 0.01, None, ok, None) == UNSUPPORTED
    assert l.hep_heads_forward_device_sync(a + 4, five, 0, 1, 128, 2, five, a, big, 0.01, None, ok, None) == INVALID
    assert called == []


# ---------------------------------------------------------------------------------------------------------------------
SHARDS = {"5+3": (5, 3), "1+1": (1, 1), "1+1+2": (1, 1, 2)}
C = 24
TOL = 1e-12


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) / max(1.0, float(np.abs(np.asarray(b)).max()))


@pytest.mark.parametrize("tag", list(SHARDS))
def test_the_exchange_arithmetic_is_training_mode_batch_norm_on_the_concatenated_batch(tag):
    rows = SHARDS[tag]
    rng = np.random.Generator(np.random.PCG64(17 + sum(rows)))
    n = sum(rows)
    z, da = rng.standard_normal((n, C)) * 1.5 + 0.3, rng.standard_normal((n, C))
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.standard_normal(C) * 0.1
    rm, rv = rng.standard_normal(C) * 0.1, rng.uniform(0.5, 1.5, C)
    cuts = np.cumsum(rows)[:-1]
    got = SB.forward_backward(np.split(z, cuts), np.split(da, cuts), gamma, beta, rm, rv)
    # the reference: one process, all rows
    t = lambda a: torch.from_numpy(np.array(a, np.float64))
    zt, gt, bt = t(z).requires_grad_(True), t(gamma).requires_grad_(True), t(beta).requires_grad_(True)
    rmt, rvt = t(rm), t(rv)
    a = F.batch_norm(zt, rmt, rvt, gt, bt, True, SB.MOMENTUM, SB.EPS)
    (a * t(da)).sum().backward()
    errs = dict(a=_rel(np.concatenate(got["a"]), a.detach().numpy()), dz=_rel(np.concatenate(got["dz"]), zt.grad.numpy()),
                dgamma=_rel(got["dgamma"], gt.grad.numpy()), dbeta=_rel(got["dbeta"], bt.grad.numpy()),
                running_mean=_rel(got["running_mean"], rmt.numpy()), running_var=_rel(got["running_var"], rvt.numpy()))
    print(f"shards {tag}, C = {C}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert got["N"] == n and max(errs.values()) <= TOL, errs
    # a replica's own d gamma / d beta is not the global one (more than one shard), their plain sum is
    assert len(got["local"]) == len(rows) and not np.allclose(got["local"][0][0], got["dgamma"])
    assert np.array_equal(sum(l[0] for l in got["local"]), got["dgamma"]) and np.array_equal(sum(l[1] for l in got["local"]), got["dbeta"])
    # not the per-shard function: a shard normalised by its own statistics is something else
    if rows[0] > 1:
        own = SB.forward_backward([z[:rows[0]]], [da[:rows[0]]], gamma, beta, rm, rv)
        assert not np.allclose(own["a"][0], got["a"][0])


# ---------------------------------------------------------------------------------------------------------------------
def test_the_modules_take_sync_refuse_nonsense_and_add_no_tensor():
    from hmd_ego_pose_amd import TrainableHeads
    from hmd_ego_pose_amd.backbone import TrainableBackbone
    from hmd_ego_pose_amd.neck import TrainableNeck
    for make in (lambda **kw: TrainableHeads(0, 1, **kw), lambda **kw: TrainableNeck(0, **kw), lambda **kw: TrainableBackbone(0, **kw)):
        m = make(batch_norm="sync")
        assert m.batch_norm == "sync" and make(batch_norm="sync", process_group=None).batch_norm == "sync"
        assert sorted(m.state_dict()) == sorted(make().state_dict())           # the mode and its hook add no tensor
        assert m.train()._sync_hook() is not None and m._bn_mode() == 1
        assert m.eval()._sync_hook() is None and m._bn_mode() == 0             # eval(): the running-statistics function
        for other in ("running", "batch"):
            o = make(batch_norm=other)
            assert o.train()._sync_hook() is None and o._bn_mode() == {"running": 0, "batch": 1}[other] and o.eval()._bn_mode() == 0
        with pytest.raises(ValueError):
            make(batch_norm="synced")
        with pytest.raises(ValueError):
            make(batch_norm="batch", process_group=object())                   # a group goes with "sync"
        with pytest.raises(ValueError):
            make(process_group=object())


def test_from_model_passes_sync_through():
    from hmd_ego_pose_amd import HMDEgoPose, TrainableHeads
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0)
    m.reset_parameters(seed=5)
    part = TrainableHeads.from_model(m, batch_norm="sync")
    assert part.batch_norm == "sync"
    sd = m.state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in part.state_dict().items())


def test_the_hook_without_a_group_is_the_identity_and_never_raises():
    h = sync.SumHook(None)
    assert h.world == 1
    block = torch.arange(6, dtype=torch.float64)
    keep = block.clone()
    h.register(block.view(torch.uint8))
    assert h._cb(None, block.data_ptr(), 6, 1, None) == 0 and h.calls == 1 and h.error is None
    assert torch.equal(block, keep)
    st = ctypes.cast(h.ref(), ctypes.POINTER(sync.HepSync)).contents
    assert st.sum(None, block.data_ptr(), 6, 1, None) == 0 and h.calls == 2      # what the library calls
    # a block outside every registered workspace, with a (pretended) second replica: non-zero, the exception kept, nothing raised
    h.world = 2
    assert h._cb(None, block.data_ptr() + 8 * 64, 6, 1, None) == 1 and isinstance(h.error, RuntimeError)
    # ... and the view of a block inside one is that memory
    v = h._view(block.data_ptr() + 16, 3, True)
    assert v.dtype == torch.float64 and v.data_ptr() == block.data_ptr() + 16 and v.tolist() == [2.0, 3.0, 4.0]
    f = h._view(block.data_ptr(), 4, False)
    assert f.dtype == torch.float32 and f.numel() == 4


def test_trainer_argument_rules_that_need_no_device():
    from hmd_ego_pose_amd.trainer import Trainer
    with pytest.raises(ValueError, match="batch_norm"):
        Trainer({}, batch_norm="synced")
    with pytest.raises(ValueError, match="drift"):
        Trainer({}, batch_norm="batch", process_group=object())
    with pytest.raises(ValueError, match="ROCm"):
        Trainer({}, batch_norm="sync", process_group=sync.LOCAL, device="cpu")      # "sync" passes the mode check and reaches the device check
    with pytest.raises(ValueError, match="process_group"):
        Trainer({}, batch_norm="sync")                            # "sync" names its replicas: a group, or sync.LOCAL
    with pytest.raises(ValueError, match="process_group"):
        Trainer({}, batch_norm="sync", process_group="world")
