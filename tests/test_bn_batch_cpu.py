"""CPU side of batch-statistics BatchNorm for the three trainable parts (``batch_norm="batch"``, hep_*_device_bn).

The GPU tests compare the device with the oracle whose one BatchNorm function is replaced by ``F.batch_norm(training=True)``
(tests/_bn_batch.py::batch_statistics).  Here that patched oracle is pinned to the REAL reference in training mode
(tests/golden/bn_batch_grads.npz, made by tests/golden/make_golden_bn_batch.py in float64): outputs, input gradients, gradients
of every trainable tensor and the running statistics after one forward.  Both sides are float64 evaluations of the same function
and the archive keeps float32 slices next to float64 sums.  So the slices are bounded by float32 storage - one float32 epsilon,
2^-23, of the tensor's largest element (rounding is half of that) - and the float64 sums by 1e-9 of the abs-sum: two float64
evaluations in possibly different operation orders behind at most ~60 layers, 2^-53 times a generous 1e7 of amplification.

Analytic zeros.  Under batch statistics a bias in front of a BatchNorm has a gradient of exactly zero (the mean is subtracted),
and so has bn2's bias of a backbone block whose output reaches, through skip adds, only bias-free 1 x 1 convs that feed a
BatchNorm.  float64 leaves ~1e-13 there against BatchNorm-bias gradients of 1e2; the relative-error metric is meaningless for
them, so the GPU tests treat the set apart - and this file caps the set: every tensor below 1e-9 of the largest BatchNorm-bias
gradient must match the structural name pattern of its part, so no weight gradient can hide among the "zeros".
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi
from tests import _bn_batch as BB
from tests._head_grad import digest_stride, golden_entry
from tests._util import seeded_state_dict_once as seeded_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
STORAGE_TOL, SUM_TOL = 2.0 ** -23, 1e-9
INVALID, UNSUPPORTED = -1, -4


def _golden_case(part):
    tag = BB.GOLDEN[part]
    case = BB.CASES[part][tag]
    sd = seeded_state_dict(case[0], case[3], num_classes=case[4] or 1)
    return tag, case, BB.oracle(part, sd, case, torch.float64)


@pytest.mark.parametrize("part", BB.PARTS)
def test_patched_oracle_reproduces_the_reference_in_training_mode(part):
    tag, case, res = _golden_case(part)
    z = np.load(os.path.join(HERE, "golden", "bn_batch_grads.npz"))
    names = BB.golden_names(part, case)
    tensors = BB.golden_tensors(part, case, res)
    assert sorted(names) == sorted(tensors) and len(names) == len(z[f"{part}.{tag}/sums"])
    zeros = set(BB.zero_set(res["grads"]))
    top = max(float(v.abs().max()) for k, v in res["grads"].items() if BB.is_bn_bias(k))
    worst, stats = 0.0, 0
    for name in names:
        shape, (s, sa), sl = golden_entry(z, f"{part}.{tag}", names, name)
        a = tensors[name].reshape(-1)
        assert list(tensors[name].shape) == shape, (name, tensors[name].shape, shape)
        mine = a[::digest_stride(a.size)]
        if name.startswith("param.") and name[6:] in zeros:      # both sides are rounding noise around zero
            assert float(np.abs(sl).max()) < BB.ZERO_REL * top and float(np.abs(mine).max()) < BB.ZERO_REL * top, name
            continue
        scale = max(float(np.abs(a).max()), 1e-300)
        err = float(np.abs(mine - sl.astype(np.float64)).max()) / scale
        worst = max(worst, err)
        assert err <= STORAGE_TOL, (name, err)
        assert abs(a.sum() - s) <= SUM_TOL * sa and abs(np.abs(a).sum() - sa) <= SUM_TOL * sa, (name, a.sum(), s, sa)
        stats += name.startswith("stat.")
    assert stats == sum(1 for k, _ in BB.keys(part, case) if not BB.trainable(k)) > 0
    # the running statistics moved: the golden values are not the ones that were loaded
    sd = seeded_state_dict(case[0], case[3], num_classes=case[4] or 1)
    moved = [k for k, v in res["stats"].items() if not torch.equal(v, sd[k].double())]
    assert len(moved) == len(res["stats"])
    print(f"{part} {tag}: {len(names)} tensors ({stats} running statistics) against the reference in train(), worst slice error / scale {worst:.2e}")


@pytest.mark.parametrize("part", BB.PARTS)
def test_the_analytic_zero_set_is_the_structural_one(part):
    _tag, _case, res = _golden_case(part)
    zeros = BB.zero_set(res["grads"])
    top = max(float(v.abs().max()) for k, v in res["grads"].items() if BB.is_bn_bias(k))
    largest = max(float(res["grads"][k].abs().max()) for k in zeros) if zeros else 0.0
    print(f"{part}: {len(zeros)} analytically zero tensors, largest float64 magnitude {largest:.2e} against a BatchNorm-bias gradient of {top:.3g}")
    assert zeros, part
    stray = [k for k in zeros if not BB.ZERO_PATTERN[part].match(k)]
    assert not stray, stray
    if part != "backbone":                                       # heads and neck: every bias in front of a BatchNorm, and nothing else
        want = [k for k in res["grads"] if BB.ZERO_PATTERN[part].match(k)]
        assert sorted(want) == zeros


def test_the_new_entry_points_exist_and_size_their_workspace():
    l = _capi.lib()
    for part in BB.PARTS:
        for name in (f"hep_{part}_workspace_bytes_bn", f"hep_{part}_forward_device_bn", f"hep_{part}_backward_device_bn"):
            assert hasattr(l, name), name
    for phi, size, batch in [(0, 128, 2), (0, 256, 16), (3, 128, 8), (5, 256, 1)]:
        for part, cfg in (("heads", (phi, 1, size, batch)), ("neck", (phi, size, batch)), ("backbone", (phi, size, batch))):
            old = getattr(l, f"hep_{part}_workspace_bytes")(*cfg)
            query = getattr(l, f"hep_{part}_workspace_bytes_bn")
            running, batch_mode = query(*cfg, _capi_mode("running")), query(*cfg, _capi_mode("batch"))
            assert old > 0 and running == old, (part, cfg, old, running)
            assert batch_mode >= running and batch_mode % 16 == 0, (part, cfg, running, batch_mode)
            print(f"{part} phi {phi} @ {size} b{batch}: workspace {running} bytes (running), {batch_mode} (batch)")


def _capi_mode(name):
    from hmd_ego_pose_amd import _trainable
    return _trainable.BN_MODES[name]


def test_too_few_rows_and_bad_modes_are_refused_before_any_hip_call():
    """All on a machine without a device: the refusals come before the first HIP call."""
    l = _capi.lib()
    run, bat = _capi_mode("running"), _capi_mode("batch")
    assert (run, bat) == (0, 1)
    # phi 0, size 128, batch 1: P7 is one pixel, a BatchNorm over one row
    assert l.hep_heads_workspace_bytes_bn(0, 1, 128, 1, bat) == UNSUPPORTED and b"2 rows" in l.hep_last_error()
    assert l.hep_neck_workspace_bytes_bn(0, 128, 1, bat) == UNSUPPORTED and b"2 rows" in l.hep_last_error()
    assert l.hep_heads_workspace_bytes_bn(0, 1, 128, 1, run) > 0 and l.hep_neck_workspace_bytes_bn(0, 128, 1, run) > 0
    assert l.hep_heads_workspace_bytes_bn(0, 1, 128, 2, bat) > 0 and l.hep_neck_workspace_bytes_bn(0, 128, 2, bat) > 0
    assert l.hep_backbone_workspace_bytes_bn(0, 128, 1, bat) > 0                      # its smallest map has 16 rows per image
    for mode in (-1, 2, 7):
        assert l.hep_heads_workspace_bytes_bn(0, 1, 128, 2, mode) < 0 and b"mode" in l.hep_last_error()
        assert l.hep_neck_workspace_bytes_bn(0, 128, 2, mode) < 0 and b"mode" in l.hep_last_error()
        assert l.hep_backbone_workspace_bytes_bn(0, 128, 2, mode) < 0 and b"mode" in l.hep_last_error()
    buf = np.zeros(64, np.float32)
    a = (buf.ctypes.data + 15) // 16 * 16                       # a non-NULL, 16-byte aligned host address: never dereferenced
    five, three = (ctypes.c_void_p * 5)(*([a] * 5)), (ctypes.c_void_p * 3)(*([a] * 3))
    big = 1 << 40                                               # "enough" workspace: the size check passes, the row check must not
    calls = {
        "heads_fwd": lambda size, batch, mode, mom=0.01: l.hep_heads_forward_device_bn(a, five, 0, 1, size, batch, five, a, big, mode, mom, None, None),
        "heads_bwd": lambda size, batch, mode, mom=0.01: l.hep_heads_backward_device_bn(a, five, 0, 1, size, batch, a, None, a, big, mode, None),
        "neck_fwd": lambda size, batch, mode, mom=0.01: l.hep_neck_forward_device_bn(a, three, 0, size, batch, five, a, big, mode, mom, None, None),
        "neck_bwd": lambda size, batch, mode, mom=0.01: l.hep_neck_backward_device_bn(a, five, 0, size, batch, a, None, a, big, mode, None),
        "backbone_fwd": lambda size, batch, mode, mom=0.01: l.hep_backbone_forward_device_bn(a, a, None, 0, size, batch, three, a, big, mode, mom, None, None),
        "backbone_bwd": lambda size, batch, mode, mom=0.01: l.hep_backbone_backward_device_bn(a, three, None, 0, size, batch, a, None, a, big, mode, None),
    }
    for name, f in calls.items():
        assert f(128, 2, 5) < 0 and b"mode" in l.hep_last_error(), name
        assert f(200, 2, bat) == UNSUPPORTED, name
        if not name.startswith("backbone"):
            assert f(128, 1, bat) == UNSUPPORTED and b"2 rows" in l.hep_last_error(), name
        if name.endswith("fwd"):
            assert f(128, 2, bat, 1.5) == INVALID and b"momentum" in l.hep_last_error(), name
            assert f(128, 2, bat, float("nan")) == INVALID, name
    # a workspace of the running-mode size is too small for batch mode where batch mode needs more
    need_run, need_bat = l.hep_heads_workspace_bytes_bn(0, 1, 128, 2, run), l.hep_heads_workspace_bytes_bn(0, 1, 128, 2, bat)
    assert need_bat > need_run
    assert l.hep_heads_forward_device_bn(a, five, 0, 1, 128, 2, five, a, need_run, bat, 0.01, None, None) == INVALID and b"workspace" in l.hep_last_error()


def test_the_modules_take_batch_norm_and_refuse_anything_else():
    from hmd_ego_pose_amd import TrainableHeads
    from hmd_ego_pose_amd.backbone import TrainableBackbone
    from hmd_ego_pose_amd.neck import TrainableNeck
    with pytest.raises(ValueError):
        TrainableHeads(0, 1, batch_norm="nonsense")
    with pytest.raises(ValueError):
        TrainableNeck(0, batch_norm="frozen")
    with pytest.raises(ValueError):
        TrainableBackbone(0, batch_norm=None)
    for make in (lambda **kw: TrainableHeads(0, 1, **kw), lambda **kw: TrainableNeck(0, **kw), lambda **kw: TrainableBackbone(0, **kw)):
        assert make().batch_norm == "running" and make(batch_norm="running").batch_norm == "running"
        m = make(batch_norm="batch")
        assert m.batch_norm == "batch"
        assert m.train()._bn_mode() == 1 and m.eval()._bn_mode() == 0 and make().train()._bn_mode() == 0
        assert sorted(m.state_dict()) == sorted(make().state_dict())           # the mode adds no tensor


def test_from_model_passes_batch_norm_through():
    from hmd_ego_pose_amd import HMDEgoPose, TrainableHeads
    from hmd_ego_pose_amd.backbone import TrainableBackbone
    from hmd_ego_pose_amd.neck import TrainableNeck
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0)
    m.reset_parameters(seed=5)
    for cls in (TrainableHeads, TrainableNeck, TrainableBackbone):
        assert cls.from_model(m).batch_norm == "running"
        part = cls.from_model(m, batch_norm="batch")
        assert part.batch_norm == "batch"
        sd = m.state_dict()
        assert all(torch.equal(v, sd[k]) for k, v in part.state_dict().items())
        with pytest.raises(ValueError):
            cls.from_model(m, batch_norm="nonsense")


def test_store_statistics_writes_the_running_slots_in_place_and_counts_the_batch():
    """The host half of the update: the statistics buffer has the layout of ``flat_parameters``; only running_mean / running_var
    are copied, in place (same storage), every num_batches_tracked goes up by one, parameters are untouched."""
    from hmd_ego_pose_amd import TrainableHeads
    h = TrainableHeads(0, 1, batch_norm="batch")
    h.load_state_dict(seeded_state_dict(0, 0), strict=False)
    before = {k: v.clone() for k, v in h.state_dict().items()}
    ptrs = {k: v.data_ptr() for k, v in h.state_dict().items()}
    flat = h.flat_parameters().detach()
    stats = torch.full_like(flat, float("nan"))
    sizes = [before[k].numel() for k in h._flat_keys]
    for k, piece in zip(h._flat_keys, stats.split(sizes)):
        if "running" in k:
            piece.copy_(before[k].reshape(-1) + 1.0)
    h._store_statistics(stats)
    after = h.state_dict()
    for k, v in after.items():
        assert v.data_ptr() == ptrs[k], k
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1, k
        elif "running" in k:
            assert torch.equal(v, before[k] + 1.0), k
        else:
            assert torch.equal(v, before[k]), k
