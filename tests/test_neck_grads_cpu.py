"""CPU side of the trainable BiFPN neck (hmd_ego_pose_amd/neck.py, hep_neck_*_device).

The oracle's autograd through ``oracle.efficientpose_ref.bifpn_cell`` is pinned to the REAL reference's autograd
(tests/golden/neck_grads.npz, made by tests/golden/make_golden_neck_grads.py), so the GPU tests may compare dense device
gradients against the oracle.  Bound of that pin: REF_F32_TOL = 1e-5 of tests/test_head_grads_cpu.py - the golden values are a
float32 evaluation, the oracle here runs in float64; measured with this seeding: 4.9e-7 (maps), 5.7e-7 (taps), 1.9e-6 (conv /
BatchNorm), 5.5e-7 (fusion) at phi 0 / 128 / batch 2 and 3.9e-7 / 1.5e-6 / 3.1e-6 / 1.0e-6 at phi 3 / 128 / batch 1.  The
fusion-weight gradients are compared on ONE scale per case, the largest |g64| over all fusion tensors: seed 0 has relu-dead
fusion weights whose surviving partner has a gradient of the order 1e-4 of the dot products behind it.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi, param_spec, seeded_state_dict
from tests import _neck_grad as N
from tests.test_head_grads_cpu import REF_F32_TOL, check_against_golden

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("tag", list(N.GOLDEN_CASES))
def test_oracle_autograd_reproduces_the_reference(tag):
    phi, size, batch, seed = N.GOLDEN_CASES[tag]
    z = np.load(os.path.join(HERE, "golden", "neck_grads.npz"))
    taps, cots = N.seeded_inputs(phi, size, batch)
    maps, grads, gtaps = N.oracle_grads(seeded_state_dict(phi, seed), taps, cots, phi, torch.float64)
    names = N.golden_names(phi)
    assert len(names) == len(z[f"{tag}/sums"]) == 8 + len(grads)
    assert set(grads) == {k for k, _ in N.neck_keys(phi) if N.trainable(k)}
    fscale = max(float(g.abs().max()) for k, g in grads.items() if N.is_fusion(k))
    worst = 0.0
    for l, m in enumerate(maps):
        worst = max(worst, check_against_golden(z, tag, names, f"map.{l}", m.numpy(), REF_F32_TOL, scale=float(m.abs().max())))
    for t, g in enumerate(gtaps):
        worst = max(worst, check_against_golden(z, tag, names, f"tap.{t}", g.numpy(), REF_F32_TOL, scale=float(g.abs().max())))
    for k, g in grads.items():
        if N.is_fusion(k):                                   # slice, sum and abs-sum on the case's common fusion scale
            shape, (s, sa), sl = N.golden_entry(z, tag, names, "param." + k)
            a = g.numpy().reshape(-1)
            assert list(g.shape) == shape
            errs = [float(np.abs(a[::N.digest_stride(a.size)] - sl).max()), abs(a.sum() - s) / a.size, abs(np.abs(a).sum() - sa) / a.size]
            assert max(errs) <= REF_F32_TOL * fscale, (k, errs, fscale)
            worst = max(worst, max(errs) / fscale)
            continue
        scale = float(g.abs().max())
        if scale == 0.0:                                     # a sub-graph behind a dead fusion weight: identically zero in the reference too
            shape, (s, sa), sl = N.golden_entry(z, tag, names, "param." + k)
            assert sa == 0.0 and not sl.any(), k
            continue
        worst = max(worst, check_against_golden(z, tag, names, "param." + k, g.numpy(), REF_F32_TOL, scale=scale))
    print(f"{tag}: oracle float64 against the reference's float32 autograd, worst slice error / scale {worst:.2e}")


@pytest.mark.parametrize("phi", [0, 3])
def test_trainable_neck_carries_the_reference_bifpn_keys(phi):
    from hmd_ego_pose_amd import TrainableNeck
    want = [(k, tuple(s)) for k, s in param_spec(phi) if k.startswith("bifpn.")]
    n = TrainableNeck(phi)
    got = [(k, tuple(v.shape)) for k, v in n.state_dict().items()]
    assert sorted(got) == sorted(want) and len(got) == len(want)
    params = dict(n.named_parameters())
    for k, _ in want:
        leaf = k.rsplit(".", 1)[1]
        assert (k in params) == (leaf in ("weight", "bias") or N.is_fusion(k)), k
    assert sum(p.numel() for p in params.values()) == sum(int(np.prod(s)) for k, s in N.neck_keys(phi) if N.trainable(k))
    for bad in (6, 7, 8):
        with pytest.raises(ValueError):
            TrainableNeck(bad)


def test_from_model_and_export_round_trip_bit_exactly():
    from hmd_ego_pose_amd import HMDEgoPose, TrainableNeck
    torch.manual_seed(3)
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0)
    m.reset_parameters(seed=5)
    n = TrainableNeck.from_model(m)
    sd = m.state_dict()
    for k, v in n.state_dict().items():
        assert k.startswith("bifpn.") and torch.equal(v, sd[k]) and v.data_ptr() != sd[k].data_ptr(), k
    with torch.no_grad():
        for p in n.parameters():
            p.add_(torch.randn_like(p))
        for _name, b in n.named_buffers():
            if b.dtype == torch.float32:
                b.add_(torch.rand_like(b))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert n.export_to(m) is m
    after, own = m.state_dict(), n.state_dict()
    for k, v in after.items():
        assert torch.equal(v, own[k] if k in own else before[k]), k
    assert not torch.equal(after["bifpn.0.p4_w2"], before["bifpn.0.p4_w2"])
    with pytest.raises(KeyError):
        TrainableNeck.from_model(type("M", (), {"compound_coef": 0, "state_dict": lambda self: {"bifpn.x": torch.zeros(1)}})())


def test_param_count_and_layout_follow_param_spec():
    from hmd_ego_pose_amd.neck import flat_keys, param_layout
    known = {0: (200121, 228), 3: (1576754, 420)}
    for phi in range(6):                                         # every phi the ABI accepts
        count, tensors = known.get(phi, (None, None))
        keys = flat_keys(phi)
        total, offsets = param_layout(phi)
        assert total == sum(int(np.prod(s)) for _, s in keys) == _capi.lib().hep_neck_param_count(phi)
        assert offsets == list(np.cumsum([0] + [int(np.prod(s)) for _, s in keys])[:-1])
        if count is not None:
            assert total == count and len(keys) == tensors


def test_neck_abi_refuses_bad_arguments_before_any_hip_call():
    """HEP_ERR_INVALID = -1 for NULL pointers / a short or misaligned workspace, HEP_ERR_UNSUPPORTED = -4 with a reason for phi 6,
    phi 8, size 200, batch 0; all of it on a machine without a device."""
    l = _capi.lib()
    for name in ("hep_neck_param_count", "hep_neck_param_layout", "hep_neck_workspace_bytes", "hep_neck_forward_device",
                 "hep_neck_backward_device", "hep_neck_stage_count", "hep_neck_stage_info"):
        assert hasattr(l, name), name
    need = l.hep_neck_workspace_bytes(0, 256, 2)
    assert need > 0 and need % 16 == 0 and l.hep_neck_workspace_bytes(0, 256, 4) > need
    buf = np.zeros(64, np.float32)
    a = (buf.ctypes.data + 15) // 16 * 16                       # a non-NULL, 16-byte aligned host address: never dereferenced
    three, five = (ctypes.c_void_p * 3)(a, a, a), (ctypes.c_void_p * 5)(*([a] * 5))
    holed3, holed5 = (ctypes.c_void_p * 3)(a, None, a), (ctypes.c_void_p * 5)(a, a, None, a, a)
    fwd = lambda params=a, taps=three, phi=0, size=256, batch=2, feats=five, ws=a, nbytes=need: \
        l.hep_neck_forward_device(params, taps, phi, size, batch, feats, ws, nbytes, None)
    bwd = lambda params=a, gfeats=five, phi=0, size=256, batch=2, gparams=a, gtaps=None, ws=a, nbytes=need: \
        l.hep_neck_backward_device(params, gfeats, phi, size, batch, gparams, gtaps, ws, nbytes, None)
    for f in (fwd, bwd):
        assert f(params=None) == -1 and f(ws=None) == -1
        assert f(phi=6) == -4 and b"plain sums" in l.hep_last_error()
        assert f(phi=8) == -4 and b"phi" in l.hep_last_error()
        assert f(phi=-1) == -4
        assert f(size=200) == -4 and b"multiple of 128" in l.hep_last_error()
        assert f(size=0) == -4
        assert f(batch=0) == -4 and b"batch" in l.hep_last_error()
        assert f(nbytes=need - 4) == -1 and b"workspace" in l.hep_last_error()
        assert f(ws=a + 4) == -1
    assert fwd(taps=None) == -1 and fwd(feats=None) == -1 and fwd(taps=holed3) == -1 and fwd(feats=holed5) == -1
    assert bwd(gfeats=None) == -1 and bwd(gparams=None) == -1 and bwd(gfeats=holed5) == -1 and bwd(gtaps=holed3) == -1
    assert l.hep_neck_param_count(6) == -4 and l.hep_neck_param_count(8) == -4
    assert l.hep_neck_workspace_bytes(0, 200, 1) == -4 and l.hep_neck_workspace_bytes(0, 256, 0) == -4 and l.hep_neck_workspace_bytes(0, 0, 0) == -4
    assert l.hep_neck_param_layout(0, None, 0) == 228 and l.hep_neck_param_layout(0, (ctypes.c_int64 * 4)(), 4) == -1
    # the stages name every pool input, inside the workspace
    from hmd_ego_pose_amd.arch import get_arch
    names = {}
    for i in range(l.hep_neck_stage_count(0)):
        nm = ctypes.c_char_p(); dims = (ctypes.c_int64 * 4)(); off = ctypes.c_int64()
        assert l.hep_neck_stage_info(0, 256, 2, i, ctypes.byref(nm), dims, ctypes.byref(off)) == 0
        assert dims[0] == 2 and dims[1] == dims[2] and dims[3] == get_arch(0).fpn_w and off.value % 16 == 0
        assert 0 <= off.value and off.value + 4 * dims[0] * dims[1] * dims[2] * dims[3] <= need
        names[nm.value.decode()] = int(dims[1])
    assert set(N.pool_names(0)) <= set(names) and names["p6_pre"] == 8 and names["bifpn0_p6_in"] == 4 and names["bifpn2_p3"] == 32
    assert l.hep_neck_stage_info(0, 256, 2, 99, None, None, None) == -1


def test_routed_pool_with_its_own_argmax_is_maxpool_same_and_first_maximum_decides_ties():
    from oracle import efficientpose_ref as R
    rng = np.random.Generator(np.random.PCG64(5))
    x = torch.from_numpy(rng.standard_normal((2, 3, 8, 8)))
    x[0, 0, :4, :4] = 0.25                                     # exact ties
    pool = N.RoutedPool()
    assert torch.equal(pool(x), R.maxpool_same(x)) and pool.slack == [0.0]
    # the oracle's own routing through the whole neck: the same maps, slack exactly 0
    phi, size, batch, seed = N.GOLDEN_CASES["phi0_s128_b2"]
    taps, _cots = N.seeded_inputs(phi, size, batch)
    sd = {k: v.double() for k, v in seeded_state_dict(phi, seed).items() if k.startswith("bifpn.") and v.dtype == torch.float32}
    t64 = [torch.from_numpy(a).double() for a in taps]
    with torch.no_grad():
        pool = N.RoutedPool()
        a, b = N.oracle_neck(sd, t64, phi, pool), N.oracle_neck(sd, t64, phi)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and max(pool.slack) == 0.0 and len(pool.slack) == len(N.pool_names(phi))
    assert R.maxpool_same is not pool
    # the three tie cases on one 2 x 2 map (one window: real elements at positions 0, 1, 3, 4, padding elsewhere)
    for values, want in (([1.0, 1.0, 1.0, 1.0], [1, 0, 0, 0]),      # all equal: the top-left element
                         ([-1.0, 0.0, -1.0, -1.0], [0, 1, 0, 0]),   # a real 0.0 comes before the padding zeros
                         ([-1.0, -2.0, -3.0, -4.0], [0, 0, 0, 0])):  # the padding zero is strictly larger: dropped
        for fn in (R.maxpool_same, N.RoutedPool()):
            v = torch.tensor(values, dtype=torch.float64).view(1, 1, 2, 2).requires_grad_(True)
            fn(v).sum().backward()
            assert v.grad.view(-1).tolist() == [float(w) for w in want], (values, v.grad)
