"""CPU side of the trainable EfficientNet trunk (hmd_ego_pose_amd/backbone.py, hep_backbone_*_device).

The oracle's autograd through ``oracle.efficientpose_ref.backbone`` is pinned to the REAL reference's autograd
(tests/golden/backbone_grads.npz, made by tests/golden/make_golden_backbone_grads.py), so the GPU tests may compare dense device
gradients against the oracle.  Bound of that pin: REF_F32_TOL = 1e-5 of tests/test_head_grads_cpu.py - the golden values are a
float32 evaluation, the oracle here runs in float64; every error relative to the tensor's largest magnitude.  Measured on the
committed slices with this seeding (one thread): taps 7.4e-7, image gradient 1.9e-6, worst parameter gradient 3.4e-6 at phi 0 /
128 / batch 2; 6.2e-7 / 1.2e-6 / 2.8e-6 at phi 3 / 128 / batch 1; 1.0e-6 / 2.5e-6 / 3.6e-6 in the drop-connect case.  Dense (every
element, reference float32 against oracle float64) the worst parameter gradient is 6.1e-6 and 3.8e-6, and 7.1e-6 at phi 0 / 256 /
batch 2, which is why the goldens stay at 128.  No gradient tensor has zero scale with this seeding (smallest max |g| 0.79) and
the reference leaves no backbone parameter without a gradient (the generator asserts it).  The drop-connect case replays the
stored scale table through the restated block loop
of tests/_backbone_grad.py.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi, param_spec, seeded_state_dict
from tests import _backbone_grad as G
from tests.test_head_grads_cpu import REF_F32_TOL, check_against_golden

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "backbone_grads.npz")


@pytest.mark.parametrize("tag", list(G.GOLDEN_CASES) + [G.DROP_TAG])
def test_oracle_autograd_reproduces_the_reference(tag):
    phi, size, batch, seed = G.DROP_CASE if tag == G.DROP_TAG else G.GOLDEN_CASES[tag]
    z = np.load(GOLDEN)
    scales = torch.from_numpy(z[f"{tag}/scales"]) if tag == G.DROP_TAG else None
    image, cots = G.seeded_inputs(phi, size, batch)
    taps, grads, gimage = G.oracle_grads(seeded_state_dict(phi, seed), image, cots, phi, torch.float64, scales)
    names = G.golden_names(phi)
    assert len(names) == len(z[f"{tag}/sums"]) == 4 + len(grads)
    assert set(grads) == {k for k, _ in G.backbone_keys(phi) if G.trainable(k)}
    worst = {"taps": 0.0, "image": 0.0, "params": 0.0}
    for t, m in enumerate(taps):
        worst["taps"] = max(worst["taps"], check_against_golden(z, tag, names, f"tap.{t}", m.numpy(), REF_F32_TOL, scale=float(m.abs().max())))
    worst["image"] = check_against_golden(z, tag, names, "image", gimage.numpy(), REF_F32_TOL, scale=float(gimage.abs().max()))
    for k, g in grads.items():
        scale = float(g.abs().max())
        assert scale > 0.0, k                                   # no dead sub-graph in the trunk
        worst["params"] = max(worst["params"], check_against_golden(z, tag, names, "param." + k, g.numpy(), REF_F32_TOL, scale=scale))
    print(f"{tag}: oracle float64 against the reference's float32 autograd, worst slice error / scale " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("phi", [0, 3])
def test_trainable_backbone_carries_the_reference_backbone_keys(phi):
    from hmd_ego_pose_amd import TrainableBackbone
    want = [(k, tuple(s)) for k, s in param_spec(phi) if k.startswith("backbone_net.")]
    n = TrainableBackbone(phi)
    got = [(k, tuple(v.shape)) for k, v in n.state_dict().items()]
    assert got == want                                           # the same order, too
    params = dict(n.named_parameters())
    for k, _ in want:
        leaf = k.rsplit(".", 1)[1]
        assert (k in params) == (leaf in ("weight", "bias")), k
    assert sum(p.numel() for p in params.values()) == sum(int(np.prod(s)) for k, s in G.backbone_keys(phi) if G.trainable(k))
    assert n.drop_connect_rate == 0.0
    with pytest.raises(ValueError):
        TrainableBackbone(8)


def test_from_model_and_export_round_trip_bit_exactly():
    from hmd_ego_pose_amd import HMDEgoPose, TrainableBackbone
    torch.manual_seed(3)
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0)
    m.reset_parameters(seed=5)
    n = TrainableBackbone.from_model(m)
    sd = m.state_dict()
    for k, v in n.state_dict().items():
        assert k.startswith("backbone_net.") and torch.equal(v, sd[k]) and v.data_ptr() != sd[k].data_ptr(), k
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
    key = "backbone_net.model._blocks.3._se_reduce.conv.bias"
    assert not torch.equal(after[key], before[key])
    with pytest.raises(KeyError):
        TrainableBackbone.from_model(type("M", (), {"compound_coef": 0, "state_dict": lambda self: {"backbone_net.x": torch.zeros(1)}})())


def test_param_count_and_layout_follow_param_spec():
    from hmd_ego_pose_amd.backbone import flat_keys, param_layout
    for phi in range(8):                                         # every phi the ABI accepts
        keys = flat_keys(phi)
        total, offsets = param_layout(phi)
        assert total == sum(int(np.prod(s)) for _, s in keys) == _capi.lib().hep_backbone_param_count(phi)
        assert offsets == list(np.cumsum([0] + [int(np.prod(s)) for _, s in keys])[:-1])
        assert [k for k, _ in keys] == [k for k, _ in G.backbone_keys(phi)]
    assert len(flat_keys(0)) == 5 + 14 + 15 * 19


def test_backbone_abi_refuses_bad_arguments_before_any_hip_call():
    """HEP_ERR_INVALID = -1 for NULL pointers / a short or misaligned workspace, HEP_ERR_UNSUPPORTED = -4 with a reason for phi 8,
    size 200, batch 0; all of it on a machine without a device."""
    l = _capi.lib()
    for name in ("hep_backbone_param_count", "hep_backbone_param_layout", "hep_backbone_workspace_bytes", "hep_backbone_forward_device",
                 "hep_backbone_backward_device", "hep_backbone_stage_count", "hep_backbone_stage_info"):
        assert hasattr(l, name), name
    need = l.hep_backbone_workspace_bytes(0, 256, 2)
    assert need > 0 and need % 16 == 0 and l.hep_backbone_workspace_bytes(0, 256, 4) > need
    buf = np.zeros(64, np.float32)
    a = (buf.ctypes.data + 15) // 16 * 16                       # a non-NULL, 16-byte aligned host address: never dereferenced
    three, holed3 = (ctypes.c_void_p * 3)(a, a, a), (ctypes.c_void_p * 3)(a, None, a)
    fwd = lambda params=a, image=a, scale=None, phi=0, size=256, batch=2, taps=three, ws=a, nbytes=need: \
        l.hep_backbone_forward_device(params, image, scale, phi, size, batch, taps, ws, nbytes, None)
    bwd = lambda params=a, gtaps=three, scale=None, phi=0, size=256, batch=2, gparams=a, gimage=None, ws=a, nbytes=need: \
        l.hep_backbone_backward_device(params, gtaps, scale, phi, size, batch, gparams, gimage, ws, nbytes, None)
    for f in (fwd, bwd):
        assert f(params=None) == -1 and f(ws=None) == -1
        assert f(phi=8) == -4 and b"phi" in l.hep_last_error()
        assert f(phi=-1) == -4
        assert f(size=200) == -4 and b"multiple of 128" in l.hep_last_error()
        assert f(size=0) == -4 and f(size=2176) == -4
        assert f(batch=0) == -4 and b"batch" in l.hep_last_error()
        assert f(nbytes=need - 4) == -1 and b"workspace" in l.hep_last_error()
        assert f(ws=a + 4) == -1
    assert fwd(image=None) == -1 and fwd(taps=None) == -1 and fwd(taps=holed3) == -1
    assert bwd(gtaps=None) == -1 and bwd(gparams=None) == -1 and bwd(gtaps=holed3) == -1
    assert l.hep_backbone_param_count(8) == -4 and l.hep_backbone_param_count(7) > l.hep_backbone_param_count(0) > 0
    assert l.hep_backbone_workspace_bytes(0, 200, 1) == -4 and l.hep_backbone_workspace_bytes(0, 256, 0) == -4 and l.hep_backbone_workspace_bytes(0, 0, 0) == -4
    count = l.hep_backbone_param_layout(0, None, 0)
    assert count == 5 + 14 + 15 * 19 and l.hep_backbone_param_layout(0, (ctypes.c_int64 * 4)(), 4) == -1
    # the stages name the stem and every block, inside the workspace, with the sides and channels of the architecture
    from hmd_ego_pose_amd.arch import get_arch
    arch = get_arch(0)
    names = {}
    assert l.hep_backbone_stage_count(0) == 1 + len(arch.blocks)
    for i in range(l.hep_backbone_stage_count(0)):
        nm = ctypes.c_char_p(); dims = (ctypes.c_int64 * 4)(); off = ctypes.c_int64()
        assert l.hep_backbone_stage_info(0, 256, 2, i, ctypes.byref(nm), dims, ctypes.byref(off)) == 0
        assert dims[0] == 2 and dims[1] == dims[2] and off.value % 16 == 0
        assert 0 <= off.value and off.value + 4 * dims[0] * dims[1] * dims[2] * dims[3] <= need
        names[nm.value.decode()] = (int(dims[1]), int(dims[3]))
    assert names["stem"] == (128, arch.stem)
    side = 128
    for i, b in enumerate(arch.blocks):
        side //= b.stride
        assert names[f"block{i}"] == (side, b.cout), i
    assert [names[f"block{i}"] for i in arch.taps] == [(32, 40), (16, 112), (8, 320)]
    assert l.hep_backbone_stage_info(0, 256, 2, 99, None, None, None) == -1


def test_drop_connect_draw_equals_the_reference_formula_for_a_fixed_seed():
    """The module's draw == the scale table stored with the golden drop-connect case, which the generator re-created with the
    reference's formula and checked against the real reference's taps; and nothing is drawn in eval() or at rate 0."""
    from hmd_ego_pose_amd import TrainableBackbone
    from hmd_ego_pose_amd.arch import get_arch
    phi, _size, batch, _seed = G.DROP_CASE
    stored = torch.from_numpy(np.load(GOLDEN)[f"{G.DROP_TAG}/scales"])
    bb = TrainableBackbone(phi)
    bb.drop_connect_rate = G.DROP_RATE
    bb.train()
    torch.manual_seed(G.DROP_TORCH_SEED)
    mine = bb.draw_branch_scale(batch, "cpu")
    assert mine.dtype == torch.float32 and torch.equal(mine, stored)
    assert torch.equal(G.reference_scales(phi, G.DROP_RATE, batch, G.DROP_TORCH_SEED), stored)
    blocks = get_arch(phi).blocks
    for i, b in enumerate(blocks):                               # blocks that add nothing, and block-rate 0, keep scale 1
        keep = 1 - G.DROP_RATE * i / len(blocks)
        allowed = {0.0, float(np.float32(1.0) / np.float32(keep))} if b.skip else {1.0}
        assert set(mine[i].tolist()) <= allowed, (i, mine[i])
    state = torch.get_rng_state()
    assert bb.eval().draw_branch_scale(batch, "cpu") is None
    bb.drop_connect_rate = 0.0
    assert bb.train().draw_branch_scale(batch, "cpu") is None
    assert torch.equal(torch.get_rng_state(), state)             # and no random number was consumed
