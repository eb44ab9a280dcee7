"""GPU (MI355X): the trainable EfficientNet trunk - hep_backbone_forward_device / hep_backbone_backward_device
(csrc/k_backbone_grad.hip) behind hmd_ego_pose_amd.backbone.TrainableBackbone.

Forward: against the fp32 inference session (FLAG_KEEP_INTERMEDIATES) on the same image: ``stem`` and every ``block{i}`` through
``stage_views``, the three taps from the module; the project's fp32 parity bound 1e-3 relative to max(1, max |stage|).
Backward: against the oracle's float64 autograd (oracle.efficientpose_ref.backbone; with the stored scale table, the restated
block loop of tests/_backbone_grad.py).  Per group (taps forward; image gradient; conv weights - stem, expand, depthwise,
squeeze-excite, project; BatchNorm weights / biases and SE biases) the device's worst per-tensor error max |a - b| / max |b| must
be within BOUND_FACTOR = 4 times the worst error of the SAME oracle evaluated in float32 on the CPU (one thread), floor 2e-6 -
the rule of tests/test_gpu_head_grads.py.  There is no routing to teacher-force: the trunk has no max-pool.  The tests print
device / CPU-float32 / bound per group.

Measured on MI355X (device | float32 torch on the CPU | bound; NOTEBOOK.md section 14):
                      taps forward                 image gradient               conv weights                 BatchNorm / SE biases
  phi0_s128_b2        1.70e-6 | 1.27e-6 | 5.08e-6   4.11e-6 | 2.59e-6 | 1.03e-5   6.72e-6 | 1.08e-5 | 4.31e-5   6.83e-6 | 1.04e-5 | 4.14e-5
  phi0_s256_b2        1.82e-6 | 1.45e-6 | 5.78e-6   4.03e-6 | 3.66e-6 | 1.46e-5   1.01e-5 | 6.88e-6 | 2.75e-5   1.03e-5 | 6.25e-6 | 2.50e-5
  phi0_s384_b1        2.37e-6 | 1.87e-6 | 7.47e-6   4.95e-6 | 4.29e-6 | 1.72e-5   1.27e-5 | 8.97e-6 | 3.59e-5   1.14e-5 | 6.73e-6 | 2.69e-5
  phi3_s128_b1        1.23e-6 | 8.49e-7 | 3.40e-6   2.40e-6 | 1.59e-6 | 6.36e-6   6.00e-6 | 3.41e-6 | 1.37e-5   5.94e-6 | 4.02e-6 | 1.61e-5
  drop-connect case   1.78e-6 | 1.30e-6 | 5.21e-6   3.15e-6 | 3.34e-6 | 1.34e-5   5.24e-6 | 5.09e-6 | 2.03e-5   5.43e-6 | 5.78e-6 | 2.31e-5
  phi1_s128_b1        2.90e-6 | 2.21e-6 | 8.85e-6   7.47e-6 | 4.61e-6 | 1.85e-5   1.22e-5 | 2.28e-5 | 9.10e-5   1.80e-5 | 2.29e-5 | 9.14e-5
  phi2_s128_b1        1.57e-6 | 1.16e-6 | 4.62e-6   4.63e-6 | 2.05e-6 | 8.18e-6   1.19e-5 | 1.51e-5 | 6.04e-5   1.20e-5 | 1.52e-5 | 6.09e-5
  phi4_s128_b1        1.93e-6 | 1.01e-6 | 4.04e-6   7.22e-6 | 4.88e-6 | 1.95e-5   1.78e-5 | 1.15e-5 | 4.59e-5   2.80e-5 | 1.15e-5 | 4.61e-5
  phi5_s128_b1        2.43e-6 | 1.69e-6 | 6.77e-6   9.88e-6 | 6.23e-6 | 2.49e-5   2.19e-5 | 1.61e-5 | 6.45e-5   2.29e-5 | 1.61e-5 | 6.45e-5
  phi6_s128_b1        1.92e-6 | 8.80e-7 | 3.52e-6   5.59e-6 | 3.80e-6 | 1.52e-5   1.49e-5 | 7.07e-6 | 2.83e-5   1.50e-5 | 6.97e-6 | 2.79e-5
  phi0_s128_b7        1.98e-6 | 1.27e-6 | 5.07e-6   3.36e-6 | 2.60e-6 | 1.04e-5   5.65e-6 | 8.48e-6 | 3.39e-5   6.65e-6 | 8.09e-6 | 3.24e-5
  phi0_s256_b9        2.45e-6 | 1.54e-6 | 6.15e-6   3.82e-6 | 3.27e-6 | 1.31e-5   7.69e-6 | 1.01e-5 | 4.05e-5   9.05e-6 | 9.56e-6 | 3.82e-5
(the last seven: NOTEBOOK.md section 16; smallest max |g64| over the tensors of a case 0.61 .. 27, never zero; nearest to its bound:
BatchNorm / SE biases at phi 4, 0.61 of it.)
Forward against the session (worst stage): phi 0 @ 256 b2 2.2e-6, b16 2.6e-6, phi 0 @ 128 2.5e-6, phi 0 @ 384 2.7e-6, phi 3 @ 512 3.1e-6,
phi 1 / 2 / 4 / 5 / 6 @ 128 3.0e-6 / 2.0e-6 / 2.5e-6 / 3.2e-6 / 2.4e-6 (bound 1e-3).
test_workspace_and_gradient_writes_stay_inside_their_buffers runs every case once more through the ABI on an exact-size workspace
between two guards: a write past either end of the workspace changes a guard word (a write past one scratch array INTO the next
one does not - that shows only as a wrong gradient in the comparison above).
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _backbone_grad as G
from tests._loss_grad import TRAIN_WEIGHTS
from tests._util import CAMS, GuardedWorkspace, seeded_input
from tests._util import seeded_state_dict_once as seeded_state_dict      # the same weights serve module, oracles and checks
from tests.test_head_grads_cpu import check_against_golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "backbone_grads.npz")
FP32_PARITY_TOL = 1e-3          # README: fp32 matches the reference within 1e-3 relative to max(1, max |map|)
FP32_HEAD_TOL = 5e-4
BOUND_FACTOR, BOUND_FLOOR = 4.0, 2e-6
BACKWARD_CASES = {              # tag -> (phi, size, batch, weight seed)
    "phi0_s128_b2": (0, 128, 2, 0),
    "phi0_s256_b2": (0, 256, 2, 0),
    "phi0_s384_b1": (0, 384, 1, 0),
    "phi3_s128_b1": (3, 128, 1, 0),
    G.DROP_TAG: G.DROP_CASE,    # with the scale table stored in the golden archive
    # EfficientNet-B1, B2, B4, B5, B6: their own channel, squeeze and tap widths; B6 sits on BG_MAX_CEXP = 3456 and BG_MAX_SE = 144,
    # the sizes of the LDS arrays of the squeeze-excite kernels (phi 7 is B6 as well: tests/test_host_cpu.py)
    "phi1_s128_b1": (1, 128, 1, 0),
    "phi2_s128_b1": (2, 128, 1, 0),
    "phi4_s128_b1": (4, 128, 1, 0),
    "phi5_s128_b1": (5, 128, 1, 0),
    "phi6_s128_b1": (6, 128, 1, 0),
    "phi0_s128_b7": (0, 128, 7, 0),             # odd batch in the per-image SE sums; a 1792-row stage: 3 slabs of 608, the last 576
    "phi0_s256_b9": (0, 256, 9, 0),             # R0 = 147456: capped at BG_MAX_SLABS = 256 slabs of 576; bg_tile_rows 64; 128 SE chunks
}
LARGEST_NEW = ("phi0_s256_b9",)                 # where the smallest gradient scale must be non-zero: no tensor passes by being all zero


def _backbone(phi, seed):
    from hmd_ego_pose_amd.backbone import TrainableBackbone
    n = TrainableBackbone(phi)
    n.load_state_dict(seeded_state_dict(phi, seed), strict=False)
    return n.cuda()


def _scales(tag):
    return torch.from_numpy(np.load(GOLDEN)[f"{tag}/scales"]) if tag == G.DROP_TAG else None


def _device(bb, image, cots, image_grad=True, scales=None):
    """Through autograd: ({key: float32 numpy}, the image gradient or None, the three taps (numpy))."""
    bb.zero_grad(set_to_none=True)
    x = torch.from_numpy(image).cuda().requires_grad_(image_grad)
    taps = bb(x, None if scales is None else scales.cuda())
    sum((m * torch.from_numpy(c).cuda()).sum() for m, c in zip(taps, cots)).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.cpu().numpy() for k, p in bb.named_parameters()}
    return grads, (x.grad.cpu().numpy() if image_grad else None), [m.detach().cpu().numpy() for m in taps]


@functools.lru_cache(maxsize=None)
def _case(tag):
    phi, size, batch, seed = BACKWARD_CASES[tag]
    image, cots = G.seeded_inputs(phi, size, batch)
    scales = _scales(tag)
    bb = _backbone(phi, seed)
    grads, gimage, taps = _device(bb, image, cots, scales=scales)
    sd = seeded_state_dict(phi, seed)
    t64, g64, i64 = G.oracle_grads(sd, image, cots, phi, torch.float64, scales)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t32, g32, i32 = G.oracle_grads(sd, image, cots, phi, torch.float32, scales)
    finally:
        torch.set_num_threads(threads)
    e32 = G.group_errors(t32, i32, g32, t64, i64, g64)
    return dict(bb=bb, image=image, cots=cots, scales=scales, grads=grads, gimage=gimage, taps=taps, t64=t64, g64=g64, i64=i64, e32=e32)


def _bound(c, grp):
    return max(BOUND_FACTOR * c["e32"][grp], BOUND_FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi,size,batch", [(0, 256, 2), (0, 256, 16), (0, 128, 2), (0, 384, 2), (3, 512, 1),
                                            (1, 128, 1), (2, 128, 1), (4, 128, 1), (5, 128, 1), (6, 128, 1)])
def test_forward_matches_the_inference_session_stage_by_stage(phi, size, batch):
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd import backbone as BB
    from hmd_ego_pose_amd.arch import get_arch
    from hmd_ego_pose_amd.model import Session
    sd = seeded_state_dict(phi, 0)
    x = torch.from_numpy(seeded_input((batch, 3, size, size), 0)).cuda()
    arch = get_arch(phi)
    names = ["stem"] + [f"block{i}" for i in range(len(arch.blocks))]
    s = Session(sd, phi, size, batch, "fp32", x.device, flags=_capi.FLAG_KEEP_INTERMEDIATES)
    try:
        s.forward(x, want_features=False)
        torch.cuda.synchronize()
        want = {n: s.stage(n, batch) for n in names}
    finally:
        s.close()
    bb = _backbone(phi, 0)
    results = []
    for training_mode in (False, True):                      # running statistics in every mode, no drop-connect at rate 0
        taps = bb.train(training_mode)(x)
        torch.cuda.synchronize()
        ws = taps[0].grad_fn.saved_tensors[1]
        views = BB.stage_views(ws, phi, size, batch)
        assert set(views) == set(names)
        worst, at = 0.0, None
        for n in names:
            g, w = views[n].cpu(), want[n]
            assert g.shape == w.shape and torch.isfinite(g).all(), n
            e = (g - w).abs().max().item() / max(1.0, w.abs().max().item())
            if e > worst:
                worst, at = e, n
        for t, i in zip(taps, arch.taps):
            assert t.grad_fn is not None and t.dtype == torch.float32
            assert torch.equal(t.detach().cpu(), views[f"block{i}"].permute(0, 3, 1, 2).cpu())     # the taps ARE those stages
        print(f"phi {phi} @ {size} b{batch} train={training_mode}: backbone forward against the session, worst stage {at} {worst:.2e}")
        assert worst <= FP32_PARITY_TOL, (at, worst)
        results.append([t.detach().clone() for t in taps])
    assert all(torch.equal(a, b) for a, b in zip(*results))  # train() and eval() give identical results


@pytest.mark.parametrize("tag", list(BACKWARD_CASES))
def test_forward_and_backward_match_float64_autograd(tag):
    c = _case(tag)
    phi = BACKWARD_CASES[tag][0]
    assert set(c["grads"]) == set(c["g64"]) == {k for k, _ in G.backbone_keys(phi) if G.trainable(k)}
    dev = G.group_errors(c["taps"], c["gimage"], c["grads"], c["t64"], c["i64"], c["g64"])
    scales = {k: float(v.abs().max()) for k, v in c["g64"].items()}
    smallest = min(scales, key=scales.get)
    print(f"{tag}: smallest tensor scale {scales[smallest]:.3g} ({smallest})")
    if tag in LARGEST_NEW:
        assert scales[smallest] > 0.0, (tag, smallest)
    bad = {}
    for grp in G.GROUPS:
        e, bound = dev[grp], _bound(c, grp)
        print(f"{tag} {grp}: device {e:.3e} | float32 torch on the CPU {c['e32'][grp]:.3e} | bound {bound:.3e}")
        if not e <= bound:
            bad[grp] = (e, bound)
    if bad:                                                   # name the worst tensors of a failing group
        for k, v in c["g64"].items():
            e = G.rel_err(c["grads"][k], v.numpy())
            if e > _bound(c, G.group_of(k)):
                print(f"  {k}: {e:.3e}")
    assert not bad, (tag, bad)


@pytest.mark.parametrize("tag", list(G.GOLDEN_CASES) + [G.DROP_TAG])
def test_device_holds_the_reference_golden_slices(tag):
    """Taps, image gradient and every parameter gradient against the digests of the REAL reference's float32 autograd."""
    c = _case(tag)
    phi = BACKWARD_CASES[tag][0]
    assert BACKWARD_CASES[tag] == (G.DROP_CASE if tag == G.DROP_TAG else G.GOLDEN_CASES[tag])
    z = np.load(GOLDEN)
    names = G.golden_names(phi)
    worst = {g: 0.0 for g in G.GROUPS}
    for t, m in enumerate(c["taps"]):
        worst["taps"] = max(worst["taps"], check_against_golden(z, tag, names, f"tap.{t}", m, _bound(c, "taps"), scale=float(c["t64"][t].abs().max())))
    worst["image"] = check_against_golden(z, tag, names, "image", c["gimage"], _bound(c, "image"), scale=float(c["i64"].abs().max()))
    for k, g in c["grads"].items():
        grp = G.group_of(k)
        worst[grp] = max(worst[grp], check_against_golden(z, tag, names, "param." + k, g, _bound(c, grp), scale=float(c["g64"][k].abs().max())))
    print(f"{tag}: against the reference's golden slices, worst " + ", ".join(f"{g} {v:.3e} (bound {_bound(c, g):.3e})" for g, v in worst.items()))


def test_structure_determinism_and_the_abi_equal_the_autograd_path():
    from hmd_ego_pose_amd import backbone as BB
    tag = "phi0_s256_b2"
    phi, size, batch, seed = BACKWARD_CASES[tag]
    c = _case(tag)
    bb, image, cots, a = c["bb"], c["image"], c["cots"], c["grads"]
    assert all(b.grad is None for b in bb.buffers())           # buffers get no .grad
    b, ib, tb = _device(bb, image, cots)                       # two runs are bit-identical
    assert all(np.array_equal(a[k], b[k]) for k in a) and np.array_equal(c["gimage"], ib) and all(np.array_equal(x, y) for x, y in zip(c["taps"], tb))
    d, none, _ = _device(bb, image, cots, image_grad=False)    # NULL grad_image leaves the parameter gradients unchanged
    assert none is None and all(np.array_equal(a[k], d[k]) for k in a)
    flat = bb.flat_parameters().detach()
    x = torch.from_numpy(image).cuda()
    g = [torch.from_numpy(t).cuda() for t in cots]
    taps, ws = BB.backbone_forward(flat, x, phi)
    l = BB._capi.lib()
    g_flat = torch.full_like(flat, float("nan"))
    g_img = torch.full_like(x, float("nan"))
    stream = torch.cuda.current_stream().cuda_stream
    rc = l.hep_backbone_backward_device(flat.data_ptr(), BB._capi.ptr_array(g), None, phi, size, batch, g_flat.data_ptr(), g_img.data_ptr(),
                                        ws.data_ptr(), ws.numel(), stream)
    assert rc == 0, l.hep_last_error()
    torch.cuda.synchronize()
    total, offsets = BB.param_layout(phi)
    host = g_flat.cpu().numpy()
    assert total == flat.numel() and np.isfinite(host).all()
    for (k, shape), off in zip(BB.flat_keys(phi), offsets):
        v = host[off:off + int(np.prod(shape))].reshape(shape)
        if G.trainable(k):
            assert np.array_equal(v, a[k]), k
        else:
            assert not v.any(), k                              # running statistics: exactly zero
    assert np.array_equal(g_img.cpu().numpy(), c["gimage"]) and all(np.array_equal(t.cpu().numpy(), y) for t, y in zip(taps, c["taps"]))
    assert l.hep_backbone_backward_device(flat.data_ptr(), BB._capi.ptr_array(g), None, phi, size, batch, g_flat.data_ptr(), None,
                                          ws.data_ptr(), ws.numel() - 4, stream) == -1
    # an all-ones scale table is the NULL table, bit for bit
    ones = torch.ones((len(bb.arch.blocks), batch), device="cuda")
    e, ie, te = _device(bb, image, cots, scales=ones)
    assert all(np.array_equal(a[k], e[k]) for k in a) and np.array_equal(c["gimage"], ie) and all(np.array_equal(x, y) for x, y in zip(c["taps"], te))


@pytest.mark.parametrize("tag", list(BACKWARD_CASES))
def test_workspace_and_gradient_writes_stay_inside_their_buffers(tag):
    """The plan sizes its scratch by maxima over blocks (m_pw, m_col, m_pdw, m_pse, ...); which block sets a maximum changes with
    phi, size and batch.  One forward and one backward through the ABI on a workspace window of exactly
    hep_backbone_workspace_bytes between two guards (tests/_util.py::GuardedWorkspace), every output and gradient buffer NaN
    first: the guards keep their pattern, every value is finite, running statistics get exactly zero, all of it equal to the
    autograd path bit for bit."""
    from hmd_ego_pose_amd import backbone as BB
    phi, size, batch, seed = BACKWARD_CASES[tag]
    c = _case(tag)
    a = c["grads"]
    flat = c["bb"].flat_parameters().detach()
    x = torch.from_numpy(c["image"]).cuda()
    g = [torch.from_numpy(t).cuda() for t in c["cots"]]
    scales = None if c["scales"] is None else c["scales"].to(device="cuda", dtype=torch.float32).contiguous()
    l = BB._capi.lib()
    nbytes = BB._capi.check(l.hep_backbone_workspace_bytes(phi, size, batch))
    gw = GuardedWorkspace(nbytes, flat.device)
    taps = [torch.full(t.shape, float("nan"), device="cuda") for t in c["taps"]]
    g_flat = torch.full_like(flat, float("nan"))
    g_img = torch.full_like(x, float("nan"))
    stream = torch.cuda.current_stream().cuda_stream
    rc = l.hep_backbone_forward_device(flat.data_ptr(), x.data_ptr(), BB._capi.ptr(scales), phi, size, batch, BB._capi.ptr_array(taps), gw.ptr, nbytes, stream)
    assert rc == 0, l.hep_last_error()
    rc = l.hep_backbone_backward_device(flat.data_ptr(), BB._capi.ptr_array(g), BB._capi.ptr(scales), phi, size, batch, g_flat.data_ptr(),
                                        g_img.data_ptr(), gw.ptr, nbytes, stream)
    assert rc == 0, l.hep_last_error()
    torch.cuda.synchronize()
    assert gw.changed() == [], (tag, nbytes, gw.changed())
    host = g_flat.cpu().numpy()
    assert np.isfinite(host).all() and bool(torch.isfinite(g_img).all()) and all(bool(torch.isfinite(t).all()) for t in taps)
    total, offsets = BB.param_layout(phi)
    assert total == flat.numel()
    for (k, shape), off in zip(BB.flat_keys(phi), offsets):
        v = host[off:off + int(np.prod(shape))].reshape(shape)
        if G.trainable(k):
            assert np.array_equal(v, a[k]), k
        else:
            assert not v.any(), k                                          # running statistics: exactly zero
    assert np.array_equal(g_img.cpu().numpy(), c["gimage"]) and all(np.array_equal(t.cpu().numpy(), y) for t, y in zip(taps, c["taps"]))


def test_parameter_gradients_are_linear_in_the_cotangents():
    """Full cotangent = the sum of the three single-tap runs.  A lost consumer of a block's output shows here: a tap feeds both
    the next block and the neck."""
    tag = "phi0_s128_b2"
    c = _case(tag)
    parts = []
    for t in range(3):
        masked = [x if i == t else np.zeros_like(x) for i, x in enumerate(c["cots"])]
        parts.append(_device(c["bb"], c["image"], masked)[0])
    worst = 0.0
    for k, v in c["grads"].items():
        s = sum(p[k].astype(np.float64) for p in parts)
        e = G.rel_err(s, v)
        bound = max(_bound(c, "conv"), _bound(c, "bn_bias"))
        worst = max(worst, e)
        assert e <= bound, (k, e, bound)
    print(f"{tag}: parameter gradients against the sum of three single-tap runs, worst {worst:.3e}")
    # the cotangent of P5 alone reaches every tensor; the cotangent of P3 alone reaches nothing behind block taps[0]
    last = f"backbone_net.model._blocks.{len(c['bb'].arch.blocks) - 1}._project_conv.conv.weight"
    assert not parts[0][last].any() and parts[2][last].any()


def test_drop_connect_module_draws_only_in_train_with_a_rate_and_backward_sees_the_same_table():
    """train() + rate: the forward draws draw_branch_scale once (same seed -> same taps as the explicit table, bit for bit);
    eval() with a rate equals rate 0."""
    from hmd_ego_pose_amd.backbone import draw_branch_scale
    c = _case("phi0_s128_b2")
    bb, phi, batch = c["bb"], 0, 2
    x = torch.from_numpy(c["image"]).cuda()
    bb.drop_connect_rate = G.DROP_RATE
    try:
        with torch.no_grad():
            calm = bb.eval()(x)
            assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(calm, c["taps"]))
            for seed in range(64):                               # the first seed whose draw drops a branch
                torch.manual_seed(seed)
                table = draw_branch_scale(phi, G.DROP_RATE, batch, x.device)
                if (table == 0).any():
                    break
            assert (table == 0).any() and (table > 1).any()
            torch.manual_seed(seed)
            drawn = bb.train()(x)
            explicit = bb.eval()(x, table)
        assert all(torch.equal(a, b) for a, b in zip(drawn, explicit)) and not torch.equal(drawn[2], calm[2])
    finally:
        bb.drop_connect_rate = 0.0
        bb.eval()


def test_backbone_neck_and_heads_chained_ten_sgd_steps_lower_the_loss_and_export_serves_them():
    """image -> TrainableBackbone -> TrainableNeck -> TrainableHeads -> format_translation -> training.losses on
    training.anchor_targets -> backward -> one torch.optim.SGD over all three modules; learning-rate loop and finiteness condition
    of test_neck_and_heads_chained_ten_sgd_steps_... (a NaN rotation loss reads as a lower total)."""
    from hmd_ego_pose_amd import HMDEgoPose, TrainableBackbone, TrainableHeads, TrainableNeck, _capi, training
    phi, size, B = 0, 256, 2
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=phi, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(phi, 4), strict=True)
    m = m.cuda().eval()
    x = torch.from_numpy(seeded_input((B, 3, size, size), 31)).cuda()
    cam = torch.from_numpy(np.stack([CAMS[0]] * B)).cuda()
    n = _capi.lib().hep_anchors(size, None, None)
    anchors = np.empty((n, 4), np.float32); t_anchors = np.empty((n, 3), np.float32)
    assert _capi.lib().hep_anchors(size, anchors.ctypes.data, t_anchors.ctypes.data) == n
    rng = np.random.Generator(np.random.PCG64(8))
    boxes = [np.array([[48., 48., 176., 176.]]), np.array([[16., 16., 80., 80.], [112., 112., 240., 240.]])]
    labels = [np.zeros((len(b),), np.int32) for b in boxes]
    tr = [np.concatenate([rng.uniform(-1, 1, (len(b), 3)), rng.standard_normal((len(b), 3)) * 100 + [0, 0, 600], np.zeros((len(b), 2))], 1).astype(np.float32) for b in boxes]
    co = [rng.standard_normal((len(b), 63)).astype(np.float32) * 50 for b in boxes]
    lab, reg_t, tra_t, crd_t = training.anchor_targets(torch.from_numpy(anchors).cuda(), boxes, labels, tr, co, [(size, size)] * B, 1)
    assert (tra_t[..., -1] == 1).sum(1).min().item() > 0, "every image needs an object anchor"
    pts = (rng.standard_normal((1, 300, 3)) * 30).astype(np.float32)
    weights = torch.tensor(TRAIN_WEIGHTS, device="cuda")

    def total(bb, neck, heads):
        outs = heads(neck(bb(x)))
        reg, cls, rot, trn_raw, hand = outs
        trn = training.format_translation(trn_raw, cam, size)
        out, _per = training.losses(lab, cls, reg_t, reg, tra_t, torch.cat((rot, trn), dim=2), crd_t, hand, pts, 3)
        return (out * weights).sum(), all(bool(torch.isfinite(o).all()) for o in outs)

    def steps(lr, count):
        mods = (TrainableBackbone.from_model(m).train(), TrainableNeck.from_model(m).train(), TrainableHeads.from_model(m).train())
        opt = torch.optim.SGD([p for mod in mods for p in mod.parameters()], lr=lr)
        values, finite = [], True
        for _ in range(count):
            opt.zero_grad(set_to_none=True)
            loss, ok = total(*mods)
            loss.backward()
            opt.step()
            values.append(float(loss.detach()))
            finite &= ok
        with torch.no_grad():
            loss, ok = total(*mods)
        return mods, values + [float(loss)], finite and ok

    lr = 1e-3
    while True:
        mods, values, finite = steps(lr, 10)
        print(f"lr {lr:g}: finite {finite}, weighted total over ten SGD steps {['%.6g' % t for t in values]}")
        assert np.isfinite(values[0]), values
        if finite and all(b < a for a, b in zip(values, values[1:])):
            break
        lr /= 2
        assert lr > 1e-7, "no learning rate down to 1e-7 gives ten descending steps: the gradient is not a descent direction"
    assert np.isfinite(values).all() and values[-1] < values[0], values
    ref = m.state_dict()
    for mod in mods:
        sd = mod.state_dict()
        assert all(torch.equal(v, ref[k]) for k, v in sd.items() if "running" in k or "num_batches" in k)     # statistics never change
        assert any(not torch.equal(v, ref[k]) for k, v in sd.items() if "running" not in k and v.dtype == torch.float32)
    bb, neck, heads = mods
    with torch.no_grad():
        want_maps = neck(bb(x))
        want = heads(want_maps)
    for mod in mods:
        mod.export_to(m)
    got = m(x)
    for l, (g, w) in enumerate(zip(got[0], want_maps)):
        err = (g - w).abs().max().item() / max(1.0, w.abs().max().item())
        assert err <= FP32_PARITY_TOL, (l, err)
    for g, w in zip(got[1:], want):
        err = (g - w).abs().max().item() / max(1.0, w.abs().max().item())
        assert err <= FP32_HEAD_TOL, err


def test_the_image_is_validated_before_the_abi_sees_a_pointer():
    from hmd_ego_pose_amd.backbone import TrainableBackbone
    bb = _backbone(0, 0)
    good = torch.zeros((2, 3, 128, 128), device="cuda")
    taps = bb(good)
    assert [tuple(t.shape) for t in taps] == [(2, 40, 16, 16), (2, 112, 8, 8), (2, 320, 4, 4)]
    for bad in (good.double(),                                   # dtype
                good.cpu(),                                      # device
                good[0],                                         # rank
                torch.zeros((2, 4, 128, 128), device="cuda"),    # channel count
                torch.zeros((2, 3, 200, 200), device="cuda"),    # size 200
                torch.zeros((2, 3, 128, 256), device="cuda")):   # not square
        with pytest.raises(ValueError):
            bb(bad)
    with pytest.raises(ValueError):
        bb(good, torch.ones((3, 2), device="cuda"))              # a scale table of the wrong shape
    with pytest.raises(ValueError):
        TrainableBackbone(8)
    with pytest.raises(ValueError):
        TrainableBackbone(0).forward(good)                       # the module on the CPU, the image on the device
