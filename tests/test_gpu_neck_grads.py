"""GPU (MI355X): the trainable BiFPN neck - hep_neck_forward_device / hep_neck_backward_device (csrc/k_neck_grad.hip) behind
hmd_ego_pose_amd.neck.TrainableNeck.

Forward: against the fp32 inference session on the session's OWN taps, the project's fp32 parity bound 1e-3.
Backward: against the oracle's float64 autograd with TEACHER-FORCED max-pool routing: the device's argmax of every pool window
(read from the workspace through hep_neck_stage_info, first maximum in row-major order of the zero-padded window) replaces
maxpool_same in the oracle, so both route alike; legitimacy of that routing: in every window the oracle's value at the device's
position is within G = 4e-5 * max(1, max |pool input|) of the oracle's true maximum.  Per group (maps forward; tap gradients;
conv / lateral / BatchNorm gradients per tensor; fusion gradients on one common scale) the device's worst error must be within
BOUND_FACTOR = 4 times the worst error of the SAME routed oracle evaluated in float32 on the CPU (one thread), floor 2e-6 - the
rule of tests/test_gpu_head_grads.py.  The tests print device / CPU-float32 / bound per group.

Measured on MI355X (device | float32 torch on the CPU | bound; NOTEBOOK.md section 13):
                 maps forward               tap gradients              conv / BatchNorm           fusion (common scale)
  phi0_s256_b2   1.36e-6 | 8.95e-7 | 3.58e-6   1.38e-6 | 1.51e-6 | 6.04e-6   2.77e-6 | 2.42e-6 | 9.69e-6   4.86e-7 | 2.70e-7 | 2.00e-6
  phi0_s128_b2   5.82e-7 | 5.52e-7 | 2.21e-6   6.92e-7 | 7.41e-7 | 2.96e-6   1.75e-6 | 1.72e-6 | 6.87e-6   1.43e-6 | 6.60e-7 | 2.64e-6
  phi0_s384_b1   1.27e-6 | 1.14e-6 | 4.56e-6   1.57e-6 | 1.50e-6 | 5.99e-6   2.54e-6 | 3.29e-6 | 1.32e-5   1.87e-6 | 1.76e-6 | 7.04e-6
  phi3_s128_b1   3.81e-7 | 4.36e-7 | 2.00e-6   1.24e-6 | 1.31e-6 | 5.25e-6   2.09e-6 | 2.79e-6 | 1.12e-5   4.81e-7 | 2.58e-7 | 2.00e-6
  phi1_s128_b1   1.15e-6 | 1.19e-6 | 4.76e-6   9.41e-7 | 9.75e-7 | 3.90e-6   1.91e-6 | 1.94e-6 | 7.77e-6   7.38e-7 | 2.09e-6 | 8.37e-6
  phi2_s128_b1   9.22e-7 | 9.87e-7 | 3.95e-6   1.21e-6 | 1.20e-6 | 4.81e-6   2.16e-6 | 2.14e-6 | 8.55e-6   3.93e-7 | 4.20e-7 | 2.00e-6
  phi4_s128_b1   6.54e-7 | 6.04e-7 | 2.42e-6   1.44e-6 | 1.05e-6 | 4.19e-6   2.70e-6 | 2.67e-6 | 1.07e-5   1.05e-6 | 3.64e-7 | 2.00e-6
  phi5_s128_b1   9.49e-7 | 6.58e-7 | 2.63e-6   1.32e-6 | 1.05e-6 | 4.20e-6   2.75e-6 | 2.05e-6 | 8.20e-6   1.98e-6 | 1.14e-6 | 4.54e-6
  phi0_s128_b7   5.64e-7 | 5.67e-7 | 2.27e-6   6.55e-7 | 6.57e-7 | 2.63e-6   2.14e-6 | 3.29e-6 | 1.32e-5   1.65e-6 | 1.11e-6 | 4.43e-6
  phi0_s256_b17  7.79e-7 | 7.51e-7 | 3.00e-6   8.75e-7 | 7.95e-7 | 3.18e-6   1.27e-6 | 6.53e-6 | 2.61e-5   5.18e-7 | 5.94e-7 | 2.38e-6
The last six (NOTEBOOK.md section 16) use weight seed 4: with seed 0, at every phi, two relu-dead fusion entries leave the whole
p5_down_channel lateral and conv6_up of cell 2 with a gradient that is identically zero, so those tensors pass by being zero;
with seed 4 every convolution, lateral and BatchNorm tensor has a gradient (smallest max |g64| 0.03 .. 14) and the test asserts it.
Legitimacy slack 0 and no window routed unlike the float64 oracle's own in the first four cases and in five of the new ones; one
window each at phi5_s128_b1 (slack 4.3e-8) and phi0_s256_b17 (1.7e-8), no window excluded.  Forward against the session (worst map):
phi 0 @ 256 b2 4.4e-6, b16 2.9e-6, phi 0 @ 128 1.0e-6, phi 0 @ 384 2.6e-6, phi 3 @ 512 7.8e-6, phi 1 / 2 / 4 / 5 @ 128 1.7e-6 / 8.9e-7 /
6.1e-7 / 1.2e-6 (bound 1e-3).
test_workspace_and_gradient_writes_stay_inside_their_buffers runs every case once more through the ABI on an exact-size workspace
between two guards: a write past either end of the workspace changes a guard word (a write past one scratch array INTO the next
one does not - that shows only as a wrong gradient in the comparison above).
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _neck_grad as N
from tests._loss_grad import TRAIN_WEIGHTS
from tests._util import CAMS, GuardedWorkspace, seeded_input
from tests._util import seeded_state_dict_once as seeded_state_dict      # the same weights serve module, oracles and checks
from tests.test_head_grads_cpu import check_against_golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FP32_PARITY_TOL = 1e-3          # README: fp32 matches the reference within 1e-3 relative to max(1, max |map|)
FP32_HEAD_TOL = 5e-4
BOUND_FACTOR, BOUND_FLOOR = 4.0, 2e-6
LEGIT = 4e-5                    # twice FP32_STAGE_TOL (tests/test_gpu_parity.py): two elements are compared
BACKWARD_CASES = {              # tag -> (phi, size, batch, weight seed)
    "phi0_s256_b2": (0, 256, 2, 0),
    "phi0_s128_b2": (0, 128, 2, 0),
    "phi0_s384_b1": (0, 384, 1, 0),
    "phi3_s128_b1": (3, 128, 1, 0),
    # every remaining width (88, 112, 224, 288) with 4 / 5 / 7 / 7 cells; the lateral products run over the tap channels of B1..B5.
    # Weight seed LIVE_SEED: with seed 0 the fusion entries bifpn.0.p5_w1[0] and bifpn.2.p6_w1[0] are relu-dead at every phi (the
    # seeded weights are keyed by tensor name), so the whole p5_down_channel lateral and conv6_up of cell 2 have a zero gradient
    # and pass by being zero; seed 4 leaves no convolution, lateral or BatchNorm tensor without a gradient at phi 0..5.
    "phi1_s128_b1": (1, 128, 1, 4),
    "phi2_s128_b1": (2, 128, 1, 4),
    "phi4_s128_b1": (4, 128, 1, 4),
    "phi5_s128_b1": (5, 128, 1, 4),
    "phi0_s128_b7": (0, 128, 7, 4),             # odd batch: R[0] = 1792, 3 slabs of 608, the last 576; 7 rows at P7
    "phi0_s256_b17": (0, 256, 17, 4),           # R[0] = 17408: capped at NG_MAX_SLABS = 32 slabs of 544
}
LIVE_SEED = 4                                   # the cases where the smallest gradient scale is asserted non-zero


def _neck(phi, seed):
    from hmd_ego_pose_amd.neck import TrainableNeck
    n = TrainableNeck(phi)
    n.load_state_dict(seeded_state_dict(phi, seed), strict=False)
    return n.cuda()


def _device(neck, taps, cots, taps_grad=True):
    """Through autograd: ({key: float32 numpy}, [three tap gradients] or None, the five maps (numpy), the device's argmax of
    every pool window in pool_names order)."""
    from hmd_ego_pose_amd import neck as NK
    neck.zero_grad(set_to_none=True)
    x = [torch.from_numpy(a).cuda().requires_grad_(taps_grad) for a in taps]
    maps = neck(x)
    ws = maps[0].grad_fn.saved_tensors[1]
    phi, size, batch = neck.compound_coef, taps[0].shape[2] * 8, taps[0].shape[0]
    views = NK.stage_views(ws, phi, size, batch)
    argmax = [N.first_argmax(views[name].permute(0, 3, 1, 2)).cpu() for name in N.pool_names(phi)]
    if cots is not None:
        sum((m * torch.from_numpy(c).cuda()).sum() for m, c in zip(maps, cots)).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.cpu().numpy() for k, p in neck.named_parameters()} if cots is not None else None
    gtaps = [a.grad.cpu().numpy() for a in x] if (taps_grad and cots is not None) else None
    return grads, gtaps, [m.detach().cpu().numpy() for m in maps], argmax


def _routed_oracle(phi, size, batch, seed, argmax):
    """float64 and float32 (CPU, one thread) oracle with the device's routing; returns (maps64, grads64, taps64, the float32
    evaluation's group errors, the float64 pool's slack and scale lists)."""
    sd = seeded_state_dict(phi, seed)
    taps, cots = N.seeded_inputs(phi, size, batch)
    p64 = N.RoutedPool(argmax)
    m64, g64, t64 = N.oracle_grads(sd, taps, cots, phi, torch.float64, p64)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        m32, g32, t32 = N.oracle_grads(sd, taps, cots, phi, torch.float32, N.RoutedPool(argmax))
    finally:
        torch.set_num_threads(threads)
    return m64, g64, t64, N.group_errors(m32, t32, g32, m64, t64, g64), p64


@functools.lru_cache(maxsize=None)
def _case(tag):
    phi, size, batch, seed = BACKWARD_CASES[tag]
    taps, cots = N.seeded_inputs(phi, size, batch)
    neck = _neck(phi, seed)
    grads, gtaps, maps, argmax = _device(neck, taps, cots)
    m64, g64, t64, e32, pool = _routed_oracle(phi, size, batch, seed, argmax)
    return dict(neck=neck, taps=taps, cots=cots, grads=grads, gtaps=gtaps, maps=maps, argmax=argmax, m64=m64, g64=g64, t64=t64, e32=e32, pool=pool)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi,size,batch", [(0, 256, 2), (0, 256, 16), (0, 128, 2), (0, 384, 2), (3, 512, 1),
                                            (1, 128, 1), (2, 128, 1), (4, 128, 1), (5, 128, 1)])
def test_forward_matches_the_inference_session_on_its_own_taps(phi, size, batch):
    from hmd_ego_pose_amd.model import HMDEgoPose
    from hmd_ego_pose_amd.neck import TrainableNeck, backbone_taps
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=phi, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(phi, 0), strict=True)
    m = m.cuda().eval()
    x = torch.from_numpy(seeded_input((batch, 3, size, size), 0)).cuda()
    want = m(x)[0]
    taps = backbone_taps(m, x)
    neck = TrainableNeck.from_model(m)
    for training_mode in (False, True):                      # running statistics in every mode
        got = neck.train(training_mode)(taps)
        torch.cuda.synchronize()
        errs = []
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.grad_fn is not None and torch.isfinite(g).all()
            errs.append((g.detach() - w).abs().max().item() / max(1.0, w.abs().max().item()))
        print(f"phi {phi} @ {size} b{batch}: neck forward against the session, per map {['%.2e' % e for e in errs]}")
        assert max(errs) <= FP32_PARITY_TOL, errs


@pytest.mark.parametrize("tag", list(BACKWARD_CASES))
def test_forward_and_backward_match_float64_autograd_with_the_devices_routing(tag):
    c = _case(tag)
    phi = BACKWARD_CASES[tag][0]
    assert set(c["grads"]) == set(c["g64"]) == {k for k, _ in N.neck_keys(phi) if N.trainable(k)}
    # legitimacy of the routing: a condition on every window of every pool
    for name, slack, scale in zip(N.pool_names(phi), c["pool"].slack, c["pool"].scale):
        assert slack <= LEGIT * max(1.0, scale), (name, slack, scale)
    flips = sum(int((a != b).sum()) for a, b in zip(c["argmax"], c["pool"].own))
    dev = N.group_errors(c["maps"], c["gtaps"], c["grads"], c["m64"], c["t64"], c["g64"])
    # no tensor passes by being all zero: every trainable tensor that is not a fusion weight has a non-zero float64 gradient
    # (a fusion weight the seed left at or below zero is relu-dead: its gradient IS zero, asserted exactly below)
    scales = {k: float(v.abs().max()) for k, v in c["g64"].items() if not N.is_fusion(k)}
    smallest = min(scales, key=scales.get)
    print(f"{tag}: worst legitimacy slack {max(c['pool'].slack):.3e}; windows routed unlike the float64 oracle's own {flips}; "
          f"smallest tensor scale {scales[smallest]:.3g} ({smallest})")
    if BACKWARD_CASES[tag][3] == LIVE_SEED:
        assert scales[smallest] > 0.0, (tag, smallest)
    bad = {}
    for grp, e in dev.items():
        bound = max(BOUND_FACTOR * c["e32"][grp], BOUND_FLOOR)
        print(f"{tag} {grp}: device {e:.3e} | float32 torch on the CPU {c['e32'][grp]:.3e} | bound {bound:.3e}")
        if not e <= bound:
            bad[grp] = (e, bound)
    assert not bad, (tag, bad)
    sd = seeded_state_dict(phi, BACKWARD_CASES[tag][3])
    for k, v in c["g64"].items():                            # dead fusion entries: exactly zero
        if N.is_fusion(k):
            p = sd[k].numpy()
            assert not c["grads"][k][p <= 0].any(), k


@pytest.mark.parametrize("tag", list(N.GOLDEN_CASES))
def test_device_holds_the_reference_golden_slices(tag):
    """The five maps against the real reference's (tests/golden/neck_grads.npz; continuous in the routing); the gradients as well
    when no window is routed unlike the float64 oracle's own - otherwise they are pinned through reference -> oracle (CPU test)
    -> device (routed comparison).  Prints which path it took."""
    assert BACKWARD_CASES[tag] == N.GOLDEN_CASES[tag]
    c = _case(tag)
    phi = BACKWARD_CASES[tag][0]
    z = np.load(os.path.join(HERE, "golden", "neck_grads.npz"))
    names = N.golden_names(phi)
    bound = lambda grp: max(BOUND_FACTOR * c["e32"][grp], BOUND_FLOOR)
    worst = max(check_against_golden(z, tag, names, f"map.{l}", m, bound("maps"), scale=float(np.abs(c["m64"][l].numpy()).max())) for l, m in enumerate(c["maps"]))
    flips = sum(int((a != b).sum()) for a, b in zip(c["argmax"], c["pool"].own))
    print(f"{tag}: maps against the reference's golden slices, worst {worst:.3e} (bound {bound('maps'):.3e}); {flips} windows routed unlike the float64 oracle")
    if flips:
        print(f"{tag}: gradients NOT compared with the golden slices ({flips} routing differences); pinned through the routed comparison")
        return
    fscale = max(float(np.abs(v.numpy()).max()) for k, v in c["g64"].items() if N.is_fusion(k))
    for t, g in enumerate(c["gtaps"]):
        check_against_golden(z, tag, names, f"tap.{t}", g, bound("taps"), scale=float(np.abs(c["t64"][t].numpy()).max()))
    for k, g in c["grads"].items():
        if N.is_fusion(k):                                   # on the case's common fusion scale (tests/test_neck_grads_cpu.py)
            _shape, (s, sa), sl = N.golden_entry(z, tag, names, "param." + k)
            a = g.astype(np.float64).reshape(-1)
            errs = [float(np.abs(a[::N.digest_stride(a.size)] - sl).max()), abs(a.sum() - s) / a.size, abs(np.abs(a).sum() - sa) / a.size]
            assert max(errs) <= bound("fusion") * fscale, (k, errs, fscale)
            continue
        scale = float(np.abs(c["g64"][k].numpy()).max())
        if scale == 0.0:
            assert not g.any(), k
            continue
        check_against_golden(z, tag, names, "param." + k, g, bound("conv_bn"), scale=scale)
    print(f"{tag}: every gradient compared with the golden slices")


def test_structure_determinism_and_the_abi_equal_the_autograd_path():
    from hmd_ego_pose_amd import neck as NK
    phi, size, batch, seed = BACKWARD_CASES["phi0_s256_b2"]
    c = _case("phi0_s256_b2")
    neck, taps, cots, a = c["neck"], c["taps"], c["cots"], c["grads"]
    assert all(b.grad is None for b in neck.buffers())
    b, tb, _, _ = _device(neck, taps, cots)
    assert all(np.array_equal(a[k], b[k]) for k in a) and all(np.array_equal(x, y) for x, y in zip(c["gtaps"], tb))
    d, none, _, _ = _device(neck, taps, cots, taps_grad=False)           # NULL grad_taps
    assert none is None and all(np.array_equal(a[k], d[k]) for k in a)
    flat = neck.flat_parameters().detach()
    x = [torch.from_numpy(t).cuda() for t in taps]
    g = [torch.from_numpy(t).cuda() for t in cots]
    feats, ws = NK.neck_forward(flat, x, phi, size)
    l = NK._capi.lib()
    g_flat = torch.full_like(flat, float("nan"))
    g_taps = [torch.full_like(t, float("nan")) for t in x]
    stream = torch.cuda.current_stream().cuda_stream
    rc = l.hep_neck_backward_device(flat.data_ptr(), NK._capi.ptr_array(g), phi, size, batch, g_flat.data_ptr(), NK._capi.ptr_array(g_taps),
                                    ws.data_ptr(), ws.numel(), stream)
    assert rc == 0, l.hep_last_error()
    torch.cuda.synchronize()
    total, offsets = NK.param_layout(phi)
    host = g_flat.cpu().numpy()
    assert total == flat.numel() and np.isfinite(host).all()
    for (k, shape), off in zip(NK.flat_keys(phi), offsets):
        v = host[off:off + int(np.prod(shape))].reshape(shape)
        if N.trainable(k):
            assert np.array_equal(v, a[k]), k
        else:
            assert not v.any(), k                                          # running statistics: exactly zero
    assert all(np.array_equal(t.cpu().numpy(), y) for t, y in zip(g_taps, c["gtaps"]))
    assert l.hep_neck_backward_device(flat.data_ptr(), NK._capi.ptr_array(g), phi, size, batch, g_flat.data_ptr(), None,
                                      ws.data_ptr(), ws.numel() - 4, stream) == -1


@pytest.mark.parametrize("tag", list(BACKWARD_CASES))
def test_workspace_and_gradient_writes_stay_inside_their_buffers(tag):
    """The plan sizes its scratch by maxima over levels and laterals (o_pw = NG_MAX_SLABS * W * kmax, ...); which one sets a
    maximum changes with phi, size and batch.  One forward and one backward through the ABI on a workspace window of exactly
    hep_neck_workspace_bytes between two guards (tests/_util.py::GuardedWorkspace), every output and gradient buffer NaN first:
    the guards keep their pattern, every value is finite, running statistics get exactly zero, all of it equal to the autograd
    path bit for bit."""
    from hmd_ego_pose_amd import neck as NK
    phi, size, batch, seed = BACKWARD_CASES[tag]
    c = _case(tag)
    a = c["grads"]
    flat = c["neck"].flat_parameters().detach()
    x = [torch.from_numpy(t).cuda() for t in c["taps"]]
    g = [torch.from_numpy(t).cuda() for t in c["cots"]]
    l = NK._capi.lib()
    nbytes = NK._capi.check(l.hep_neck_workspace_bytes(phi, size, batch))
    gw = GuardedWorkspace(nbytes, flat.device)
    maps = [torch.full(m.shape, float("nan"), device="cuda") for m in c["maps"]]
    g_flat = torch.full_like(flat, float("nan"))
    g_taps = [torch.full_like(t, float("nan")) for t in x]
    stream = torch.cuda.current_stream().cuda_stream
    rc = l.hep_neck_forward_device(flat.data_ptr(), NK._capi.ptr_array(x), phi, size, batch, NK._capi.ptr_array(maps), gw.ptr, nbytes, stream)
    assert rc == 0, l.hep_last_error()
    rc = l.hep_neck_backward_device(flat.data_ptr(), NK._capi.ptr_array(g), phi, size, batch, g_flat.data_ptr(), NK._capi.ptr_array(g_taps),
                                    gw.ptr, nbytes, stream)
    assert rc == 0, l.hep_last_error()
    torch.cuda.synchronize()
    assert gw.changed() == [], (tag, nbytes, gw.changed())
    host = g_flat.cpu().numpy()
    assert np.isfinite(host).all() and all(bool(torch.isfinite(t).all()) for t in g_taps + maps)
    total, offsets = NK.param_layout(phi)
    assert total == flat.numel()
    for (k, shape), off in zip(NK.flat_keys(phi), offsets):
        v = host[off:off + int(np.prod(shape))].reshape(shape)
        if N.trainable(k):
            assert np.array_equal(v, a[k]), k
        else:
            assert not v.any(), k                                          # running statistics: exactly zero
    assert all(np.array_equal(t.cpu().numpy(), y) for t, y in zip(g_taps, c["gtaps"]))
    assert all(np.array_equal(m.cpu().numpy(), y) for m, y in zip(maps, c["maps"]))


def test_parameter_gradients_are_linear_in_the_cotangents():
    """Full cotangent = the sum of the five single-level runs (a lost consumer in the gather-form accumulation shows here)."""
    tag = "phi0_s128_b2"
    c = _case(tag)
    parts = []
    for l in range(5):
        masked = [x if i == l else np.zeros_like(x) for i, x in enumerate(c["cots"])]
        parts.append(_device(c["neck"], c["taps"], masked)[0])
    fscale = max(float(np.abs(v).max()) for k, v in c["grads"].items() if N.is_fusion(k))
    worst = 0.0
    for k, v in c["grads"].items():
        fus = N.is_fusion(k)
        s = sum(p[k].astype(np.float64) for p in parts)
        e = float(np.abs(s - v).max()) / fscale if fus else N.rel_err(s, v)
        bound = max(BOUND_FACTOR * c["e32"]["fusion" if fus else "conv_bn"], BOUND_FLOOR)
        worst = max(worst, e)
        assert e <= bound, (k, e, bound)
    print(f"{tag}: parameter gradients against the sum of five single-level runs, worst {worst:.3e}")


def test_neck_and_heads_chained_ten_sgd_steps_lower_the_loss_and_export_serves_them():
    """taps -> TrainableNeck -> TrainableHeads -> format_translation -> training.losses on training.anchor_targets -> backward ->
    one torch.optim.SGD over both modules; learning-rate loop and finiteness condition of
    test_ten_sgd_steps_on_the_device_lower_the_training_loss_and_export_serves_them (a NaN rotation loss reads as a lower total)."""
    from hmd_ego_pose_amd import HMDEgoPose, TrainableHeads, _capi, training
    from hmd_ego_pose_amd.neck import TrainableNeck, backbone_taps
    phi, size, B = 0, 256, 2
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=phi, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(phi, 4), strict=True)
    m = m.cuda().eval()
    x = torch.from_numpy(seeded_input((B, 3, size, size), 31)).cuda()
    cam = torch.from_numpy(np.stack([CAMS[0]] * B)).cuda()
    taps = backbone_taps(m, x)
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

    def total(neck, heads):
        outs = heads(neck(taps))
        reg, cls, rot, trn_raw, hand = outs
        trn = training.format_translation(trn_raw, cam, size)
        out, _per = training.losses(lab, cls, reg_t, reg, tra_t, torch.cat((rot, trn), dim=2), crd_t, hand, pts, 3)
        return (out * weights).sum(), all(bool(torch.isfinite(o).all()) for o in outs)

    def steps(lr, count):
        neck, heads = TrainableNeck.from_model(m).train(), TrainableHeads.from_model(m).train()
        opt = torch.optim.SGD(list(neck.parameters()) + list(heads.parameters()), lr=lr)
        values, finite = [], True
        for _ in range(count):
            opt.zero_grad(set_to_none=True)
            loss, ok = total(neck, heads)
            loss.backward()
            opt.step()
            values.append(float(loss.detach()))
            finite &= ok
        with torch.no_grad():
            loss, ok = total(neck, heads)
        return neck, heads, values + [float(loss)], finite and ok

    lr = 1e-3
    while True:
        neck, heads, values, finite = steps(lr, 10)
        print(f"lr {lr:g}: finite {finite}, weighted total over ten SGD steps {['%.6g' % t for t in values]}")
        assert np.isfinite(values[0]), values
        if finite and all(b < a for a, b in zip(values, values[1:])):
            break
        lr /= 2
        assert lr > 1e-7, "no learning rate down to 1e-7 gives ten descending steps: the gradient is not a descent direction"
    assert np.isfinite(values).all() and values[-1] < values[0], values
    ref = m.state_dict()
    for mod in (neck, heads):
        sd = mod.state_dict()
        assert all(torch.equal(v, ref[k]) for k, v in sd.items() if "running" in k)                # statistics never change
        assert any(not torch.equal(v, ref[k]) for k, v in sd.items() if "running" not in k and v.dtype == torch.float32)
    with torch.no_grad():
        want_maps = neck(taps)
        want = heads(want_maps)
    neck.export_to(m)
    heads.export_to(m)
    got = m(x)
    for l, (g, w) in enumerate(zip(got[0], want_maps)):
        err = (g - w).abs().max().item() / max(1.0, w.abs().max().item())
        assert err <= FP32_PARITY_TOL, (l, err)
    for g, w in zip(got[1:], want):
        err = (g - w).abs().max().item() / max(1.0, w.abs().max().item())
        assert err <= FP32_HEAD_TOL, err


def test_taps_are_validated_before_the_abi_sees_a_pointer():
    from hmd_ego_pose_amd.neck import TrainableNeck
    neck = _neck(0, 0)
    good = [torch.zeros((2, c, s, s), device="cuda") for c, s in ((40, 32), (112, 16), (320, 8))]
    assert neck(good)[0].shape == (2, 64, 32, 32)
    for i, shape in ((1, (2, 112, 15, 16)), (2, (2, 320, 4, 4)), (0, (2, 48, 32, 32)), (1, (1, 112, 16, 16)), (2, (2, 320, 8))):
        bad = list(good)
        bad[i] = torch.zeros(shape, device="cuda")
        with pytest.raises(ValueError):
            neck(bad)
    with pytest.raises(ValueError):
        neck(good[:2])
    with pytest.raises(ValueError):
        neck([g.double() for g in good])
    with pytest.raises(ValueError):
        neck([torch.zeros((2, c, s, s), device="cuda") for c, s in ((40, 25), (112, 13), (320, 7))])      # size 200
    with pytest.raises(ValueError):
        neck([g.cpu() for g in good])
    with pytest.raises(ValueError):
        TrainableNeck(6)
