"""GPU (MI355X): batch-statistics BatchNorm of the three trainable parts - ``batch_norm="batch"`` of TrainableHeads / TrainableNeck /
TrainableBackbone over hep_{heads,neck,backbone}_{forward,backward}_device_bn (the shared passes of csrc/grad_dev.h).

Reference: float64 autograd of the oracle with its one BatchNorm function replaced by ``F.batch_norm(training=True, 0.01, 1e-3)``
(tests/_bn_batch.py; pinned to the real reference in train() by tests/test_bn_batch_cpu.py).  Per tensor
e = max |g - g64| / max |g64|.  The bound is measured, not fixed (the rule of tests/test_gpu_head_grads.py): the same patched oracle
runs in float32 on the CPU with one thread, its worst e per group is e32, the device gets 4 x e32, floor 2e-6.  Groups: outputs;
gradients (input gradients and every trainable tensor that is neither analytically zero nor a fusion scalar); the neck's fusion
scalars on one common scale (tests/_neck_grad.py).  The analytically zero tensors (tests/test_bn_batch_cpu.py) are bounded apart:
max |g_dev| <= 4 x the largest max |g32_cpu| over that set - the device writes exact zeros there.  The neck feeds the device's
max-pool argmax to the oracle (teacher-forced routing, tests/test_gpu_neck_grads.py).  The updated running statistics: 4 x the
float32 CPU oracle's error per buffer kind.  Every gradient case has >= 8 rows at every BatchNorm; 2 rows (P7 at size 128,
batch 2) is ill-conditioned and gets a forward-only check, 1 row is refused.

Measured on MI355X (device | float32 torch on the CPU | bound), see NOTEBOOK.md section 18; the tests print the values they reach:
                              outputs                       gradients                     zero set (tensors: device, CPU float32 max |g|)
  heads phi0_s128_b8          6.0e-7 | 6.7e-7 | 2.7e-6      1.65e-6 | 2.01e-6 | 8.0e-6    15: 0, 1.7e-4
  heads phi0_s256_b2          4.9e-7 | 5.1e-7 | 2.0e-6      1.24e-6 | 1.54e-6 | 6.1e-6    15: 0, 2.8e-4
  heads phi3_s128_b8          8.4e-7 | 8.4e-7 | 3.4e-6      2.33e-6 | 2.38e-6 | 9.5e-6    20: 0, 2.2e-4
  neck phi0_s128_b8           2.5e-6 | 3.0e-6 | 1.2e-5      5.24e-6 | 3.29e-6 | 1.3e-5    30: 0, 1.5e-4     fusion 7.4e-7 | 1.5e-6 | 6.1e-6
  neck phi0_s256_b2           1.8e-6 | 1.1e-6 | 4.6e-6      2.98e-6 | 2.23e-6 | 8.9e-6    30: 0, 7.6e-5     fusion 7.6e-7 | 8.7e-7 | 3.5e-6
  neck phi3_s128_b8           8.1e-6 | 4.7e-6 | 1.9e-5      1.32e-5 | 1.01e-5 | 4.0e-5    54: 0, 2.4e-4     fusion 4.2e-6 | 3.7e-6 | 1.5e-5
  backbone phi0_s128_b2       6.1e-6 | 5.8e-6 | 2.3e-5      1.65e-5 | 1.53e-5 | 6.1e-5    10: 1.5e-4, 4.0e-4
  backbone phi3_s128_b1       1.4e-5 | 1.4e-5 | 5.8e-5      5.21e-5 | 7.68e-5 | 3.1e-4    15: 2.9e-4, 5.2e-4
  backbone ..b2_dropconnect   6.2e-6 | 5.2e-6 | 2.1e-5      2.95e-5 | 1.63e-5 | 6.5e-5     9: 1.4e-4, 3.5e-4
Running statistics after one train() forward (device | CPU float32): heads 5.5e-8 | 1.1e-7 (mean), 4.2e-8 | 8.8e-8 (var); neck 5.6e-8 |
1.1e-7, 5.3e-8 | 8.7e-8; backbone phi 0 8.0e-8 | 8.4e-8, 3.6e-7 | 3.1e-7; phi 3 3.2e-7 | 2.9e-7, 1.8e-6 | 1.5e-6.  Two rows at P7, outputs:
heads 5.6e-7 | 5.6e-7 | 2.3e-6, neck 2.0e-5 | 2.5e-5 | 9.8e-5.  Composed step: outputs 2.1e-5 | 1.8e-5 | 7.0e-5, gradients 2.3e-5 | 1.3e-5 | 5.1e-5.
Neck routing: no window routed unlike the float64 oracle's own at phi 0, one at phi 3 (legitimacy slack 6.8e-7).
"""
import functools

import numpy as np
import pytest
import torch

from tests import _backbone_grad as G
from tests import _bn_batch as BB
from tests import _head_grad as H
from tests import _neck_grad as N
from tests._util import GuardedWorkspace
from tests._util import seeded_state_dict_once as seeded_state_dict

pytestmark = pytest.mark.gpu

ALL_CASES = [(part, tag) for part in BB.PARTS for tag in BB.CASES[part]]
IDS = [f"{part}-{tag}" for part, tag in ALL_CASES]


def _module(part, case, batch_norm="batch", sd=None):
    from hmd_ego_pose_amd import TrainableHeads
    from hmd_ego_pose_amd.backbone import TrainableBackbone
    from hmd_ego_pose_amd.neck import TrainableNeck
    phi, _size, _batch, seed, classes, _drop = case
    kw = {} if batch_norm is None else {"batch_norm": batch_norm}
    m = TrainableHeads(phi, classes, **kw) if part == "heads" else TrainableNeck(phi, **kw) if part == "neck" else TrainableBackbone(phi, **kw)
    m.load_state_dict(sd if sd is not None else seeded_state_dict(phi, seed, num_classes=classes or 1), strict=False)
    return m.cuda()


def _buffers(m):
    return {k: b.detach().clone() for k, b in m.named_buffers()}


def _neck_argmax(neck, maps, case):
    """The device's argmax of every pool window, in pool_names order, from the workspace of the forward that made ``maps``."""
    from hmd_ego_pose_amd import neck as NK
    phi, size, batch = case[0], case[1], case[2]
    views = NK.stage_views(maps[0].grad_fn.saved_tensors[1], phi, size, batch)
    return [N.first_argmax(views[name].permute(0, 3, 1, 2)).cpu() for name in N.pool_names(phi)]


def _run(part, m, case, backward=True):
    """One forward (+ backward) through autograd: dict(outs, grads, gin, argmax) of device tensors; the module's buffers as they
    are afterwards stay with the module."""
    x_np, cots_np = BB.inputs(part, case)
    m.zero_grad(set_to_none=True)
    xs = [torch.from_numpy(a).cuda().requires_grad_(backward) for a in x_np]
    if part == "backbone":
        sc = BB.scales_of(part, case)
        outs = m(xs[0], None if sc is None else sc.cuda())
    else:
        outs = m(xs)
    argmax = _neck_argmax(m, outs, case) if part == "neck" and outs[0].grad_fn is not None else None
    res = dict(outs=[o.detach() for o in outs], argmax=argmax)
    if backward:
        sum((o * torch.from_numpy(c).cuda()).sum() for o, c in zip(outs, cots_np)).backward()
        res["grads"] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        res["gin"] = [a.grad for a in xs]
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _case(part, tag):
    """The case once: a batch-statistics module in train(), ONE forward and backward, the buffers before and after it, and the
    patched oracle in float64 and in float32 (one thread) with the device's pool routing.  Read-only for every test."""
    case = BB.CASES[part][tag]
    sd = seeded_state_dict(case[0], case[3], num_classes=case[4] or 1)
    m = _module(part, case).train()
    before = _buffers(m)
    dev = _run(part, m, case)
    after = _buffers(m)
    r64 = BB.oracle(part, sd, case, torch.float64, dev["argmax"])
    r32 = BB.one_thread(BB.oracle, part, sd, case, torch.float32, dev["argmax"])
    zeros = BB.zero_set(r64["grads"])
    return dict(case=case, module=m, before=before, after=after, dev=dev, r64=r64, r32=r32, zeros=zeros,
                e32=BB.group_errors(r32, r64, zeros), s32=BB.stat_errors(r32["stats"], r64["stats"]))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part,tag", ALL_CASES, ids=IDS)
def test_gradients_and_outputs_match_float64_autograd_of_the_patched_oracle(part, tag):
    c = _case(part, tag)
    dev, r64, zeros = c["dev"], c["r64"], c["zeros"]
    assert set(dev["grads"]) == set(r64["grads"]) == {k for k, _ in BB.keys(part, c["case"]) if BB.trainable(k)}
    assert zeros and all(BB.ZERO_PATTERN[part].match(k) for k in zeros), zeros
    e = BB.group_errors(dev, r64, zeros)
    bad = {}
    for grp in ("outputs", "gradients", "fusion"):
        if grp not in e:
            continue
        bound = BB.bound(c["e32"][grp])
        print(f"{part} {tag} {grp}: device {e[grp]:.3e} | float32 torch on the CPU {c['e32'][grp]:.3e} | bound {bound:.3e}"
              + (f" (worst: {e['worst_gradient']})" if grp == "gradients" else ""))
        if not e[grp] <= bound:
            bad[grp] = (e[grp], bound)
    zbound = BB.BOUND_FACTOR * c["e32"]["zeros"]
    print(f"{part} {tag} zeros: {len(zeros)} tensors, device max |g| {e['zeros']:.3e} | float32 torch on the CPU {c['e32']['zeros']:.3e} | bound {zbound:.3e}")
    if not e["zeros"] <= zbound:
        bad["zeros"] = (e["zeros"], zbound)
    assert not bad, (part, tag, bad)
    if part == "neck":                                           # legitimacy of the routing, the condition of tests/test_gpu_neck_grads.py
        pool = r64["pool"]
        for name, slack, scale in zip(N.pool_names(c["case"][0]), pool.slack, pool.scale):
            assert slack <= 4e-5 * max(1.0, scale), (name, slack, scale)
        print(f"{part} {tag}: worst legitimacy slack {max(pool.slack):.3e}; windows routed unlike the float64 oracle's own "
              f"{sum(int((a != b).sum()) for a, b in zip(dev['argmax'], pool.own))}")
    assert all(b.grad is None for b in c["module"].buffers())    # the running statistics receive no gradient


@pytest.mark.parametrize("part,tag", ALL_CASES, ids=IDS)
def test_running_statistics_move_as_the_oracles_do_and_only_in_train_mode(part, tag):
    c = _case(part, tag)
    before, after, r64 = c["before"], c["after"], c["r64"]
    got = {k: after[k] for k in r64["stats"]}
    e = BB.stat_errors(got, r64["stats"])
    bad = {}
    for kind, v in e.items():
        bound = BB.BOUND_FACTOR * c["s32"][kind]
        print(f"{part} {tag} {kind}: device {v:.3e} | float32 torch on the CPU {c['s32'][kind]:.3e} | bound {bound:.3e}")
        if not v <= bound:
            bad[kind] = (v, bound)
    assert not bad, (part, tag, bad)
    assert all(not torch.equal(after[k], before[k]) for k in r64["stats"])
    counters = [k for k in after if k.endswith("num_batches_tracked")]
    assert counters and all(int(after[k]) == int(before[k]) + 1 for k in counters)
    # eval(): a forward changes nothing; under no_grad in train() the statistics move again
    m = _module(part, c["case"]).eval()
    b0 = _buffers(m)
    _run(part, m, c["case"], backward=False)
    assert all(torch.equal(v, b0[k]) for k, v in _buffers(m).items())
    m.train()
    with torch.no_grad():
        _run(part, m, c["case"], backward=False)
    b1 = _buffers(m)
    assert all(torch.equal(b1[k], after[k]) for k in r64["stats"])        # the same first step, bit for bit
    assert all(int(b1[k]) == int(b0[k]) + 1 for k in counters)


@pytest.mark.parametrize("part", BB.PARTS)
def test_batch_mode_in_eval_is_the_default_module_bit_for_bit(part):
    tag = next(iter(BB.CASES[part])) if part != "backbone" else "phi0_s128_b2_dropconnect"
    case = BB.CASES[part][tag]
    default = _module(part, case, batch_norm=None)
    assert default.batch_norm == "running"
    b0 = _buffers(default)
    want = _run(part, default.eval(), case)
    same = _run(part, default.train(), case)                     # a default module: running statistics in every mode
    got = _run(part, _module(part, case).eval(), case)
    for other in (same, got):
        assert all(torch.equal(a, b) for a, b in zip(other["outs"], want["outs"]))
        assert all(torch.equal(a, b) for a, b in zip(other["gin"], want["gin"]))
        assert set(other["grads"]) == set(want["grads"]) and all(torch.equal(other["grads"][k], v) for k, v in want["grads"].items())
    assert all(torch.equal(v, b0[k]) for k, v in _buffers(default).items())
    # ... and it is not the batch-statistics function
    assert not all(torch.equal(a, b) for a, b in zip(_case(part, tag)["dev"]["outs"], want["outs"]))


@pytest.mark.parametrize("part", BB.PARTS)
def test_two_identical_batch_mode_runs_are_bit_equal(part):
    tag = next(iter(BB.CASES[part])) if part != "backbone" else "phi0_s128_b2_dropconnect"
    case = BB.CASES[part][tag]
    first = _case(part, tag)["dev"]
    again = _run(part, _module(part, case).train(), case)
    assert all(torch.equal(a, b) for a, b in zip(again["outs"], first["outs"]))
    assert all(torch.equal(a, b) for a, b in zip(again["gin"], first["gin"]))
    assert all(torch.equal(again["grads"][k], v) for k, v in first["grads"].items())


@pytest.mark.parametrize("part", ["heads", "neck"])
def test_two_rows_give_a_finite_forward_within_the_bound_and_one_row_is_refused(part):
    case = BB.N2_CASE if part == "heads" else BB.N2_CASE[:3] + (4, None, None)
    sd = seeded_state_dict(case[0], case[3], num_classes=case[4] or 1)
    dev = _run(part, _module(part, case).train(), case)
    r64 = BB.oracle(part, sd, case, torch.float64, dev["argmax"])
    r32 = BB.one_thread(BB.oracle, part, sd, case, torch.float32, dev["argmax"])
    e = max(H.rel_err(a.cpu().numpy(), b.numpy()) for a, b in zip(dev["outs"], r64["outs"]))
    e32 = max(H.rel_err(a.numpy(), b.numpy()) for a, b in zip(r32["outs"], r64["outs"]))
    print(f"{part} phi0_s128_b2 (2 rows at P7) outputs: device {e:.3e} | float32 torch on the CPU {e32:.3e} | bound {BB.bound(e32):.3e}")
    assert e <= BB.bound(e32)
    assert all(bool(torch.isfinite(g).all()) for g in list(dev["grads"].values()) + dev["gin"])      # no gradient bound with 2 rows
    one = BB.N1_CASE if part == "heads" else BB.N1_CASE[:3] + (4, None, None)
    m = _module(part, one).train()
    b0 = _buffers(m)
    with pytest.raises(ValueError):
        _run(part, m, one, backward=False)
    assert all(torch.equal(v, b0[k]) for k, v in _buffers(m).items())
    _run(part, m.eval(), one, backward=False)                    # the running-statistics function takes one row


def _abi(part, case, flat, xs, cots, outs, ws_ptr, nbytes, stats_ptr, g_flat, g_in):
    """Forward and backward through the hep_*_device_bn entry points in HEP_BN_BATCH; returns the two return codes."""
    from hmd_ego_pose_amd import _capi
    l = _capi.lib()
    phi, size, batch, _seed, classes, _drop = case
    stream = torch.cuda.current_stream().cuda_stream
    P = _capi.ptr_array
    if part == "heads":
        rc1 = l.hep_heads_forward_device_bn(flat.data_ptr(), P(xs), phi, classes, size, batch, P(outs), ws_ptr, nbytes, 1, BB.MOMENTUM, stats_ptr, stream)
        rc2 = l.hep_heads_backward_device_bn(flat.data_ptr(), P(cots), phi, classes, size, batch, g_flat.data_ptr(), P(g_in), ws_ptr, nbytes, 1, stream)
    elif part == "neck":
        rc1 = l.hep_neck_forward_device_bn(flat.data_ptr(), P(xs), phi, size, batch, P(outs), ws_ptr, nbytes, 1, BB.MOMENTUM, stats_ptr, stream)
        rc2 = l.hep_neck_backward_device_bn(flat.data_ptr(), P(cots), phi, size, batch, g_flat.data_ptr(), P(g_in), ws_ptr, nbytes, 1, stream)
    else:
        sc = BB.scales_of(part, case)
        sc = None if sc is None else sc.cuda().contiguous()
        rc1 = l.hep_backbone_forward_device_bn(flat.data_ptr(), xs[0].data_ptr(), _capi.ptr(sc), phi, size, batch, P(outs), ws_ptr, nbytes, 1,
                                               BB.MOMENTUM, stats_ptr, stream)
        rc2 = l.hep_backbone_backward_device_bn(flat.data_ptr(), P(cots), _capi.ptr(sc), phi, size, batch, g_flat.data_ptr(), g_in[0].data_ptr(),
                                                ws_ptr, nbytes, 1, stream)
    torch.cuda.synchronize()
    return rc1, rc2, l.hep_last_error()


@pytest.mark.parametrize("part,tag", ALL_CASES, ids=IDS)
def test_the_abi_on_an_exact_workspace_between_guards_equals_the_autograd_path(part, tag):
    """Forward and backward through hep_*_device_bn on a workspace window of exactly hep_*_workspace_bytes_bn(HEP_BN_BATCH) between
    two guards, the statistics output in a guarded window of its own, every output and gradient buffer NaN first: the guards keep
    their pattern, everything is finite and equals the autograd path bit for bit, running statistics get a gradient of exactly
    zero, and the statistics output holds the module's new buffers in its running slots and is untouched (still NaN) elsewhere."""
    from hmd_ego_pose_amd import _capi
    c = _case(part, tag)
    case, dev = c["case"], c["dev"]
    phi, size, batch, _seed, classes, _drop = case
    l = _capi.lib()
    flat = _module(part, case).flat_parameters().detach()        # the parameters and the LOADED statistics, as the cached run saw them
    cfg = (phi, classes, size, batch) if part == "heads" else (phi, size, batch)
    nbytes = _capi.check(getattr(l, f"hep_{part}_workspace_bytes_bn")(*cfg, 1))
    gw = GuardedWorkspace(nbytes, flat.device)
    gs = GuardedWorkspace((flat.numel() * 4 + 15) // 16 * 16, flat.device)
    x_np, cots_np = BB.inputs(part, case)
    xs = [torch.from_numpy(a).cuda() for a in x_np]
    cots = [torch.from_numpy(a).cuda() for a in cots_np]
    outs = [torch.full_like(o, float("nan")) for o in dev["outs"]]
    g_flat = torch.full_like(flat, float("nan"))
    g_in = [torch.full_like(a, float("nan")) for a in xs]
    rc1, rc2, why = _abi(part, case, flat, xs, cots, outs, gw.ptr, nbytes, gs.ptr, g_flat, g_in)
    assert rc1 == 0 and rc2 == 0, why
    assert gw.changed() == [] and gs.changed() == [], (part, tag, nbytes, gw.changed(), gs.changed())
    assert all(torch.equal(a, b) for a, b in zip(outs, dev["outs"]))
    assert all(torch.equal(a, b) for a, b in zip(g_in, dev["gin"]))
    assert bool(torch.isfinite(g_flat).all())
    stats = gs.window.view(torch.float32)[:flat.numel()]
    tail = gs.window.view(torch.float32)[flat.numel():]
    assert bool(torch.isnan(tail).all())
    flat_keys = [k for k, _ in BB.keys(part, case)]
    sizes = [int(np.prod(s)) for _, s in BB.keys(part, case)]
    assert sum(sizes) == flat.numel()
    for k, g, s in zip(flat_keys, g_flat.split(sizes), stats.split(sizes)):
        if BB.trainable(k):
            assert torch.equal(g, dev["grads"][k].reshape(-1)), k
            assert bool(torch.isnan(s).all()), k                 # not a statistics slot: untouched
        else:
            assert not bool(g.any()), k
            assert torch.equal(s, c["after"][k].reshape(-1)), k


def test_one_composed_training_step_matches_the_composed_oracle():
    """heads(neck(backbone(x))) at phi 0, size 128, batch 8, all three in batch mode and train(): the five outputs and the
    gradients of the stem conv, one BiFPN pointwise conv and one head header against the composed patched oracle in float64, the
    4 x float32-CPU rule per group."""
    from hmd_ego_pose_amd import TrainableHeads
    from hmd_ego_pose_amd.backbone import TrainableBackbone
    from hmd_ego_pose_amd.neck import TrainableNeck
    from oracle import efficientpose_ref as R
    phi, size, batch, seed = 0, 128, 8, 4
    picks = ("backbone_net.model._conv_stem.conv.weight", "bifpn.1.conv4_down.pointwise_conv.conv.weight", "regressor.header.pointwise_conv.conv.weight")
    sd = seeded_state_dict(phi, seed)
    image, _ = G.seeded_inputs(phi, size, batch)
    cots = H.seeded_cotangents(1, size, batch, seed + 2)
    parts = [cls(phi, batch_norm="batch") for cls in (TrainableBackbone, TrainableNeck)] + [TrainableHeads(phi, 1, batch_norm="batch")]
    for p in parts:
        p.load_state_dict(sd, strict=False)
        p.cuda().train()
    bb, neck, heads = parts
    maps = neck(bb(torch.from_numpy(image).cuda()))
    argmax = _neck_argmax(neck, maps, (phi, size, batch))        # before the backward frees the graph's workspace
    outs = heads(maps)
    sum((o * torch.from_numpy(c).cuda()).sum() for o, c in zip(outs, cots)).backward()
    torch.cuda.synchronize()
    named = {k: v for p in parts for k, v in p.named_parameters()}
    assert all(int(b) == 1 for p in parts for k, b in p.named_buffers() if k.endswith("num_batches_tracked"))

    def composed(dtype):
        t = lambda a: (torch.from_numpy(a) if isinstance(a, np.ndarray) else a.detach().cpu()).to(dtype)
        p = {k: t(v).clone() for k, v in sd.items() if v.dtype == torch.float32}
        for k in picks:
            p[k].requires_grad_(True)
        with BB.batch_statistics():
            taps = G.oracle_backbone(p, t(image), phi)
            o = H.oracle_heads(p, N.oracle_neck(p, taps, phi, N.RoutedPool(argmax)), phi, 1)
            sum((a * t(c)).sum() for a, c in zip(o, cots)).backward()
        return [a.detach() for a in o], {k: p[k].grad for k in picks}

    own = R.bn
    o64, g64 = composed(torch.float64)
    o32, g32 = BB.one_thread(composed, torch.float32)
    assert R.bn is own                                           # the oracle's own BatchNorm is back
    bad = {}
    for grp, dev, c32, ref in (("outputs", [o.detach().cpu() for o in outs], o32, o64),
                               ("gradients", [named[k].grad.cpu() for k in picks], [g32[k] for k in picks], [g64[k] for k in picks])):
        e = max(H.rel_err(a.numpy(), b.numpy()) for a, b in zip(dev, ref))
        e32 = max(H.rel_err(a.numpy(), b.numpy()) for a, b in zip(c32, ref))
        print(f"composed phi0_s128_b8 {grp}: device {e:.3e} | float32 torch on the CPU {e32:.3e} | bound {BB.bound(e32):.3e}")
        if not e <= BB.bound(e32):
            bad[grp] = (e, BB.bound(e32))
    assert not bad, bad
