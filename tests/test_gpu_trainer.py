"""GPU (MI355X): the one-call training step - hep_optim_grad_norm_device / hep_optim_update_device / hep_transformation_*_device
(csrc/k_train.hip) and ``hmd_ego_pose_amd.Trainer`` over them.

Kernels: the definition is the float64 oracle tests/_optim.py (pinned to torch.optim / clip_grad_norm_ / format_translation by
tests/test_trainer_cpu.py).  The bound rule is the project's own (tests/test_gpu_head_grads.py): the same oracle in float32 numpy
gives e32 = max |a32 - a64| / max |a64| per array, the device may reach 4 x e32, floor one float32 ulp of the array's largest
magnitude (1.2e-7: the last rounding of p alone costs half an ulp on either side).  The hyper-parameters are float32 values (the
ABI takes floats), so both oracles see exactly what the device sees.

Trainer: the yardstick is the parent path - TrainableBackbone / TrainableNeck / TrainableHeads, training.format_translation,
training.losses and torch.optim, as INTEGRATION.md section 1 composes them.  The two device paths may differ by no more than the old
one may differ from its oracle: the gradient-group bound of tests/test_gpu_bn_batch.py's composed-step case, computed here the same
way (composed float32 CPU oracle against the float64 one, device-routed max-pools, 4 x, floor 2e-6) on this file's step.

The tests print what they reach; NOTEBOOK.md section 21 records the values measured on MI355X.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _backbone_grad as G
from tests import _bn_batch as BB
from tests import _head_grad as H
from tests import _neck_grad as N
from tests import _optim as O
from tests._util import CAMS, GuardedWorkspace, seeded_input
from tests._util import seeded_state_dict_once as seeded_state_dict

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 257, 1023, 65539, 3 * 2 ** 20 + 1]      # vector body, tail and grid-stride loop can each go wrong here
F = lambda v: float(np.float32(v))
LR, B1, B2, EPS, MOM = F(1e-3), F(0.9), F(0.999), F(1e-8), F(0.9)
TRAIN_WEIGHTS = (1.0, 1.0, 100.0, 0.1, 1.0)                       # train.py:61-65


def _r16(nbytes):
    return (nbytes + 15) // 16 * 16


class _Buffers:
    """p, g, m, v, stats, kind, the state block and the norm workspace, each an exact window between guard words."""

    def __init__(self, n):
        from hmd_ego_pose_amd import _capi
        self.n, self.lib = n, _capi.lib()
        self.f = {k: GuardedWorkspace(_r16(4 * n), "cuda") for k in ("p", "g", "m", "v", "stats")}
        self.kind = GuardedWorkspace(_r16(n), "cuda")
        self.state = GuardedWorkspace(32, "cuda")
        self.ws = GuardedWorkspace(_capi.check(self.lib.hep_optim_workspace_bytes(n)), "cuda")
        self.state.window.zero_()                                 # "zeroed once"

    def view(self, k):
        return self.f[k].window.view(torch.float32)[:self.n]

    def set(self, k, a):
        self.view(k).copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))

    def set_kind(self, kind):
        self.kind.window[:self.n].copy_(torch.from_numpy(kind))

    def get(self, k):
        return self.view(k).cpu().numpy()

    def bits(self, k):
        return self.f[k].window.clone()                           # the whole window: the padding behind n as well

    def norm(self, opt, max_norm):
        rc = self.lib.hep_optim_grad_norm_device(self.f["g"].ptr, self.kind.ptr, self.n, opt, B1 if opt == O.ADAM else MOM, B2 if opt == O.ADAM else 0.0,
                                                 max_norm, self.state.ptr, self.ws.ptr, self.ws.nbytes, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.lib.hep_last_error()

    def update(self, opt, stats):
        rc = self.lib.hep_optim_update_device(self.f["p"].ptr, self.f["g"].ptr, self.f["m"].ptr, self.f["v"].ptr if opt == O.ADAM else None,
                                              self.f["stats"].ptr if stats else None, self.kind.ptr, self.n, opt, LR, B1 if opt == O.ADAM else MOM,
                                              B2 if opt == O.ADAM else 0.0, EPS, self.state.ptr, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.lib.hep_last_error()

    def read_state(self):
        raw = self.state.window.cpu().numpy()
        f, i = raw[:16].view(np.float32), raw[16:32].view(np.int32)
        return dict(norm=float(f[0]), clip_coef=float(f[1]), bias1=float(f[2]), bias2_sqrt=float(f[3]), step=int(i[0]), skipped=int(i[1]), pad=(int(i[2]), int(i[3])))

    def guards(self):
        bad = {k: g.changed() for k, g in list(self.f.items()) + [("kind", self.kind), ("state", self.state), ("ws", self.ws)]}
        return {k: v for k, v in bad.items() if v}


def _three_steps(n, opt, stats, max_norm, seed=0):
    """Three consecutive device steps with fresh gradients; returns per step the device's (p, m, v) and state, and the buffers."""
    p0, grads, st_arr, zero = O.case_arrays(n, seed)
    kind = O.mixed_kinds(n, seed)
    b = _Buffers(n)
    b.set("p", p0); b.set("m", np.zeros(n)); b.set("v", np.zeros(n)); b.set("stats", st_arr); b.set_kind(kind)
    out = []
    for g in grads:
        b.set("g", g)
        b.norm(opt, max_norm)
        b.update(opt, stats)
        torch.cuda.synchronize()
        out.append((b.get("p"), b.get("m"), b.get("v") if opt == O.ADAM else None, b.read_state()))
    return (p0, grads, st_arr, zero, kind), out, b


def _oracle_steps(arrs, opt, stats, max_norm, dtype):
    p0, grads, st_arr, _zero, kind = arrs
    b1, b2 = (B1, B2) if opt == O.ADAM else (MOM, 0.0)
    p, m, v, st = p0.astype(dtype), np.zeros(p0.size, dtype), (np.zeros(p0.size, dtype) if opt == O.ADAM else None), O.State()
    out = []
    for g in grads:
        O.grad_norm(g, kind, st, b1, b2, max_norm, dtype)
        p, m, v = O.update(p, g, m, v, st_arr if stats else None, kind, opt, LR, b1, b2, EPS, st, dtype)
        out.append((p, m, v, dict(norm=st.norm, clip_coef=st.clip_coef, step=st.step, skipped=st.skipped)))
    return out


# ---- 1. the update kernel alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [O.ADAM, O.SGD_NESTEROV], ids=["adam", "sgd"])
@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_three_steps_against_the_oracle(n, opt):
    # with stats and a max_norm that the large-gradient steps exceed and (for n > 5) the seeded small ones may not; without stats, no clipping
    for stats, max_norm in ((True, F(0.5)), (False, 0.0)):
        arrs, dev, b = _three_steps(n, opt, stats, max_norm)
        p0, grads, st_arr, zero, kind = arrs
        r64 = _oracle_steps(arrs, opt, stats, max_norm, np.float64)
        r32 = _oracle_steps(arrs, opt, stats, max_norm, np.float32)
        assert b.guards() == {}, b.guards()
        bad = []
        for s, (d, a64, a32) in enumerate(zip(dev, r64, r32)):
            for name, x, y64, y32 in zip("pmv", d[:3], a64[:3], a32[:3]):
                if x is None:
                    continue
                e, e32 = O.rel_err(x, y64), O.rel_err(y32, y64)
                print(f"update n={n} {'adam' if opt == O.ADAM else 'sgd'} stats={stats} step {s + 1} {name}: device {e:.3e} | float32 numpy {e32:.3e} | bound {O.bound(e32):.3e}")
                if not e <= O.bound(e32):
                    bad.append((s, name, e, O.bound(e32)))
            st = d[3]
            assert st["step"] == s + 1 and st["skipped"] == 0 and st["pad"] == (0, 0)
            assert abs(st["clip_coef"] - a64[3]["clip_coef"]) <= 2 * O.ULP32
            if max_norm == 0.0:
                assert st["clip_coef"] == 1.0
            # what must not move: frozen elements, statistics without `stats`, the moments of both kinds
            p, m, v = d[:3]
            assert np.array_equal(p[kind == 2].view(np.uint32), p0[kind == 2].view(np.uint32))
            if stats:
                assert np.array_equal(p[kind == 1].view(np.uint32), st_arr[kind == 1].view(np.uint32))
            else:
                assert np.array_equal(p[kind == 1].view(np.uint32), p0[kind == 1].view(np.uint32))
            assert not m[kind != 0].any() and (v is None or not v[kind != 0].any())
            # a trainable element whose gradient was zero in every step has zero moments: bit-unchanged
            still = zero & (kind == 0)
            assert np.array_equal(p[still].view(np.uint32), p0[still].view(np.uint32)) and not m[still].any()
        assert not bad, bad
        if stats and n > 5:
            assert any(d[3]["clip_coef"] < 1.0 for d in dev)
        if not stats:
            continue
        again = _three_steps(n, opt, stats, max_norm)[1]
        for d, a in zip(dev, again):                                # two runs: bit-identical
            assert all(x is None or np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(d[:3], a[:3])) and d[3] == a[3]


# ---- 2. the norm --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_gradient_norm_and_the_skip_of_a_non_finite_step(n):
    p0, grads, st_arr, _zero = O.case_arrays(n, 1)
    kind = O.mixed_kinds(n, 1)
    g = grads[0]
    b = _Buffers(n)
    b.set("p", p0); b.set("m", grads[1]); b.set("v", np.abs(grads[2])); b.set("stats", st_arr); b.set_kind(kind); b.set("g", g)
    b.norm(O.ADAM, 0.0)
    torch.cuda.synchronize()
    st = b.read_state()
    g0 = g[kind == 0]
    n64 = float(np.sqrt(np.sum(g0.astype(np.float64) ** 2)))
    n32 = float(np.sqrt(np.sum(g0 * g0, dtype=np.float32)))
    e, e32 = abs(st["norm"] - n64) / max(n64, 1e-300), abs(n32 - n64) / max(n64, 1e-300)
    print(f"norm n={n}: device {e:.3e} | float32 numpy {e32:.3e} | bound {O.bound(e32):.3e}")
    assert e <= O.bound(e32) and (st["step"], st["skipped"]) == (1, 0) and st["clip_coef"] == 1.0
    assert abs(st["bias1"] - (1 - B1)) <= 2 * O.ULP32 and abs(st["bias2_sqrt"] - np.sqrt(1 - B2)) <= 2 * O.ULP32
    if not (kind == 0).any() or not (kind == 2).any():
        assert b.guards() == {}
        return
    before = {k: b.bits(k) for k in ("p", "m", "v")}
    first, frozen = int(np.flatnonzero(kind == 0)[-1]), int(np.flatnonzero(kind == 2)[0])
    for bad in (np.inf, np.nan):
        s0 = b.read_state()
        gb = g.copy(); gb[first] = bad
        b.set("g", gb)
        b.norm(O.ADAM, F(1.0)); b.update(O.ADAM, True)
        torch.cuda.synchronize()
        s1 = b.read_state()
        assert (s1["step"], s1["skipped"], s1["clip_coef"]) == (s0["step"], s0["skipped"] + 1, 0.0) and not np.isfinite(s1["norm"])
        assert all(torch.equal(b.bits(k), v) for k, v in before.items())        # p (statistics included), m, v: bit-unchanged
        gf = g.copy(); gf[frozen] = bad                             # the same value where nothing trains: not seen
        b.set("g", gf)
        b.norm(O.ADAM, 0.0)
        torch.cuda.synchronize()
        s2 = b.read_state()
        assert s2["norm"] == st["norm"] and (s2["step"], s2["skipped"]) == (s1["step"] + 1, s1["skipped"])
    assert b.guards() == {}, b.guards()


# ---- 3. pack / unpack ---------------------------------------------------------------------------------------------------------------
def test_transformation_pack_and_unpack_against_the_oracle():
    from hmd_ego_pose_amd import _capi, training
    l = _capi.lib()
    size, B, R = 128, 2, 3
    ta = training.translation_anchors(size).numpy()
    Nn = ta.shape[0]
    rng = np.random.Generator(np.random.PCG64(8))
    rot, raw, cot = (rng.standard_normal(s).astype(np.float32) for s in ((B, Nn, R), (B, Nn, 3), (B, Nn, R + 3)))
    bufs = {k: GuardedWorkspace(_r16(4 * n), "cuda") for k, n in (("out", B * Nn * (R + 3)), ("g_rot", B * Nn * R), ("g_raw", B * Nn * 3))}
    d = lambda a: torch.from_numpy(a).cuda()
    d_rot, d_raw, d_cam, d_ta, d_cot = d(rot), d(raw), d(CAMS), d(ta), d(cot)
    stream = torch.cuda.current_stream().cuda_stream
    assert l.hep_transformation_pack_device(d_rot.data_ptr(), d_raw.data_ptr(), d_cam.data_ptr(), d_ta.data_ptr(), B, Nn, R, bufs["out"].ptr, stream) == 0
    assert l.hep_transformation_unpack_grad_device(d_cot.data_ptr(), d_raw.data_ptr(), d_cam.data_ptr(), d_ta.data_ptr(), B, Nn, R, bufs["g_rot"].ptr,
                                                   bufs["g_raw"].ptr, stream) == 0
    torch.cuda.synchronize()
    got = {k: g.window.view(torch.float32)[:n].cpu().numpy().reshape(s) for (k, g), (n, s) in
           zip(bufs.items(), ((B * Nn * (R + 3), (B, Nn, R + 3)), (B * Nn * R, (B, Nn, R)), (B * Nn * 3, (B, Nn, 3))))}
    want = {}
    for T in (np.float64, np.float32):
        g_rot, g_raw = O.unpack_grad(cot, raw, CAMS, ta, R, T)
        want[T] = dict(out=O.pack(rot, raw, CAMS, ta, T), g_rot=g_rot, g_raw=g_raw)
    for k in bufs:
        # per column: the translation columns differ in scale by the focal length
        for c in range(got[k].shape[2]):
            e, e32 = O.rel_err(got[k][..., c], want[np.float64][k][..., c]), O.rel_err(want[np.float32][k][..., c], want[np.float64][k][..., c])
            print(f"pack/unpack {k}[{c}]: device {e:.3e} | float32 numpy {e32:.3e} | bound {O.bound(e32):.3e}")
            assert e <= O.bound(e32), (k, c, e, O.bound(e32))
        assert bufs[k].changed() == []
    # ... and the parent's path: format_translation + cat on the device
    t = torch.cat((d_rot, training.format_translation(d_raw, d_cam, size)), 2)
    assert torch.equal(bufs["out"].window.view(torch.float32)[:t.numel()].view_as(t), t)      # bit for bit: the same operations in the same order
    # ... and its autograd gradient on the device equals unpack bit for bit
    a_rot, a_raw = d_rot.clone().requires_grad_(True), d_raw.clone().requires_grad_(True)
    (torch.cat((a_rot, training.format_translation(a_raw, d_cam, size)), 2) * d_cot).sum().backward()
    assert np.array_equal(got["g_rot"], a_rot.grad.cpu().numpy()) and np.array_equal(got["g_raw"], a_raw.grad.cpu().numpy())


# ---- 4. the composed step against the parent's path -----------------------------------------------------------------------------------
PHI, SIZE, BATCH = 0, 128, 8


@functools.lru_cache(maxsize=None)
def _problem(size=SIZE, batch=BATCH, hand=True, image_seed=None, points=60):
    """Image, camera, targets from training.anchor_targets (one or two boxes per image), model points: device tensors.  With
    size 256, batch 2, image_seed 31, points 300 these are the inputs of NOTEBOOK.md section 14's fit
    (tests/test_gpu_backbone_grads.py), camera included."""
    from hmd_ego_pose_amd import _capi, training
    x = G.seeded_inputs(PHI, size, batch)[0] if image_seed is None else seeded_input((batch, 3, size, size), image_seed)
    n = _capi.lib().hep_anchors(size, None, None)
    anchors = np.empty((n, 4), np.float32); t_anchors = np.empty((n, 3), np.float32)
    assert _capi.lib().hep_anchors(size, anchors.ctypes.data, t_anchors.ctypes.data) == n
    rng = np.random.Generator(np.random.PCG64(8))
    k = size / 256.0
    two = [np.array([[48., 48., 176., 176.]]) * k, np.array([[16., 16., 80., 80.], [112., 112., 240., 240.]]) * k]
    boxes = [two[i % 2] + (i // 2) * 2.0 * k for i in range(batch)]
    labels = [np.zeros((len(b),), np.int32) for b in boxes]
    tr = [np.concatenate([rng.uniform(-1, 1, (len(b), 3)), rng.standard_normal((len(b), 3)) * 100 + [0, 0, 600], np.zeros((len(b), 2))], 1).astype(np.float32) for b in boxes]
    co = [rng.standard_normal((len(b), 63)).astype(np.float32) * 50 for b in boxes] if hand else None
    lab, reg_t, tra_t, crd_t = training.anchor_targets(torch.from_numpy(anchors).cuda(), boxes, labels, tr, co, [(size, size)] * batch, 1)
    assert (tra_t[..., -1] == 1).sum(1).min().item() > 0, "every image needs an object anchor"
    pts = torch.from_numpy((rng.standard_normal((1, points, 3)) * 30).astype(np.float32)).cuda()
    cam = torch.from_numpy(np.stack([CAMS[i % 2 if image_seed is None else 0] for i in range(batch)])).cuda()
    return dict(image=torch.from_numpy(x).cuda(), camera=cam, lab=lab, reg_t=reg_t, tra_t=tra_t, crd_t=crd_t, pts=pts, size=size)


def _modules(sd, batch_norm):
    from hmd_ego_pose_amd import TrainableHeads
    from hmd_ego_pose_amd.backbone import TrainableBackbone
    from hmd_ego_pose_amd.neck import TrainableNeck
    mods = [TrainableBackbone(PHI, batch_norm=batch_norm), TrainableNeck(PHI, batch_norm=batch_norm), TrainableHeads(PHI, 1, batch_norm=batch_norm)]
    for m in mods:
        m.load_state_dict(sd, strict=False)
        m.cuda().train()
    return mods


def _parent_step(mods, opt, pr, max_norm=None, keep=None):
    """One step of the parent commit's loop (the stock-optimiser variant).  Returns the six weighted losses."""
    from hmd_ego_pose_amd import training
    bb, neck, heads = mods
    opt.zero_grad(set_to_none=True)
    maps = neck(bb(pr["image"]))
    if keep is not None:
        keep["maps"] = maps
    reg, cls, rot, raw, hand = heads(maps)
    trn = training.format_translation(raw, pr["camera"], pr["size"])
    out, _per = training.losses(pr["lab"], cls, pr["reg_t"], reg, pr["tra_t"], torch.cat((rot, trn), 2), pr["crd_t"], hand if pr["crd_t"] is not None else None, pr["pts"], 3)
    w = out * torch.tensor(TRAIN_WEIGHTS, device="cuda")
    total = w.sum()
    total.backward()
    if keep is not None:
        keep["grads"] = [_flat_grad(m) for m in mods]
    if max_norm:
        torch.nn.utils.clip_grad_norm_([p for m in mods for p in m.parameters()], max_norm)
    opt.step()
    return torch.cat((w.detach(), total.detach()[None]))


def _flat_grad(m):
    """The module's gradients in its flat ABI order, zeros in the running-statistics slots."""
    named = dict(m.named_parameters())
    buffers = dict(m.named_buffers())
    return torch.cat([(named[k].grad if k in named else torch.zeros_like(buffers[k])).reshape(-1) for k in m._flat_keys])


def _flat_values(m):
    return m.flat_parameters().detach().clone()


def _trainer(sd, **kw):
    from hmd_ego_pose_amd import Trainer
    return Trainer(sd, PHI, 1, "cuda", **kw)


def _step(tr, pr):
    return tr.step(pr["image"], pr["camera"], pr["lab"], pr["reg_t"], pr["tra_t"], pr["crd_t"], pr["pts"])


@functools.lru_cache(maxsize=None)
def _composed_bound(batch_norm):
    """The gradient-group bound and the per-kind statistics bound of tests/test_gpu_bn_batch.py's composed-step case, computed as
    that test computes them, for the composed model of this file (seed-0 weights, phi 0 @ 128 batch 8): the composed oracle in
    float32 on the CPU (one thread) against the same in float64, max-pools routed as the device routed them."""
    import contextlib
    from hmd_ego_pose_amd import neck as NK
    sd = seeded_state_dict(PHI, 0)
    pr = _problem()
    mods = _modules(sd, batch_norm)
    maps = mods[1](mods[0](pr["image"]))
    views = NK.stage_views(maps[0].grad_fn.saved_tensors[1], PHI, SIZE, BATCH)
    argmax = [N.first_argmax(views[name].permute(0, 3, 1, 2)).cpu() for name in N.pool_names(PHI)]
    picks = ("backbone_net.model._conv_stem.conv.weight", "bifpn.1.conv4_down.pointwise_conv.conv.weight", "regressor.header.pointwise_conv.conv.weight")
    cots = H.seeded_cotangents(1, SIZE, BATCH, 2)
    image = pr["image"].cpu().numpy()

    def composed(dtype):
        t = lambda a: (torch.from_numpy(a) if isinstance(a, np.ndarray) else a.detach().cpu()).to(dtype)
        p = {k: t(v).clone() for k, v in sd.items() if v.dtype == torch.float32}
        for k in picks:
            p[k].requires_grad_(True)
        stats = {}
        with (BB.batch_statistics(stats) if batch_norm == "batch" else contextlib.nullcontext()):
            taps = G.oracle_backbone(p, t(image), PHI)
            o = H.oracle_heads(p, N.oracle_neck(p, taps, PHI, N.RoutedPool(argmax)), PHI, 1)
            sum((a * t(c)).sum() for a, c in zip(o, cots)).backward()
        return {k: p[k].grad for k in picks}, stats

    g64, s64 = composed(torch.float64)
    g32, s32 = BB.one_thread(composed, torch.float32)
    e32 = max(H.rel_err(g32[k].numpy(), g64[k].numpy()) for k in picks)
    stat32 = BB.stat_errors(s32, s64) if batch_norm == "batch" else {}
    print(f"composed oracle ({batch_norm}): float32 torch on the CPU, gradients {e32:.3e} -> bound {BB.bound(e32):.3e}; statistics {stat32}")
    return BB.bound(e32), {k: BB.BOUND_FACTOR * v for k, v in stat32.items()}


@pytest.mark.parametrize("batch_norm", ["batch", "running"])
def test_step_losses_gradients_and_statistics_equal_the_parent_path(batch_norm):
    """(a) and (d): one step of both paths from the same weights."""
    sd = seeded_state_dict(PHI, 0)
    pr = _problem()
    bound, stat_bound = _composed_bound(batch_norm)
    mods = _modules(sd, batch_norm)
    opt = torch.optim.Adam([p for m in mods for p in m.parameters()], lr=LR)
    keep = {}
    want = _parent_step(mods, opt, pr, keep=keep)
    tr = _trainer(sd, optimizer="adam", lr=LR, batch_norm=batch_norm)
    before = tr.params.clone()
    got = _step(tr, pr).clone()
    torch.cuda.synchronize()
    assert got.shape == (6,) and bool(torch.isfinite(got).all())
    bad = []
    for i, name in enumerate(("classification", "regression", "rotation", "translation", "hand", "total")):
        e = abs(float(got[i]) - float(want[i])) / max(abs(float(want[i])), 1e-30)
        print(f"step ({batch_norm}) loss {name}: trainer {float(got[i]):.8g} | parent {float(want[i]):.8g} | rel {e:.3e} | bound {bound:.3e}")
        if not e <= bound:
            bad.append((name, e))
    assert float(got[4]) > 0                                       # the hand loss is on
    for name, g_parent in zip(("backbone", "neck", "heads"), keep["grads"]):
        g = tr.part(tr.grad, name)
        e = H.rel_err(g.cpu().numpy(), g_parent.cpu().numpy())
        print(f"step ({batch_norm}) flat gradient {name}: rel {e:.3e} | bound {bound:.3e} | bit-identical {torch.equal(g, g_parent)}")
        if not e <= bound:
            bad.append((name, e))
    assert not bad, bad
    views, kinds = tr.named_views(), tr.kind.cpu().numpy()
    assert (tr.steps_taken, tr.steps_skipped) == (1, 0) and tr.grad_norm > 0
    buffers = {k: b for m in mods for k, b in m.named_buffers() if k.endswith(("running_mean", "running_var"))}
    if batch_norm == "batch":                                      # (d)
        e = BB.stat_errors({k: views[k] for k in buffers}, buffers)
        for kind, v in e.items():
            print(f"step statistics {kind}: trainer against the modules {v:.3e} | bound {stat_bound[kind]:.3e}")
            assert v <= stat_bound[kind], (kind, v, stat_bound[kind])
        assert all(not torch.equal(views[k].cpu(), sd[k]) for k in buffers)
    else:
        assert torch.equal(tr.params[torch.from_numpy(kinds != 0).cuda()], before[torch.from_numpy(kinds != 0).cuda()])
    assert not torch.equal(tr.params[torch.from_numpy(kinds == 0).cuda()], before[torch.from_numpy(kinds == 0).cuda()])


@pytest.mark.parametrize("optimizer,max_norm", [("adam", None), ("adam", 5.0), ("sgd", 5.0)])
def test_update_on_identical_gradients_equals_torch_optim(optimizer, max_norm):
    """(b): the trainer's own gradients fed to torch.optim (+ clip_grad_norm_) over clones of its initial views; compared after one
    and after three ACCUMULATED steps within the bound of the update-kernel test (the float32 numpy oracle accumulating the same
    three steps on the same flat arrays).  The trainable parameters change through the update alone, so the twins, the oracles and
    the trainer each carry their own parameters and moments from step to step and see the same three gradients."""
    sd = seeded_state_dict(PHI, 0)
    pr = _problem(hand=False)
    tr = _trainer(sd, optimizer=optimizer, lr=LR, batch_norm="batch", max_grad_norm=max_norm)
    kind = tr.kind.cpu().numpy()
    trainable = [k for k in tr.named_views() if not k.endswith(("running_mean", "running_var"))]
    twins = {k: torch.nn.Parameter(v.detach().clone()) for k, v in tr.named_views().items() if k in trainable}
    opt = torch.optim.Adam(twins.values(), lr=LR) if optimizer == "adam" else torch.optim.SGD(twins.values(), lr=LR, momentum=MOM, nesterov=True)
    oid, b1, b2 = (O.ADAM, B1, B2) if optimizer == "adam" else (O.SGD_NESTEROV, MOM, 0.0)
    st64, st32 = O.State(), O.State()
    o64 = [tr.params.cpu().numpy().astype(np.float64), np.zeros(tr.total), np.zeros(tr.total) if optimizer == "adam" else None]
    o32 = [tr.params.cpu().numpy(), np.zeros(tr.total, np.float32), np.zeros(tr.total, np.float32) if optimizer == "adam" else None]
    clipped = []
    for s in range(3):
        _step(tr, pr)
        g = tr.grad.cpu().numpy()
        for k, v in tr.grad_views().items():
            if k in twins:
                twins[k].grad = v.detach().clone()
        if max_norm:
            total = float(torch.nn.utils.clip_grad_norm_(twins.values(), max_norm))
            assert abs(tr.grad_norm - total) <= 1e-5 * total      # torch: a float32 norm of ~700 float32 norms; the trainer sums in double
            clipped.append(total > max_norm)
        opt.step()
        for o, st, T in ((o64, st64, np.float64), (o32, st32, np.float32)):
            O.grad_norm(g, kind, st, b1, b2, max_norm or 0.0, T)
            o[0], o[1], o[2] = O.update(o[0], g, o[1], o[2], None, kind, oid, LR, b1, b2, EPS, st, T)
        if s in (0, 2):
            got = np.concatenate([v.detach().cpu().numpy().reshape(-1) for k, v in tr.named_views().items() if k in twins])
            want = np.concatenate([twins[k].detach().cpu().numpy().reshape(-1) for k in tr.named_views() if k in twins])
            e32 = O.rel_err(o32[0][kind == 0], o64[0][kind == 0])
            e, e_or = O.rel_err(got, want), O.rel_err(tr.params.cpu().numpy()[kind == 0], o64[0][kind == 0])
            print(f"update ({optimizer}, max_norm {max_norm}) after step {s + 1}: trainer against torch.optim {e:.3e} | against the float64 oracle {e_or:.3e} | "
                  f"float32 numpy {e32:.3e} | bound {O.bound(e32):.3e}")
            assert e <= O.bound(e32) and e_or <= O.bound(e32)
    if max_norm:
        print(f"clipping active per step: {clipped}")
        assert any(clipped)


def test_three_sgd_steps_of_both_paths_stay_within_the_accumulated_gradient_bound():
    """(c): under SGD (momentum 0.9, Nesterov) the parameters of the two PATHS agree within lr x (gradient bound) x max |g| per step,
    accumulated over the steps.  The learning rate is NOTEBOOK.md section 14's 1.95e-6.  Measured on MI355X (NOTEBOOK.md section 21):
    the two paths are bit-identical over the three steps - the gradients are, and hep_optim_update_device rounds SGD as
    torch.optim.SGD's kernels do (both multiply-adds fused).  The bound needs that: the curvature of this loss is about 5e5 (plain
    descent oscillates from lr 3.9e-6 on), so a difference of one float32 ulp in a parameter grows step by step."""
    sd = seeded_state_dict(PHI, 0)
    pr = _problem(hand=False)
    bound, _ = _composed_bound("batch")
    lr = F(1e-3 / 512)
    mods = _modules(sd, "batch")
    opt = torch.optim.SGD([p for m in mods for p in m.parameters()], lr=lr, momentum=MOM, nesterov=True)
    tr = _trainer(sd, optimizer="sgd", lr=lr, batch_norm="batch")
    allowed = {n: 0.0 for n in ("backbone", "neck", "heads")}
    bad = []
    for s in range(3):
        keep = {}
        _parent_step(mods, opt, pr, keep=keep)
        _step(tr, pr)
        for (name, m), g in zip(zip(allowed, mods), keep["grads"]):
            allowed[name] += lr * bound * float(g.abs().max())
            kinds = tr.part(tr.kind, name) == 0
            mine, theirs = tr.part(tr.params, name)[kinds], _flat_values(m)[kinds]
            d = float((mine - theirs).abs().max())
            print(f"sgd step {s + 1} {name}: max |p_trainer - p_parent| {d:.3e} | allowed {allowed[name]:.3e} | max |g| {float(g.abs().max()):.3e}, "
                  f"max |p| {float(theirs.abs().max()):.3e}, |p| where they differ most {float(theirs[(mine - theirs).abs().argmax()].abs()):.3e}")
            if not d <= allowed[name]:
                bad.append((s, name, d, allowed[name]))
    assert not bad, bad


# ---- 5. export ------------------------------------------------------------------------------------------------------------------------
def test_export_to_copies_the_views_counts_the_steps_and_the_model_serves_them():
    from hmd_ego_pose_amd import HMDEgoPose
    sd = seeded_state_dict(PHI, 0)
    pr = _problem(hand=False)
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=PHI, onnx_export=True, input_sizes=[SIZE] * 9)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m(pr["image"])                                                  # a session exists before the export
    tr = _trainer(m.state_dict(), optimizer="adam", lr=F(1e-4), batch_norm="batch")
    for _ in range(2):
        _step(tr, pr)
    assert tr.steps_taken == 2
    counters = {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
    tr.export_to(m)
    assert not m._sessions                                           # invalidated: the next forward packs the new weights
    after = m.state_dict()
    for k, v in tr.named_views().items():
        assert torch.equal(after[k], v), k
    assert counters and all(int(after[k]) == c + 2 for k, c in counters.items())
    tr.export_to(m)                                                  # again without a step: the counters stay
    assert all(int(m.state_dict()[k]) == c + 2 for k, c in counters.items())
    want = tr.forward_eval(pr["image"])
    got = m(pr["image"])
    for g, w in zip(got[1:], want):
        err = (g - w).abs().max().item() / max(1.0, w.abs().max().item())
        print(f"export: model against the trainer's eval forward {err:.3e}")
        assert err <= 5e-4, err
    assert any(not torch.equal(after[k].cpu(), sd[k]) for k in ("regressor.header.pointwise_conv.conv.weight", "backbone_net.model._bn0.running_mean"))


# ---- 6. a frozen backbone ---------------------------------------------------------------------------------------------------------------
def test_freeze_backbone_leaves_it_bit_unchanged_and_the_other_gradients_as_they_are():
    sd = seeded_state_dict(PHI, 0)
    pr = _problem(hand=False)
    frozen = _trainer(sd, optimizer="adam", lr=LR, batch_norm="running", freeze_backbone=True)
    free = _trainer(sd, optimizer="adam", lr=LR, batch_norm="running")
    bb0 = frozen.part(frozen.params, "backbone").clone()
    _step(frozen, pr); _step(free, pr)
    for name in ("neck", "heads"):
        assert torch.equal(frozen.part(frozen.grad, name), free.part(free.grad, name)), name
    assert bool(free.part(free.grad, "backbone").any()) and not bool(frozen.part(frozen.grad, "backbone").any())
    assert frozen.grad_norm < free.grad_norm
    _step(frozen, pr)
    assert torch.equal(frozen.part(frozen.params, "backbone"), bb0)
    assert not bool(frozen.part(frozen.m, "backbone").any()) and not bool(frozen.part(frozen.v, "backbone").any())
    assert not torch.equal(free.part(free.params, "backbone"), bb0)
    # with batch statistics elsewhere the frozen trunk keeps its statistics too
    fb = _trainer(sd, optimizer="sgd", lr=LR, batch_norm="batch", freeze_backbone=True)
    neck0 = fb.part(fb.params, "neck").clone()
    _step(fb, pr)
    assert torch.equal(fb.part(fb.params, "backbone"), bb0) and not torch.equal(fb.part(fb.params, "neck"), neck0)


# ---- 7. no allocation, validation, resuming, the wrapper ----------------------------------------------------------------------------------
def test_a_warm_step_allocates_nothing():
    sd = seeded_state_dict(PHI, 0)
    pr = _problem(hand=True)
    tr = _trainer(sd, optimizer="adam", lr=LR, batch_norm="batch", max_grad_norm=1.0)
    _step(tr, pr)
    torch.cuda.synchronize()
    before, peak0 = torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(3):
        out = _step(tr, pr)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    print(f"allocated {before} bytes before and after three steps; peak inside them {torch.cuda.max_memory_allocated() - before} above")
    assert tr.steps_taken == 4 and bool(torch.isfinite(out).all())


def test_step_validates_before_the_abi_sees_a_pointer():
    sd = seeded_state_dict(PHI, 0)
    pr = _problem(hand=True)
    tr = _trainer(sd, optimizer="sgd", lr=LR, batch_norm="running")
    good = [pr["image"], pr["camera"], pr["lab"], pr["reg_t"], pr["tra_t"], pr["crd_t"], pr["pts"]]
    p0 = tr.params.clone()
    cases = [(0, good[0].double()), (0, good[0].cpu()), (0, good[0][0]), (0, good[0][:, :, :100, :100]), (0, good[0][:, :2]),
             (1, good[1][:, :5]), (1, good[1][:4]), (2, good[2][:, :-1]), (3, good[3][..., :4]), (4, good[4][..., :8]), (4, good[4].cpu()),
             (5, good[5][..., :63]), (6, good[6][0]), (6, torch.zeros((1, 3000, 3), device="cuda")), (2, None)]
    for i, badv in cases:
        args = list(good); args[i] = badv
        with pytest.raises(ValueError):
            tr.step(*args)
    assert tr.steps_taken == 0 and torch.equal(tr.params, p0)
    with pytest.raises(ValueError):                                  # one row at P7 under batch statistics: the parts' own refusal
        _trainer(sd, batch_norm="batch").step(*[g[:1] if g is not None and g.shape[0] == BATCH else g for g in good])
    tr.lr = 0.5 * LR
    assert tr.lr == 0.5 * LR


def test_state_dict_resumes_bit_for_bit_and_fit_step_builds_a_trainer():
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    sd = seeded_state_dict(PHI, 0)
    pr = _problem(hand=False)
    a = _trainer(sd, optimizer="adam", lr=LR, batch_norm="batch")
    _step(a, pr); _step(a, pr)
    saved = a.state_dict()
    _step(a, pr)
    b = _trainer(sd, optimizer="adam", lr=LR, batch_norm="batch")
    b.load_state_dict(saved)
    assert b.steps_taken == 2
    _step(b, pr)
    assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.state, b.state)
    with pytest.raises(ValueError):
        _trainer(sd, optimizer="sgd").load_state_dict(saved)
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=PHI, onnx_export=True, input_sizes=[SIZE] * 9)
    m.load_state_dict(sd, strict=True)
    w = TrainModelWithLoss(m.cuda().eval())
    first = w.fit_step(pr["image"], pr["camera"], pr["lab"], pr["reg_t"], pr["tra_t"], None, pr["pts"], optimizer="adam", lr=LR, batch_norm="batch").clone()
    c = _trainer(sd, optimizer="adam", lr=LR, batch_norm="batch")
    assert torch.equal(first, _step(c, pr)) and torch.equal(w.trainer.params, c.params)
    w.fit_step(pr["image"], pr["camera"], pr["lab"], pr["reg_t"], pr["tra_t"], None, pr["pts"])
    assert w.trainer.steps_taken == 2


# ---- 8. descent ---------------------------------------------------------------------------------------------------------------------------
# The largest relative distance between the trainer's and the parent path's weighted total over the ten steps of the test below, measured on
# MI355X, times ten (source: NOTEBOOK.md section 21, "Descent").  Measured: 0.0 in every step, the ten totals are bit-identical.  Ten times
# nothing would leave no room for the last bit of a float32 total, so the figure is ten times the resolution of that measurement, one
# float32 ulp (1.19e-7).  The issue caps it at 1e-3.
DESCENT_REL = 1.2e-6


def test_ten_sgd_steps_descend_like_the_parent_path():
    """NOTEBOOK.md section 14's fit: phi 0 @ 256 batch 2, seed-4 weights, plain SGD at lr 1.95e-6, running statistics - ten strictly
    descending steps on record for the parent's path.  The trainer's ten totals descend strictly too and stay next to the parent's."""
    assert DESCENT_REL <= 1e-3
    sd = seeded_state_dict(PHI, 4)
    pr = _problem(size=256, batch=2, hand=True, image_seed=31, points=300)
    lr = F(1e-3 / 512)                                               # 1.95e-6
    mods = _modules(sd, "running")
    opt = torch.optim.SGD([p for m in mods for p in m.parameters()], lr=lr)
    tr = _trainer(sd, optimizer="sgd", momentum=0.0, lr=lr, batch_norm="running")
    parent = [float(_parent_step(mods, opt, pr)[5]) for _ in range(10)]
    mine = [float(_step(tr, pr)[5]) for _ in range(10)]
    rel = [abs(a - b) / abs(b) for a, b in zip(mine, parent)]
    print(f"parent totals {['%.6g' % t for t in parent]}\ntrainer totals {['%.6g' % t for t in mine]}\nrelative distance per step {['%.2e' % r for r in rel]}, worst {max(rel):.3e}")
    assert np.isfinite(mine).all() and all(b < a for a, b in zip(mine, mine[1:])), mine
    assert all(b < a for a, b in zip(parent, parent[1:])), parent
    assert max(rel) <= DESCENT_REL, (max(rel), DESCENT_REL)


def test_drop_connect_tables_reach_forward_and_backward():
    """``drop_connect_rate`` > 0: the step draws ``backbone.draw_branch_scale`` as ``TrainableBackbone`` does (same torch generator state,
    same table) and hands it to the backbone's forward AND backward.  Against the parent path with the same seed: losses and the flat
    gradient of every part bit-identical; against rate 0 they differ."""
    sd = seeded_state_dict(PHI, 0)
    pr = _problem(hand=False)
    mods = _modules(sd, "running")
    mods[0].drop_connect_rate = 0.2
    opt = torch.optim.SGD([p for m in mods for p in m.parameters()], lr=F(1e-9))
    keep = {}
    torch.manual_seed(77)
    want = _parent_step(mods, opt, pr, keep=keep)
    tr = _trainer(sd, optimizer="sgd", lr=F(1e-9), batch_norm="running", drop_connect_rate=0.2)
    torch.manual_seed(77)
    got = _step(tr, pr).clone()
    assert torch.equal(got, want)
    for name, g in zip(("backbone", "neck", "heads"), keep["grads"]):
        assert torch.equal(tr.part(tr.grad, name), g), name
    calm = _trainer(sd, optimizer="sgd", lr=F(1e-9), batch_norm="running")
    assert not torch.equal(_step(calm, pr), got) and not torch.equal(calm.part(calm.grad, "backbone"), tr.part(tr.grad, "backbone"))
