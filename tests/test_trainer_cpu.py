"""CPU: the one-call training step's host side.  The numpy oracle of the optimiser kernels (tests/_optim.py) pinned to torch, the
pack / unpack oracle pinned to ``training.format_translation`` and its autograd, the combined flat layout of ``Trainer`` at every
supported phi, and the argument checks of the new C-ABI entry points (they run before any HIP call, so without a device)."""
import ctypes

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi, training
from hmd_ego_pose_amd.weights import seeded_state_dict
from tests import _optim as O
from tests._util import CAMS


def _steps(n=4099, steps=5, seed=3):
    rng = np.random.Generator(np.random.PCG64([seed, 0x7a11]))
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * s for s in (0.001, 3.0, 0.0005, 10.0, 0.002)][:steps]      # norms around 0.06, 190, 0.03, 640, 0.13
    return p0, grads


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_oracle_equals_torch_optim_and_clip_grad_norm_in_float64(optimizer):
    """Five steps, max_norm 1: clipping is active on the second and fourth step and inactive on the others.  The parameters are
    split over three tensors of unequal size, as torch sees a model."""
    p0, grads = _steps()
    max_norm, lr = 1.0, 1e-2
    split = [1000, 3, 3096]
    tp = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in np.split(p0, np.cumsum(split)[:-1])]
    opt = torch.optim.Adam(tp, lr=lr) if optimizer == "adam" else torch.optim.SGD(tp, lr=lr, momentum=0.9, nesterov=True)
    oid, b1, b2 = (O.ADAM, 0.9, 0.999) if optimizer == "adam" else (O.SGD_NESTEROV, 0.9, 0.0)
    kind = np.zeros(p0.size, np.uint8)
    p, m, v, st = p0.copy(), np.zeros_like(p0), (np.zeros_like(p0) if optimizer == "adam" else None), O.State()
    clipped = []
    for g in grads:
        for t, gi in zip(tp, np.split(g, np.cumsum(split)[:-1])):
            t.grad = torch.from_numpy(gi.copy())
        total = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        opt.step()
        assert O.grad_norm(g, kind, st, b1, b2, max_norm)
        p, m, v = O.update(p, g, m, v, None, kind, oid, lr, b1, b2, 1e-8, st)
        clipped.append(st.clip_coef < 1.0)
        assert abs(st.norm - float(total)) <= 1e-12 * float(total)
        want = np.concatenate([t.detach().numpy() for t in tp])
        assert O.rel_err(p, want) <= 1e-12, (optimizer, st.step, O.rel_err(p, want))
    assert clipped == [False, True, False, True, False] and st.step == 5 and st.skipped == 0


def test_oracle_kinds_and_skip():
    n = 64
    rng = np.random.Generator(np.random.PCG64(5))
    p0, g, stats = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    kind = O.mixed_kinds(n, 0)
    assert {0, 1, 2} <= set(kind.tolist())
    st = O.State()
    assert O.grad_norm(g, kind, st, 0.9, 0.999, 0.0)
    assert abs(st.norm - np.linalg.norm(g[kind == 0])) < 1e-12 and st.clip_coef == 1.0
    p, m, v = O.update(p0, g, np.zeros(n), np.zeros(n), stats, kind, O.ADAM, 1e-3, 0.9, 0.999, 1e-8, st)
    assert np.array_equal(p[kind == 2], p0[kind == 2]) and np.array_equal(p[kind == 1], stats[kind == 1])
    assert not m[kind != 0].any() and not v[kind != 0].any() and np.all(p[kind == 0] != p0[kind == 0])
    p1, _, _ = O.update(p0, g, np.zeros(n), np.zeros(n), None, kind, O.ADAM, 1e-3, 0.9, 0.999, 1e-8, st)
    assert np.array_equal(p1[kind == 1], p0[kind == 1])
    # a non-finite gradient at a trainable position skips the step; at a frozen position it is not seen
    for bad in (np.inf, np.nan):
        gb = g.copy(); gb[np.flatnonzero(kind == 0)[3]] = bad
        s2 = O.State(); s2.step = 4
        assert not O.grad_norm(gb, kind, s2, 0.9, 0.999, 1.0) and (s2.step, s2.skipped, s2.clip_coef) == (4, 1, 0.0)
        q, mm, vv = O.update(p0, gb, np.ones(n), np.ones(n), stats, kind, O.ADAM, 1e-3, 0.9, 0.999, 1e-8, s2)
        assert np.array_equal(q, p0) and np.array_equal(mm, np.ones(n)) and np.array_equal(vv, np.ones(n))
        gf = g.copy(); gf[np.flatnonzero(kind == 2)[0]] = bad
        s3 = O.State()
        assert O.grad_norm(gf, kind, s3, 0.9, 0.999, 1.0) and s3.norm == st.norm


def test_pack_and_unpack_oracle_equal_format_translation_and_its_autograd():
    size, B, R = 128, 2, 3
    ta = training.translation_anchors(size).numpy()
    N = ta.shape[0]
    rng = np.random.Generator(np.random.PCG64(8))
    rot, raw, cot = rng.standard_normal((B, N, R)), rng.standard_normal((B, N, 3)), rng.standard_normal((B, N, R + 3))
    cam = CAMS.astype(np.float64)                                  # two different camera rows
    assert not np.array_equal(cam[0], cam[1])
    t_rot = torch.from_numpy(rot).requires_grad_(True)
    t_raw = torch.from_numpy(raw).requires_grad_(True)
    want = torch.cat((t_rot, training.format_translation(t_raw, torch.from_numpy(cam), size)), 2)
    got = O.pack(rot, raw, cam, ta)
    assert got.shape == (B, N, R + 3) and O.rel_err(got, want.detach().numpy()) <= 1e-14
    (want * torch.from_numpy(cot)).sum().backward()
    g_rot, g_raw = O.unpack_grad(cot, raw, cam, ta, R)
    assert np.array_equal(g_rot, t_rot.grad.numpy())
    assert O.rel_err(g_raw, t_raw.grad.numpy()) <= 1e-13


@pytest.mark.parametrize("phi", range(6))
def test_combined_layout_offsets_kinds_and_views(phi):
    from hmd_ego_pose_amd import backbone, heads, neck
    from hmd_ego_pose_amd.trainer import PARTS, combined_layout
    lay = combined_layout(phi, 1)
    counts = {"backbone": backbone.param_layout(phi)[0], "neck": neck.param_layout(phi)[0], "heads": heads.param_layout(phi, 1)[0]}
    base = 0
    for name in PARTS:
        off, n = lay["parts"][name]
        assert off % 4 == 0 and off == base and n == counts[name]
        base += (n + 3) // 4 * 4
    assert lay["total"] == base == sum((c + 3) // 4 * 4 for c in counts.values())
    kind = lay["kind"]
    assert kind.dtype == np.uint8 and kind.shape == (base,)
    covered = np.zeros(base, bool)
    for k, s, o in lay["entries"]:
        n = int(np.prod(s)) if len(s) else 1
        assert not covered[o:o + n].any()
        covered[o:o + n] = True
        want = 1 if k.endswith(("running_mean", "running_var")) else 0
        assert (kind[o:o + n] == want).all(), k
    assert (kind[~covered] == 2).all() and (~covered).sum() == base - sum(counts.values())
    frozen = combined_layout(phi, 1, freeze_backbone=True)["kind"]
    off, n = lay["parts"]["backbone"]
    assert (frozen[off:off + n] == 2).all() and np.array_equal(frozen[off + n:], kind[off + n:])
    # the views round-trip a seeded state dict (host copy of what Trainer.named_views does on the device)
    sd = seeded_state_dict(phi, 0)
    keys = {k for k, v in sd.items() if v.dtype == torch.float32}
    assert {k for k, _, _ in lay["entries"]} == keys
    flat = torch.zeros(base)
    for k, s, o in lay["entries"]:
        flat[o:o + sd[k].numel()] = sd[k].reshape(-1)
    for k, s, o in lay["entries"]:
        assert tuple(sd[k].shape) == s and torch.equal(flat[o:o + sd[k].numel()].view(s), sd[k])


def test_combined_layout_refuses_what_the_neck_refuses():
    from hmd_ego_pose_amd.trainer import combined_layout
    for phi in (6, 7, 8, -1):
        with pytest.raises(ValueError):
            combined_layout(phi)


def test_new_entry_points_check_their_arguments_before_any_hip_call():
    l = _capi.lib()
    for name in ("hep_optim_workspace_bytes", "hep_optim_grad_norm_device", "hep_optim_update_device", "hep_transformation_pack_device",
                 "hep_transformation_unpack_grad_device"):
        assert hasattr(l, name) and name in _capi.SYMBOLS
    n = 1000
    buf = (ctypes.c_char * (5 * 4096 + 64))()
    base = (ctypes.addressof(buf) + 15) // 16 * 16                # host memory: every call below must return before touching it
    a, b, c, d, ws = (base + i * 4096 for i in range(5))
    kind = state = ws + 2048
    nws = l.hep_optim_workspace_bytes(n)
    assert nws > 0 and nws % 16 == 0 and l.hep_optim_workspace_bytes(0) == -1 and l.hep_optim_workspace_bytes(-5) == -1
    assert l.hep_optim_workspace_bytes(3 << 30) <= 1024 * 8      # a fixed grid: the figure stops growing
    norm = lambda grad=a, kind=kind, n=n, opt=0, state=state, ws=ws, nbytes=nws: l.hep_optim_grad_norm_device(
        grad, kind, n, opt, 0.9, 0.999, 1.0, state, ws, nbytes, None)
    upd = lambda p=a, g=b, m=c, v=d, stats=None, kind=kind, n=n, opt=0, state=state: l.hep_optim_update_device(
        p, g, m, v, stats, kind, n, opt, 1e-3, 0.9, 0.999, 1e-8, state, None)
    assert norm(grad=None) == -1 and norm(kind=None) == -1 and norm(state=None) == -1 and norm(ws=None) == -1
    assert norm(n=0) == -1 and norm(n=-1) == -1 and norm(grad=a + 4) == -1 and norm(ws=ws + 4) == -1 and norm(nbytes=nws - 1) == -1
    assert norm(opt=7) == -4 and b"optimizer 7" in l.hep_last_error()
    assert upd(p=None) == -1 and upd(g=None) == -1 and upd(m=None) == -1 and upd(v=None) == -1 and upd(kind=None) == -1 and upd(state=None) == -1
    assert upd(n=0) == -1 and upd(p=a + 4) == -1 and upd(g=b + 4) == -1 and upd(m=c + 4) == -1 and upd(v=d + 4) == -1 and upd(stats=a + 4) == -1
    assert upd(opt=7) == -4 and b"optimizer 7" in l.hep_last_error()
    assert upd(opt=7, v=None) == -1                              # v may be NULL under SGD only
    pack = lambda rot=a, raw=b, cam=c, ta=d, B=1, N=10, R=3, out=ws: l.hep_transformation_pack_device(rot, raw, cam, ta, B, N, R, out, None)
    unpack = lambda g=a, raw=b, cam=c, ta=d, B=1, N=10, R=3, g_rot=ws, g_raw=ws + 1024: l.hep_transformation_unpack_grad_device(
        g, raw, cam, ta, B, N, R, g_rot, g_raw, None)
    for fn, names in ((pack, ("rot", "raw", "cam", "ta", "out")), (unpack, ("g", "raw", "cam", "ta", "g_rot", "g_raw"))):
        assert all(fn(**{k: None}) == -1 for k in names)
        assert fn(B=0) == -1 and fn(N=0) == -1 and fn(R=0) == -1 and fn(R=9) == -1


def test_trainer_refuses_the_cpu_and_bad_options():
    from hmd_ego_pose_amd import Trainer
    sd = seeded_state_dict(0, 0)
    with pytest.raises(ValueError):
        Trainer(sd, 0, 1, "cpu")
    with pytest.raises(ValueError):
        Trainer(sd, 0, 1, "cuda", optimizer="lion")
    with pytest.raises(ValueError):
        Trainer(sd, 0, 1, "cuda", batch_norm="sync")
    with pytest.raises(ValueError):
        Trainer(sd, 6, 1, "cuda")
