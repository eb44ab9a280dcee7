"""GPU (MI355X): the HIP backward of the training losses (hep_losses_backward_device, csrc/k_loss_grad.hip) behind
training.losses' grad_fn and training.batch_iterate.

Tolerances: max |g_hip - g_ref| <= 1e-5 max |g_ref| per tensor (classification, regression, translation, hand: float32
element-wise arithmetic) and 1e-4 for the rotation columns (sums over the model points in another order); exactly 0
wherever the reference is exactly 0.  References: the real reference's autograd (tests/golden/loss_grads.npz) and the float64
restatement of tests/_loss_grad.py run on the GPU.
"""
import os

import numpy as np
import pytest
import torch

from tests._loss_grad import TRAIN_WEIGHTS, batch_losses, expand_golden, restated_grads
from tests._util import loss_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PRED = ("classification", "regression", "transformation", "hand")


def _dev(c):
    return {k: (torch.from_numpy(v).cuda() if v is not None else None) for k, v in c.items() if k != "model_points"}


def _args(d, c, hand=True):
    return (d["gt_classification"], d["classification"], d["gt_regression"], d["regression"], d["gt_transformation"], d["transformation"],
            d["gt_hand"] if hand else None, d["hand"] if hand else None, c["model_points"], 3)


def _hip_grads(c, weights=TRAIN_WEIGHTS, hand=True, upstream=None):
    """Gradients through training.losses' grad_fn; returns ({name: numpy}, out, per)."""
    from hmd_ego_pose_amd.training import losses
    d = _dev(c)
    for k in PRED:
        if d.get(k) is not None and (hand or k != "hand"):
            d[k].requires_grad_(True)
    out, per = losses(*_args(d, c, hand))
    total = (out * torch.tensor(weights, device="cuda")).sum() if upstream is None else upstream(out, per)
    total.backward()
    torch.cuda.synchronize()
    g = {k: (d[k].grad.cpu().numpy().astype(np.float64) if d[k].grad is not None else None) for k in PRED}
    return g, out.detach(), per.detach()


def _split(g):
    return {"classification": g["classification"], "regression": g["regression"], "rotation": g["transformation"][..., :3],
            "translation": g["transformation"][..., 3:], "hand": g["hand"]}


def _compare(got, want, what):
    got, want = _split(got), _split(want)
    for k, w in want.items():
        if w is None:
            assert got[k] is None, (what, k)
            continue
        m = np.abs(w).max()
        tol = 1e-4 if k == "rotation" else 1e-5
        err = np.abs(got[k] - w).max()
        assert np.isfinite(got[k]).all(), (what, k)
        assert err <= tol * max(m, 1e-30), (what, k, err, m)
        assert (got[k][w == 0] == 0).all(), (what, k, "non-zero where the reference is exactly zero")


def make_case(B, N, K, P, npos, seed, sym=None, classes=1):
    """Seeded inputs shaped like tests/_util.py::loss_cases; sym None: random per anchor, 0 / 1: all (a)symmetric."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x6a11]))
    state = np.zeros((B, N), np.float32)
    for b in range(B):
        state[b, rng.choice(N, size=N // 10, replace=False)] = -1.0
        state[b, rng.choice(N, size=npos + b % 3, replace=False)] = 1.0
    cls = rng.integers(0, K, size=(B, N))
    labels = np.zeros((B, N, K), np.float32)
    pos = state == 1
    labels[pos, cls[pos]] = 1.0
    gt_reg = np.concatenate([rng.standard_normal((B, N, 4)).astype(np.float32) * 0.3, state[..., None]], 2)
    rot_t = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    tr_t = (rng.standard_normal((B, N, 3)) * 100).astype(np.float32)
    s = rng.integers(0, 2, size=(B, N, 1)).astype(np.float32) if sym is None else np.full((B, N, 1), float(sym), np.float32)
    ci = rng.integers(0, classes, size=(B, N, 1)).astype(np.float32)
    gt_hand = np.concatenate([(rng.standard_normal((B, N, 63)) * 0.2).astype(np.float32), state[..., None]], 2)
    return dict(
        gt_classification=np.concatenate([labels, state[..., None]], 2).astype(np.float32),
        classification=(1.0 / (1.0 + np.exp(-rng.standard_normal((B, N, K)) * 3))).astype(np.float32),
        gt_regression=gt_reg.astype(np.float32),
        regression=(gt_reg[..., :4] + rng.standard_normal((B, N, 4)) * 0.15).astype(np.float32),
        gt_transformation=np.concatenate([rot_t, tr_t, s, ci, state[..., None]], 2).astype(np.float32),
        transformation=np.concatenate([rot_t + rng.standard_normal((B, N, 3)).astype(np.float32) * 0.1,
                                       tr_t + rng.standard_normal((B, N, 3)).astype(np.float32) * 5], 2).astype(np.float32),
        gt_hand=gt_hand.astype(np.float32),
        hand=(gt_hand[..., :63] + rng.standard_normal((B, N, 63)) * 0.1).astype(np.float32),
        model_points=(rng.standard_normal((classes, P, 3)) * np.array([40, 25, 60])).astype(np.float32))


def plant_edges(c):
    """Exact edge values: probabilities at / beyond the clamp bounds, residuals at +-1/9 and 0 (regression, hand) and at
    +-1 and 0 (translation), on object and background anchors of image 0."""
    f = np.float32
    st = c["gt_classification"][0, :, -1]
    obj, bg = np.nonzero(st == 1)[0], np.nonzero(st == 0)[0]
    probs = [f(1e-4), f(1 - 1e-4), np.nextafter(f(1e-4), f(0)), np.nextafter(f(1 - 1e-4), f(1)), np.nextafter(f(1e-4), f(1)),
             np.nextafter(f(1 - 1e-4), f(0)), f(0), f(1), f(5e-5)]
    for i, p in enumerate(probs):
        c["classification"][0, bg[i], :] = p
        if i < len(obj):
            c["classification"][0, obj[i], :] = p
    knee = f(1) / f(9)
    res = [knee, -knee, f(0), np.nextafter(knee, f(1))]
    for i in range(min(3, len(obj))):
        n = obj[i]
        c["gt_regression"][0, n, :4] = 0
        c["regression"][0, n, :4] = res
        c["gt_hand"][0, n, :4] = 0
        c["hand"][0, n, :4] = res
        c["gt_transformation"][0, n, 3:6] = 0
        c["transformation"][0, n, 3:6] = [(f(1), f(-1), f(0)), (np.nextafter(f(1), f(2)), f(0.5), f(-2)), (f(-1), f(1), f(1))][i]
    return c


def test_gradients_match_the_reference_fixtures():
    fx = np.load(os.path.join(HERE, "golden", "loss_grads.npz"))
    for name, c in loss_cases().items():
        B, N, _K = c["classification"].shape
        got, _, _ = _hip_grads(c)
        want = expand_golden(fx, name, {"regression": (B, N, 4), "transformation": (B, N, 6), "hand": (B, N, 63)})
        _compare(got, want, name)


@pytest.mark.parametrize("tag,B,N,K,P,npos,sym,hand", [
    ("k3_edges", 3, 3000, 3, 80, 20, None, True),
    ("all_symmetric", 2, 2000, 1, 300, 25, 1, True),
    ("all_asymmetric", 2, 2000, 1, 300, 25, 0, True),
    ("no_hand", 2, 1500, 2, 60, 10, None, False),
    ("p2048", 2, 1000, 1, 2048, 12, None, True),
    ("b16_full", 16, 12276, 1, 500, 40, None, True),
])
def test_edges_and_sizes_match_the_restatement(tag, B, N, K, P, npos, sym, hand):
    c = plant_edges(make_case(B, N, K, P, npos, sum(map(ord, tag)), sym, classes=2 if tag == "k3_edges" else 1))
    got, _, _ = _hip_grads(c, hand=hand)
    cc = dict(c)
    if not hand:
        cc["gt_hand"] = cc["hand"] = None
    want = restated_grads(cc, device="cuda")
    _compare(got, want, tag)


def test_autograd_plumbing_direct_call_mixed_upstream_values_and_reproducibility():
    from hmd_ego_pose_amd.training import _MEAN_SCALE, _loss_inputs, losses, losses_backward
    c = plant_edges(make_case(3, 4000, 2, 120, 30, 7))
    w = torch.tensor(TRAIN_WEIGHTS, device="cuda")
    g1, out, per = _hip_grads(c)
    g2, _, _ = _hip_grads(c)
    for k in PRED:
        assert np.array_equal(g1[k], g2[k]), k                                      # two backward calls: bit-identical
    # the same gradients as a direct ABI call with the folded upstream, bit for bit
    d = _dev(c)
    t, sizes = _loss_inputs(*_args(d, c))
    u = torch.zeros((3, 5), device="cuda") + (w * torch.tensor(_MEAN_SCALE, device="cuda") / 3)[None]
    direct = losses_backward(t, sizes, u)
    torch.cuda.synchronize()
    for k, gd in zip(PRED, direct):
        assert np.array_equal(g1[k], gd.cpu().numpy().astype(np.float64)), k
    # forward values bit-identical to losses() without grad
    o0, p0 = losses(*_args(d, c))
    assert o0.grad_fn is None and np.array_equal(o0.cpu().numpy(), out.cpu().numpy(), equal_nan=True)
    assert np.array_equal(p0.cpu().numpy(), per.cpu().numpy(), equal_nan=True)
    # gradients arriving on both outputs
    W = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).standard_normal((3, 5)).astype(np.float32)).cuda()
    wm = torch.tensor([0.5, -2.0, 3.0, 0.25, 1.5], device="cuda")
    mixed = lambda o, p: (o * wm.to(o.dtype)).sum() + (torch.nan_to_num(p, nan=0.0) * W.to(p.dtype)).sum()
    gm, _, _ = _hip_grads(c, upstream=mixed)
    _compare(gm, restated_grads(c, device="cuda", upstream=mixed), "mixed upstream")
    # with no prediction requiring grad nothing changes
    o3, _ = losses(*_args(d, c))
    assert o3.grad_fn is None


def test_batch_iterate_is_a_differentiable_drop_in():
    from hmd_ego_pose_amd.training import batch_iterate
    fx = np.load(os.path.join(HERE, "golden", "losses.npz"))
    for name, c in loss_cases().items():
        d = _dev(c)
        nc = {k: torch.cat([v, v], 2)[..., :v.shape[2]] for k, v in d.items()}            # non-contiguous views
        assert not nc["hand"].is_contiguous()
        res = batch_iterate(nc["gt_classification"], nc["classification"], nc["gt_regression"], nc["regression"], nc["gt_transformation"],
                            nc["transformation"], nc["gt_hand"], nc["hand"], c["model_points"], 3)
        assert len(res) == 5 and all(r.shape == (1,) for r in res)
        got = np.array([float(r) for r in res])
        want = fx[name]
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, got, want)
        ok = ~np.isnan(want)
        assert np.allclose(got[ok], want[ok], rtol=2e-5, atol=1e-6), (name, got, want)

    # one training step of a small model through batch_iterate vs through the restatement, then 30 Adam steps
    c = make_case(2, 3000, 1, 100, 20, 11)
    torch.manual_seed(0)
    B, N, C = 2, 3000, 16
    feats = torch.randn(B, C, N, device="cuda")

    class Heads(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cls, self.reg, self.rot = torch.nn.Conv1d(C, 1, 1), torch.nn.Conv1d(C, 4, 1), torch.nn.Conv1d(C, 3, 1)
            self.tr, self.hand = torch.nn.Conv1d(C, 3, 1), torch.nn.Conv1d(C, 63, 1)

        def forward(self, x):
            p = lambda h: h(x).permute(0, 2, 1)                                 # [B, N, k], non-contiguous
            return torch.sigmoid(p(self.cls)), p(self.reg), torch.cat([p(self.rot) * 0.5, p(self.tr) * 50], 2), p(self.hand)

    model = Heads().cuda()
    d = _dev(c)
    wts = TRAIN_WEIGHTS

    def step_loss(through_hip):
        cls, reg, tr, hand = model(feats)
        if through_hip:
            res = batch_iterate(d["gt_classification"], cls, d["gt_regression"], reg, d["gt_transformation"], tr, d["gt_hand"], hand,
                                c["model_points"], 3)
            return sum(wt * r.mean() for wt, r in zip(wts, res))
        f = lambda x: x.to(torch.float64)
        out, _ = batch_losses(f(d["gt_classification"]), f(cls), f(d["gt_regression"]), f(reg), f(d["gt_transformation"]), f(tr),
                              f(d["gt_hand"]), f(hand), c["model_points"], 3)
        return (out * torch.tensor(wts, dtype=torch.float64, device="cuda")).sum()

    grads = []
    for through_hip in (True, False):
        model.zero_grad()
        step_loss(through_hip).backward()
        grads.append([p.grad.detach().double().cpu().numpy() for p in model.parameters()])
    for gh, gr in zip(*grads):
        assert np.abs(gh - gr).max() <= 1e-4 * np.abs(gr).max(), (np.abs(gh - gr).max(), np.abs(gr).max())
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    first = None
    for _ in range(30):
        opt.zero_grad()
        loss = step_loss(True)
        first = float(loss.detach()) if first is None else first
        loss.backward()
        opt.step()
    last = float(step_loss(True))
    assert np.isfinite(first) and last < first, (first, last)


def test_errors_raise_before_any_launch():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd.training import _loss_inputs, losses, losses_backward
    c = make_case(2, 500, 1, 40, 5, 3)
    d = _dev(c)
    d["classification"].requires_grad_(True)
    a = list(_args(d, c))
    with pytest.raises(ValueError):                                                      # a hand without a GT hand
        losses(*(a[:6] + [None, d["hand"]] + a[8:]))
    with pytest.raises(ValueError):                                                      # wrong shapes
        losses(*(a[:3] + [d["regression"][..., :3]] + a[4:]))
    with pytest.raises(ValueError):
        losses(*(a[:5] + [d["transformation"][..., :5]] + a[6:]))
    big = np.zeros((1, 2049, 3), np.float32)
    with pytest.raises(_capi.HepUnsupported):
        losses(*(a[:8] + [big, 3]))
    # the backward entry point refuses 2049 points and leaves the gradient buffers untouched
    t, sizes = _loss_inputs(*(a[:8] + [big, 3]))
    with pytest.raises(_capi.HepUnsupported):
        losses_backward(t, sizes, torch.ones((2, 5), device="cuda"))
    t, sizes = _loss_inputs(*a)
    sentinel = torch.full((2, 500, 1), 7.0, device="cuda")
    ws = torch.zeros(2 * 504, dtype=torch.int32, device="cuda")
    l = _capi.lib()
    gc, pc, gr, pr, gt, pt, gh, ph, pts = t
    rc = l.hep_losses_backward_device(gc.data_ptr(), pc.data_ptr(), gr.data_ptr(), pr.data_ptr(), gt.data_ptr(), pt.data_ptr(), None, ph.data_ptr(),
                                      pts.data_ptr(), 2, 500, 1, 3, 63, 1, 40, torch.ones((2, 5), device="cuda").data_ptr(), sentinel.data_ptr(),
                                      None, None, None, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and bool((sentinel == 7.0).all()) and bool((ws == 0).all())
