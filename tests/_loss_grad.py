"""Test-side float64 restatement of the reference's ``batch_iterate`` (hmdegopose/loss.py:54-428) for torch autograd, and
helpers shared by tests/test_loss_grad_cpu.py and tests/test_gpu_loss_grad.py.

The restatement is vectorised over the batch (no per-image loop) and computes in float64, but every branch decision is
taken on the float32 values the reference and the kernels see: the classification clamp bounds are float32(1e-4) and
float32(1 - 1e-4) (inclusive, like torch.clamp's gradient), the smooth-L1 knee compares the float32 residual with
float32(1 / 9), and the symmetric nearest target point is the first minimum of the forward's float32 distance.  Gradients of the predictions come from
``torch.autograd`` on it.
"""
import math

import numpy as np
import torch

LO, HI, KNEE = float(np.float32(1e-4)), float(np.float32(1 - 1e-4)), float(np.float32(1 / 9))


def _f32(x):
    return x.detach().to(torch.float32)


def _rotate(p, axis, angle):
    # p [M,P,3], axis [M,1,3], angle [M,1,1]: Rodrigues (loss.py:570-609)
    c, s = torch.cos(angle), torch.sin(angle)
    return p * c + torch.cross(axis.expand_as(p), p, dim=-1) * s + axis * (axis * p).sum(-1, keepdim=True) * (1 - c)


def _smooth_l1_sigma3(pred, gt):
    d = pred - gt
    small = (_f32(pred) - _f32(gt)).abs() <= KNEE
    return torch.where(small, 4.5 * d * d, d.abs() - 0.5 / 9.0)


def _rotate_f32(p, r):
    # the forward's float32 expressions (csrc/loss_dev.h: axis_angle, rotate_pt), one rounding per operation
    f = np.float32
    pi = f(np.pi)
    x, y, z = r[:, 0:1] * pi, r[:, 1:2] * pi, r[:, 2:3] * pi
    ang = np.sqrt((x * x + y * y) + z * z)
    ax, ay, az, c, s = x / ang, y / ang, z / ang, np.cos(ang), np.sin(ang)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    dt, omc = (ax * px + ay * py) + az * pz, f(1) - c
    cx, cy, cz = ay * pz - az * py, az * px - ax * pz, ax * py - ay * px
    return np.stack([(px * c + cx * s) + (ax * dt) * omc, (py * c + cy * s) + (ay * dt) * omc, (pz * c + cz * s) + (az * dt) * omc], -1)


def nearest_f32(points, r_pred, r_tgt):
    """points [M,P,3], rotation vectors [M,3] (float32): for every predicted point the index of the FIRST nearest target
    point by the forward's float32 distance sqrt((dx*dx + dy*dy) + dz*dz) - the point the kernels take."""
    with np.errstate(all="ignore"):
        op, ot = _rotate_f32(points, r_pred), _rotate_f32(points, r_tgt)
        out = np.empty(points.shape[:2], np.int64)
        for i in range(points.shape[0]):
            d = op[i][:, None, :] - ot[i][None, :, :]
            out[i] = np.argmin(np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]), axis=1)
    return out


def batch_losses(gc, pc, gr, pr, gt, pt, gh, ph, model_points, R=3):
    """Float64 tensors laid out as training.losses takes them (gh / ph may be None).  Returns (losses [5] = batch means with
    regression x 50, per_image [B, 5]) with autograd through pc / pr / pt / ph."""
    B, N, K = pc.shape
    dev, f64 = pc.device, torch.float64
    per = []
    # classification: focal, alpha 0.25, gamma 1.5
    st, lab = gc[..., K], gc[..., :K]
    x = pc
    inside = (_f32(x) >= LO) & (_f32(x) <= HI)
    p = torch.where(inside, x, torch.where(_f32(x) < LO, torch.full_like(x, LO), torch.full_like(x, HI)).detach())
    af = torch.where(lab == 1, 0.25, 0.75)
    fw = af * torch.where(lab == 1, 1 - p, p) ** 1.5
    bce = -(lab * torch.log(p) + (1 - lab) * torch.log(1 - p))
    keep = (st != -1)[..., None] & (lab != -1)
    n_c = (st == 1).sum(1).to(f64)
    per.append(torch.where(keep, fw * bce, torch.zeros_like(p)).sum((1, 2)) / n_c.clamp(min=1))
    # regression: smooth-L1 sigma 3 on the object anchors
    obj_r = gr[..., 4] == 1
    l_r = torch.where(obj_r[..., None], _smooth_l1_sigma3(pr, gr[..., :4]), torch.zeros_like(pr))
    per.append(l_r.sum((1, 2)) / obj_r.sum(1).to(f64).clamp(min=1))
    # rotation / translation on the object anchors of the transformation state
    obj_t = torch.round(gt[..., R + 5]) == 1
    n_t = obj_t.sum(1).to(f64)
    bi, ni = torch.nonzero(obj_t, as_tuple=True)
    rot_img = torch.zeros(B, dtype=f64, device=dev)
    tr_img = torch.zeros(B, dtype=f64, device=dev)
    if bi.numel():
        pts = torch.as_tensor(np.asarray(model_points), device=dev).to(f64)
        g = gt[bi, ni]
        cls = torch.round(g[:, R + 4]).long().clamp(0, pts.shape[0] - 1)
        sym = torch.round(g[:, R + 3]) == 1
        P = pts.shape[1]
        vp, vt = pt[bi, ni, :R] * math.pi, g[:, :R] * math.pi
        ang_p, ang_t = vp.norm(dim=-1, keepdim=True), vt.norm(dim=-1, keepdim=True)
        mp = pts[cls]
        op = _rotate(mp, (vp / ang_p)[:, None], ang_p[:, None])
        ot = _rotate(mp, (vt / ang_t)[:, None], ang_t[:, None])
        idx = torch.arange(P, device=dev).expand(len(bi), P).clone()
        si = torch.nonzero(sym).flatten()
        if si.numel():
            near = nearest_f32(pts[cls[si]].cpu().numpy().astype(np.float32), pt[bi[si], ni[si], :R].detach().cpu().numpy().astype(np.float32),
                               g[si, :R].detach().cpu().numpy().astype(np.float32))
            idx[si] = torch.from_numpy(near).to(dev)
        diff = op - torch.gather(ot, 1, idx[..., None].expand(-1, -1, 3))
        sq = (diff * diff).sum(-1)
        pos = sq > 0
        dist = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))   # gradient 0 at 0
        rot_img = rot_img.index_add(0, bi, dist.mean(1))
        d = pt[bi, ni, R:R + 3] - g[:, R:R + 3]
        tr_img = tr_img.index_add(0, bi, torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).sum(1))
    per.append(torch.where(n_t > 0, rot_img / n_t.clamp(min=1), torch.zeros_like(rot_img)))
    per.append(tr_img / (3 * n_t))                                  # NaN without object anchors, like the reference
    # hand
    if ph is not None:
        obj_h = gh[..., -1] == 1
        l_h = torch.where(obj_h[..., None], _smooth_l1_sigma3(ph, gh[..., :-1]), torch.zeros_like(ph))
        per.append(l_h.sum((1, 2)) / obj_h.sum(1).to(f64).clamp(min=1))
    else:
        per.append(torch.zeros(B, dtype=f64, device=dev))
    per = torch.stack(per, 1)
    out = per.mean(0) * torch.tensor([1.0, 50.0, 1.0, 1.0, 1.0], dtype=f64, device=dev)
    return out, per


TRAIN_WEIGHTS = (1.0, 1.0, 100.0, 0.1, 1.0)          # reference train.py:61-65


def restated_grads(case, weights=TRAIN_WEIGHTS, device="cpu", upstream=None):
    """Gradients of sum(weights * losses) (or of ``upstream(out, per)``) through the float64 restatement for a dict of
    float32 arrays shaped like tests/_util.py::loss_cases.  Returns {classification, regression, transformation, hand} as
    float64 numpy arrays (hand None without a hand)."""
    t = {k: torch.from_numpy(np.asarray(v)).to(device).to(torch.float64) for k, v in case.items()
         if k != "model_points" and v is not None}
    preds = {k: t[k].clone().requires_grad_(True) for k in ("classification", "regression", "transformation", "hand") if k in t}
    out, per = batch_losses(t["gt_classification"], preds["classification"], t["gt_regression"], preds["regression"],
                            t["gt_transformation"], preds["transformation"], t.get("gt_hand"), preds.get("hand"), case["model_points"], 3)
    if upstream is None:
        w = torch.tensor(weights, dtype=torch.float64, device=device)
        total = (out * w).sum()          # NaN when an image has no object anchors (its translation loss), like the
        # reference's total - its gradients are finite all the same: the NaN term has no prediction to reach
    else:
        total = upstream(out, per)
    names = [k for k in ("classification", "regression", "transformation", "hand") if k in preds]
    grads = torch.autograd.grad(total, [preds[k] for k in names], allow_unused=True)
    res = {k: (g.detach().cpu().numpy() if g is not None else np.zeros(preds[k].shape)) for k, g in zip(names, grads)}
    res.setdefault("hand", None)
    return res


def expand_golden(fx, name, shapes):
    """Dense float64 gradients of case ``name`` from tests/golden/loss_grads.npz (rows stored sparsely)."""
    out = {"classification": fx[f"{name}.classification"].astype(np.float64)}
    for key in ("regression", "transformation", "hand"):
        B, N, W = shapes[key]
        g = np.zeros((B * N, W))
        g[fx[f"{name}.{key}_rows"]] = fx[f"{name}.{key}"]
        out[key] = g.reshape(B, N, W)
    return out
