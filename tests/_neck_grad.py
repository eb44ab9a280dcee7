"""Shared by the neck-gradient tests and tests/golden/make_golden_neck_grads.py: seeded taps / cotangents, the oracle's
autograd through ``fpn_cells`` calls of oracle.efficientpose_ref.bifpn_cell, the routed max-pool (gather at given argmax
positions, for teacher-forced routing) and the tensor order of the golden archive.  Digests: tests/_head_grad.py."""
import re

import numpy as np
import torch
import torch.nn.functional as F

from hmd_ego_pose_amd.arch import get_arch, level_sizes, param_spec
from tests._head_grad import digest, digest_stride, golden_entry, pack_digests, rel_err  # noqa: F401

# tag -> (phi, size, batch, weight seed): the cases of tests/golden/neck_grads.npz (input seed 0)
GOLDEN_CASES = {
    "phi0_s128_b2": (0, 128, 2, 0),
    "phi3_s128_b1": (3, 128, 1, 0),
}
INPUT_SEED = 0
_FUSION = re.compile(r"\.p\d_w[12]$")


def neck_keys(phi):
    """(key, shape) of the float bifpn.* tensors in state_dict order (no num_batches_tracked)."""
    return [(k, s) for k, s in param_spec(phi) if k.startswith("bifpn.") and not k.endswith("num_batches_tracked")]


def trainable(key):
    return not key.endswith(("running_mean", "running_var"))


def is_fusion(key):
    return _FUSION.search(key) is not None


def seeded_inputs(phi, size, batch, seed=INPUT_SEED):
    """ONE generator: the taps P3, P4, P5 [B, tap_channels[t], s, s], then the five cotangents [B, W, s_l, s_l] (float32 numpy)."""
    a = get_arch(phi)
    rng = np.random.Generator(np.random.PCG64([seed, 77]))
    taps = [rng.standard_normal((batch, c, size // (8 << t), size // (8 << t))).astype(np.float32) for t, c in enumerate(a.tap_channels)]
    cots = [rng.standard_normal((batch, a.fpn_w, s, s)).astype(np.float32) for s in level_sizes(size)]
    return taps, cots


def pool_names(phi):
    """The inputs of the max-pools in the order bifpn_cell calls maxpool_same (names of hep_neck_stage_info / the oracle's trace)."""
    names = ["p6_pre", "bifpn0_p6_in"]
    for r in range(get_arch(phi).fpn_cells):
        names += [f"bifpn{r}_p{l}" for l in (3, 4, 5, 6)]
    return names


def pool_windows(x):
    """[B, C, s/2, s/2, 9]: the zero-padded 3 x 3 stride-2 windows of maxpool_same (one column right, one row below), row-major."""
    assert x.shape[-1] % 2 == 0 and x.shape[-2] % 2 == 0
    xp = F.pad(x, [0, 1, 0, 1])
    w = xp.unfold(2, 3, 2).unfold(3, 3, 2)
    return w.reshape(*w.shape[:4], 9)


def first_argmax(x):
    """Position 0..8 of the first maximum of every padded window (torch.argmax returns the first)."""
    return pool_windows(x).argmax(dim=-1)


class RoutedPool:
    """Stands in for efficientpose_ref.maxpool_same: call k gathers the input's own values at ``argmax[k]`` (so autograd routes
    there) and records slack = max over windows of (true window maximum - gathered value) and the input's largest magnitude.
    argmax=None: use the input's own first maximum (then the values equal maxpool_same and the slack is 0)."""

    def __init__(self, argmax=None):
        self.argmax, self.k, self.slack, self.scale, self.own = argmax, 0, [], [], []

    def __call__(self, x):
        w = pool_windows(x)
        own = w.argmax(dim=-1)
        idx = own if self.argmax is None else self.argmax[self.k].to(x.device)
        self.k += 1
        v = w.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
        self.slack.append(float((w.max(dim=-1).values - v).max().detach()))
        self.scale.append(float(x.abs().max().detach()))
        self.own.append(own)
        return v


def oracle_neck(sd, taps, phi, pool=None):
    """The five maps through fpn_cells calls of oracle.efficientpose_ref.bifpn_cell (autograd-tracked when the inputs are).
    pool: a RoutedPool to stand in for maxpool_same during the call (the module attribute is restored afterwards)."""
    from oracle import efficientpose_ref as R
    keep = R.maxpool_same
    if pool is not None:
        R.maxpool_same = pool
    try:
        feats = tuple(taps)
        for r in range(get_arch(phi).fpn_cells):
            feats = R.bifpn_cell(sd, f"bifpn.{r}", feats, first=(r == 0), attention=True)
    finally:
        R.maxpool_same = keep
    return feats


def oracle_grads(sd, taps, cots, phi, dtype=torch.float64, pool=None):
    """Gradients of sum_l <map_l, cot_l> through the oracle's neck, evaluated in ``dtype`` on the CPU.  Returns (maps,
    {key: grad} for the trainable tensors - zeros where autograd reaches none -, [three tap gradients]) as ``dtype`` tensors."""
    t = lambda a: (torch.from_numpy(a) if isinstance(a, np.ndarray) else a.detach().cpu()).to(dtype)
    p = {}
    for k, _ in neck_keys(phi):
        v = t(sd[k]).clone()
        p[k] = v.requires_grad_(True) if trainable(k) else v
    x = [t(a).clone().requires_grad_(True) for a in taps]
    feats = oracle_neck(p, x, phi, pool)
    sum((f * t(c)).sum() for f, c in zip(feats, cots)).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items() if trainable(k)}
    return [f.detach() for f in feats], grads, [a.grad for a in x]


def golden_names(phi):
    """Order of the tensors of one golden case: the five maps, the three tap gradients, gradients of the trainable tensors."""
    return [f"map.{l}" for l in range(5)] + [f"tap.{t}" for t in range(3)] + ["param." + k for k, _ in neck_keys(phi) if trainable(k)]


def group_errors(maps, gtaps, grads, ref_maps, ref_taps, ref_grads):
    """Worst error per group against the float64 reference values: maps forward and tap gradients and conv / BatchNorm gradients
    per tensor (max |a - b| / max |b|), the fusion gradients on ONE scale (the largest |g64| over all fusion tensors)."""
    n = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    out = {"maps": max(rel_err(n(a), n(b)) for a, b in zip(maps, ref_maps)),
           "taps": max(rel_err(n(a), n(b)) for a, b in zip(gtaps, ref_taps)),
           "conv_bn": max(rel_err(n(grads[k]), n(v)) for k, v in ref_grads.items() if not is_fusion(k))}
    fscale = max(float(np.abs(n(v)).max()) for k, v in ref_grads.items() if is_fusion(k))
    out["fusion"] = max(float(np.abs(n(grads[k]) - n(v)).max()) for k, v in ref_grads.items() if is_fusion(k)) / fscale
    return out
