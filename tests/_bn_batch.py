"""Shared by the batch-statistics BatchNorm tests and tests/golden/make_golden_bn_batch.py.

The oracle's one BatchNorm function (``oracle.efficientpose_ref.bn``) is replaced by ``F.batch_norm(training=True, momentum
0.01, eps 1e-3)`` on cloned buffers for the length of a ``with`` block; the seeded inputs, the oracle autograd and the digest
convention are those of tests/_head_grad.py, _neck_grad.py and _backbone_grad.py, used as they are.  On top: the cases, the
analytic-zero rule and one error bookkeeping for the three parts."""
import contextlib
import re

import numpy as np
import torch
import torch.nn.functional as F

from tests import _backbone_grad as G
from tests import _head_grad as H
from tests import _neck_grad as N

MOMENTUM, EPS = 0.01, 1e-3
BOUND_FACTOR, BOUND_FLOOR = 4.0, 2e-6             # the project's convention (tests/test_gpu_head_grads.py)
ZERO_REL = 1e-9                                    # "analytically zero": max |g64| below this x the largest BatchNorm-bias gradient
PARTS = ("heads", "neck", "backbone")
# part -> tag -> (phi, size, batch, weight seed, num_classes | None, drop-connect (rate, torch seed) | None).  Every gradient case
# has at least 8 rows at every BatchNorm: a BatchNorm with 2 rows is ill-conditioned (float32 torch on the CPU is 1.6e-5 off there
# against 2e-6 with 8 rows).  Neck: weight seed 4, which leaves no conv / lateral / BatchNorm tensor behind a relu-dead fusion
# entry (tests/test_gpu_neck_grads.py), so the analytic-zero set is the structural one.
CASES = {
    "heads": {
        "phi0_s128_b8": (0, 128, 8, 0, 1, None),   # 2 728 rows: several split-K slabs; 8 rows at P7
        "phi0_s256_b2": (0, 256, 2, 0, 1, None),   # a 2 x 2 top level
        "phi3_s128_b8": (3, 128, 8, 0, 1, None),   # width 160, depth 4, n-tiles that are not full
    },
    "neck": {
        "phi0_s128_b8": (0, 128, 8, 4, None, None),
        "phi0_s256_b2": (0, 256, 2, 4, None, None),
        "phi3_s128_b8": (3, 128, 8, 4, None, None),
    },
    "backbone": {
        "phi0_s128_b2": (0, 128, 2, 0, None, None),
        "phi3_s128_b1": (3, 128, 1, 0, None, None),
        "phi0_s128_b2_dropconnect": (0, 128, 2, 0, None, (G.DROP_RATE, G.DROP_TORCH_SEED)),   # a recorded table at rate 0.2
    },
}
GOLDEN = {"heads": "phi0_s128_b8", "neck": "phi0_s128_b8", "backbone": "phi0_s128_b2"}
N2_CASE = (0, 128, 2, 0, 1, None)                  # heads and neck: 2 rows at P7, forward only
N1_CASE = (0, 128, 1, 0, 1, None)                  # 1 row at P7: refused
# the tensors whose gradient is analytically zero under batch statistics: a bias in front of a BatchNorm (heads, neck); bn2's bias
# of the blocks whose output reaches, through skip adds, only bias-free 1 x 1 convs that feed a BatchNorm (backbone)
ZERO_PATTERN = {
    "heads": re.compile(r"^\w+\.conv_list\.\d+\.pointwise_conv\.conv\.bias$"),
    "neck": re.compile(r"^bifpn\.\d+\.\w+(\.pointwise_conv|\.0)\.conv\.bias$"),
    "backbone": re.compile(r"^backbone_net\.model\._blocks\.\d+\._bn2\.bias$"),
}


@contextlib.contextmanager
def batch_statistics(record=None, observe=None):
    """``oracle.efficientpose_ref.bn`` as training-mode BatchNorm.  The running statistics of the state dict are cloned, never
    written; ``record`` (a dict) receives the updated clones under their state_dict keys; ``observe(prefix, x)`` sees every
    BatchNorm's input."""
    from oracle import efficientpose_ref as R

    def bn(sd, p, x):
        if observe is not None:
            observe(p, x.detach())
        rm, rv = sd[p + ".running_mean"].detach().clone(), sd[p + ".running_var"].detach().clone()
        y = F.batch_norm(x, rm, rv, sd[p + ".weight"], sd[p + ".bias"], True, MOMENTUM, EPS)
        if record is not None:
            record[p + ".running_mean"], record[p + ".running_var"] = rm, rv
        return y

    saved = R.bn
    R.bn = bn
    try:
        yield
    finally:
        R.bn = saved


def one_thread(fn, *args, **kwargs):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn(*args, **kwargs)
    finally:
        torch.set_num_threads(threads)


def keys(part, case):
    """(key, shape) of the part's float tensors in flat-buffer order."""
    phi, classes = case[0], case[4]
    return H.head_keys(phi, classes) if part == "heads" else N.neck_keys(phi) if part == "neck" else G.backbone_keys(phi)


def trainable(key):
    return not key.endswith(("running_mean", "running_var"))


def is_bn_bias(key):
    """A BatchNorm's beta: a ``bias`` that is not a conv's."""
    return key.endswith(".bias") and not key.endswith("conv.bias")


def scales_of(part, case):
    """The backbone's drop-connect table [blocks, B] (float32 CPU tensor) of a case, or None."""
    phi, _size, batch, _seed, _classes, drop = case
    return G.reference_scales(phi, drop[0], batch, drop[1]) if part == "backbone" and drop else None


def inputs(part, case):
    """(list of input arrays, list of cotangent arrays), float32 numpy."""
    phi, size, batch, seed, classes, _drop = case
    if part == "heads":
        return H.seeded_maps(phi, size, batch, seed + 1), H.seeded_cotangents(classes, size, batch, seed + 2)
    if part == "neck":
        return N.seeded_inputs(phi, size, batch)
    image, cots = G.seeded_inputs(phi, size, batch)
    return [image], cots


def oracle(part, sd, case, dtype, argmax=None, statistics="batch", observe=None):
    """The patched oracle in ``dtype`` on the CPU: dict(outs, grads {key: grad of every trainable tensor}, gin [input gradients],
    stats {running key: the buffer after the forward}, pool).  Neck: ``argmax`` routes the max-pools and ``pool`` is the
    tests/_neck_grad.RoutedPool that did it (its slack and scale lists).  ``statistics`` "running": the oracle as it is (eval-mode
    BatchNorm, no stats); ``observe``: see ``batch_statistics``."""
    phi, classes = case[0], case[4]
    x, cots = inputs(part, case)
    stats, pool = {}, None
    with batch_statistics(stats, observe) if statistics == "batch" else contextlib.nullcontext():
        if part == "heads":
            outs, grads, gin = H.oracle_grads(sd, x, cots, phi, classes, dtype)
        elif part == "neck":
            pool = N.RoutedPool(argmax)
            outs, grads, gin = N.oracle_grads(sd, x, cots, phi, dtype, pool)
        else:
            outs, grads, gimg = G.oracle_grads(sd, x[0], cots, phi, dtype, scales_of(part, case))
            gin = [gimg]
    return dict(outs=list(outs), grads=grads, gin=list(gin), stats=stats, pool=pool)


def zero_set(g64):
    """Names of the tensors with max |g64| < ZERO_REL x the largest max |g64| among the BatchNorm ``bias`` gradients."""
    amax = {k: float(v.abs().max()) for k, v in g64.items()}
    top = max(v for k, v in amax.items() if is_bn_bias(k))
    return sorted(k for k, v in amax.items() if v < ZERO_REL * top)


def _np(a):
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def group_errors(got, ref, zeros):
    """Worst error against the float64 ``ref`` per group.  outputs / gradients: per tensor max |a - b| / max |b| (gradients: the
    input gradients and every trainable tensor outside ``zeros`` and outside the fusion scalars); fusion (neck): on ONE scale, the
    largest |g64| over all fusion tensors (tests/_neck_grad.group_errors); zeros: the largest |g| over the analytic-zero set."""
    out = {"outputs": max(H.rel_err(_np(a), _np(b)) for a, b in zip(got["outs"], ref["outs"]))}
    errs = {k: H.rel_err(_np(got["grads"][k]), _np(v)) for k, v in ref["grads"].items() if k not in zeros and not N.is_fusion(k)}
    errs.update({f"input.{i}": H.rel_err(_np(a), _np(b)) for i, (a, b) in enumerate(zip(got["gin"], ref["gin"]))})
    worst = max(errs, key=errs.get)
    out["gradients"], out["worst_gradient"] = errs[worst], worst
    fusion = [k for k in ref["grads"] if N.is_fusion(k)]
    if fusion:
        fscale = max(float(np.abs(_np(ref["grads"][k])).max()) for k in fusion)
        out["fusion"] = max(float(np.abs(_np(got["grads"][k]) - _np(ref["grads"][k])).max()) for k in fusion) / fscale
    out["zeros"] = max(float(np.abs(_np(got["grads"][k])).max()) for k in zeros) if zeros else 0.0
    return out


def tensor_errors(got, ref, zeros):
    """Error against the float64 ``ref`` PER TENSOR, name -> e: every output ("out.<i>"), every input gradient ("input.<i>") and
    every trainable tensor outside ``zeros``, each max |a - b| / max |b|; the neck's fusion scalars on their one common scale
    (``group_errors``).  A tensor whose gradient nearly cancels then widens only its own bound."""
    errs = {f"out.{i}": H.rel_err(_np(a), _np(b)) for i, (a, b) in enumerate(zip(got["outs"], ref["outs"]))}
    errs.update({f"input.{i}": H.rel_err(_np(a), _np(b)) for i, (a, b) in enumerate(zip(got["gin"], ref["gin"]))})
    fusion = [k for k in ref["grads"] if N.is_fusion(k) and k not in zeros]
    fscale = max([float(np.abs(_np(ref["grads"][k])).max()) for k in fusion] or [1.0])
    for k, v in ref["grads"].items():
        if k in zeros:
            continue
        errs[k] = float(np.abs(_np(got["grads"][k]) - _np(v)).max()) / fscale if N.is_fusion(k) else H.rel_err(_np(got["grads"][k]), _np(v))
    return errs


def stat_errors(got, ref):
    """Worst max |a - b| / max |b| per buffer kind over the updated running statistics."""
    return {kind: max(H.rel_err(_np(got[k]), _np(v)) for k, v in ref.items() if k.endswith(kind)) for kind in ("running_mean", "running_var")}


def bound(e32):
    return max(BOUND_FACTOR * e32, BOUND_FLOOR)


def golden_names(part, case):
    """Order of the tensors of one case of tests/golden/bn_batch_grads.npz: the part's existing order (outputs, input gradients,
    gradients of the trainable tensors), then the running statistics after one forward."""
    phi, classes = case[0], case[4]
    base = H.golden_names(phi, classes) if part == "heads" else N.golden_names(phi) if part == "neck" else G.golden_names(phi)
    return base + ["stat." + k for k, _ in keys(part, case) if not trainable(k)]


def golden_tensors(part, case, res):
    """name -> array for ``golden_names`` from a result dict (``oracle``'s layout)."""
    phi, classes = case[0], case[4]
    base = H.golden_names(phi, classes) if part == "heads" else N.golden_names(phi) if part == "neck" else G.golden_names(phi)
    nouts, nin = len(res["outs"]), len(res["gin"])
    t = dict(zip(base[:nouts], res["outs"]))
    t.update(zip(base[nouts:nouts + nin], res["gin"]))
    t.update({"param." + k: v for k, v in res["grads"].items()})
    t.update({"stat." + k: v for k, v in res["stats"].items()})
    return {k: _np(v) for k, v in t.items()}
