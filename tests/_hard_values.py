"""Weights that put every kernel where a trained network puts it, shared by tests/test_hard_values_cpu.py and
tests/test_gpu_hard_values.py.

``hmd_ego_pose_amd.weights.seeded_state_dict`` keeps activations O(1) on purpose, so no seeded parity case reaches an activation
tail (|x| > 88.7, where exp overflows in float32), a dead BatchNorm channel, a saturated squeeze-excite gate, a fusion node whose
weights are all relu-dead, or a classification score of exactly 0 or 1.  The recipe here starts from the seeded weights, shifts
BatchNorm and squeeze-excite biases into both tails, zeroes and negates some gammas, sets a focal-loss prior on the classifier
and four hostile fusion vectors, and then re-measures every BatchNorm's running statistics on seeded calibration frames (without
that the shifted network overflows within a dozen blocks).  Nothing measured is committed: the statistics are computed when a
test asks for them (one CPU oracle pass over CAL_FRAMES frames of CAL_SIZE x CAL_SIZE).

Offsets stay out of (-104, -87): there x * sigmoid(x) is a float32 denormal and the CPU oracle slows down fifty-fold.  -105 and
-120 still overflow exp(-x) on the device and give exactly 0 on the CPU."""
import functools

import numpy as np
import torch

from tests._bn_batch import BOUND_FACTOR, BOUND_FLOOR
from tests._head_grad import OUT_NAMES as HEADS
from tests._util import seeded_input

BN_OFFSETS = (0.0, -120.0, -105.0, -30.0, 30.0, 95.0, 120.0, 0.0)      # bias[c] += BN_OFFSETS[c % 8]
GAMMA_ZERO, GAMMA_NEGATED, GAMMA_PERIOD = 9, 11, 16                      # weight[c] = 0 / negated where c % 16 is 9 / 11
SE_OFFSETS = (0.0, -100.0, 100.0, 0.0)                                   # squeeze-excite reduce and expand biases, c % 4
CLASSIFIER_BIAS = -4.595                                                 # -log((1 - 0.01) / 0.01): the focal-loss prior
FUSION = {"bifpn.0.p6_w1": (-0.5, -1.0),        # every weight below zero: relu sum 0, divisor 1e-4, node input exactly 0
          "bifpn.0.p4_w2": (0.0, 0.0, 0.0),     # every weight exactly zero
          "bifpn.1.p5_w1": (1e3, 1e-3),         # six orders of magnitude apart
          "bifpn.1.p7_w2": (-1.0, 2.0)}         # one relu-dead entry
CAL_SIZE, CAL_FRAMES = 128, 4
CONSTANT_FRAME = (0.75, -1.5, 2.25)             # image 0 of every hard input: one value per colour channel

# The inference sessions tests/test_gpu_hard_values.py holds to the oracle: (phi, size, batch, dtype, num_classes).  The CPU suite
# checks that these reach every device function of the benchmarked plans (test_hard_values_cpu.py).
SESSIONS = [(0, 256, 16, "fp32", 1), (0, 256, 16, "bf16", 1), (3, 512, 8, "bf16", 1), (0, 256, 2, "fp32", 3)]
# the benchmarked configurations (BASELINE.json) whose default plans the sessions above must cover
BASELINE_PLANS = [(0, 256, 16, "fp32"), (0, 256, 16, "bf16"), (3, 512, 8, "bf16")]


def _is_bn(sd, key):
    return key.endswith(".weight") and key[:-len("weight")] + "running_var" in sd


def hard_edits(sd, phi):
    """The edits of the recipe on a copy of ``sd`` (any float dtype), running statistics untouched."""
    out = {k: v.clone() for k, v in sd.items()}
    for key in sd:
        if _is_bn(sd, key):
            w, b = out[key], out[key[:-len("weight")] + "bias"]
            c = torch.arange(w.numel())
            b += torch.tensor(BN_OFFSETS, dtype=b.dtype)[c % len(BN_OFFSETS)]
            w[c % GAMMA_PERIOD == GAMMA_ZERO] = 0
            w[c % GAMMA_PERIOD == GAMMA_NEGATED] *= -1
        elif key.endswith(("_se_reduce.conv.bias", "_se_expand.conv.bias")):
            b = out[key]
            b += torch.tensor(SE_OFFSETS, dtype=b.dtype)[torch.arange(b.numel()) % len(SE_OFFSETS)]
    out["classifier.header.pointwise_conv.conv.bias"].fill_(CLASSIFIER_BIAS)
    if phi < 6:                                  # phi 6 and 7 fuse with a plain sum
        for key, w in FUSION.items():
            if key in out:
                out[key] = torch.tensor(w, dtype=out[key].dtype)
    return out


def calibrate(sd, phi, size, frames, seed=0):
    """{running_mean / running_var key: tensor}: one pass of the CPU oracle over ``frames`` seeded calibration frames in which every
    BatchNorm measures the per-channel mean and (biased) variance of its own input, behind the already calibrated layers in front
    of it, and normalises with them.  ``sd`` is not written."""
    from oracle import efficientpose_ref as R
    work = dict(sd)
    rng = np.random.Generator(np.random.PCG64([seed, 0xCA1B]))             # calibration frames: not the frames any test evaluates
    x = torch.from_numpy(rng.standard_normal((frames, 3, size, size)).astype(np.float32))
    stats = {}
    plain_bn = R.bn

    def measuring_bn(sd_, p, t):
        m = t.mean(dim=(0, 2, 3)); v = t.var(dim=(0, 2, 3), unbiased=False)
        sd_[p + ".running_mean"] = stats[p + ".running_mean"] = m.clone()
        sd_[p + ".running_var"] = stats[p + ".running_var"] = v.clone()
        return plain_bn(sd_, p, t)

    R.bn = measuring_bn
    try:
        with torch.no_grad():
            R.forward(work, x, phi)
    finally:
        R.bn = plain_bn
    return stats


@functools.lru_cache(maxsize=4)
def hard_state_dict(phi, seed=0, num_classes=1):
    """The recipe on ``seeded_state_dict(phi, seed)``, calibrated.  Deterministic; kept for the next caller, read-only for all."""
    from hmd_ego_pose_amd.weights import seeded_state_dict
    sd = hard_edits(seeded_state_dict(phi, seed, num_classes=num_classes), phi)
    sd.update(calibrate(sd, phi, CAL_SIZE, CAL_FRAMES, seed))
    return sd


def as_double(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def hard_input(size, batch, seed=0):
    """``seeded_input`` with image 0 replaced by a constant frame: every interior depthwise output of that image is the same
    value, so a SAME-padding or halo error stands alone at the border."""
    x = torch.from_numpy(seeded_input((batch, 3, size, size), seed))
    x[0] = torch.tensor(CONSTANT_FRAME).view(3, 1, 1)
    return x


def stage_outputs(st, kind, index, inputs):
    """name -> output of one stage of ``oracle.efficientpose_ref.emulated_stages`` (kind "stem", "block", "cell" or "heads"), named
    as the teacher-forced helpers of tests/test_gpu_parity.py name the device's tensors."""
    if kind == "stem":
        return {"stem": st["stem"](inputs)}
    if kind == "block":
        return {f"block{index}": st["block"](index, inputs)}
    if kind == "cell":
        return {f"c{index}.p{l + 3}_out": t for l, t in enumerate(st["cell"](index, list(inputs)))}
    return dict(zip(HEADS, st["heads"](list(inputs))))


def _abs_err(got, want64):
    return (torch.as_tensor(got).double() - want64).abs(), want64.abs()


def tensor_err(got, want64):
    """max |got - want| / max(1, max |want|) over the tensor."""
    err, mag = _abs_err(got, want64)
    return err.max().item() / max(1.0, mag.max().item())


def channel_err(got, want64, dim=1):
    """The same per output channel (``dim``: 1 for NCHW maps, -1 for the [B, N, K] heads): the worst channel.  Sees a dead or
    small channel next to one of magnitude 1e2 .. 1e5, which the tensor-wide scale hides."""
    err, mag = _abs_err(got, want64)
    other = [d for d in range(err.dim()) if d != dim % err.dim()]
    return (err.amax(dim=other) / mag.amax(dim=other).clamp(min=1.0)).max().item()


def channel_bound(want32, want64, dim=1):
    """Bound of ``channel_err`` for a device stage: BOUND_FACTOR x the float32 CPU oracle's own channel_err against the float64
    oracle on the same input, floor BOUND_FLOOR (tests/_bn_batch.py).  Never computed from a device value."""
    return max(BOUND_FLOOR, BOUND_FACTOR * channel_err(want32, want64, dim))
