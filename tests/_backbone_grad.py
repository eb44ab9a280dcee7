"""Shared by the backbone-gradient tests and tests/golden/make_golden_backbone_grads.py: seeded image / cotangents, the
oracle's autograd through oracle.efficientpose_ref.backbone, a restatement of its block loop with drop-connect branch scales
(built from the oracle's conv_same / bn / swish), the error groups and the tensor order of the golden archive.  Digests:
tests/_head_grad.py."""
import numpy as np
import torch
import torch.nn.functional as F

from hmd_ego_pose_amd.arch import get_arch, param_spec
from tests._head_grad import digest, digest_stride, golden_entry, pack_digests, rel_err  # noqa: F401

# tag -> (phi, size, batch, weight seed): the deterministic cases of tests/golden/backbone_grads.npz (eval(), input seed 0)
GOLDEN_CASES = {
    "phi0_s128_b2": (0, 128, 2, 0),
    "phi3_s128_b1": (3, 128, 1, 0),
}
# the drop-connect case of the archive: model.train() with every BatchNorm in eval(), torch.manual_seed(DROP_TORCH_SEED) right
# before the reference's forward, the reference's own global rate (efficientnet/utils.py: drop_connect_rate = 0.2)
DROP_TAG, DROP_CASE, DROP_TORCH_SEED, DROP_RATE = "phi0_s128_b2_dropconnect", (0, 128, 2, 0), 11, 0.2
INPUT_SEED = 0
PREFIX = "backbone_net."
GROUPS = ("taps", "image", "conv", "bn_bias")


def backbone_keys(phi):
    """(key, shape) of the float backbone_net.* tensors in state_dict order (no num_batches_tracked)."""
    return [(k, s) for k, s in param_spec(phi) if k.startswith(PREFIX) and not k.endswith("num_batches_tracked")]


def trainable(key):
    return not key.endswith(("running_mean", "running_var"))


def is_conv_weight(key):
    """Stem, expand, depthwise, squeeze-excite and project weights; the rest of the trainable tensors are BatchNorm weight /
    bias and the two squeeze-excite biases."""
    return key.endswith("conv.weight")


def seeded_inputs(phi, size, batch, seed=INPUT_SEED):
    """ONE generator: the image [B, 3, S, S], then the three cotangents [B, tap_channels[t], s, s] (float32 numpy)."""
    a = get_arch(phi)
    rng = np.random.Generator(np.random.PCG64([seed, 78]))
    image = rng.standard_normal((batch, 3, size, size)).astype(np.float32)
    cots = [rng.standard_normal((batch, c, size // (8 << t), size // (8 << t))).astype(np.float32) for t, c in enumerate(a.tap_channels)]
    return image, cots


def reference_scales(phi, rate, batch, torch_seed):
    """The drop-connect scale table [blocks, B] the reference's formula gives after torch.manual_seed(torch_seed)
    (efficientnet/utils.py:85-94, rate of efficientdet/model.py:447-449): in block order one torch.rand([B, 1, 1, 1]) per block
    that adds its input and has a non-zero rate; floor(keep + U) / keep.  float32, CPU."""
    from oracle import efficientpose_ref as R
    blocks = R.block_table(phi)
    torch.manual_seed(torch_seed)
    rows = []
    for idx, blk in enumerate(blocks):
        p = rate * float(idx) / len(blocks) if rate else rate
        if blk["skip"] and p:
            keep = 1 - p
            random_tensor = keep + torch.rand([batch, 1, 1, 1], dtype=torch.float32)
            rows.append((torch.floor(random_tensor) / keep).reshape(batch))
        else:
            rows.append(torch.ones(batch, dtype=torch.float32))
    return torch.stack(rows)


def oracle_backbone(sd, x, phi, scales=None, trace=None):
    """The three taps.  scales None: oracle.efficientpose_ref.backbone itself.  Otherwise its loop restated with the residual
    branch of every block that adds its input multiplied by scales[i][b] (MBConvBlock.forward with drop_connect)."""
    from oracle import efficientpose_ref as R
    if scales is None:
        return R.backbone(sd, phi, x, trace)
    bb = "backbone_net.model"
    x = R.swish(R.bn(sd, bb + "._bn0", R.conv_same(x, sd[bb + "._conv_stem.conv.weight"], stride=2)))
    taps, last = [], None
    blocks = R.block_table(phi)
    for i, blk in enumerate(blocks):
        p, inp = f"{bb}._blocks.{i}", x
        if blk["e"] != 1:
            x = R.swish(R.bn(sd, p + "._bn0", R.conv_same(x, sd[p + "._expand_conv.conv.weight"])))
        wdw = sd[p + "._depthwise_conv.conv.weight"]
        x = R.swish(R.bn(sd, p + "._bn1", R.conv_same(x, wdw, stride=blk["s"], groups=wdw.shape[0])))
        sq = F.adaptive_avg_pool2d(x, 1)
        sq = R.swish(F.conv2d(sq, sd[p + "._se_reduce.conv.weight"], sd[p + "._se_reduce.conv.bias"]))
        sq = F.conv2d(sq, sd[p + "._se_expand.conv.weight"], sd[p + "._se_expand.conv.bias"])
        x = torch.sigmoid(sq) * x
        x = R.bn(sd, p + "._bn2", R.conv_same(x, sd[p + "._project_conv.conv.weight"]))
        if blk["skip"]:
            x = x * scales[i].to(x.dtype).view(-1, 1, 1, 1) + inp
        if blk["s"] == 2:
            taps.append(last)
        elif i == len(blocks) - 1:
            taps.append(x)
        last = x
    return taps[-3:]


def oracle_grads(sd, image, cots, phi, dtype=torch.float64, scales=None):
    """Gradients of sum_t <tap_t, cot_t> through the oracle's backbone, evaluated in ``dtype`` on the CPU.  Returns (taps,
    {key: grad} for the trainable tensors - zeros where autograd reaches none -, the image gradient) as ``dtype`` tensors."""
    t = lambda a: (torch.from_numpy(a) if isinstance(a, np.ndarray) else a.detach().cpu()).to(dtype)
    p = {}
    for k, _ in backbone_keys(phi):
        v = t(sd[k]).clone()
        p[k] = v.requires_grad_(True) if trainable(k) else v
    x = t(image).clone().requires_grad_(True)
    taps = oracle_backbone(p, x, phi, None if scales is None else t(scales))
    sum((f * t(c)).sum() for f, c in zip(taps, cots)).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items() if trainable(k)}
    return [f.detach() for f in taps], grads, x.grad


def golden_names(phi):
    """Order of the tensors of one golden case: the three taps, the image gradient, gradients of the trainable tensors."""
    return [f"tap.{t}" for t in range(3)] + ["image"] + ["param." + k for k, _ in backbone_keys(phi) if trainable(k)]


def group_errors(taps, gimage, grads, ref_taps, ref_image, ref_grads):
    """Worst per-tensor error (max |a - b| / max |b|) per group against the float64 reference values: taps forward, image
    gradient, conv weights (stem, expand, depthwise, squeeze-excite, project), BatchNorm weights / biases and SE biases."""
    n = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    return {"taps": max(rel_err(n(a), n(b)) for a, b in zip(taps, ref_taps)),
            "image": rel_err(n(gimage), n(ref_image)),
            "conv": max(rel_err(n(grads[k]), n(v)) for k, v in ref_grads.items() if is_conv_weight(k)),
            "bn_bias": max(rel_err(n(grads[k]), n(v)) for k, v in ref_grads.items() if not is_conv_weight(k))}


def group_of(key):
    return "conv" if is_conv_weight(key) else "bn_bias"
