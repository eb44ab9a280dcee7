"""Shared by the head-gradient tests and tests/golden/make_golden_head_grads.py: seeded maps / cotangents, the oracle's
autograd through the five head nets (oracle.efficientpose_ref.head) and the digest convention of the golden archive."""
import numpy as np
import torch

from hmd_ego_pose_amd.arch import HEAD_NAMES, NUM_ANCHORS, get_arch, level_sizes, param_spec

OUT_NAMES = ("regression", "classification", "rotation", "translation_raw", "hand")
# tag -> (phi, num_classes, size, batch, weight seed): the cases of tests/golden/head_grads.npz
GOLDEN_CASES = {
    "phi0_s128_b2": (0, 1, 128, 2, 0),
    "phi0_s128_b2_k3": (0, 3, 128, 2, 0),
    "phi3_s128_b1": (3, 1, 128, 1, 0),
}


def digest_stride(numel):
    """Prime stride of the committed slice of a flattened tensor: small tensors keep every 7th value."""
    return 97 if numel > 4096 else 7


def head_keys(phi, num_classes=1):
    """(key, shape) of the float head tensors in state_dict order (no num_batches_tracked)."""
    return [(k, s) for k, s in param_spec(phi, num_classes) if k.split(".", 1)[0] in HEAD_NAMES and not k.endswith("num_batches_tracked")]


def trainable(key):
    return not key.endswith(("running_mean", "running_var"))


def out_widths(num_classes):
    return (4, num_classes, 3, 3, 63)


def seeded_maps(phi, size, batch, seed):
    """Five unit-normal maps [B, W, s, s] (float32 numpy)."""
    w = get_arch(phi).fpn_w
    rng = np.random.Generator(np.random.PCG64([seed, 0x4ead]))
    return [rng.standard_normal((batch, w, s, s)).astype(np.float32) for s in level_sizes(size)]


def seeded_cotangents(num_classes, size, batch, seed):
    """Five unit-normal cotangents [B, N, K] (float32 numpy)."""
    n = NUM_ANCHORS * sum(s * s for s in level_sizes(size))
    rng = np.random.Generator(np.random.PCG64([seed, 0xc07a]))
    return [rng.standard_normal((batch, n, k)).astype(np.float32) for k in out_widths(num_classes)]


def oracle_heads(sd, feats, phi, num_classes):
    """The five head outputs through oracle.efficientpose_ref.head (autograd-tracked when the inputs are)."""
    from oracle import efficientpose_ref as R
    d = get_arch(phi).head_depth
    return (R.head(sd, "regressor", d, feats, [("header", 4)]),
            R.head(sd, "classifier", d, feats, [("header", num_classes)], sigmoid=True),
            R.head(sd, "rotation_net", d, feats, [("initial_rotation", 3)]),
            R.head(sd, "translation_net", d, feats, [("initial_translation_xy", 2), ("initial_translation_z", 1)]),
            R.head(sd, "hand_net", d, feats, [("initial_hand_coords", 63)]))


def oracle_grads(sd, feats, cots, phi, num_classes, dtype=torch.float64):
    """Gradients of sum_k <out_k, cot_k> through the oracle's heads, evaluated in ``dtype`` on the CPU.
    sd: head tensors (any float dtype), feats / cots: sequences of arrays or tensors.  Returns (outs, {key: grad} for the
    trainable tensors, [five map gradients]) as ``dtype`` CPU tensors."""
    t = lambda a: (torch.from_numpy(a) if isinstance(a, np.ndarray) else a.detach().cpu()).to(dtype)
    p = {}
    for k, _ in head_keys(phi, num_classes):
        v = t(sd[k]).clone()
        p[k] = v.requires_grad_(True) if trainable(k) else v
    f = [t(a).clone().requires_grad_(True) for a in feats]
    outs = oracle_heads(p, f, phi, num_classes)
    total = sum((o * t(c)).sum() for o, c in zip(outs, cots))
    total.backward()
    return [o.detach() for o in outs], {k: v.grad for k, v in p.items() if trainable(k)}, [a.grad for a in f]


def golden_names(phi, num_classes):
    """Order of the tensors of one golden case: head outputs, map gradients, gradients of the trainable head tensors."""
    return ([f"out.{n}" for n in OUT_NAMES] + [f"feat.{l}" for l in range(5)] +
            ["param." + k for k, _ in head_keys(phi, num_classes) if trainable(k)])


def digest(arr):
    """shape (padded to four), float64 sum and abs-sum, strided float32 slice (the check_digest convention of tests/_util.py)."""
    a = np.ascontiguousarray(np.asarray(arr, dtype=np.float64)).reshape(-1)
    shape = list(np.shape(arr))
    return (np.asarray(shape + [0] * (4 - len(shape)), np.int64), np.array([a.sum(), np.abs(a).sum()], np.float64),
            a[::digest_stride(a.size)].astype(np.float32))


def pack_digests(tensors, names):
    """One golden case as four arrays: shapes [T, 4], sums [T, 2], the concatenated slices and their offsets [T + 1]."""
    d = [digest(tensors[n]) for n in names]
    off = np.cumsum([0] + [len(x[2]) for x in d]).astype(np.int64)
    return dict(shapes=np.stack([x[0] for x in d]), sums=np.stack([x[1] for x in d]), slices=np.concatenate([x[2] for x in d]), offsets=off)


def golden_entry(z, tag, names, name):
    """(shape list, (sum, abs-sum), slice) of one tensor of a case of the archive ``z``."""
    i = names.index(name)
    off = z[f"{tag}/offsets"]
    shape = [int(v) for v in z[f"{tag}/shapes"][i]]
    while len(shape) > 1 and shape[-1] == 0:
        shape.pop()
    return shape, z[f"{tag}/sums"][i], z[f"{tag}/slices"][off[i]:off[i + 1]]


def rel_err(got, ref):
    """max |got - ref| / max |ref| (float64)."""
    g = np.asarray(got, dtype=np.float64)
    r = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(r).max())
    return float(np.abs(g - r).max()) / scale if scale > 0 else float(np.abs(g).max())
