"""The oracle of hep_optim_*_device and hep_transformation_*_device (csrc/k_train.hip) in numpy, in the dtype it is given.

float64 is the definition (pinned to ``torch.optim.Adam``, ``torch.optim.SGD(momentum=0.9, nesterov=True)``,
``torch.nn.utils.clip_grad_norm_`` and ``training.format_translation`` by tests/test_trainer_cpu.py); the same functions in float32
give ``e32``, the error that arithmetic of the device's width makes on the same step, and the device may reach 4 x e32 with a floor
of one float32 ulp of the array's largest magnitude (tests/test_gpu_trainer.py; the rule of tests/test_gpu_head_grads.py).  The
operations are written in the order the kernels use, one rounding per operation (k_train.hip compiles with contraction off); SGD's
two multiply-adds are fused, as the kernel writes them (fmaf).  ``unpack_grad`` sums the three uses of tz in autograd's order."""
import numpy as np

PK_TRAIN, PK_STAT, PK_FROZEN = 0, 1, 2
ADAM, SGD_NESTEROV = 0, 1
ULP32 = 1.2e-7                      # one float32 ulp, relative
BOUND_FACTOR = 4.0


class State:
    """The state block: norm, clip_coef, bias1, bias2_sqrt, step, skipped."""

    def __init__(self):
        self.norm = self.clip_coef = self.bias1 = self.bias2_sqrt = 0.0
        self.step = self.skipped = 0


def grad_norm(grad, kind, state, beta1, beta2, max_norm, dtype=np.float64):
    """Pass 1 + 2: the norm of the kind-0 gradients (always summed in float64, as the device does) and the state update; the
    coefficients are rounded to ``dtype`` as the state block stores them."""
    g = np.asarray(grad)[np.asarray(kind) == PK_TRAIN].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        norm = float(np.sqrt(np.sum(g * g)))
    state.norm = norm
    if np.isfinite(norm) and np.isfinite(np.float32(norm)):
        state.step += 1
        state.clip_coef = float(dtype(min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0))
        state.bias1 = float(dtype(1.0 - beta1 ** state.step))
        state.bias2_sqrt = float(dtype(np.sqrt(1.0 - beta2 ** state.step)))
        return True
    state.skipped += 1
    state.clip_coef = 0.0
    return False


def update(p, g, m, v, stats, kind, optimizer, lr, beta1, beta2, eps, state, dtype=np.float64):
    """hep_optim_update_device after ``grad_norm`` of the same gradient: returns new (p, m, v) in ``dtype`` (v None under SGD
    stays None).  A skipped step (norm not finite) returns the inputs unchanged."""
    T = dtype
    p, m = np.array(p, dtype=T), np.array(m, dtype=T)
    v = None if v is None else np.array(v, dtype=T)
    if not (np.isfinite(state.norm) and np.isfinite(np.float32(state.norm))):
        return p, m, v
    kind = np.asarray(kind)
    tr = kind == PK_TRAIN
    lr, b1, b2, eps, clip = T(lr), T(beta1), T(beta2), T(eps), T(state.clip_coef)
    with np.errstate(all="ignore"):
        gc = clip * np.asarray(g, dtype=T)[tr]
        if optimizer == ADAM:
            mt = m[tr] + (T(1) - b1) * (gc - m[tr])
            vt = b2 * v[tr] + (T(1) - b2) * (gc * gc)
            step_size = lr / T(state.bias1)
            p[tr] = p[tr] - step_size * (mt / (np.sqrt(vt) / T(state.bias2_sqrt) + eps))
            m[tr], v[tr] = mt, vt
        else:
            mt = b1 * m[tr] + gc
            p[tr] = _fma(-lr, _fma(b1, mt, gc, T), p[tr], T)
            m[tr] = mt
    if stats is not None:
        st = kind == PK_STAT
        p[st] = np.asarray(stats, dtype=T)[st]
    return p, m, v


def _fma(a, b, c, T):
    """a * b + c with one rounding: a float32 product is exact in float64."""
    return a * b + c if T is np.float64 else (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(T)


def pack(rotation, raw, camera, anchors, dtype=np.float64):
    """cat(rotation, format_translation(raw)): [B,N,R], [B,N,3], [B,6], [N,3] -> [B,N,R+3]."""
    T = dtype
    rot, raw, cam, ta = (np.asarray(a, dtype=T) for a in (rotation, raw, camera, anchors))
    fx, fy, px, py, tzs, isc = (cam[:, i:i + 1] for i in range(6))
    x = (ta[None, :, 0] + raw[..., 0] * ta[None, :, 2]) / isc - px
    y = (ta[None, :, 1] + raw[..., 1] * ta[None, :, 2]) / isc - py
    tz = raw[..., 2] * tzs
    return np.concatenate([rot, np.stack([x * tz / fx, y * tz / fy, tz], axis=-1)], axis=2).astype(T)


def unpack_grad(grad, raw, camera, anchors, num_rotation=3, dtype=np.float64):
    """The backward of ``pack``: the gradient [B,N,R+3] -> (grad_rotation [B,N,R], grad_raw [B,N,3])."""
    T, R = dtype, num_rotation
    g, raw, cam, ta = (np.asarray(a, dtype=T) for a in (grad, raw, camera, anchors))
    fx, fy, px, py, tzs, isc = (cam[:, i:i + 1] for i in range(6))
    stride = ta[None, :, 2]
    x = (ta[None, :, 0] + raw[..., 0] * stride) / isc - px
    y = (ta[None, :, 1] + raw[..., 1] * stride) / isc - py
    tz = raw[..., 2] * tzs
    gx, gy = g[..., R] / fx, g[..., R + 1] / fy
    g_raw = np.stack([gx * tz / isc * stride, gy * tz / isc * stride, ((g[..., R + 2] + gy * y) + gx * x) * tzs], axis=-1)
    return g[..., :R].astype(T), g_raw.astype(T)


def rel_err(a, ref):
    """max |a - ref| / max |ref| (0 / 0 = 0)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top = float(np.abs(ref).max()) if ref.size else 0.0
    d = float(np.abs(a - ref).max()) if ref.size else 0.0
    return d / top if top > 0 else d


def bound(e32):
    return max(BOUND_FACTOR * e32, ULP32)


def mixed_kinds(n, seed):
    """Kinds for ``n`` elements: mostly trainable, with runs of kind 1 and kind 2 that start and end INSIDE a float4 (at 4 k + 1 ..
    4 k + 6 style offsets) wherever n leaves room, and whole float4s of each kind."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x0971]))
    kind = np.zeros((n,), np.uint8)
    pos = 1
    while pos + 3 <= n:
        length = int(rng.integers(2, 12))
        k = PK_STAT if (pos // 7) % 2 == 0 else PK_FROZEN
        kind[pos:min(n, pos + length)] = k
        pos += length + int(rng.integers(3, 40)) | 1          # odd gaps: runs begin at every residue mod 4
    if n <= 5 and n >= 3:
        kind[1] = PK_STAT
        kind[n - 1] = PK_FROZEN if n > 3 else kind[n - 1]
    return kind


def case_arrays(n, seed):
    """Seeded float32 arrays of one update case: p, m0 (zeros), three gradients, stats; a few exact-zero gradients."""
    rng = np.random.Generator(np.random.PCG64([seed, n & 0xffff, 0x0972]))
    p = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32) for _ in range(3)]
    zero = rng.random(n) < 0.05
    for g in grads:
        g[zero] = 0.0
    stats = rng.standard_normal(n).astype(np.float32)
    return p, grads, stats, zero
