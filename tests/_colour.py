"""numpy oracle of the colour augmentation (hmd_ego_pose_amd/augment.py colour_augment, csrc/k_colour.hip, hep_colour_augment_device):
the 14 operations of the reference's RandAugment (pytorch-sandbox/generators/randaug.py:244-279, applied in generators/common.py:334-341
before the 6DoF warp), one function per operation on a uint8 [H, W, 3] RGB image, ids in the reference's order.

This file is the DEFINITION the kernels reproduce bit for bit (id 13, the noise, within the band tests/test_gpu_colour.py states).
tests/test_colour_cpu.py pins ids 1, 2, 4, 5, 6, 7, 8, 9, 11 and 12 against PIL (imgaug's pillike augmenters call PIL) with zero differing
bytes.  PARITY-UNPINNED: imgaug is not installed where this project is built, so Cutout's rectangle convention, Invert and the rounding
of the additive noise are restated, not compared; imgaug's random stream is not reproduced (hmd_ego_pose_amd.augment.draw_colour defines
the project's, and the noise comes from the counter-based generator below)."""
import math

import numpy as np

NAMES = ("Identity", "Autocontrast", "Equalize", "Invert", "Posterize", "Solarize", "EnhanceColor", "EnhanceContrast", "EnhanceBrightness",
         "EnhanceSharpness", "Cutout", "FilterBlur", "FilterSmooth", "AdditiveGaussianNoise")
NEEDS_STATS = (1, 2, 7)


def _histogram(channel):
    return np.bincount(channel.ravel(), minlength=256).astype(np.int64)


def identity(img):
    return img.copy()


def autocontrast(img):
    """ImageOps.autocontrast(cutoff=0): per channel, the first and last non-empty bins are stretched to 0 and 255."""
    out = img.copy()
    for c in range(3):
        nz = np.nonzero(_histogram(img[..., c]))[0]
        lo, hi = int(nz[0]), int(nz[-1])
        if hi <= lo:
            continue
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        lut = np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)], np.uint8)      # two roundings, no fma
        out[..., c] = lut[img[..., c]]
    return out


def equalize(img):
    """ImageOps.equalize."""
    out = img.copy()
    for c in range(3):
        h = _histogram(img[..., c])
        nz = h[h != 0]
        if len(nz) <= 1:
            continue
        step = int(nz.sum() - nz[-1]) // 255
        if step == 0:
            continue
        before = np.concatenate(([0], np.cumsum(h)[:-1]))
        lut = np.minimum((step // 2 + before) // step, 255).astype(np.uint8)
        out[..., c] = lut[img[..., c]]
    return out


def invert(img):
    return (255 - img.astype(np.int32)).astype(np.uint8)


def posterize(img, bits):
    return (img & np.uint8(~((1 << (8 - int(bits))) - 1) & 0xFF)).astype(np.uint8)


def solarize(img, threshold):
    v = img.astype(np.int32)
    return np.where(v < int(threshold), v, 255 - v).astype(np.uint8)


def luma(img):
    """PIL's RGB -> L: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    v = img.astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.int32)


def blend(d, x, f):
    """Image.blend(d, x, f) on integer arrays: t = float32(d + float32(f * float32(x - d))); inside 0 <= f <= 1 truncated, else clipped."""
    f = np.float32(f)
    d = np.asarray(d, np.int32)
    x = np.asarray(x, np.int32)
    t = (d.astype(np.float32) + (f * (x - d).astype(np.float32)).astype(np.float32)).astype(np.float32)
    if np.float32(0) <= f <= np.float32(1):
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def _filter(img, weights, scale):
    k = np.asarray(weights, np.int64)
    r = k.shape[0] // 2
    H, W = img.shape[:2]
    out = img.copy()
    if H <= 2 * r or W <= 2 * r:
        return out
    v = img.astype(np.int64)
    acc = np.zeros((H - 2 * r, W - 2 * r, 3), np.int64)
    for dy in range(k.shape[0]):
        for dx in range(k.shape[1]):
            if k[dy, dx]:
                acc += k[dy, dx] * v[dy:dy + H - 2 * r, dx:dx + W - 2 * r]
    out[r:H - r, r:W - r] = np.clip((2 * acc + scale) // (2 * scale), 0, 255).astype(np.uint8)
    return out


def smooth(img):
    """ImageFilter.SMOOTH: 3 x 3, scale 13; the 1-pixel border is copied."""
    return _filter(img, [[1, 1, 1], [1, 5, 1], [1, 1, 1]], 13)


def blur(img):
    """ImageFilter.BLUR: 5 x 5, the outer ring, scale 16; the 2-pixel border is copied."""
    k = np.ones((5, 5), np.int64)
    k[1:4, 1:4] = 0
    return _filter(img, k, 16)


def enhance_color(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, axis=2), img, f)


def contrast_grey(img):
    return int(int(luma(img).astype(np.int64).sum()) / (img.shape[0] * img.shape[1]) + 0.5)


def enhance_contrast(img, f):
    return blend(np.full(img.shape, contrast_grey(img), np.int32), img, f)


def enhance_brightness(img, f):
    return blend(np.zeros(img.shape, np.int32), img, f)


def enhance_sharpness(img, f):
    return blend(smooth(img), img, f)


def cutout(img, x1, y1, x2, y2):
    out = img.copy()
    out[int(y1):int(y2), int(x1):int(x2)] = 128
    return out


# ---- the noise: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11), Box-Muller in float64 ----
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox_round(ctr, key):
    """One round on uint64 arrays holding 32-bit words: ctr [..., 4], key [..., 2]."""
    p0 = PHILOX_M0 * ctr[..., 0]
    p1 = PHILOX_M1 * ctr[..., 2]
    mask = np.uint64(0xFFFFFFFF)
    return np.stack(((p1 >> np.uint64(32)) ^ ctr[..., 1] ^ key[..., 0], p1 & mask, (p0 >> np.uint64(32)) ^ ctr[..., 3] ^ key[..., 1], p0 & mask), axis=-1)


def philox4x32_10(ctr, key):
    ctr = np.asarray(ctr, np.uint64)
    key = np.broadcast_to(np.asarray(key, np.uint64), ctr.shape[:-1] + (2,)).copy()
    mask = np.uint64(0xFFFFFFFF)
    for r in range(10):
        ctr = philox_round(ctr, key)
        key = (key + np.array([PHILOX_W0, PHILOX_W1], np.uint64)) & mask
    return ctr


def noise_normals(shape, image_index, slot, seed):
    """float64 [H, W, 3]: element e (in [H][W][3] order) is output e % 4 of the block with counter (e // 4, 0, image_index, slot)."""
    n = int(np.prod(shape))
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack((q, np.zeros_like(q), np.full_like(q, image_index), np.full_like(q, slot)), axis=-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10(ctr, [seed & 0xFFFFFFFF, seed >> 32])
    u = ((x >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    z = np.empty(u.shape, np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[:, a]))
        z[:, a] = r * np.cos(2.0 * math.pi * u[:, a + 1])
        z[:, a + 1] = r * np.sin(2.0 * math.pi * u[:, a + 1])
    return z.reshape(-1)[:n].reshape(shape)


def noise_scaled(shape, image_index, slot, seed, sigma):
    """sigma * z in float64 (sigma is the float32 the device gets)."""
    return float(np.float32(sigma)) * noise_normals(shape, image_index, slot, seed)


def additive_gaussian_noise(img, sigma, seed, image_index=0, slot=0):
    d = np.rint(noise_scaled(img.shape, image_index, slot, seed, sigma)).astype(np.int64)
    return np.clip(img.astype(np.int64) + d, 0, 255).astype(np.uint8)


def near_boundary(shape, image_index, slot, seed, sigma, band=1e-3):
    """Elements whose sigma * z lies within ``band`` of a half-integer: a float32 evaluation may round them the other way."""
    s = noise_scaled(shape, image_index, slot, seed, sigma)
    return np.abs((s - 0.5) - np.rint(s - 0.5)) <= band


# ---- the table rows (include/hep.h): ops [B][3][8] = (id or -1, i0, i1, i2, i3, seed_lo, seed_hi, 0), args [B][3][2] = (f or sigma, 0) ----
def slot_valid(op, i, f, H, W):
    """What the device accepts; anything else runs as Identity (hmd_ego_pose_amd.augment.colour_augment refuses it on the host)."""
    f = np.float32(f)
    if op in (0, 1, 2, 3, 11, 12):
        return True
    if op == 4:
        return 2 <= i[0] <= 8
    if op == 5:
        return 0 <= i[0] <= 256
    if op in (6, 7, 8, 9):
        return bool(np.float32(0.1) <= f <= np.float32(1.9))
    if op == 10:
        return 0 <= i[0] <= i[2] <= W and 0 <= i[1] <= i[3] <= H
    if op == 13:
        return bool(np.float32(0) <= f <= np.float32(255))
    return False


def apply_slot(img, row, arg, image_index, slot):
    op, i, f = int(row[0]), [int(v) for v in row[1:5]], np.float32(arg[0])
    if not slot_valid(op, i, f, img.shape[0], img.shape[1]):
        return img.copy()
    if op == 13:
        seed = (int(row[5]) & 0xFFFFFFFF) | ((int(row[6]) & 0xFFFFFFFF) << 32)
        return additive_gaussian_noise(img, f, seed, image_index, slot)
    return {0: identity, 1: autocontrast, 2: equalize, 3: invert, 4: lambda m: posterize(m, i[0]), 5: lambda m: solarize(m, i[0]),
            6: lambda m: enhance_color(m, f), 7: lambda m: enhance_contrast(m, f), 8: lambda m: enhance_brightness(m, f),
            9: lambda m: enhance_sharpness(m, f), 10: lambda m: cutout(m, *i), 11: blur, 12: smooth}[op](img)


def colour_augment(frames, ops, args):
    """frames uint8 [B, H, W, 3]; each image's operations are its leading slots up to the first id of -1."""
    frames = np.asarray(frames)
    out = frames.copy()
    for b in range(frames.shape[0]):
        img = frames[b]
        for k in range(3):
            if int(ops[b, k, 0]) == -1:
                break
            img = apply_slot(img, ops[b, k], args[b, k], b, k)
        out[b] = img
    return out


def table(rows, batch=None):
    """rows: per image a list of up to three (id, {i0.., seed, f}) tuples -> (ops int32 [B,3,8], args float32 [B,3,2])."""
    B = len(rows) if batch is None else batch
    ops = np.zeros((B, 3, 8), np.int32)
    ops[:, :, 0] = -1
    args = np.zeros((B, 3, 2), np.float32)
    for b, row in enumerate(rows):
        for k, (op, kw) in enumerate(row):
            ops[b, k, 0] = op
            ops[b, k, 1:5] = kw.get("i", (0, 0, 0, 0))
            seed = int(kw.get("seed", 0))
            ops[b, k, 5:7] = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32).view(np.int32)
            args[b, k, 0] = kw.get("f", 0.0)
    return ops, args


def random_frames(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)


def step0_image():
    """16 x 16, random, the highest value twice in every channel (equalize's step is (256 - 2) // 255 == 0) and a constant green channel."""
    img = random_frames((16, 16), 3)
    img[0, 0] = img[0, 1] = 255
    img[..., 1] = 77
    return img


def step1_image():
    """step0_image with the highest value once in the red and blue channels: step == (256 - 1) // 255 == 1."""
    img = np.minimum(step0_image(), 254)
    img[0, 0] = (255, 77, 255)
    return img
