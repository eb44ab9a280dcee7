"""CPU side of the colour augmentation (hmd_ego_pose_amd.augment.draw_colour / colour_augment, hep_colour_augment_device): the numpy
oracle tests/_colour.py (the definition the kernels reproduce) held to PIL with zero differing bytes where the operation is PIL's, its
known answers where it is restated (Invert, Cutout, the noise, the Philox block: PARITY-UNPINNED), the draws of draw_colour, the host
checks of colour_augment and the error paths of the ABI, all of which return before any HIP call."""
import random

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi
from tests import _colour as C

INVALID, UNSUPPORTED = -1, -4
FACTORS = (0.1, 0.58, 0.97, 1.03, 1.42, 1.9)


def _images():
    for shape, seed in (((37, 50), 1), ((64, 64), 2)):
        img = C.random_frames(shape, seed)
        yield f"random {shape}", img
        yield f"lower range {shape}", (img // 2 + 30).astype(np.uint8)


def _same(pil_image, ours, what):
    bad = np.asarray(pil_image) != ours
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- the oracle against PIL ----
def test_oracle_equals_pil_histogram_and_point_operations():
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    for name, img in _images():
        p = Image.fromarray(img)
        _same(ImageOps.autocontrast(p, cutoff=0), C.autocontrast(img), (name, "autocontrast"))
        _same(ImageOps.equalize(p), C.equalize(img), (name, "equalize"))
        for bits in (2, 3, 6, 7, 8):
            _same(ImageOps.posterize(p, bits), C.posterize(img, bits), (name, "posterize", bits))
        for t in (0, 1, 137, 171, 214, 248, 255, 256):
            _same(ImageOps.solarize(p, t), C.solarize(img, t), (name, "solarize", t))
        _same(p.convert("L"), C.luma(img).astype(np.uint8), (name, "L"))
    low = (C.random_frames((64, 64), 2) // 2 + 30).astype(np.uint8)
    assert C.equalize(low).max() == 255                                    # the table reaches the 255 clip


def test_oracle_equals_pil_enhance():
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    for name, img in _images():
        p = Image.fromarray(img)
        for f in FACTORS:
            f32 = float(np.float32(f))                                     # the float32 that reaches the device
            _same(ImageEnhance.Color(p).enhance(f32), C.enhance_color(img, f), (name, "color", f))
            _same(ImageEnhance.Contrast(p).enhance(f32), C.enhance_contrast(img, f), (name, "contrast", f))
            _same(ImageEnhance.Brightness(p).enhance(f32), C.enhance_brightness(img, f), (name, "brightness", f))
            _same(ImageEnhance.Sharpness(p).enhance(f32), C.enhance_sharpness(img, f), (name, "sharpness", f))


def test_oracle_equals_pil_filters():
    Image = pytest.importorskip("PIL.Image")
    ImageFilter = pytest.importorskip("PIL.ImageFilter")
    for name, img in _images():
        p = Image.fromarray(img)
        _same(p.filter(ImageFilter.BLUR), C.blur(img), (name, "blur"))
        _same(p.filter(ImageFilter.SMOOTH), C.smooth(img), (name, "smooth"))


def test_degenerate_images():
    img = C.step0_image()
    a, e = C.autocontrast(img), C.equalize(img)
    assert np.array_equal(a[..., 1], img[..., 1]) and np.array_equal(e[..., 1], img[..., 1])
    assert not np.array_equal(a[..., 0], img[..., 0]) or img[..., 0].min() == 0 and img[..., 0].max() == 255
    # 16 x 16 = 256 pixels and the highest value occurs twice: step = (256 - 2) // 255 == 0, equalize changes nothing
    assert np.array_equal(e, img)
    one = C.step1_image()                                                   # the highest value once: step == 1, the table is the running count
    assert not np.array_equal(C.equalize(one)[..., 0], one[..., 0])
    try:
        from PIL import Image, ImageOps
    except ImportError:
        return
    _same(ImageOps.autocontrast(Image.fromarray(img)), a, "autocontrast, constant channel")
    _same(ImageOps.equalize(Image.fromarray(img)), e, "equalize, step 0")
    _same(ImageOps.equalize(Image.fromarray(one)), C.equalize(one), "equalize, step 1")


# ---- known answers of what is restated ----
def _four_by_four():
    return (np.arange(48, dtype=np.int32).reshape(4, 4, 3) * 5 + 3).astype(np.uint8)


def test_invert_and_cutout_by_hand():
    img = _four_by_four()
    inv = C.invert(img)
    assert inv[0, 0].tolist() == [252, 247, 242] and inv[3, 3].tolist() == [255 - 228, 255 - 233, 255 - 238]
    assert np.array_equal(C.invert(inv), img)
    cut = C.cutout(img, 1, 2, 3, 4)                                         # x1, y1, x2, y2: columns 1..2 of rows 2..3
    exp = img.copy()
    for y in (2, 3):
        for x in (1, 2):
            exp[y, x] = 128
    assert np.array_equal(cut, exp) and (cut != img).sum() == 12
    assert np.array_equal(C.cutout(img, 2, 2, 2, 4), img)                   # a side of 0


def test_philox_known_answers():
    # Random123's kat_vectors for philox4x32 with 10 rounds: counter and key all zero, all ones
    zero = C.philox4x32_10(np.zeros((1, 4), np.uint64), [0, 0])[0]
    assert [int(v) for v in zero] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = C.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint64), [0xFFFFFFFF, 0xFFFFFFFF])[0]
    assert [int(v) for v in ones] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # one round by hand: counter (1, 0, 0, 0), key (0, 0): M0 * 1 = 0xD2511F53 (high word 0), M1 * 0 = 0
    one = C.philox_round(np.array([[1, 0, 0, 0]], np.uint64), np.array([[0, 0]], np.uint64))[0]
    assert [int(v) for v in one] == [0, 0, 0, 0xD2511F53]


def test_noise_by_hand():
    img = _four_by_four()
    seed = 0x0123456789ABCDEF
    z = C.noise_normals(img.shape, 2, 1, seed)
    # element 5 = output 1 of the block with counter (1, 0, image 2, slot 1), key (low, high) of the seed
    x = C.philox4x32_10(np.array([[1, 0, 2, 1]], np.uint64), [seed & 0xFFFFFFFF, seed >> 32])[0]
    u0, u1 = ((int(x[0]) >> 8) + 0.5) / 2.0 ** 24, ((int(x[1]) >> 8) + 0.5) / 2.0 ** 24
    assert z.reshape(-1)[5] == np.sqrt(-2.0 * np.log(u0)) * np.sin(2.0 * np.pi * u1)
    assert z.reshape(-1)[4] == np.sqrt(-2.0 * np.log(u0)) * np.cos(2.0 * np.pi * u1)
    out = C.additive_gaussian_noise(img, 35.7, seed, 2, 1)
    exp = np.clip(img.astype(np.int64) + np.rint(float(np.float32(35.7)) * z).astype(np.int64), 0, 255)
    assert np.array_equal(out, exp) and not np.array_equal(out, img)
    assert np.array_equal(C.additive_gaussian_noise(img, 0.0, seed), img)
    assert np.rint(0.5) == 0 and np.rint(1.5) == 2 and np.rint(-0.5) == 0  # half to even
    # another image index, slot or seed is another stream
    assert not np.array_equal(z, C.noise_normals(img.shape, 3, 1, seed)) and not np.array_equal(z, C.noise_normals(img.shape, 2, 0, seed))
    big = C.noise_normals((64, 64, 3), 0, 0, 7)
    assert abs(big.mean()) < 0.03 and abs(big.std() - 1.0) < 0.03 and np.abs(big).max() < 6.0


@pytest.mark.parametrize("sigma", [2.55, 35.7])
def test_share_of_noise_elements_near_a_rounding_boundary(sigma):
    """What tests/test_gpu_colour.py's noise cases rely on: the 1 % cap of elements that may differ by one is far above the oracle's
    own share (a uniform fractional part gives 0.2 % for a band of 1e-3)."""
    for image, slot, seed in ((0, 0, 0x5EED0000 + int(sigma * 100)), (1, 1, 0xFEDCBA9876543210)):      # the two streams of the GPU test
        near = C.near_boundary((37, 50, 3), image, slot, seed, sigma)
        print(f"sigma {sigma} image {image}: {near.mean():.4%} of the elements lie within 1e-3 of a half-integer")
        assert near.mean() <= 0.01


# ---- draw_colour ----
def test_draw_colour_is_deterministic_and_well_formed():
    from hmd_ego_pose_amd.augment import COLOUR_OPS, check_colour_table, draw_colour
    import hmd_ego_pose_amd
    assert COLOUR_OPS == C.NAMES and len(COLOUR_OPS) == 14 and hmd_ego_pose_amd.draw_colour is draw_colour and hmd_ego_pose_amd.colour_augment
    apply = np.array([1, 0, 1, 1] * 64, np.int32)
    ops, args = draw_colour(random.Random(5), 256, apply=apply, height=48, width=64)
    ops2, args2 = draw_colour(random.Random(5), 256, apply=apply, height=48, width=64)
    assert ops.dtype == np.int32 and ops.shape == (256, 3, 8) and args.dtype == np.float32 and args.shape == (256, 3, 2)
    assert np.array_equal(ops, ops2) and np.array_equal(args, args2)
    assert not np.array_equal(ops, draw_colour(random.Random(6), 256, apply=apply, height=48, width=64)[0])
    counts, seen = set(), set()
    for b in range(256):
        ids = ops[b, :, 0].tolist()
        if apply[b] == 0:
            assert ids == [-1, -1, -1] and not ops[b, :, 1:].any() and not args[b].any()
            continue
        n = sum(i >= 0 for i in ids)
        assert 1 <= n <= 3 and all(i >= 0 for i in ids[:n]) and all(i == -1 for i in ids[n:])      # filled from the front
        assert len(set(ids[:n])) == n and all(0 <= i < 14 for i in ids[:n])                          # distinct
        counts.add(n); seen.update(ids[:n])
        for k in range(n):
            if ids[k] == 10:
                x1, y1, x2, y2 = ops[b, k, 1:5].tolist()
                assert 0 <= x1 <= x2 <= 64 and 0 <= y1 <= y2 <= 48
    assert counts == {1, 2, 3} and len(seen) == 14
    check_colour_table(ops, args, 256, 48, 64)                               # what it draws passes the host check
    assert (draw_colour(random.Random(1), 8, n=(0, 0), height=16, width=16)[0][:, :, 0] == -1).all()
    assert all((draw_colour(random.Random(s), 4, n=(2, 2), height=16, width=16)[0][:, :, 0] >= 0).sum() == 8 for s in range(4))
    for bad in (dict(n=(1, 4)), dict(n=(2, 1)), dict(m=(1, 31)), dict(height=8), dict(apply=[1, 1])):
        with pytest.raises(ValueError):
            draw_colour(random.Random(1), 4, **dict(dict(height=16, width=16), **bad))


def test_parameter_formulas():
    from hmd_ego_pose_amd.augment import colour_parameters
    ms = (1, 5, 10, 14)
    assert [colour_parameters(4, m, 64, 64)[0] for m in ms] == [8, 7, 6, 6]
    assert [colour_parameters(5, m, 64, 64)[0] for m in ms] == [248, 214, 171, 137]
    for op in (6, 7, 8, 9):
        assert np.allclose([colour_parameters(op, m, 64, 64, sign=1)[5] for m in ms], [1.03, 1.15, 1.3, 1.42], rtol=0, atol=1e-12)
        assert np.allclose([colour_parameters(op, m, 64, 64, sign=-1)[5] for m in ms], [0.97, 0.85, 0.7, 0.58], rtol=0, atol=1e-12)
    assert colour_parameters(6, 30, 64, 64, sign=1)[5] == 1.9 and colour_parameters(6, 30, 64, 64, sign=-1)[5] == 0.1
    assert np.allclose([colour_parameters(13, m, 64, 64)[5] for m in ms], [2.55, 12.75, 25.5, 35.7])
    assert colour_parameters(13, 3, 64, 64, seed=(7 << 32) | 9)[4] == (7 << 32) | 9
    # Cutout: side = m (20/32)/30 of the height; m = 12 on 96 rows of 128: a quarter of the height, 24 pixels
    assert 12 * ((20 / 32) / 30) * 96 == 24.0
    assert colour_parameters(10, 12, 96, 128, centre=(0.5, 0.5))[:4] == (52, 36, 76, 60)
    assert colour_parameters(10, 12, 96, 128, centre=(0.0, 0.0))[:4] == (0, 0, 12, 12)              # clipped at two borders
    assert colour_parameters(10, 12, 96, 128, centre=(0.96875, 0.96875))[:4] == (112, 81, 128, 96)   # 124 - 12 .. 136 -> 128; 93 - 12 .. 105 -> 96
    assert colour_parameters(10, 0, 96, 128, centre=(0.3, 0.3))[:4] == (38, 28, 38, 28)             # side 0
    assert colour_parameters(10, 30, 96, 128, centre=(0.5, 0.5))[:4] == (34, 18, 94, 78)            # the largest side: 0.625 of the height, 60 pixels
    for m in range(0, 31):
        for centre in ((0.0, 0.0), (0.999999, 0.999999), (0.5, 0.0)):
            x1, y1, x2, y2 = colour_parameters(10, m, 17, 4096, centre=centre)[:4]
            assert 0 <= x1 <= x2 <= 4096 and 0 <= y1 <= y2 <= 17


def test_host_check_refuses_a_bad_table():
    from hmd_ego_pose_amd.augment import check_colour_table, colour_augment
    good = C.table([[(4, dict(i=(8, 0, 0, 0))), (6, dict(f=1.9))], [], [(10, dict(i=(0, 0, 16, 16))), (13, dict(f=255.0, seed=1)), (5, dict(i=(256, 0, 0, 0)))]])
    check_colour_table(*good, 3, 16, 16)
    bad_rows = ([[(14, {})]], [[(-2, {})]], [[(4, dict(i=(1, 0, 0, 0)))]], [[(4, dict(i=(9, 0, 0, 0)))]], [[(5, dict(i=(257, 0, 0, 0)))]], [[(5, dict(i=(-1, 0, 0, 0)))]],
                [[(6, dict(f=2.0))]], [[(9, dict(f=0.05))]], [[(7, dict(f=float("nan")))]], [[(13, dict(f=256.0))]], [[(13, dict(f=-1.0))]],
                [[(10, dict(i=(0, 0, 17, 16)))]], [[(10, dict(i=(5, 0, 4, 16)))]], [[(10, dict(i=(0, -1, 4, 16)))]])
    for rows in bad_rows:
        with pytest.raises(ValueError):
            check_colour_table(*C.table(rows), 1, 16, 16)
        assert not C.slot_valid(rows[0][0][0], list(rows[0][0][1].get("i", (0, 0, 0, 0))), rows[0][0][1].get("f", 0.0), 16, 16)      # the device's rule is the same
    ops, args = C.table([[(3, {})]])
    ops[0, 0, 0], ops[0, 1, 0] = -1, 3                                      # a gap before a filled slot
    with pytest.raises(ValueError, match="empty slot"):
        check_colour_table(ops, args, 1, 16, 16)
    with pytest.raises(ValueError):
        check_colour_table(ops[:, :2], args, 1, 16, 16)
    with pytest.raises(ValueError, match="ROCm"):                          # a CPU tensor never reaches the ABI
        colour_augment(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), *C.table([[]]))


def test_oracle_treats_a_bad_slot_as_identity_and_stops_at_an_empty_one():
    frames = C.random_frames((2, 16, 16), 4)
    ops, args = C.table([[(3, {}), (6, dict(f=2.5)), (3, {})], [(3, {})]])
    ops[1, 2, 0] = 3                                                        # behind an empty slot: not applied
    out = C.colour_augment(frames, ops, args)
    assert np.array_equal(out[0], frames[0]) and np.array_equal(out[1], C.invert(frames[1]))


# ---- the C ABI: every error below returns before a HIP call ----
def _call(l, batch=2, height=64, width=64, nbytes=None, null=None, same=False, ws=0x100000):
    p = dict(rgb=0x10000, ops=0x20000, args=0x30000, out=0x40000)
    if null:
        p[null] = None
    if same:
        p["out"] = p["rgb"]
    if nbytes is None:
        nbytes = max(0, l.hep_colour_workspace_bytes(batch, height, width))
    return l.hep_colour_augment_device(p["rgb"], p["ops"], p["args"], batch, height, width, p["out"], ws, nbytes, None)


def test_abi_error_codes_and_reasons():
    l = _capi.lib()
    assert "hep_colour_augment_device" in _capi.SYMBOLS and "hep_colour_workspace_bytes" in _capi.SYMBOLS
    for name in ("rgb", "ops", "args"):
        assert _call(l, null=name) == INVALID and b"input pointer" in l.hep_last_error(), name
    assert _call(l, null="out") == INVALID and b"output pointer" in l.hep_last_error()
    assert _call(l, ws=None) == INVALID and b"workspace is NULL" in l.hep_last_error()
    assert _call(l, same=True) == INVALID and b"must not be rgb_hwc" in l.hep_last_error()
    need = l.hep_colour_workspace_bytes(2, 64, 64)
    assert need > 0
    assert _call(l, nbytes=need - 1) == INVALID and b"workspace too small" in l.hep_last_error()
    assert _call(l, nbytes=0) == INVALID
    assert _call(l, ws=0x100004) == INVALID and b"aligned" in l.hep_last_error()
    for batch in (0, -3):
        assert _call(l, batch=batch) == INVALID and b"batch" in l.hep_last_error()
        assert l.hep_colour_workspace_bytes(batch, 64, 64) == INVALID
    for kw in (dict(height=15), dict(height=4097), dict(width=8), dict(width=5000)):
        assert _call(l, **kw) == UNSUPPORTED and b"[16, 4096]" in l.hep_last_error(), kw
        assert l.hep_colour_workspace_bytes(2, kw.get("height", 64), kw.get("width", 64)) == UNSUPPORTED
    assert _call(l, batch=65536) == UNSUPPORTED and b"65535" in l.hep_last_error()
    assert l.hep_abi_version() == 1


def test_workspace_is_monotone_and_holds_two_frames():
    l = _capi.lib()
    base = dict(batch=2, height=64, width=96)
    steps = dict(batch=(1, 2, 3, 16, 64), height=(16, 63, 64, 65, 128, 1000, 4096), width=(16, 95, 96, 128, 129, 4096))
    for key, values in steps.items():
        got = [l.hep_colour_workspace_bytes(*[dict(base, **{key: v})[k] for k in ("batch", "height", "width")]) for v in values]
        assert all(g > 0 for g in got) and got == sorted(got) and len(set(got)) == len(got), (key, got)
    for B, H, W in ((1, 16, 16), (2, 37, 50), (16, 512, 512), (4, 4096, 4096)):
        assert l.hep_colour_workspace_bytes(B, H, W) >= 2 * B * H * W * 3 + B * 3 * 769 * 4
