"""CPU side of the training input path (hmd_ego_pose_amd/augment.py, hep_augment_6dof_device): the known answers of the numpy
oracle tests/_augment.py (the definition the kernels reproduce; OpenCV's conventions restated, PARITY-UNPINNED), the host
functions of the module, the error paths of the ABI (all of which return before any HIP call) and what the fixed cases of
tests/test_gpu_augment.py contain, so that the GPU test exercises what it says it does."""
import math
import random

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi
from hmd_ego_pose_amd.evaluate import axis_angle_to_matrix
from tests import _augment as A

INVALID, UNSUPPORTED = -1, -4


def _image(h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(1, 256, (h, w), dtype=np.uint8)


def test_identity_returns_image_and_mask_unchanged():
    img, mask = _image(19, 23, 1)
    for M in (np.array([1.0, 0, 0, 0, 1.0, 0]), A.forward_matrix(0.0, 1.0, 11.0, 9.0)):
        assert np.array_equal(A.warp_bilinear(img, M), img)
        assert np.array_equal(A.warp_nearest(mask, M), mask)


@pytest.mark.parametrize("angle", [90, 180, 270])
def test_right_angles_are_exact_permutations(angle):
    # a 6 x 10 frame about (4.5, 2.5): cx - cy and cx + cy are integers, so every output pixel maps onto a pixel centre
    h, w, cx, cy = 6, 10, 4.5, 2.5
    img, mask = _image(h, w, 2)
    M = A.forward_matrix(angle, 1.0, cx, cy)
    a, b = {90: (0, -1), 180: (-1, 0), 270: (0, 1)}[angle]          # cos, sin of -angle
    exp_img, exp_mask = np.zeros_like(img), np.zeros_like(mask)
    outside = 0
    for y in range(h):
        for x in range(w):
            # forward: d = [[a, b], [-b, a]] (s - c) + c, so s = [[a, -b], [b, a]] (d - c) + c
            sx, sy = a * (x - cx) - b * (y - cy) + cx, b * (x - cx) + a * (y - cy) + cy
            assert sx == int(sx) and sy == int(sy)
            if 0 <= sx < w and 0 <= sy < h:
                exp_img[y, x], exp_mask[y, x] = img[int(sy), int(sx)], mask[int(sy), int(sx)]
            else:
                outside += 1
    assert (outside > 0) == (angle != 180)
    assert np.array_equal(A.warp_bilinear(img, M), exp_img)
    assert np.array_equal(A.warp_nearest(mask, M), exp_mask)


def test_square_quarter_turn_is_rot90():
    img, mask = _image(8, 8, 3)
    M = A.forward_matrix(90, 1.0, 3.5, 3.5)
    out = A.warp_nearest(mask, M)
    assert np.array_equal(out, np.rot90(mask, 1)) or np.array_equal(out, np.rot90(mask, -1))
    assert sorted(out.reshape(-1).tolist()) == sorted(mask.reshape(-1).tolist())


def test_hand_computed_bilinear_case():
    # source = output + (0.25, 0.75): fractions 8/32 and 24/32; weights 6144, 2048, 18432, 6144
    p = np.array([[10, 50], [200, 90]], np.uint8)
    img = np.repeat(p[:, :, None], 3, axis=2)
    out = A.warp_bilinear(img, np.array([1.0, 0.0, -0.25, 0.0, 1.0, -0.75]))
    assert A.bilinear_weights(8, 24) == (6144, 2048, 18432, 6144)
    # (6144*10 + 2048*50 + 18432*200 + 6144*90 + 16384) >> 15 = 4419584 >> 15 = 134; taps outside the source count 0:
    # (6144*50 + 18432*90 + 16384) >> 15 = 60 ; (6144*200 + 2048*90 + 16384) >> 15 = 43 ; (6144*90 + 16384) >> 15 = 17
    assert out[:, :, 0].tolist() == [[134, 60], [43, 17]]
    assert np.array_equal(out[:, :, 1], out[:, :, 0]) and np.array_equal(out[:, :, 2], out[:, :, 0])


def test_weights_sum_to_32768():
    for fy in range(32):
        for fx in range(32):
            w = A.bilinear_weights(fx, fy)
            assert sum(w) == 32768 and min(w) >= 0
    assert A.bilinear_weights(0, 0) == (32768, 0, 0, 0)      # zero fractions: exactly the source pixel


def test_lrint_is_half_even_and_saturates():
    assert A._lrint_sat(np.array([0.5, 1.5, 2.5, -0.5, -1.5])).tolist() == [0, 2, 2, 0, -2]
    assert A._lrint_sat(np.array([1e300, -1e300, float("nan")])).tolist() == [A.INT32_MAX, A.INT32_MIN, A.INT32_MIN]


def test_inverse_is_warpaffines():
    M = A.forward_matrix(37.3, 0.7, 64.0, 61.5)
    a00, a01, a02, a10, a11, a12 = A.invert_affine(M)
    F = np.array([[M[0], M[1], M[2]], [M[3], M[4], M[5]], [0, 0, 1]])
    assert np.allclose(np.array([[a00, a01, a02], [a10, a11, a12], [0, 0, 1]]) @ F, np.eye(3), atol=1e-12)
    assert A.invert_affine(np.zeros(6)) == (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)      # D = 0 -> 0


@pytest.mark.parametrize("seed", [0, 7, 12345])
def test_draw_6dof_follows_the_reference_sequence(seed):
    from hmd_ego_pose_amd.augment import draw_6dof
    for chance in (0.02, 0.5):
        got = draw_6dof(random.Random(seed), 64, (0.7, 1.3), chance)
        exp = A.reference_draws(random.Random(seed), 64, (0.7, 1.3), chance)
        for g, e in zip(got, exp):
            assert g.dtype == e.dtype and np.array_equal(g, e)
    a, s, ap = draw_6dof(random.Random(seed), 256, (0.7, 1.3), 0.5)
    assert 0 < ap.sum() < 256 and ((s >= 0.7) & (s <= 1.3)).all() and ((a >= 0) & (a < 360)).all()
    assert (a[ap == 0] == 0).all() and (s[ap == 0] == 1).all()


def test_rotation_matrices_match_the_oracle_and_refuse_a_bad_scale():
    from hmd_ego_pose_amd.augment import rotation_matrices
    import hmd_ego_pose_amd
    assert hmd_ego_pose_amd.rotation_matrices is rotation_matrices and hmd_ego_pose_amd.draw_6dof and hmd_ego_pose_amd.augment_6dof
    ang, sc, c = [0.0, 37.3, 211.7], [1.0, 0.7, 1.3], [[64.0, 64.0], [63.5, 60.25], [100.0, 3.0]]
    M = rotation_matrices(ang, sc, c)
    assert M.dtype == np.float64 and M.shape == (3, 6)
    for i in range(3):
        assert np.array_equal(M[i], A.forward_matrix(ang[i], sc[i], *c[i]))
    assert np.array_equal(M[0], [1, 0, 0, 0, 1, 0])
    for bad in (0.2, 4.5, float("nan"), -1.0):
        with pytest.raises(ValueError, match="scale"):
            rotation_matrices([10.0], [bad], [[8.0, 8.0]])
    with pytest.raises(ValueError):
        rotation_matrices([float("inf")], [1.0], [[8.0, 8.0]])


def test_python_api_validates_before_the_abi():
    from hmd_ego_pose_amd.augment import augment_6dof
    with pytest.raises(ValueError, match="ROCm"):      # host tensors never reach a pointer
        augment_6dof(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), torch.zeros((1, 16, 16), dtype=torch.uint8), [], np.zeros((1, 4)), [0.0], [1.0], [0], 16)
    from hmd_ego_pose_amd.training import anchor_targets_device
    with pytest.raises(ValueError, match="anchors"):
        anchor_targets_device(torch.zeros((4, 4)), None, None, None, None, None, (16, 16))


@pytest.mark.parametrize("seed", range(4))
def test_pose_update_composes_rotations(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    for _ in range(16):
        axis = rng.standard_normal(3); axis /= np.linalg.norm(axis)
        rvec = (axis * rng.uniform(0.05, 3.0)).astype(np.float32)
        tvec = rng.uniform(-500, 500, 3).astype(np.float32)
        angle, scale = rng.uniform(0, 2 * math.pi), rng.uniform(0.7, 1.3)
        r2, t2 = A.pose_update(rvec, tvec, angle, scale)
        assert r2.dtype == np.float32 and t2.dtype == np.float32
        Rz = axis_angle_to_matrix([0.0, 0.0, angle])
        # float32 storage of the result: 2^-24 relative on a vector of norm <= pi -> 4e-7 on the matrix; 1e-6 with margin
        assert np.abs(axis_angle_to_matrix(r2) - Rz @ axis_angle_to_matrix(rvec)).max() < 1e-6
        exp_t = Rz @ tvec.astype(np.float64); exp_t[2] /= scale
        assert np.abs(t2 - exp_t).max() <= 2 ** -24 * np.abs(exp_t).max() * 1.01
        r32, t32 = A.pose_update(rvec, tvec, angle, scale, np.float32)
        assert np.abs(axis_angle_to_matrix(r32) - axis_angle_to_matrix(r2)).max() < 2e-5


def test_out_of_range_scale_is_not_applied_by_the_oracle():
    c = A.make_case("D")
    size = c.pop("size"); c.pop("angles_deg")
    base = A.augment_6dof(size=size, **c)
    assert base["applied"].tolist() == [1]
    c["xform"] = c["xform"].copy(); c["xform"][0, 7] = 5.0
    o = A.augment_6dof(size=size, **c)
    assert o["applied"].tolist() == [0] and np.array_equal(o["mask"], c["masks"]) and np.array_equal(o["gt_boxes"][0, 0], c["boxes"][0, 0])


# ---- the C ABI: every error below returns before a HIP call ----
def _call(l, null=None, **kw):
    p = dict(batch=2, height=64, width=64, size=128, kmax=3, nbytes=None)
    p.update(kw)
    ptrs = [0x10000 + 0x1000 * i for i in range(19)]      # never dereferenced on these paths
    names = ["rgb", "mask", "xform", "camera_k", "boxes", "labels", "mask_values", "rvec", "tvec", "extra", "num_gt",
             "image", "mask_out", "camera", "gt_boxes", "gt_labels", "gt_transform", "gt_num", "applied"]
    v = dict(zip(names, ptrs))
    ws = 0x100000
    if null == "workspace":
        ws = None
    elif null is not None:
        v[null] = None
    if p["nbytes"] is None:
        p["nbytes"] = max(0, l.hep_augment_workspace_bytes(p["batch"], p["height"], p["width"], p["size"], p["kmax"]))
    return l.hep_augment_6dof_device(*[v[n] for n in names[:11]], p["batch"], p["height"], p["width"], p["size"], p["kmax"], 1000.0,
                                     *[v[n] for n in names[11:]], ws, p["nbytes"], None)


def test_abi_error_codes_and_reasons():
    l = _capi.lib()
    assert "hep_augment_6dof_device" in _capi.SYMBOLS and "hep_augment_workspace_bytes" in _capi.SYMBOLS
    for name in ("rgb", "mask", "xform", "camera_k", "boxes", "labels", "mask_values", "rvec", "tvec", "extra", "num_gt"):
        assert _call(l, null=name) == INVALID and b"input pointer" in l.hep_last_error(), name
    for name in ("image", "camera", "gt_boxes", "gt_labels", "gt_transform", "gt_num", "applied"):
        assert _call(l, null=name) == INVALID and b"output pointer" in l.hep_last_error(), name
    assert _call(l, null="workspace") == INVALID and b"workspace" in l.hep_last_error()
    need = l.hep_augment_workspace_bytes(2, 64, 64, 128, 3)
    assert need > 0
    assert _call(l, nbytes=need - 1) == INVALID and b"workspace too small" in l.hep_last_error()
    assert _call(l, nbytes=0) == INVALID
    assert _call(l, batch=0) == INVALID and b"batch" in l.hep_last_error()
    for kw in (dict(height=15), dict(height=4097), dict(width=8), dict(width=5000)):
        assert _call(l, **kw) == UNSUPPORTED and b"[16, 4096]" in l.hep_last_error(), kw
        assert l.hep_augment_workspace_bytes(2, kw.get("height", 64), kw.get("width", 64), 128, 3) == UNSUPPORTED
    for kmax in (0, 17, -1):
        assert _call(l, kmax=kmax) == UNSUPPORTED and b"kmax" in l.hep_last_error()
        assert l.hep_augment_workspace_bytes(2, 64, 64, 128, kmax) == UNSUPPORTED
    for size in (0, 8, 130, 4100):
        assert _call(l, size=size) == UNSUPPORTED and b"size" in l.hep_last_error()
    assert l.hep_abi_version() == 1


def test_workspace_is_monotone():
    l = _capi.lib()
    base = dict(batch=2, height=64, width=96, size=128, kmax=3)
    steps = dict(batch=(1, 2, 3, 16), height=(16, 63, 64, 65, 128, 1000, 4096), width=(16, 95, 96, 128, 129, 4096), size=(16, 64, 96, 128, 256, 4096),
                 kmax=(1, 2, 3, 8, 16))
    for key, values in steps.items():
        got = [l.hep_augment_workspace_bytes(*[dict(base, **{key: v})[k] for k in ("batch", "height", "width", "size", "kmax")]) for v in values]
        assert all(g > 0 for g in got) and got == sorted(got), (key, got)
    assert l.hep_augment_workspace_bytes(1, 16, 16, 16, 1) >= 16 * 16 * 3


# ---- what the GPU test's fixed cases contain ----
def test_fixed_cases_contain_what_the_gpu_test_relies_on():
    c, o = A.make_case("A"), A.oracle_case("A")
    assert c["frames"].shape == (4, 128, 128, 3) and c["size"] == 128 and c["boxes"].shape[1] == 3
    assert np.allclose(np.degrees(c["xform"][:, 6]), [0, 37.3, 90, 211.7]) and c["xform"][:, 7].tolist() == [1, 0.7, 1.3, 1]
    # one image with apply = 0
    assert c["xform"][:, 8].tolist() == [0, 1, 1, 1] and o["applied"][0] == 0
    assert np.array_equal(o["mask"][0], c["masks"][0])
    # one whose warped mask is empty: the fallback runs although apply = 1
    assert not A.warp_nearest(c["masks"][3], c["xform"][3, :6]).any() and o["applied"][3] == 0 and o["gt_num"][3] == c["num_gt"][3] == 1
    assert np.array_equal(o["image"][3], A.D.preprocess_image(c["frames"][3], 128)[0].transpose(2, 0, 1))
    # one three-object image in which exactly one object leaves the frame: compaction, order kept (the MIDDLE one leaves)
    assert c["num_gt"][2] == 3 and o["applied"][2] == 1 and o["gt_num"][2] == 2
    wm = A.warp_nearest(c["masks"][2], c["xform"][2, :6])
    present = [bool((wm == v).any()) for v in c["mask_values"][2]]
    assert present == [True, False, True]
    assert o["gt_labels"][2, :2].tolist() == [c["labels"][2, 0], c["labels"][2, 2]] and o["gt_transform"][2, :2, 7].tolist() == [c["extra"][2, 0, 1], c["extra"][2, 2, 1]]
    # a plain augmented image, and rows at and beyond gt_num are zero
    assert o["applied"][1] == 1 and o["gt_num"][1] == 2
    for name in "ABCD":
        c, o = A.make_case(name), A.oracle_case(name)
        for b in range(c["frames"].shape[0]):
            n = int(o["gt_num"][b])
            assert not o["gt_boxes"][b, n:].any() and not o["gt_transform"][b, n:].any() and not o["gt_labels"][b, n:].any()
            bx = o["gt_boxes"][b, :n]
            # no box narrower than 2 pixels (hep_anchor_targets_device divides by the sides)
            assert ((bx[:, 2] - bx[:, 0]) >= 2).all() and ((bx[:, 3] - bx[:, 1]) >= 2).all(), (name, b)
        assert o["image"].shape == (c["frames"].shape[0], 3, c["size"], c["size"])
    # B pads (96 rows of 128), C resizes (64 -> 128) and has one unaugmented image, D's object touches the border after the warp
    assert A.make_case("B")["frames"].shape[1:3] == (96, 128) and not A.oracle_case("B")["image"][:, :, 96:, :].any() and A.oracle_case("B")["applied"].tolist() == [1, 1]
    assert A.make_case("C")["frames"].shape[1:3] == (64, 64) and A.oracle_case("C")["applied"].tolist() == [0, 1] and A.oracle_case("C")["camera"][0, 5] == 2.0
    e = A.oracle_case("E")
    assert e["applied"].tolist() == [1] and 8 <= e["gt_num"][0] < 16 and A.make_case("E")["boxes"].shape[1] == 16
    d = A.oracle_case("D")
    assert d["applied"].tolist() == [1] and d["gt_boxes"][0, 0, 2] == 127 and d["gt_boxes"][0, 0, 3] == 127
    # the bound of the GPU test's pose comparison is not vacuous: the float32 evaluation differs from the float64 one
    er, et = A.rotation_error(A.oracle_case("A", np.float32)["gt_transform"], A.oracle_case("A")["gt_transform"])
    assert 0 < er < 1e-5 and 0 < et < 1e-3
