"""CPU (no GPU): the numpy definition of the pose overlays (tests/_draw.py) against hand-written cases, the host helpers of
hmd_ego_pose_amd/draw.py, the folder readers' cuboids, and hep_draw_poses_device's existence and refusals before any HIP call."""
import os
import re

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi
from hmd_ego_pose_amd import draw as DR
from hmd_ego_pose_amd import evaluate as E
from tests import _draw as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(h=32, w=32):
    return np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")


# ---- the oracle's primitives -----------------------------------------------------------------------------------------------------
def test_horizontal_segment_of_thickness_1_covers_exactly_its_pixels():
    ys, xs = _grid()
    m = D.segment_mask(xs, ys, (5, 9), (20, 9), 1)
    want = np.zeros((32, 32), bool)
    want[9, 5:21] = True
    assert np.array_equal(m, want)
    assert np.array_equal(D.segment_mask(xs, ys, (20, 9), (5, 9), 1), want)          # the direction does not matter


def test_axis_aligned_widths_are_1_3_3_5():
    ys, xs = _grid()
    for t, width in ((1, 1), (2, 3), (3, 3), (4, 5)):
        m = D.segment_mask(xs, ys, (4, 16), (27, 16), t)
        assert set(m[:, 15].nonzero()[0]) == set(range(16 - width // 2, 16 + width // 2 + 1)), t      # a column in the middle
        m = D.segment_mask(xs, ys, (16, 4), (16, 27), t)
        assert int(m[15].sum()) == width, t


def test_diagonal_of_thickness_1_has_no_gaps():
    ys, xs = _grid()
    for b in ((29, 13), (13, 29), (29, 29), (3, 17)):
        m = D.segment_mask(xs, ys, (2, 2), b, 1)
        steps = max(abs(b[0] - 2), abs(b[1] - 2))
        # every column (or row, along the longer axis) between the end points holds a pixel, and neighbours touch (8-connected)
        along = m.any(axis=0) if abs(b[0] - 2) >= abs(b[1] - 2) else m.any(axis=1)
        assert int(along.sum()) == steps + 1, b
        pts = np.argwhere(m)
        for p in pts:
            assert len(pts) == 1 or (np.abs(pts - p).max(axis=1) == 1).any(), (b, p)


def test_degenerate_segment_is_a_disc_of_radius_half_the_thickness():
    ys, xs = _grid()
    assert int(D.segment_mask(xs, ys, (10, 10), (10, 10), 1).sum()) == 1
    assert int(D.segment_mask(xs, ys, (10, 10), (10, 10), 2).sum()) == 5           # |p|^2 <= 1
    assert int(D.segment_mask(xs, ys, (10, 10), (10, 10), 4).sum()) == 13          # |p|^2 <= 4


def test_disc_of_radius_3_has_29_pixels():
    ys, xs = _grid()
    m = D.disc_mask(xs, ys, (12, 15))
    assert int(m.sum()) == 29 and m[15, 9] and m[15, 15] and m[12, 12] and not m[12, 10] and not m[13, 9]


def test_coverage_products_stay_inside_int64_at_the_extremes():
    """Frames up to 4096 and points saturated to [-8192, 8191]: the largest products, in Python integers, stay below 2^62."""
    worst = 0
    for a in ((-8192, -8192), (8191, 8191), (-8192, 8191)):
        for b in ((8191, 8191), (-8192, -8192), (8191, -8192)):
            for p in ((0, 0), (4095, 4095), (0, 4095), (4095, 0)):
                dx, dy, qx, qy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
                worst = max(worst, 4 * (qx * dy - qy * dx) ** 2, 64 * (dx * dx + dy * dy), 4 * (qx * qx + qy * qy), abs(qx * dx + qy * dy))
    assert worst < 2 ** 62


# ---- the oracle's order, sources and special cases -------------------------------------------------------------------------------
def _flat_case():
    """One image 32 x 40 whose single annotation and single detection share the pose: the detection overwrites the annotation."""
    cam = np.array([100.0, 100.0, 20.0, 16.0, 1.0])
    g = np.zeros((1, 1, 88))
    g[0, 0, 0], g[0, 0, 1:5], g[0, 0, 5:8], g[0, 0, 8:11], g[0, 0, 14:19] = 1.0, [4, 5, 30, 25], [0.3, -0.2, 0.1], [3.0, -2.0, 400.0], cam
    det = dict(boxes=np.array([[[4, 5, 30, 25]]], np.float32), scores=np.array([[0.9]], np.float32), labels=np.array([[0]], np.int32),
               rotation=(np.array([[[0.3, -0.2, 0.1]]]) / np.pi).astype(np.float32), translation=np.array([[[3.0, -2.0, 400.0]]], np.float32), hand=None)
    return np.full((1, 32, 40, 3), 9, np.uint8), g, det, D.case_cuboids(1), np.array([[200, 10, 30]], np.uint8)


def test_later_shape_overwrites_earlier_and_untouched_pixels_keep_their_bytes():
    frames, g, det, cub, col = _flat_case()
    only_ann = D.draw_poses(frames, cub, col, gt=g, ann_layers=3, thickness=2)
    both = D.draw_poses(frames, cub, col, gt=g, det=det, ann_layers=3, det_layers=3, thickness=2)
    only_det = D.draw_poses(frames, cub, col, camera=g[:, 0, 14:19], det=det, det_layers=3, thickness=2)
    green = (only_ann == np.array([0, 255, 0], np.uint8)).all(axis=3)
    assert green.sum() > 50 and (only_ann[~green & ~(only_ann == np.array([0, 127, 0], np.uint8)).all(axis=3)] == 9).all()
    # the float32 detection pose projects to the annotation's pixels here (asserted), so the detection's colours replace the annotation's everywhere
    assert np.array_equal((only_ann != 9).any(axis=3), (only_det != 9).any(axis=3))
    assert np.array_equal(both, only_det)
    assert ((both == np.array([200, 10, 30], np.uint8)).all(axis=3) == green).all()
    assert np.array_equal((both == np.array([255, 0, 255], np.uint8)).all(axis=3), (only_ann == np.array([0, 127, 0], np.uint8)).all(axis=3))
    # within ONE shape the cuboid is drawn after the box: where they cross the cuboid's colour stands
    box_only = D.draw_poses(frames, cub, col, gt=g, ann_layers=1, thickness=2)
    crossing = (box_only != 9).any(axis=3) & green
    assert crossing.any()


def test_image_without_shapes_is_unchanged_and_main_case_holds_what_it_says():
    c = D.case_main()
    sh = []
    out = D.draw_poses(c["frames"], c["cuboids"], c["colours"], gt=c["gt"], det=c["det"], score_threshold=0.5, max_detections=3, ann_layers=7,
                       det_layers=7, thickness=2, shapes_out=sh)
    D.assert_input_condition(sh)
    assert np.array_equal(out[1], c["frames"][1]) and sh[1] == []
    assert not np.array_equal(out[0], c["frames"][0]) and not np.array_equal(out[2], c["frames"][2])
    # image 0: annotations of slots 0 and 2 (slot 1 padding, slot 3 label 3 of 3 labels); rows 0 and 4 (1 at the threshold, 2 padding, 3 label 5, 5 beyond the cap)
    assert [s.annotation for s in sh[0]] == [True, True, False, False]
    assert sum(p is not None for p in sh[0][0].pts[13:]) == 21 and all(p is None for p in sh[0][1].pts[13:])
    assert (c["det"]["scores"][0] > np.float32(0.5)).tolist() == [True, False, False, True, True, True] and c["det"]["labels"][0, 3] == 5
    # image 2: off-frame points, a corner behind the camera, a saturated coordinate, zero rotations, a one-point box and coinciding joints
    a0, a1, a2, d0, d1, d2 = sh[2]
    assert any(not (0 <= p[0] < 64 and 0 <= p[1] < 48) for p in a0.pts[4:12]) and any(0 <= p[0] < 64 and 0 <= p[1] < 48 for p in a0.pts[4:13])
    assert min(a1.depths) < 0 and any(p is None for p in a1.pts[4:12])
    assert any(v in (-8192, 8191) for p in a1.pts[4:12] if p is not None for v in p)
    assert a2.angle == 0.0 and d0.angle == 0.0 and len(set(a2.pts[:4])) == 1 and a2.pts[13 + 5] == a2.pts[13 + 6]
    assert all(p is None for p in d2.pts[4:13]) and all(p is not None for p in d2.pts[:4])          # behind the camera: only its 2D box
    # the layers: nothing but the cuboid layer by default; the hand layer only adds pixels of the hand colours
    cub = D.draw_poses(c["frames"], c["cuboids"], c["colours"], gt=c["gt"], det=c["det"], max_detections=3)
    assert (cub != out).any() and not (cub == np.array(D.ANN_HAND, np.uint8)).all(axis=3)[(c["frames"] != np.array(D.ANN_HAND, np.uint8)).any(axis=3)].any()


def test_caps_case_meets_the_input_condition_and_cuts_at_64():
    c = D.case_caps()
    sh = []
    D.draw_poses(c["frames"], c["cuboids"], c["colours"], gt=c["gt"], det=c["det"], score_threshold=0.5, max_detections=64, ann_layers=7,
                 det_layers=7, thickness=2, shapes_out=sh)
    D.assert_input_condition(sh)
    cand = np.nonzero(c["det"]["scores"][0] > np.float32(0.5))[0]
    assert len(cand) > 64
    kept = cand[:64]
    assert len(sh[0]) == 16 + int((c["det"]["labels"][0, kept] < 5).sum()) < 16 + 64           # some kept rows carry the label 5 of 5 labels


def test_rodrigues_is_the_evaluators():
    rng = np.random.Generator(np.random.PCG64(4))
    for _ in range(20):
        r = rng.standard_normal(3) * rng.uniform(0.01, 3.0)
        R, th = D.rodrigues(r)
        assert np.allclose(np.array(R).reshape(3, 3), E.axis_angle_to_matrix(r), rtol=0, atol=1e-14) and abs(th - np.linalg.norm(r)) < 1e-15
    assert D.rodrigues(np.zeros(3))[0] == [1, 0, 0, 0, 1, 0, 0, 0, 1]


# ---- host helpers ----------------------------------------------------------------------------------------------------------------
def test_cuboid_corners_against_typed_in_corners():
    got = DR.cuboid_corners([-100.0, -80.0, -150.0], [200.0, 160.0, 300.0])
    want = [[-100, -80, -150], [100, -80, -150], [100, 80, -150], [-100, 80, -150], [-100, -80, 150], [100, -80, 150], [100, 80, 150], [-100, 80, 150]]
    assert got.dtype == np.float32 and got.tolist() == want
    assert np.array_equal(D.corners([-100.0, -80.0, -150.0], [200.0, 160.0, 300.0]), got)


def test_label_colours_deterministic_and_distinct():
    for n in (1, 7, 16, 63):
        a, b = DR.label_colours(n), DR.label_colours(n)
        assert a.dtype == np.uint8 and a.shape == (n, 3) and np.array_equal(a, b)
        assert len({tuple(c) for c in a.tolist()}) == n
        assert np.array_equal(a, DR.label_colours(63)[:n])
    assert DR.label_colours(3).tolist() == [[255, 200, 0], [0, 238, 255], [255, 0, 166]]          # hue 47, 184, 321 by the docstring's formula


def test_detections_from_records_on_synthetic_records():
    rec = np.zeros((2, 3, 80), np.int32)
    f = rec.view(np.float32)
    f[...] = np.arange(2 * 3 * 80, dtype=np.float32).reshape(2, 3, 80) * 0.5
    rec[..., 0], rec[..., 1], rec[..., 2] = 1, [[0, 1, 2], [2, 1, 0]], 7
    d = DR.detections_from_records(torch.from_numpy(rec))
    assert {k: tuple(v.shape) for k, v in d.items()} == dict(boxes=(2, 3, 4), scores=(2, 3), labels=(2, 3), rotation=(2, 3, 3), translation=(2, 3, 3), hand=(2, 3, 63))
    assert all(v.is_contiguous() for v in d.values()) and d["labels"].dtype == torch.int32 and d["boxes"].dtype == torch.float32
    assert np.array_equal(d["boxes"].numpy(), f[..., 5:9]) and np.array_equal(d["scores"].numpy(), f[..., 4]) and np.array_equal(d["labels"].numpy(), rec[..., 1])
    assert np.array_equal(d["rotation"].numpy(), f[..., 9:12]) and np.array_equal(d["translation"].numpy(), f[..., 12:15]) and np.array_equal(d["hand"].numpy(), f[..., 15:78])
    one = DR.detections_from_records(torch.from_numpy(rec[:, 0]))                   # Session.top1: one row per image
    assert tuple(one["boxes"].shape) == (2, 1, 4) and np.array_equal(one["hand"].numpy()[:, 0], f[:, 0, 15:78])
    for bad in (torch.zeros(2, 80), torch.zeros(2, 79, dtype=torch.int32), torch.zeros(80, dtype=torch.int32), np.zeros((2, 80), np.int32)):
        with pytest.raises(ValueError):
            DR.detections_from_records(bad)


def test_lazy_exports():
    import hmd_ego_pose_amd as H
    assert H.draw_poses is DR.draw_poses and H.cuboid_corners is DR.cuboid_corners and H.label_colours is DR.label_colours
    assert H.detections_from_records is DR.detections_from_records


def test_folder_readers_return_the_cuboid_the_folder_holds(tmp_path):
    from tests._util import make_linemod_folder
    make_linemod_folder(str(tmp_path / "ds"), n=2, size=64)
    want = DR.cuboid_corners([-100.0, -80.0, -150.0], [200.0, 160.0, 300.0])            # what make_linemod_folder writes into models_info.yml
    ds = E.LinemodFolder(str(tmp_path / "ds"))
    assert ds.cuboid.dtype == np.float32 and np.array_equal(ds.cuboid, want)
    sc = E.SceneFolder(str(tmp_path / "ds"), [1])
    assert sc.cuboids.shape == (1, 8, 3) and np.array_equal(sc.cuboids[0], want)
    assert E._model_cuboid({"diameter": 1.0, "min_x": 0.0}) is None


# ---- the entry point: symbol, ABI version, refusals ------------------------------------------------------------------------------
NAMES = ("frames", "batch", "height", "width", "gt", "amax", "camera", "det_boxes", "det_scores", "det_labels", "det_rotation", "det_translation",
         "det_hand", "rows", "score_threshold", "max_detections", "cuboids", "colours", "num_labels", "ann_layers", "det_layers", "thickness", "stream")


def test_symbol_in_header_binding_and_library():
    assert "hep_draw_poses_device" in _capi.SYMBOLS and len(_capi.SYMBOLS["hep_draw_poses_device"][1]) == len(NAMES)
    l = _capi.lib()
    assert hasattr(l, "hep_draw_poses_device") and l.hep_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "hep.h")).read()
    decl = re.search(r"int hep_draw_poses_device\(([^;]*)\);", header)
    assert decl and len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(NAMES)
    for name, value in (("HEP_DRAW_BOX2D", 1), ("HEP_DRAW_CUBOID", 2), ("HEP_DRAW_HAND", 4), ("HEP_DRAW_MAX_DETECTIONS", 64)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert (_capi.DRAW_BOX2D, _capi.DRAW_CUBOID, _capi.DRAW_HAND, _capi.DRAW_MAX_DETECTIONS) == (1, 2, 4, 64)
    assert re.search(r"#define HEP_ABI_VERSION 1\b", header)


def test_entry_point_refuses_invalid_arguments_before_any_hip_call():
    l = _capi.lib()
    buf = np.zeros(256, np.float64)
    a = buf.ctypes.data
    good = dict(zip(NAMES, (a, 2, 48, 64, a, 4, a, a, a, a, a, a, a, 12, 0.5, 10, a, a, 3, 2, 7, 2, None)))
    det5 = ("det_boxes", "det_scores", "det_labels", "det_rotation", "det_translation")
    cases = [({p: None}, p.encode() + b" is NULL", -1) for p in ("frames", "cuboids", "colours")]
    cases += [({"gt": None, "camera": None}, b"gt and camera are both NULL", -1),
              ({"amax": 0}, b"amax outside 1..16", -1), ({"amax": 17}, b"amax outside 1..16", -1)]
    cases += [({p: None}, b"must all be given or all be NULL", -1) for p in det5]
    cases += [({p: None for p in det5[:k]}, b"must all be given or all be NULL", -1) for k in (2, 3, 4)]
    cases += [({p: None for p in det5}, b"det_hand without the other det_* arrays", -1),
              ({"rows": 0}, b"rows outside 1..256", -1), ({"rows": 257}, b"rows outside 1..256", -1),
              ({"max_detections": 0}, b"max_detections outside 1..min(rows, 64)", -1), ({"max_detections": 13}, b"max_detections outside 1..min(rows, 64)", -1),
              ({"rows": 256, "max_detections": 65}, b"max_detections outside 1..min(rows, 64)", -1),
              ({"num_labels": 0}, b"num_labels outside 1..63", -1), ({"num_labels": 64}, b"num_labels outside 1..63", -1),
              ({"thickness": 0}, b"thickness outside 1..8", -1), ({"thickness": 9}, b"thickness outside 1..8", -1),
              ({"ann_layers": 8}, b"layer bits", -1), ({"det_layers": 9}, b"layer bits", -1), ({"ann_layers": -1}, b"layer bits", -1),
              ({"batch": 0}, b"batch must be >= 1", -1), ({"batch": -3}, b"batch must be >= 1", -1),
              ({"height": 15}, b"height and width must be in 16..4096", -4), ({"height": 4097}, b"height and width must be in 16..4096", -4),
              ({"width": 15}, b"height and width must be in 16..4096", -4), ({"width": 4097}, b"height and width must be in 16..4096", -4)]
    for change, reason, code in cases:
        assert l.hep_anchors(100, None, None) < 0                   # another message in between: the text below is never a stale one
        args = dict(good, **change)
        assert l.hep_draw_poses_device(*[args[n] for n in NAMES]) == code, change          # HEP_ERR_INVALID / HEP_ERR_UNSUPPORTED, and no HIP call was made
        msg = l.hep_last_error()
        assert b"hep_draw_poses_device" in msg and reason in msg, (change, msg)
    assert l.hep_abi_version() == 1                                 # additive: the ABI version stays


def test_draw_poses_raises_value_error_for_each_wrong_argument():
    """Every check of draw_poses that does not need a device tensor: with host tensors the first refusals are dtype, rank and device."""
    cub = D.case_cuboids(2)
    with pytest.raises(ValueError, match="uint8 tensor"):
        DR.draw_poses(torch.zeros(1, 32, 32, 3), cuboids=cub, camera=torch.zeros(1, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="uint8 tensor"):
        DR.draw_poses(torch.zeros(32, 32, 3, dtype=torch.uint8), cuboids=cub, camera=torch.zeros(1, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="uint8 tensor"):
        DR.draw_poses(torch.zeros(1, 32, 32, 4, dtype=torch.uint8), cuboids=cub, camera=torch.zeros(1, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="uint8 tensor"):
        DR.draw_poses(np.zeros((1, 32, 32, 3), np.uint8), cuboids=cub, camera=torch.zeros(1, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="on the GPU"):
        DR.draw_poses(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), cuboids=cub, camera=torch.zeros(1, 5, dtype=torch.float64))
