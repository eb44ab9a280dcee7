"""CPU (no GPU): hep_score_scene_device exists and refuses every invalid argument before any HIP call; gt_scene_table's layout and
refusals; the scene oracle (tests/_score_scene.py) is tests/_score.py's for one annotation and one label, and does what its special
scenes say; SceneEvaluator's averaging against a hand-computed example; SceneFolder on a synthetic folder."""
import ctypes
import math
import os

import numpy as np
import pytest

from hmd_ego_pose_amd import _capi
from hmd_ego_pose_amd import evaluate as E
from tests import _score as S
from tests import _score_scene as SS


def test_scene_entry_point_exists_and_refuses_invalid_arguments():
    assert "hep_score_scene_device" in _capi.SYMBOLS
    l = _capi.lib()
    assert hasattr(l, "hep_score_scene_device")
    buf = np.zeros(256, np.float64)
    a = buf.ctypes.data
    off = lambda *v: (ctypes.c_int32 * len(v))(*v)
    names = ("det_boxes", "det_scores", "det_labels", "det_rotation", "det_translation", "det_hand", "batch", "rows", "gt", "amax", "points",
             "point_offsets", "num_labels", "max_points", "score_threshold", "max_detections", "iou_threshold", "records", "out_scores", "out_tp",
             "out_labels", "out_count", "stream")
    good = dict(zip(names, (a, a, a, a, a, None, 2, 12, a, 4, a, off(0, 1, 38, 1039), 3, 1000, 0.05, 10, 0.5, a, a, a, a, a, None)))
    cases = [({p: None}, p.encode() + b" is NULL") for p in ("det_boxes", "det_scores", "det_labels", "det_rotation", "det_translation", "gt", "points",
                                                              "point_offsets", "records", "out_scores", "out_tp", "out_labels", "out_count")]
    cases += [({"batch": 0}, b"batch"), ({"batch": -2}, b"batch"), ({"rows": 0}, b"rows outside 1..256"), ({"rows": 257, "max_detections": 257}, b"rows outside 1..256"),
              ({"max_detections": 0}, b"max_detections outside 1..rows"), ({"max_detections": 13}, b"max_detections outside 1..rows"),
              ({"amax": 0}, b"amax outside 1..16"), ({"amax": 17}, b"amax outside 1..16"),
              ({"num_labels": 0}, b"num_labels outside 1..63"), ({"num_labels": 64, "point_offsets": off(*range(65))}, b"num_labels outside 1..63"),
              ({"point_offsets": off(1, 2, 38, 1039)}, b"point_offsets[0] must be 0"),
              ({"point_offsets": off(0, 1, 1, 1039)}, b"point_offsets must increase"), ({"point_offsets": off(0, 38, 1, 1039)}, b"point_offsets must increase"),
              ({"max_points": 0}, b"max_points"), ({"max_points": 1025}, b"max_points")]
    for change, reason in cases:
        assert l.hep_anchors(100, None, None) < 0                   # another message in between: the text below is never a stale one
        args = dict(good, **change)
        assert l.hep_score_scene_device(*[args[n] for n in names]) == -1, change            # HEP_ERR_INVALID, and no HIP call was made
        msg = l.hep_last_error()
        assert b"hep_score_scene_device" in msg and reason in msg, (change, msg)
    assert l.hep_abi_version() == 1                                 # additive: the ABI version stays


def _ann(label, **kw):
    d = dict(bbox=np.array([3, 4, 50, 60], np.float32), rotation=np.array([0.1, -0.2, 0.3]), translation=np.array([1.0, 2.0, 500.0]),
             drill_tip=np.array([10.0, -20.0, 30.0, 1.0]), label=label)
    d.update(kw)
    return d


def test_gt_scene_table_layout_and_refusals():
    K = np.array([[480.0, 0, 128.0], [0, 470.0, 120.0], [0, 0, 1]])
    anns = [[_ann(2, coords_3d=np.arange(63, dtype=np.float64).reshape(21, 3)), _ann(0, bbox=np.array([0, 0, 9, 9], np.float32))], [], [_ann(1)]]
    t = E.gt_scene_table(anns, [K, K, K], [0.5, 1.0, 0.25])
    assert t.shape == (3, 2, 88) and t.dtype == np.float64
    assert t[0, 0, :20].tolist() == [1, 3, 4, 50, 60, 0.1, -0.2, 0.3, 1, 2, 500, 10, -20, 30, 480, 470, 128, 120, 0.5, 1]
    assert t[0, 0, 20:83].tolist() == list(range(63)) and t[0, 0, 83] == 2 and not t[0, 0, 84:].any()
    assert t[0, 1, :5].tolist() == [1, 0, 0, 9, 9] and t[0, 1, 19] == 0 and not t[0, 1, 20:].any()            # label 0, no hand joints
    # the single-annotation table is the row with slot 83 cleared
    one = E.gt_table([anns[0][0]], [K], 0.5)[0]
    row = t[0, 0].copy(); row[83] = 0
    assert np.array_equal(row, one)
    # padding rows: slot 0 zero, camera and scale repeated
    for r in (t[1, 0], t[1, 1], t[2, 1]):
        assert r[0] == 0 and r[14:18].tolist() == [480, 470, 128, 120] and not r[1:14].any() and not r[19:].any()
    assert t[1, 0, 18] == 1.0 and t[2, 1, 18] == 0.25 and t[2, 0, 83] == 1
    assert E.gt_scene_table(anns, [K, K, K], 1.0, amax=5).shape == (3, 5, 88)
    assert E.gt_scene_table([[]], [K], 1.0).shape == (1, 1, 88)
    with pytest.raises(ValueError, match="at most 16"):
        E.gt_scene_table([[_ann(0)] * 17], [K], 1.0)
    with pytest.raises(ValueError, match="amax"):
        E.gt_scene_table(anns, [K, K, K], 1.0, amax=1)
    with pytest.raises(ValueError, match="label"):
        E.gt_scene_table([[_ann(-1)]], [K], 1.0)
    with pytest.raises(ValueError, match="label"):
        E.gt_scene_table([[_ann(1.5)]], [K], 1.0)
    bad = _ann(0); del bad["translation"]
    with pytest.raises(ValueError, match="translation"):
        E.gt_scene_table([[bad]], [K], 1.0)
    bad = _ann(0); del bad["label"]
    with pytest.raises(ValueError, match="label"):
        E.gt_scene_table([[bad]], [K], 1.0)
    with pytest.raises(ValueError, match="camera"):
        E.gt_scene_table(anns, [K], 1.0)


@pytest.mark.parametrize("M", [10, 4])
def test_scene_oracle_is_the_single_object_oracle_for_one_annotation_and_one_label(M):
    """synthetic(0) with every detection label set to 0 (the new entry drops foreign labels AFTER the cap like the old one, but a row
    labelled 1 would be a row of another evaluated label's; with one label it is simply dropped - the relabelled rows state the equality):
    records slots 0-11 (slot 0: the old count against the new valid mark aside), score rows and flag rows, record for record."""
    det, gt, pts = S.synthetic(0)
    det = dict(det, labels=np.where(det["labels"] >= 0, 0, det["labels"]).astype(np.int32))
    want, want_s, want_tp = S.score_batch(det, gt, pts, max_detections=M)
    rec, out_s, out_tp, out_l, counts = SS.score_scene_batch(det, gt[:, None, :], [pts], max_detections=M)
    assert np.array_equal(counts, want[:, 0]) and np.array_equal(rec[:, 0, 0], gt[:, 0])
    assert np.array_equal(rec[:, 0, 1:12], want[:, 1:12], equal_nan=True)
    assert np.array_equal(out_s.view(np.int32), want_s.view(np.int32)) and np.array_equal(out_tp, want_tp)
    assert np.array_equal(out_l, np.where(want_tp >= 0, 0, -1)) and np.all(rec[:, 0, 12] == 0) and not rec[:, 0, 13:].any()
    assert want[:, 1].sum() >= 3


def test_special_scenes_do_what_their_names_say():
    det, gt, cl, (rec, out_s, out_tp, out_l, counts), M = SS.case("special")
    assert gt.shape == (8, SS.AMAX, 88) and det["scores"].shape == (8, SS.ROWS) and [len(c) for c in cl] == [1, 37, 1001]
    assert SS.margins_ok(rec)
    iou = lambda b, r, k: float(E.compute_overlap(det["boxes"][b, r:r + 1] / np.float32(gt[b, 0, 18]), gt[b, k:k + 1, 1:5])[0, 0])
    # (a) row 1 prefers the taken slot 1 although it reaches the threshold on the free slot 3; row 2 takes slot 3
    assert iou(0, 1, 1) > iou(0, 1, 3) >= 0.5 and out_tp[0, :4].tolist() == [1, 0, 1, 1] and rec[0, :, 2].tolist() == [3, 0, -1, 2]
    assert rec[0, :, 0].tolist() == [1, 1, 0, 1] and rec[0, :, 12].tolist() == [2, 1, -1, 1]
    # (b), (i)
    assert out_tp[1, :2].tolist() == [1, 0] and rec[1, 0, 1] == 1 and gt[1, 0, 19] == 0 and np.isnan(rec[1, 0, 11]) and not np.isnan(rec[1, 0, 10])
    # (c) the tie is exact and goes to slot 0; the second row meets the same tie and finds slot 0 taken
    assert iou(2, 0, 0) == iou(2, 0, 1) == 80 / 120 and rec[2, :2, 1].tolist() == [1, 0] and rec[2, 0, 4] == 80 / 120 and out_tp[2, :2].tolist() == [1, 0]
    # (d) label 2 annotated, never detected; scale 0.5
    assert gt[3, 0, 18] == 0.5 and rec[3, 1, 0] == 1 and rec[3, 1, 1] == 0 and rec[3, 1, 12] == 2 and 2 not in out_l[3] and rec[3, 0, 1] == 1
    # (e) label 0 rows without label 0 annotations: considered, flag 0 - even the one lying exactly on the label 1 box
    assert out_l[4, :3].tolist() == [0, 1, 0] and out_tp[4, :3].tolist() == [0, 1, 0] and counts[4] == 3
    # (f) twelve candidates, ten kept, the first dropped for its label: nine considered, the tenth candidate matches
    assert (det["scores"][5] > 0.05).sum() == 12 and det["labels"][5, 0] == 3 and counts[5] == 9 and rec[5, 0, 2] == 9 and out_tp[5, 8] == 1
    # (g) the overlap is the eleventh candidate
    assert counts[6] == 10 and rec[6, 0, 0] == 1 and rec[6, 0, 1] == 0 and not out_tp[6].any() and iou(6, 10, 0) > 0.9
    # (h) no valid slot: every record invalid, the rows are considered (labels 1 and 2 are in range) and flagged 0
    assert not rec[7, :, 0].any() and (rec[7, :, 2] == -1).all() and (rec[7, :, 12] == -1).all() and np.isnan(rec[7, :, 3:12]).all()
    assert counts[7] == 2 and out_tp[7, :2].tolist() == [0, 0] and gt[7, 2, 0] == 1 and gt[7, 2, 83] == 7
    # padding of the rows
    for b in range(8):
        assert (out_s[b, counts[b]:] == -1).all() and (out_tp[b, counts[b]:] == -1).all() and (out_l[b, counts[b]:] == -1).all()
    # every random case satisfies the margins by the oracle alone, and matches something under every label
    for name in ("limits", "wide", "evaluator"):
        r = SS.case(name)[3][0]
        assert SS.margins_ok(r), name
        assert all(((r[..., 1] == 1) & (r[..., 12] == l)).any() for l in range(3)), name


def test_scene_mean_against_a_hand_computed_example():
    """Two labels, records written by hand.  Label 0 (diameter 100, asymmetric): two annotations, one matched with ADD 4, ADD-S 3; one
    considered row beside the match.  Label 1 (diameter 200, symmetric): one annotation, rows but no match."""
    nan = float("nan")
    rec = np.zeros((2, 2, 16))
    rec[..., 2], rec[..., 3:12], rec[..., 12] = -1, nan, -1
    rec[0, 0] = [1, 1, 0, 0.9, 0.8, 4.0, 3.0, 20.0, 2.0, 21.0, 1.5, nan, 0, 0, 0, 0]
    rec[0, 1, 0], rec[0, 1, 12] = 1, 1
    rec[1, 0, 0], rec[1, 0, 12] = 1, 0
    sc = np.array([[0.9, 0.8, 0.7], [0.6, -1, -1]], np.float32)
    tp = np.array([[1, 0, 0], [0, -1, -1]], np.int32)
    lab = np.array([[0, 1, 0], [1, -1, -1]], np.int32)
    got = E.summarise_scene(rec, sc, tp, lab, np.array([3, 1], np.int32), [100.0, 200.0], [False, True])
    l0, l1, mean = got["labels"][0], got["labels"][1], got["mean"]
    assert l0["num_annotations"] == 2 and l0["num_matched"] == 1 and l1["num_annotations"] == 1 and l1["num_matched"] == 0
    # label 0: rows 0.9 (hit) and 0.7 (miss): recall 0.5 at precision 1 -> AP 0.5; every fraction 1 / 2
    assert l0["AP"] == 0.5 and l0["ADD"] == 0.5 and l0["ADD-S"] == 0.5 and l0["ADD(-S)"] == 0.5 and l0["5cm_5deg"] == 0.5 and l0["2D_projection"] == 0.5
    assert l0["mixed_distance_mean"] == 4.0 and l0["ADD-S_distance_mean"] == 3.0 and l0["mixed_distance_std"] == 0.0
    assert l1["AP"] == 0.0 and l1["ADD(-S)"] == 0.0 and math.isnan(l1["mixed_distance_mean"]) and "translation_mean" not in l1
    # the mean: fractions (0.5 + 0) / 2 labels with annotations; the label without a match turns every mean / std into NaN
    for k in E.FRACTION_KEYS:
        assert mean[k] == 0.25, (k, mean[k])
    assert mean["num_annotations"] == 3 and mean["num_matched"] == 1 and mean["num_labels"] == 2
    for k in ("mixed_distance_mean", "mixed_distance_std", "translation_mean", "rotation_std", "ADD_distance_mean", "2D_projection_distance_mean"):
        assert math.isnan(mean[k]), (k, mean[k])
    # with label 1 matched too (ADD 9, ADD-S 6, symmetric -> mixed 6) the mean is the plain average; a third label without annotations
    # adds 0 to the sums and nothing to the divisor
    rec[0, 1] = [1, 1, 1, 0.8, 0.7, 9.0, 6.0, 60.0, 1.0, 61.0, 8.0, nan, 1, 0, 0, 0]
    tp[0, 1] = 1
    got = E.summarise_scene(rec, sc, tp, lab, np.array([3, 1], np.int32), [100.0, 200.0, 50.0], [False, True, False])
    mean = got["mean"]
    assert got["labels"][2]["num_annotations"] == 0 and got["labels"][2]["AP"] == 0.0 and mean["num_labels"] == 2
    assert got["labels"][1]["AP"] == 1.0 and got["labels"][1]["ADD(-S)"] == 1.0 and got["labels"][1]["5cm_5deg"] == 0.0 and got["labels"][1]["2D_projection"] == 0.0
    assert mean["AP"] == 0.75 and mean["ADD"] == 0.75 and mean["ADD(-S)"] == 0.75 and mean["5cm_5deg"] == 0.25 and mean["2D_projection"] == 0.25
    assert mean["mixed_distance_mean"] == 5.0 and mean["ADD_distance_mean"] == 6.5 and mean["translation_mean"] == 40.0 and mean["mixed_distance_std"] == 0.0
    assert math.isnan(mean["hand_mean"]) if "hand_mean" in mean else True
    # ... and it is the restated tail of tests/_score_scene.py on a random case
    r = SS.case("evaluator")[3]
    got, want = E.summarise_scene(*r, SS.DIAMETERS, SS.SYMMETRIC), SS.oracle_scene_result(*r)
    for l in range(3):
        assert got["labels"][l] == want["labels"][l]
    assert {k: v for k, v in got["mean"].items() if not math.isnan(v)} == {k: v for k, v in want["mean"].items() if not math.isnan(v)}


def _write_scene_folder(root, size=64):
    """Scene folder data/01 with objects 1, 5 and 6 (6 is not asked for): frame 0 holds 1 and 5, frame 1 holds 5 twice and 1, frame 2 (not
    in the split) holds 6 only.  One merged mask per frame: object 1 is byte 40, object 5 byte 90 (its second instance shares the byte)."""
    import yaml
    from PIL import Image
    from scipy.spatial.transform import Rotation
    rng = np.random.Generator(np.random.PCG64(5))
    obj = os.path.join(root, "data", "01")
    for d in ("rgb", "mask"):
        os.makedirs(os.path.join(obj, d), exist_ok=True)
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    info_models, clouds = {}, {}
    for o, n in ((1, 5), (5, 9), (6, 3)):
        clouds[o] = rng.standard_normal((n, 3)).astype(np.float32)
        with open(os.path.join(root, "models", f"obj_{o:02}.ply"), "wb") as f:
            f.write(b"ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % n)
            for p in clouds[o]:
                f.write(("%r %r %r\n" % (float(p[0]), float(p[1]), float(p[2]))).encode())
        info_models[o] = {"diameter": 100.0 + o}
    info_models[5]["symmetries_continuous"] = [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]
    with open(os.path.join(root, "models", "models_info.yml"), "w") as f:
        yaml.safe_dump(info_models, f)
    boxes = {0: [(1, [5, 6, 20, 18]), (5, [30, 10, 12, 25])], 1: [(5, [2, 3, 10, 10]), (1, [25, 25, 15, 12]), (5, [40, 40, 8, 9])], 2: [(6, [1, 1, 5, 5])]}
    gt, info, truth = {}, {}, {}
    for i, entries in boxes.items():
        Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(obj, "rgb", f"{i:06d}.png"))
        m = np.zeros((size, size), np.uint8)
        m[8:15, 7:19] = 40                                     # object 1's visible pixels: x 7..18, y 8..14 (smaller than its obj_bb)
        m[50:60, 45:50] = 90                                   # object 5's
        Image.fromarray(m).save(os.path.join(obj, "mask", f"{i:06d}.png"))
        gt[i], truth[i] = [], []
        for o, bb in entries:
            R = Rotation.from_rotvec(rng.standard_normal(3)).as_matrix()
            t = [float(v) for v in (rng.normal(0, 40), rng.normal(0, 40), 500 + rng.normal(0, 50))]
            gt[i].append({"cam_R_m2c": [float(v) for v in R.reshape(-1)], "cam_t_m2c": t, "obj_bb": bb, "obj_id": o})
            truth[i].append((o, bb, R, t))
        info[i] = {"cam_K": [480.0, 0.0, 32.0, 0.0, 470.0, 30.0, 0.0, 0.0, 1.0], "depth_scale": 1.0}
    for name, d in (("gt_0.yml", gt), ("info_0.yml", info)):
        with open(os.path.join(obj, name), "w") as f:
            yaml.safe_dump(d, f)
    with open(os.path.join(obj, "test_0.txt"), "w") as f:
        f.write("000000\n000001\n")
    return clouds, truth


def test_scene_folder_reads_every_entry(tmp_path):
    clouds, truth = _write_scene_folder(str(tmp_path))
    ds = E.SceneFolder(str(tmp_path), [5, 1], scene_id=1)                                # label 0 = object 5, label 1 = object 1
    assert len(ds) == 2 and ds.amax == 3 and [len(a) for a in ds.annotations] == [2, 3]
    assert [m[1] for m in ds.models] == [105.0, 101.0] and [m[2] for m in ds.models] == [True, False]
    assert np.array_equal(ds.models[0][0], clouds[5]) and np.array_equal(ds.models[1][0], clouds[1])
    assert [a["label"] for a in ds.annotations[0]] == [1, 0] and [a["label"] for a in ds.annotations[1]] == [0, 1, 0]      # the file's order, both 5s kept
    for i in range(2):
        for a, (o, bb, R, t) in zip(ds.annotations[i], truth[i]):
            assert a["bbox"].tolist() == [bb[0], bb[1], bb[0] + bb[2], bb[1] + bb[3]] and a["translation"].tolist() == t
            assert np.allclose(E.axis_angle_to_matrix(a["rotation"]), R, atol=1e-12) and a["drill_tip"].tolist() == [0, 0, 0, 1]
    assert ds.load_image(0).shape == (64, 64, 3) and ds.camera_input(1, 0.5).tolist() == [480, 470, 32, 30, 1000, 0.5]
    t = E.gt_scene_table(ds.annotations, ds.camera, 1.0, ds.amax)
    assert t.shape == (2, 3, 88) and t[:, :, 0].tolist() == [[1, 1, 0], [1, 1, 1]] and t[:, :, 83].tolist() == [[1, 0, 0], [0, 1, 0]]
    # boxes from the merged mask for the objects the mapping names, obj_bb for the others
    dm = E.SceneFolder(str(tmp_path), [5, 1], scene_id=1, mask_values={1: 40})
    assert dm.annotations[0][0]["bbox"].tolist() == [7, 8, 18, 14] and dm.annotations[0][1]["bbox"].tolist() == ds.annotations[0][1]["bbox"].tolist()
    dm = E.SceneFolder(str(tmp_path), [1, 5], mask_values={1: 40, 5: 90})        # the folder defaults to the first id
    assert [a["bbox"].tolist() for a in dm.annotations[1]] == [[45, 50, 49, 59], [7, 8, 18, 14], [45, 50, 49, 59]]
    assert E.SceneFolder(str(tmp_path), [1, 5], mask_values={5: 7}).annotations[0][1]["bbox"].tolist() == [0, 0, 0, 0]          # a byte the mask lacks
    only = E.SceneFolder(str(tmp_path), [6, 1], scene_id=1)                  # frames of the split hold no object 6: label 0 has no annotation
    assert [[a["label"] for a in fr] for fr in only.annotations] == [[1], [1]] and only.amax == 1
    with pytest.raises(ValueError):
        E.SceneFolder(str(tmp_path), [1, 1])
