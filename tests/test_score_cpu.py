"""CPU (no GPU): hep_score_detections_device exists and refuses every invalid argument before any HIP call; its numpy statement
(tests/_score.py) makes evaluate()'s per-image decisions; PlateauSchedule is torch's ReduceLROnPlateau."""
import math

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi
from hmd_ego_pose_amd import evaluate as E
from oracle import decode_ref as D
from tests import _score as S


def test_score_entry_point_exists_and_refuses_invalid_arguments():
    assert "hep_score_detections_device" in _capi.SYMBOLS
    l = _capi.lib()
    assert hasattr(l, "hep_score_detections_device")
    buf = np.zeros(256, np.float64)
    a = buf.ctypes.data
    names = ("det_boxes", "det_scores", "det_labels", "det_rotation", "det_translation", "det_hand", "batch", "rows", "gt", "points",
             "num_points", "max_points", "label", "score_threshold", "max_detections", "iou_threshold", "records", "out_scores", "out_tp", "stream")
    good = dict(zip(names, (a, a, a, a, a, None, 2, 12, a, a, 37, 1000, 0, 0.05, 10, 0.5, a, a, a, None)))
    cases = [({p: None}, p.encode() + b" is NULL") for p in ("det_boxes", "det_scores", "det_labels", "det_rotation", "det_translation", "gt",
                                                              "points", "records", "out_scores", "out_tp")]
    cases += [({"batch": 0}, b"batch"), ({"batch": -2}, b"batch"), ({"rows": 0}, b"rows outside 1..256"), ({"rows": 257, "max_detections": 257}, b"rows outside 1..256"),
              ({"max_detections": 0}, b"max_detections outside 1..rows"), ({"max_detections": 13}, b"max_detections outside 1..rows"),
              ({"num_points": 0}, b"num_points"), ({"max_points": 0}, b"max_points"), ({"max_points": 1025}, b"max_points")]
    for change, reason in cases:
        assert l.hep_anchors(100, None, None) < 0                   # another message in between: the text below is never a stale one
        args = dict(good, **change)
        assert l.hep_score_detections_device(*[args[n] for n in names]) == -1, change      # HEP_ERR_INVALID, and no HIP call was made
        msg = l.hep_last_error()
        assert b"hep_score_detections_device" in msg and reason in msg, (change, msg)
    assert l.hep_abi_version() == 1                                 # additive: the ABI version stays


def test_gt_table_layout():
    ann = [dict(bbox=np.array([3, 4, 50, 60], np.float32), rotation=np.array([0.1, -0.2, 0.3]), translation=np.array([1.0, 2.0, 500.0]),
                drill_tip=np.array([10.0, -20.0, 30.0, 1.0]), coords_3d=np.arange(63, dtype=np.float64).reshape(21, 3)),
           dict(bbox=np.array([0, 0, 9, 9], np.float32), rotation=np.zeros(3), translation=np.ones(3), drill_tip=np.array([0, 0, 0, 1.0]))]
    K = np.array([[480.0, 0, 128.0], [0, 470.0, 120.0], [0, 0, 1]])
    t = E.gt_table(ann, [K, K], 0.5)
    assert t.shape == (2, 88) and t.dtype == np.float64
    assert t[0, :20].tolist() == [1, 3, 4, 50, 60, 0.1, -0.2, 0.3, 1, 2, 500, 10, -20, 30, 480, 470, 128, 120, 0.5, 1]
    assert t[0, 20:83].tolist() == list(range(63)) and not t[0, 83:].any()
    assert t[1, 19] == 0 and not t[1, 20:].any() and t[1, 18] == 0.5
    with pytest.raises(ValueError):
        E.gt_table(ann, [K], 1.0)


def test_numpy_statement_makes_evaluates_decisions():
    """tests/_score.py against an independent recomputation in the manner of test_evaluator_on_a_synthetic_linemod_folder: evaluate.py's
    post_filter and compute_overlap for the decisions, the oracle's rodrigues / add_metric / add_s_metric and point-by-point loops for
    the values, on randomised rows (all six special images and 60 random ones, caps 10 and 4, two thresholds)."""
    checked = matched = 0
    for seed, M, iou_thr in ((1, 10, 0.5), (2, 4, 0.5), (3, 10, 0.75)):
        det, gt, pts = S.synthetic(seed, extra=20, num_points=37)
        rec, out_s, out_tp = S.score_batch(det, gt, pts, max_detections=M, iou_threshold=iou_thr)
        for b in range(gt.shape[0]):
            scale = gt[b, 18]
            boxes, sc, labels, rots, trans, hands = E.post_filter({k: torch.from_numpy(v[b]) for k, v in det.items()}, scale, 0.05, M)
            own = labels == 0
            boxes, sc, rots, trans, hands = boxes[own], sc[own], rots[own], trans[own], hands[own]
            assert rec[b, 0] == len(sc) and np.array_equal(out_s[b, :len(sc)], sc) and np.all(out_s[b, len(sc):] == -1) and np.all(out_tp[b, len(sc):] == -1)
            hit = [d for d in range(len(sc)) if E.compute_overlap(boxes[d:d + 1], gt[b, None, 1:5])[0, 0] >= iou_thr]
            want_tp = np.zeros(len(sc), np.int32)
            want_tp[hit[:1]] = 1
            assert np.array_equal(out_tp[b, :len(sc)], want_tp) and rec[b, 1] == bool(hit)
            checked += 1
            if not hit:
                assert rec[b, 2] == -1 and np.isnan(rec[b, 3:12]).all() and not rec[b, 12:].any()
                continue
            matched += 1
            d = hit[0]
            row = int(rec[b, 2])
            assert det["scores"][b, row] == sc[d] and np.array_equal(det["translation"][b, row], trans[d]) and rec[b, 3] == sc[d]
            P = pts.astype(np.float64)
            Rg, Rp = D.rodrigues(gt[b, 5:8].astype(np.float32)), D.rodrigues(rots[d])
            tg32 = gt[b, 8:11].astype(np.float32).astype(np.float64)
            assert rec[b, 5] == D.add_metric(P, 1.0, Rg, tg32, Rp, trans[d].astype(np.float64))[1]
            assert rec[b, 6] == D.add_s_metric(P, 1.0, Rg, tg32, Rp, trans[d].astype(np.float64))[1]
            Rg, tg, tp = D.rodrigues(gt[b, 5:8]), gt[b, 8:11], trans[d].astype(np.float64)
            fx, fy, cx, cy = gt[b, 14:18]
            px = lambda R_, t_: np.array([[fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy] for q in (P @ R_.T + t_)])
            want = {7: math.sqrt(sum((tg - tp) ** 2)), 8: abs(math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(Rp @ Rg.T) - 1) / 2))))),
                    9: np.linalg.norm(Rg @ gt[b, 11:14] + tg - Rp @ gt[b, 11:14] - tp), 10: np.linalg.norm(px(Rg, tg) - px(Rp, tp), axis=1).mean()}
            if gt[b, 19]:
                want[11] = np.linalg.norm(gt[b, 20:83].reshape(21, 3) - hands[d].astype(np.float64).reshape(21, 3), axis=1).mean() * 1000.0
            else:
                assert np.isnan(rec[b, 11])
            for slot, w in want.items():
                assert abs(rec[b, slot] - w) <= 1e-12 * max(1.0, abs(w)), (b, slot, rec[b, slot], w)
        # the special images do what their names say (tests/_score.py SPECIAL)
        assert rec[0, 0] == 0 and rec[0, 1] == 0
        assert rec[1, 1] == 1 and rec[1, 2] == 1 and gt[1, 18] == 0.5 and det["labels"][1, 0] == 1
        assert out_tp[2, 0] == 0 and not gt[2, 5:8].any()
        if iou_thr == 0.5:
            assert rec[2, 2] == 1 and rec[3, 1] == 1 and rec[3, 4] == 0.5 and rec[3, 5] <= 1e-12
        else:
            assert rec[3, 1] == 0                                   # ... and a threshold above 0.5 does not take it
        assert rec[4, 0] == M and rec[4, 1] == 0 and (det["scores"][4] > 0.05).sum() == S.ROWS
        assert gt[5, 19] == 0 and rec[5, 1] == 1 and np.isnan(rec[5, 11])
    assert checked == 78 and matched >= 30, (checked, matched)


def test_tail_of_evaluate_and_the_numpy_tail_agree():
    """metric_summary (the tail ``evaluate`` and ``DeviceEvaluator.result`` share) against the restated tail of tests/_score.py on
    the same records: equal bit for bit, for both settings of ``symmetric``; without a match the distance keys are NaN."""
    det, gt, pts = S.synthetic(5, extra=14, num_points=37)
    rec, out_s, out_tp = S.score_batch(det, gt, pts)
    keep = np.arange(out_s.shape[1])[None, :] < rec[:, 0:1]
    r = rec[rec[:, 1] == 1.0]
    m = dict(add=r[:, 5], add_s=r[:, 6], t_diff=r[:, 7], r_diff=r[:, 8], tip=r[:, 9], reproj=r[:, 10], hand=r[:, 11][~np.isnan(r[:, 11])])
    for sym in (False, True):
        got = E.metric_summary(float(len(rec)), [float(v) for v in out_s[keep]], out_tp[keep], m, S.DIAMETER * 0.1, symmetric=sym)
        assert got == S.oracle_result(rec, out_s, out_tp, symmetric=sym)
    base = E.metric_summary(float(len(rec)), [float(v) for v in out_s[keep]], out_tp[keep], m, S.DIAMETER * 0.1)
    assert set(got) - set(base) == {"ADD(-S)", "translation_tip_std", "mixed_distance_mean", "mixed_distance_std"}      # evaluate()'s own keys are untouched
    none = E.metric_summary(2.0, [0.9], [0], None, 18.0, symmetric=False)
    assert none["num_matched"] == 0 and none["ADD(-S)"] == 0.0 and math.isnan(none["mixed_distance_mean"]) and none["AP"] == 0.0


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_plateau_schedule_is_reduce_lr_on_plateau(seed):
    """200 epochs of a random metric sequence - improvements, plateaus, relative changes right at the threshold, a NaN - on a dummy
    optimiser with the reference's arguments (train.py:107-109); the two rates are equal at every epoch, down to min_lr."""
    from hmd_ego_pose_amd.trainer import PlateauSchedule
    rng = np.random.Generator(np.random.PCG64(70 + seed))
    lr0, patience = (1e-4 if seed < 2 else 4e-7), 15
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr0)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=patience, threshold=1e-4, threshold_mode="rel",
                                                     cooldown=0, min_lr=1e-7, eps=1e-8)
    mine = PlateauSchedule(lr0, factor=0.5, patience=patience, threshold=1e-4, min_lr=1e-7, eps=1e-8)
    best, lrs = 30.0, []
    for epoch in range(200):
        u = rng.random()
        if epoch < 12 and u < 0.6:
            best *= 1.0 - rng.uniform(0.001, 0.05); metric = best          # a real improvement
        elif u < 0.1:
            metric = best * (1.0 - 1e-4 * rng.choice([0.5, 0.999, 1.0, 1.001]))    # at the relative threshold, either side
            best = min(best, metric)
        elif u < 0.12:
            metric = float("nan")
        else:
            metric = best * (1.0 + rng.uniform(0, 0.2))                     # a plateau
        ref.step(metric)
        lr = mine.step(metric)
        assert lr == opt.param_groups[0]["lr"], (epoch, lr, opt.param_groups[0]["lr"])
        assert mine.best == ref.best or (math.isnan(mine.best) and math.isnan(ref.best))
        lrs.append(lr)
    assert lrs[-1] < lr0 and len(set(lrs)) >= 3
    if seed >= 2:
        assert lrs[-1] == 1e-7                                              # the floor is reached and held
