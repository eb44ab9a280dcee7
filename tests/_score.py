"""hep_score_detections_device stated in numpy - one image's record, score row and flag row - from evaluate.py's own functions and
the oracle's ADD / ADD-S, a generator of synthetic detection rows with their ground truth, and the tail that turns records into
the metric dictionary.  Shared by tests/test_score_cpu.py and tests/test_gpu_score.py.

The definition (include/hep.h) is what ``evaluate`` does for one image: evaluate.py ``post_filter`` (boxes / scale and
rotations x pi in float32, score > threshold, first max_detections), the label cut, the first candidate whose IoU reaches the
threshold, and the metrics of that pair."""
import math

import numpy as np

from hmd_ego_pose_amd import evaluate as E
from oracle import decode_ref as D

GT, REC = 88, 16
NAN = float("nan")
DIAMETER = 180.0
# tolerances of the GPU tests, by record slot: float64 sums in another order 1e-9 relative with a floor of 1 (the project's bound
# for them); ADD-S 1e-6 (float32 minima, numpy averages them in float32 pairwise: tests/test_gpu_parity.py); rotation 1e-5 degrees
# absolute (a few ulp on the trace move arccos near 1 by about 5e-8 rad)
REL = {5: 1e-9, 6: 1e-6, 7: 1e-9, 9: 1e-9, 10: 1e-9, 11: 1e-9}
ROT_ABS = 1e-5


def tolerance(slot: int, want: float) -> float:
    return ROT_ABS if slot == 8 else REL[slot] * max(1.0, abs(want))


def score_image(det, gt, points, label=0, score_threshold=0.05, max_detections=10, iou_threshold=0.5, max_points=1000):
    """det: one image's filter rows (boxes [R,4], scores [R], labels [R], rotation [R,3], translation [R,3], hand [R,63], padding
    -1); gt: its table row [88].  Returns (record [16] float64, out_scores [max_detections] float32, out_tp [max_detections] int32)."""
    gt = np.asarray(gt, np.float64)
    boxes = det["boxes"].astype(np.float32) / np.float32(gt[18])                 # evaluate.py post_filter
    scores = det["scores"].astype(np.float32)
    rots = det["rotation"].astype(np.float32) * np.float32(math.pi)
    ind = np.nonzero(scores > score_threshold)[0]
    sel = ind[np.argsort(-scores[ind], kind="stable")[:max_detections]]
    sel = sel[det["labels"][sel] == label]                                      # the label cut comes after the cap
    rec = np.zeros(REC, np.float64)
    rec[2], rec[3:12] = -1.0, NAN
    out_s, out_tp = np.full(max_detections, -1.0, np.float32), np.full(max_detections, -1, np.int32)
    rec[0] = len(sel)
    m = -1
    for j, r in enumerate(sel):
        ov = float(E.compute_overlap(boxes[r:r + 1], gt[None, 1:5])[0, 0]) if gt[0] else 0.0
        hit = bool(gt[0]) and m < 0 and ov >= iou_threshold
        out_s[j], out_tp[j] = scores[r], int(hit)
        if hit:
            m = int(r)
            rec[1], rec[2], rec[3], rec[4] = 1.0, r, float(scores[r]), ov
    if m >= 0:
        rg, tg = gt[5:8], gt[8:11]
        rp, tp = rots[m].astype(np.float64), det["translation"][m].astype(np.float64)
        pts = np.asarray(points, np.float64)
        # ADD / ADD-S: the ground truth rounded to float32, as evaluate.pose_errors feeds the kernel
        Rg32, tg32, Rp32 = D.rodrigues(rg.astype(np.float32)), tg.astype(np.float32).astype(np.float64), D.rodrigues(rp)
        rec[5] = D.add_metric(pts, DIAMETER, Rg32, tg32, Rp32, tp)[1]
        rec[6] = D.add_s_metric(pts, DIAMETER, Rg32, tg32, Rp32, tp, max_points=max_points)[1]
        Rg, Rp = E.axis_angle_to_matrix(rg), E.axis_angle_to_matrix(rp)
        rec[7] = float(np.linalg.norm(tg - tp))
        rec[8] = E.calc_rotation_diff(Rg, Rp)
        rec[9] = float(np.linalg.norm((Rg @ gt[11:14] + tg) - (Rp @ gt[11:14] + tp)))
        K = np.array([[gt[14], 0, gt[16]], [0, gt[15], gt[17]], [0, 0, 1.0]])
        rec[10] = E.reprojection_distance(points, Rg, tg, Rp, tp, K)
        if gt[19]:
            rec[11] = float(np.linalg.norm(gt[20:83].reshape(21, 3) - det["hand"][m].astype(np.float64).reshape(21, 3), axis=-1).mean() * 1000.0)
    return rec, out_s, out_tp


def score_batch(rows, gt, points, **kw):
    """score_image over a batch (rows: dict of [B, ...] arrays): records [B,16], out_scores [B,M], out_tp [B,M]."""
    out = [score_image({k: v[b] for k, v in rows.items()}, gt[b], points, **kw) for b in range(gt.shape[0])]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def oracle_result(rec, out_s, out_tp, diameter=DIAMETER, diameter_threshold=0.1, symmetric=False):
    """The metric dictionary of one pass over the records: the tail of ``evaluate`` (evaluate.py) restated, plus the keys
    train.py reports (eval/common.py:1075-1119)."""
    n = float(rec.shape[0])
    scores, tp = [], []
    for b in range(rec.shape[0]):
        c = int(rec[b, 0])
        scores += [float(v) for v in out_s[b, :c]]
        tp += [float(v) for v in out_tp[b, :c]]
    tp = np.asarray(tp, np.float64)
    order = np.argsort(-np.asarray(scores), kind="stable") if scores else np.zeros(0, np.int64)
    tpc, fpc = np.cumsum(tp[order]), np.cumsum(1.0 - tp[order])
    out = {"num_annotations": n, "AP": E.compute_ap(tpc / n, tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps))}
    r = rec[rec[:, 1] == 1.0]
    out["num_matched"] = float(len(r))
    thr = diameter * diameter_threshold
    if len(r):
        hand = r[:, 11][~np.isnan(r[:, 11])]
        out.update({"ADD": np.sum(r[:, 5] <= thr) / n, "ADD-S": np.sum(r[:, 6] <= thr) / n, "5cm_5deg": np.sum((r[:, 7] <= 50) & (r[:, 8] <= 5)) / n,
                    "2D_projection": np.sum(r[:, 10] <= 5.0) / n, "2D_projection_distance_mean": r[:, 10].mean(),
                    "translation_mean": r[:, 7].mean(), "translation_std": r[:, 7].std(), "rotation_mean": r[:, 8].mean(),
                    "rotation_std": r[:, 8].std(), "translation_tip_mean": r[:, 9].mean(), "translation_tip_std": r[:, 9].std(),
                    "ADD_distance_mean": r[:, 5].mean(), "ADD_distance_std": r[:, 5].std(),
                    "ADD-S_distance_mean": r[:, 6].mean(), "ADD-S_distance_std": r[:, 6].std()})
        if len(hand):
            out.update({"hand_mean": hand.mean(), "hand_std": hand.std()})
        mixed = "ADD-S" if symmetric else "ADD"
        out.update({"ADD(-S)": out[mixed], "mixed_distance_mean": out[mixed + "_distance_mean"], "mixed_distance_std": out[mixed + "_distance_std"]})
    return {k: float(v) for k, v in out.items()}


EXACT_KEYS = ("num_annotations", "num_matched", "AP", "ADD", "ADD-S", "ADD(-S)", "5cm_5deg", "2D_projection")
KEY_SLOT = {"2D_projection_distance_mean": 10, "translation_mean": 7, "translation_std": 7, "rotation_mean": 8, "rotation_std": 8,
            "translation_tip_mean": 9, "translation_tip_std": 9, "ADD_distance_mean": 5, "ADD_distance_std": 5, "ADD-S_distance_mean": 6,
            "ADD-S_distance_std": 6, "hand_mean": 11, "hand_std": 11, "mixed_distance_mean": 5, "mixed_distance_std": 5}


def assert_results_close(got, want, symmetric=False):
    """Counts, fractions and AP equal; means and standard deviations within the tolerance of their record slot."""
    assert set(want) <= set(got), sorted(set(want) - set(got))
    for k, w in want.items():
        if k in EXACT_KEYS:
            assert got[k] == w, (k, got[k], w)
        else:
            slot = 6 if (k.startswith("mixed") and symmetric) else KEY_SLOT[k]
            assert abs(got[k] - w) <= tolerance(slot, w), (k, got[k], w)


def margins_ok(rec, diameter=DIAMETER, diameter_threshold=0.1):
    """Every thresholded quantity of the matched records keeps at least ten times its tolerance from its threshold (0.1 diameter
    for ADD and ADD-S, 50 for the translation, 5 degrees, 5 pixels): a flipped count is then a failure, never noise."""
    ok = True
    for r in rec[rec[:, 1] == 1.0]:
        for slot, thr in ((5, diameter * diameter_threshold), (6, diameter * diameter_threshold), (7, 50.0), (8, 5.0), (10, 5.0)):
            ok = ok and abs(r[slot] - thr) >= 10.0 * tolerance(slot, r[slot])
    return bool(ok)


# ------------------------------------------------------------------------------------------------------------------
# synthetic rows
# ------------------------------------------------------------------------------------------------------------------
ROWS = 12
SPECIAL = ("nothing above the threshold", "first candidate of another label; scale 0.5", "first candidate misses, second matches; zero rotation",
           "IoU exactly 0.5; identical poses", "the only overlap lies beyond the cap", "no hand ground truth")


def _empty_rows(rows):
    return dict(boxes=np.full((rows, 4), -1, np.float32), scores=np.full(rows, -1, np.float32), labels=np.full(rows, -1, np.int32),
                rotation=np.full((rows, 3), -1, np.float32), translation=np.full((rows, 3), -1, np.float32), hand=np.full((rows, 63), -1, np.float32))


def _image(rng, rows, ncand, overlap, labels=None, scale=1.0, hand=True, threshold=0.05):
    """One image: ncand candidates in descending score order; candidate j overlaps the ground-truth box (IoU > 0.7) where
    overlap[j], else lies apart from it (IoU 0); predicted poses are the ground truth plus noise."""
    det, gt = _empty_rows(rows), np.zeros(GT, np.float64)
    x0, y0 = rng.uniform(20, 100, 2)
    w, h = rng.uniform(40, 100, 2)
    box = np.array([x0, y0, x0 + w, y0 + h], np.float32)
    rot = rng.standard_normal(3)
    rot *= rng.uniform(0.3, 2.8) / np.linalg.norm(rot)
    t = np.array([rng.normal(0, 40), rng.normal(0, 40), 500 + rng.normal(0, 50)])
    gt[0], gt[1:5], gt[5:8], gt[8:11], gt[11:14] = 1.0, box, rot, t, (10.0, -20.0, 30.0)
    gt[14:18], gt[18] = (480.0, 470.0, 128.0, 120.0), scale
    if hand:
        gt[19], gt[20:83] = 1.0, rng.standard_normal(63) * 0.05
    det["scores"][:ncand] = np.sort(rng.uniform(threshold + 0.01, 0.99, ncand).astype(np.float32))[::-1]
    det["labels"][:ncand] = 0 if labels is None else labels
    for j in range(ncand):
        wide = rng.random() < 0.3                                                             # some poses miss 5 degrees / 5 cm / 5 px
        shift = rng.uniform(-2, 2, 4) if overlap[j] else np.array([300.0, 300.0, 300.0, 300.0]) + rng.uniform(0, 40)
        det["boxes"][j] = ((box.astype(np.float64) + shift) * scale).astype(np.float32)        # the network's boxes live in the scaled image
        det["rotation"][j] = ((rot + rng.standard_normal(3) * (0.12 if wide else 0.02)) / math.pi).astype(np.float32)
        det["translation"][j] = (t + rng.standard_normal(3) * np.array([1.0, 1.0, 8.0]) * (8.0 if wide else 1.0)).astype(np.float32)
        det["hand"][j] = (gt[20:83] + rng.standard_normal(63) * 0.004).astype(np.float32)
    return det, gt


def synthetic(seed=0, extra=0, rows=ROWS, num_points=37):
    """The six images of SPECIAL, in that order, then ``extra`` random ones.  Returns (rows dict of [B, ...] arrays, gt [B,88],
    points [num_points,3])."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x5c07e]))
    points = (rng.standard_normal((num_points, 3)) * np.array([40.0, 25.0, 60.0])).astype(np.float32)
    imgs = []
    d, g = _image(rng, rows, 3, [True] * 3)                                   # 0: scores at or below the threshold, and padding
    d["scores"][:3] = (0.05, 0.04, 0.01)
    imgs.append((d, g))
    imgs.append(_image(rng, rows, 3, [True, True, False], labels=np.array([1, 0, 0], np.int32), scale=0.5))          # 1
    d, g = _image(rng, rows, 4, [False, True, True, False])                   # 2: ground-truth rotation zero (the identity branch)
    g[5:8] = 0.0
    imgs.append((d, g))
    d, g = _image(rng, rows, 2, [True, False])                                # 3: integer boxes at scale 1, IoU = 50 / 100; identical poses
    g[1:5], d["boxes"][0] = (0, 0, 9, 9), (0, 0, 9, 4)
    g[5:8] = (d["rotation"][0] * np.float32(math.pi)).astype(np.float64)
    g[8:11] = d["translation"][0].astype(np.float64)
    imgs.append((d, g))
    imgs.append(_image(rng, rows, rows, [j == 10 for j in range(rows)]))        # 4: 12 candidates, the overlapping one is the 11th
    imgs.append(_image(rng, rows, 5, [False, False, True, True, False], labels=np.array([0, 1, 0, 0, 1], np.int32), hand=False))      # 5
    for _ in range(extra):
        n = int(rng.integers(0, rows + 1))
        imgs.append(_image(rng, rows, n, list(rng.random(n) < 0.4), labels=(rng.random(n) < 0.2).astype(np.int32),
                           scale=float(rng.choice([1.0, 0.5, 0.8])), hand=bool(rng.random() < 0.7)))
    det = {k: np.stack([d[k] for d, _ in imgs]) for k in imgs[0][0]}
    return det, np.stack([g for _, g in imgs]), points
