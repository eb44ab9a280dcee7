"""CPU (no GPU): the per-label entry points exist and refuse a NULL handle before any HIP call, and the rule they implement
(tests/_top_labels.py) against the oracle's filter_detections in class-specific mode:
  (a) the definition - record c is row 0 of the filter on the classification with every column but c masked out, for any
      max_detections and NMS threshold;
  (b) without a cut - an image with at most 256 candidate pairs, max_detections = 256 - record c is the first row with
      det_labels == c of the UNMASKED filter, and not found when there is none;
  (c) the best record over the labels, ties to the lower class, is the top-1 rule of tests/_top1.py."""
import numpy as np
import pytest

from hmd_ego_pose_amd import _capi
from oracle import decode_ref as D
from tests._top1 import random_scores, top1_rule
from tests._top_labels import masked, top_labels_rule

N = 3069


def test_top_labels_entry_points_exist_and_refuse_a_null_handle():
    l = _capi.lib()
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data
    names = ("hep_top_labels_device", "hep_poses_from_i420", "hep_poses_from_input")
    for name in names:
        assert name in _capi.SYMBOLS and hasattr(l, name), name
    calls = {
        "hep_top_labels_device": lambda: l.hep_top_labels_device(None, None, None, None, None, None, a, 1, 0.5, a, None),
        "hep_poses_from_i420": lambda: l.hep_poses_from_i420(None, a, 1, 480, 640, 256, 512, a, 0.5, a, *([None] * 6)),
        "hep_poses_from_input": lambda: l.hep_poses_from_input(None, a, 1, a, 0.5, a, *([None] * 6)),
    }
    for name in names:
        assert l.hep_anchors(100, None, None) < 0                   # another message in between: the text below is never a stale one
        assert calls[name]() == -1, name                            # HEP_ERR_INVALID
        msg = l.hep_last_error()
        assert name.encode() in msg and b"handle is NULL" in msg, (name, msg)
    assert l.hep_abi_version() == 1                                 # additive: the ABI version stays


@pytest.fixture(scope="module")
def anchors_data():
    """per-anchor arrays shared by every case (never modified): spread boxes, so that NMS both keeps and suppresses"""
    rng = np.random.Generator(np.random.PCG64(2900))
    cxy = rng.uniform(10, 118, (N, 2)); wh = rng.uniform(6, 60, (N, 2))
    boxes = np.concatenate([cxy - wh / 2, cxy + wh / 2], axis=1).astype(np.float32)
    rot, tr = (rng.standard_normal((N, 3)).astype(np.float32) for _ in range(2))
    hand = rng.standard_normal((N, 63)).astype(np.float32)
    return boxes, rot, tr, hand


def rows_equal(o, row, found, c, n, score, data):
    """row `row` of the oracle's output o (None: no such row) is the rule's (found, c, n, score)"""
    if row is None or o[6][row] < 0:
        return found == 0 and n == -1 and score == np.float32(-1)
    boxes, rot, tr, hand = data
    return (found == 1 and n == int(o[6][row]) and c == int(o[2][row]) and score == o[1][row] and np.array_equal(boxes[n], o[0][row])
            and np.array_equal(rot[n], o[3][row]) and np.array_equal(tr[n], o[4][row]) and np.array_equal(hand[n], o[5][row]))


@pytest.mark.parametrize("K", [1, 3, 5])
def test_top_labels_rule_against_the_oracle_filter(K, anchors_data):
    boxes, rot, tr, hand = anchors_data
    rng = np.random.Generator(np.random.PCG64(290 + K))
    comparisons = mismatches = 0
    some_found_some_not = False
    for ncand in (0, 1, 2, 7, 50):
        for thr in (0.05, 0.5):
            for rep in range(3):
                cls = random_scores(rng, N, K, ncand, thr, ties=rep != 1)
                found, idx, score = top_labels_rule(cls, thr)
                pairs = int((cls > np.float32(thr)).sum())
                assert pairs <= 256, (K, ncand, pairs)              # the condition of (b): stated, not skipped
                some_found_some_not |= bool(found.any() and not found.all())
                # (a) the masked definition
                M = int(rng.choice([1, 10, 100, 256])); nms = float(rng.choice([0.0, 0.3, 0.5, 0.9]))
                ok = True
                for c in range(K):
                    o = D.filter_detections(boxes, masked(cls, c), rot, tr, hand, thr, M, nms, class_specific_filter=True)
                    ok = ok and rows_equal(o, 0, found[c], c, idx[c], score[c], anchors_data)
                comparisons += 1; mismatches += not ok
                # (b) no cut: the first row of label c of the unmasked filter
                o = D.filter_detections(boxes, cls, rot, tr, hand, thr, 256, nms, class_specific_filter=True)
                ok = True
                for c in range(K):
                    rows = np.nonzero(o[2] == c)[0]
                    ok = ok and rows_equal(o, int(rows[0]) if len(rows) else None, found[c], c, idx[c], score[c], anchors_data)
                comparisons += 1; mismatches += not ok
                # (c) the best over the labels is the top-1 rule
                best = (0, -1, -1, np.float32(-1))
                if found.any():
                    c = int(np.argmax(np.where(found == 1, score, -np.inf)))      # first maximum: ties to the lower class
                    best = (1, c, int(idx[c]), score[c])
                want = top1_rule(cls, thr, True)
                comparisons += 1; mismatches += not (best[:3] == want[:3] and best[3] == want[3])
                if ncand == 0:
                    assert not found.any() and (cls == np.float32(thr)).any()     # scores AT the threshold are no candidates
    assert comparisons == 90 and mismatches == 0, (mismatches, comparisons)
    assert K == 1 or some_found_some_not
