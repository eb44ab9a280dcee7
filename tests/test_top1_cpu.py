"""CPU (no GPU): the frame-to-pose entry points exist and refuse a NULL handle before any HIP call, and the top-detection rule
they implement (tests/_top1.py) is row 0 of the oracle's filter_detections."""
import ctypes

import numpy as np
import pytest

from hmd_ego_pose_amd import _capi
from oracle import decode_ref as D
from tests._top1 import random_scores, top1_rule


def test_pose_entry_points_exist_and_refuse_a_null_handle():
    l = _capi.lib()
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data
    for name in ("hep_top1_device", "hep_pose_from_i420", "hep_pose_from_input"):
        assert name in _capi.SYMBOLS and hasattr(l, name), name
    calls = {
        "hep_top1_device": lambda: l.hep_top1_device(None, None, None, None, None, None, a, 1, 0.5, a, None),
        "hep_pose_from_i420": lambda: l.hep_pose_from_i420(None, a, 1, 480, 640, 256, 512, a, 0.5, a, *([None] * 7)),
        "hep_pose_from_input": lambda: l.hep_pose_from_input(None, a, 1, a, 0.5, a, *([None] * 7)),
    }
    for name, call in calls.items():
        assert l.hep_anchors(100, None, None) < 0                   # another message in between: the text below is never a stale one
        assert call() == -1, name                                   # HEP_ERR_INVALID
        msg = l.hep_last_error()
        assert name.encode() in msg and b"handle is NULL" in msg, (name, msg)
    assert l.hep_abi_version() == 1                                 # additive: the ABI version stays


@pytest.mark.parametrize("K", [1, 3, 5])
def test_top1_rule_is_row_0_of_the_oracle_filter(K):
    """Randomised: 0 to N candidates, ties across anchors and classes, scores exactly at the threshold, both filter modes, three
    max_detections values and four NMS thresholds - the rule needs none of the last two."""
    rng = np.random.Generator(np.random.PCG64(40 + K))
    N, mismatches, cases = 48, 0, 0
    for case in range(136):
        ncand = int(rng.choice([0, 1, 2, 7, 20, N]))
        thr = float(rng.choice([0.05, 0.5]))
        cls = random_scores(rng, N, K, ncand, thr, ties=case % 2 == 0)
        cxy = rng.uniform(10, 118, (N, 2)); wh = rng.uniform(6, 60, (N, 2))
        boxes = np.concatenate([cxy - wh / 2, cxy + wh / 2], axis=1).astype(np.float32)
        rot, tr = (rng.standard_normal((N, 3)).astype(np.float32) for _ in range(2))
        hand = rng.standard_normal((N, 63)).astype(np.float32)
        M = int(rng.choice([1, 10, 100])); nms = float(rng.choice([0.0, 0.3, 0.5, 0.9]))
        for mode in (True, False):
            found, label, n, score = top1_rule(cls, thr, mode)
            o = D.filter_detections(boxes, cls, rot, tr, hand, thr, M, nms, class_specific_filter=mode)
            cases += 1
            ok = (found == int(o[6][0] >= 0) and n == int(o[6][0]) and label == int(o[2][0]) and np.float32(score) == o[1][0])
            if found:
                ok = ok and np.array_equal(boxes[n], o[0][0]) and np.array_equal(hand[n], o[5][0])
            mismatches += not ok
        if ncand == 0:
            assert top1_rule(cls, thr, True)[0] == 0 and (cls == np.float32(thr)).any()      # scores AT the threshold are no candidates
    assert cases >= 270 and mismatches == 0, (mismatches, cases)
