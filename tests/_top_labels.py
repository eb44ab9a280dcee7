"""The per-label top-detection rule of hep_top_labels_device stated in numpy, and the helpers its CPU and GPU tests share.

In class-specific mode filter_detections (hmdegopose/layers.py:347-358) thresholds and suppresses every class on its own, so the
best candidate of a class is first in that class's order and nothing can suppress it: per class c, the maximal
classification[n, c] over the anchors n with a score > threshold, ties to the lower anchor index.  A score exactly at the
threshold is no candidate.  As a definition: record c is row 0 of the filter on the classification with every column but c set
to -1.0 (``masked``)."""
import numpy as np

from tests._top1 import RECORD_WORDS, record_of_row0

MASKED = np.float32(-1.0)


def top_labels_rule(classification, score_threshold):
    """classification [N, K] float32 -> (found [K] int32, anchor index [K] int32, score [K] float32); (0, -1, -1.0) for a label
    without a candidate."""
    cls = np.asarray(classification, np.float32)
    cls = cls.reshape(cls.shape[0], -1)
    K = cls.shape[1]
    s = np.where(cls > np.float32(score_threshold), cls, -np.inf)
    n = s.argmax(axis=0)                                 # the first maximum of a column: the lower anchor index
    found = np.isfinite(s[n, np.arange(K)])
    return (found.astype(np.int32), np.where(found, n, -1).astype(np.int32),
            np.where(found, cls[n, np.arange(K)], np.float32(-1)).astype(np.float32))


def masked(classification, c):
    """the classification with every column but c set to -1.0: class c alone in front of the filter"""
    out = np.full_like(classification, MASKED)
    out[..., c] = classification[..., c]
    return out


def rule_records(classification, score_threshold, boxes, rotation, translation, hand):
    """[K, 80] int32 records of one image from the rule and the decoded per-anchor arrays (boxes [N,4], translation [N,3])."""
    found, idx, score = top_labels_rule(classification, score_threshold)
    recs = np.zeros((len(found), RECORD_WORDS), np.int32)
    for c in range(len(found)):
        if found[c]:
            n = idx[c]
            recs[c] = record_of_row0(1, boxes[n:n + 1], score[c:c + 1], [c], rotation[n:n + 1], translation[n:n + 1], hand[n:n + 1], [n])
        else:
            recs[c] = padding_record()
    return recs


def padding_record():
    """the record of a label without a candidate: found 0, the filter's -1 / -1.0f everywhere else, words 3, 78, 79 zero"""
    rec = np.zeros(RECORD_WORDS, np.int32)
    rec[1] = rec[2] = -1
    rec.view(np.float32)[4:78] = -1
    return rec


def best_over_labels(recs):
    """[K, 80] records -> the record with the largest score, ties to the lower class (the top-1 record in class-specific mode)"""
    found = recs[:, 0] == 1
    if not found.any():
        return padding_record()
    score = np.where(found, recs[:, 4].view(np.float32), -np.inf)
    return recs[int(np.argmax(score))]
