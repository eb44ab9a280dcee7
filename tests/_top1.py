"""The top-detection rule of hep_top1_device stated in numpy, and the helpers its CPU and GPU tests share.

Row 0 of filter_detections (hmdegopose/layers.py:264-400) needs no sort and no NMS: the best-scoring candidate is first in every
sorted order and nothing can suppress it.
  class-specific mode: the maximal score over all (anchor, class) pairs with score > threshold, ties to the lower class, then to
                       the lower anchor index;
  other mode:          per anchor the maximum over the class columns (label = first argmax), then the maximal such score above
                       the threshold, ties to the lower anchor index.
A score exactly at the threshold is no candidate."""
import numpy as np

RECORD_WORDS = 80


def top1_rule(classification, score_threshold, class_specific_filter=True):
    """classification [N, K] float32 -> (found, label, anchor index, score); (0, -1, -1, -1.0) without a candidate."""
    cls = np.asarray(classification, np.float32)
    cls = cls.reshape(cls.shape[0], -1)
    thr = np.float32(score_threshold)
    if class_specific_filter:
        s = cls.T.reshape(-1)                       # position = class * N + anchor: the first maximum is the lower class, then the lower anchor
        s = np.where(s > thr, s, -np.inf)
        p = int(np.argmax(s))
        if not np.isfinite(s[p]):
            return 0, -1, -1, np.float32(-1)
        label, n = divmod(p, cls.shape[0])
    else:
        labels = cls.argmax(axis=1)                 # first argmax
        s = np.where(cls.max(axis=1) > thr, cls.max(axis=1), -np.inf)
        n = int(np.argmax(s))
        if not np.isfinite(s[n]):
            return 0, -1, -1, np.float32(-1)
        label = int(labels[n])
    return 1, int(label), int(n), cls[n, label]


def random_scores(rng, N, K, ncand, thr, ties):
    """[N, K] scores with ncand candidate anchors above thr, a few scores exactly AT thr (no candidates), and - ties - the maximal
    score shared by several anchors and, with K > 1, by several classes of one anchor and of different anchors."""
    thr = np.float32(thr)
    cls = rng.uniform(0, thr * 0.99, (N, K)).astype(np.float32)
    at = rng.choice(N, min(N, 5), replace=False)
    cls[at, rng.integers(0, K, len(at))] = thr                                  # exactly at the threshold
    idx = rng.choice(N, min(ncand, N), replace=False)
    if len(idx):
        above = np.nextafter(thr, np.float32(2))
        sc = np.maximum((rng.integers(1, 64, (len(idx), K)) / 64.0).astype(np.float32) * (1 - thr) + thr, above)   # 63 levels: ties everywhere
        keep = rng.random((len(idx), K)) < 0.6
        keep[np.arange(len(idx)), rng.integers(0, K, len(idx))] = True           # every chosen anchor has a candidate class
        cls[idx] = np.where(keep, sc, cls[idx])
        if ties and len(idx) >= 2:
            top = np.float32(cls.max())
            share = rng.choice(idx, min(len(idx), 3), replace=False)
            cls[share, rng.integers(0, K, len(share))] = top                      # equal maxima across anchors (and classes)
            if K > 1:
                cls[share[0], :2] = top                                           # ... and across classes of one anchor
    return cls


def record_of_row0(count, boxes, scores, labels, rotation, translation, hand, index):
    """The 80-word record (int32 bit patterns) that row 0 of one image's filter output amounts to."""
    rec = np.zeros(RECORD_WORDS, np.int32)
    f = rec.view(np.float32)
    rec[0] = 1 if count > 0 else 0
    rec[1], rec[2] = int(labels[0]), int(index[0])
    f[4] = scores[0]
    f[5:9], f[9:12], f[12:15], f[15:78] = boxes[0], rotation[0], translation[0], hand[0]
    return rec
