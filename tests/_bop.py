"""hep_bop_point_errors_device and hep_bop_vsd_device stated in numpy float64, vertex by vertex and pixel by pixel: THE definition of this
project's MSSD, MSPD and VSD - the kernels (csrc/k_bop.hip) reproduce it, include/hep.h states the same in words.  It is BOP's mssd, mspd
and vsd (bop19 visibility, step cost) restated with this project's own roundings; parity with bop_toolkit itself is unpinned.  The depth
maps come from tests/_render.py, not from a second rasteriser.  Shared by tests/test_bop_cpu.py and tests/test_gpu_bop.py.

Every rounding, in order:
  symmetry     R' = R_gt R_s, t' = R_gt t_s + t_gt, each element ((a0 b0 + a1 b1) + a2 b2) [+ t].
  points       p = ((R0 v0 + R1 v1) + R2 v2) + t under the estimate, q alike under (R', t'), v the float32 vertex widened.
  MSSD         mssd2(s) = max_v ((dx dx + dy dy) + dz dz); MSSD = sqrt(min_s mssd2(s)).  A NaN squared distance: MSSD is NaN.
  MSPD         u = (fx X) / Z + cx, v = (fy Y) / Z + cy; mspd2(s) = max_v (du du + dv dv); MSPD = sqrt(min_s mspd2(s)).  NaN when any vertex
               has not Z > 0 under the estimate or any (R', t'), or a squared pixel distance is NaN.
  VSD          see ``vsd_pixels``."""
import math

import numpy as np

from tests import _render as R

PAIR = 32
NAN = float("nan")


def pair_row(label, R_gt, t_gt, R_est, t_est, cam, image=0, valid=1.0):
    row = np.zeros(PAIR)
    row[0], row[1], row[2] = valid, label, image
    row[4:13], row[13:16] = np.asarray(R_gt, np.float64).reshape(9), t_gt
    row[16:25], row[25:28] = np.asarray(R_est, np.float64).reshape(9), t_est
    row[28:32] = cam[:4]
    return row


def row_label(row, num_labels):
    """The label of a pair row, or None when the row is skipped."""
    valid, lab = float(row[0]), float(row[1])
    if not valid != 0.0 or not (lab >= 0.0 and lab < num_labels) or np.isnan(row[4:28]).any():
        return None
    return int(lab)


def compose(row, sym):
    """(R' [9], t' [3]) of a pair row's ground truth with one symmetry [12]."""
    G, tg, S = row[4:13], row[13:16], np.asarray(sym, np.float64)
    Rp, tp = np.zeros(9), np.zeros(3)
    for r in range(3):
        for c in range(3):
            Rp[3 * r + c] = (G[3 * r] * S[c] + G[3 * r + 1] * S[3 + c]) + G[3 * r + 2] * S[6 + c]
        tp[r] = ((G[3 * r] * S[9] + G[3 * r + 1] * S[10]) + G[3 * r + 2] * S[11]) + tg[r]
    return Rp, tp


def transform(Rm, t, v):
    return [((Rm[3 * r] * v[0] + Rm[3 * r + 1] * v[1]) + Rm[3 * r + 2] * v[2]) + t[r] for r in range(3)]


def squared_errors(row, sym, vertices):
    """(mssd2, mspd2, flags) of one pair and one symmetry: flags bit 0 a NaN squared distance, bit 1 a vertex with not Z > 0 or a NaN
    squared pixel distance.  Elementwise over the vertices: the statements of ``squared_errors_loop``, which takes them one by one."""
    Rp, tp = compose(row, sym)
    fx, fy, cx, cy = row[28:32]
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    c = (v[:, 0], v[:, 1], v[:, 2])
    with np.errstate(all="ignore"):
        p, q = transform(row[16:25], row[25:28], c), transform(Rp, tp, c)
        dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        front = (p[2] > 0.0) & (q[2] > 0.0)
        du = ((fx * p[0]) / p[2] + cx) - ((fx * q[0]) / q[2] + cx)
        dv = ((fy * p[1]) / p[2] + cy) - ((fy * q[1]) / q[2] + cy)
        e2 = (du * du + dv * dv)[front]
    bad = (1 if np.isnan(d2).any() else 0) | (2 if (not front.all()) or np.isnan(e2).any() else 0)
    return float(np.max(d2[~np.isnan(d2)], initial=0.0)), float(np.max(e2[~np.isnan(e2)], initial=0.0)), bad


def squared_errors_loop(row, sym, vertices):
    """``squared_errors`` vertex by vertex, in Python floats."""
    Rp, tp = compose(row, sym)
    fx, fy, cx, cy = (float(c) for c in row[28:32])
    ms, mp, bad = 0.0, 0.0, 0
    with np.errstate(all="ignore"):
        for vert in np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3):
            p, q = transform(row[16:25], row[25:28], vert), transform(Rp, tp, vert)
            dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 != d2:
                bad |= 1
            elif d2 > ms:
                ms = d2
            if not p[2] > 0.0 or not q[2] > 0.0:
                bad |= 2
                continue
            du = ((fx * p[0]) / p[2] + cx) - ((fx * q[0]) / q[2] + cx)
            dv = ((fy * p[1]) / p[2] + cy) - ((fy * q[1]) / q[2] + cy)
            e2 = du * du + dv * dv
            if e2 != e2:
                bad |= 2
            elif e2 > mp:
                mp = e2
    return float(ms), float(mp), bad


def point_errors(pairs, vertices, vertex_start, symmetries, sym_start):
    """float64 [n,2] MSSD, MSPD of the pair table [n,32]; NaN rows where skipped."""
    pairs = np.asarray(pairs, np.float64)
    out = np.full((len(pairs), 2), NAN)
    for i, row in enumerate(pairs):
        lab = row_label(row, len(vertex_start) - 1)
        if lab is None:
            continue
        verts = vertices[vertex_start[lab]:vertex_start[lab + 1]]
        best_s, best_p, bad = math.inf, math.inf, 0
        for s in range(sym_start[lab], sym_start[lab + 1]):
            ms, mp, b = squared_errors(row, symmetries[s], verts)
            best_s, best_p, bad = min(best_s, ms), min(best_p, mp), bad | b
        out[i, 0] = NAN if bad & 1 else math.sqrt(best_s)
        out[i, 1] = NAN if bad & 2 else math.sqrt(best_p)
    return out


def far(k2, zm, zr, d):
    """Is the surface at depth ``zm`` farther than ``d`` BEHIND the one at ``zr``, by distance from the camera: sqrt-free.  False when
    zm - zr <= 0, else k2 ((zm - zr)(zm - zr)) > d d.  Scalars or arrays."""
    diff = zm - zr
    with np.errstate(all="ignore"):
        return np.logical_and(diff > 0.0, k2 * (diff * diff) > d * d)


def vsd_pixels(row, zg, ze, zt, delta, taus):
    """int counts [2 + T] (union, intersection, cost per tau) of one pair's depth triple ([H,W] each, ``zt`` None: no test image).
    Elementwise over the pixels, float64:  a = (x - cx) / fx, b = (y - cy) / fy, k2 = (a a + b b) + 1;  visible(zm) = zm > 0 and (zt == 0
    or not far(zm, zt, delta));  vis_gt = visible(zg);  vis_est = visible(ze) or (vis_gt and ze > 0);  cost at tau:
    k2 ((zg - ze)(zg - ze)) >= tau tau.  ``vsd_pixels_loop`` takes the pixels one by one."""
    fx, fy, cx, cy = (np.float64(c) for c in row[28:32])
    H, W = zg.shape
    g, e = np.asarray(zg, np.float32).astype(np.float64), np.asarray(ze, np.float32).astype(np.float64)
    t = np.zeros((H, W)) if zt is None else np.asarray(zt, np.float32).astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    delta = np.float64(delta)
    with np.errstate(all="ignore"):
        a, b = (xs - cx) / fx, (ys - cy) / fy
        k2 = (a * a + b * b) + 1.0
        vis_gt = (g > 0.0) & ((t == 0.0) | ~far(k2, g, t, delta))
        vis_est = ((e > 0.0) & ((t == 0.0) | ~far(k2, e, t, delta))) | (vis_gt & (e > 0.0))
        inter = vis_gt & vis_est
        d = g - e
        c = k2 * (d * d)
        return [int((vis_gt | vis_est).sum()), int(inter.sum())] + [int((inter & (c >= np.float64(tau) * np.float64(tau))).sum()) for tau in taus]


def vsd_pixels_loop(row, zg, ze, zt, delta, taus):
    """``vsd_pixels`` pixel by pixel."""
    fx, fy, cx, cy = (np.float64(c) for c in row[28:32])
    H, W = zg.shape
    counts = [0] * (2 + len(taus))
    delta = np.float64(delta)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                g, e = np.float64(zg[y, x]), np.float64(ze[y, x])
                t = np.float64(0.0) if zt is None else np.float64(zt[y, x])
                a, b = (np.float64(x) - cx) / fx, (np.float64(y) - cy) / fy
                k2 = (a * a + b * b) + 1.0
                vis_gt = bool(g > 0.0) and (bool(t == 0.0) or not far(k2, g, t, delta))
                vis_est = (bool(e > 0.0) and (bool(t == 0.0) or not far(k2, e, t, delta))) or (vis_gt and bool(e > 0.0))
                counts[0] += int(vis_gt or vis_est)
                if vis_gt and vis_est:
                    counts[1] += 1
                    d = g - e
                    c = k2 * (d * d)
                    for j, tau in enumerate(taus):
                        counts[2 + j] += int(bool(c >= np.float64(tau) * np.float64(tau)))
    return counts


def vsd_from_counts(counts):
    un, inter = int(counts[0]), int(counts[1])
    return [1.0 if un == 0 else float(np.float64(int(c) + (un - inter)) / np.float64(un)) for c in counts[2:]]


def vsd(pairs, depth_gt, depth_est, depth_test, delta, taus, num_labels):
    """(vsd float64 [n,T], counts int32 [n,2+T]); a skipped row (``row_label``, and with a depth_test an image index outside it): NaN, -1."""
    pairs = np.asarray(pairs, np.float64)
    n, T = len(pairs), len(taus)
    out, counts = np.full((n, T), NAN), np.full((n, 2 + T), -1, np.int32)
    for i, row in enumerate(pairs):
        if row_label(row, num_labels) is None:
            continue
        zt = None
        if depth_test is not None:
            if not (row[2] >= 0.0 and row[2] < len(depth_test)):
                continue
            zt = depth_test[int(row[2])]
        counts[i] = vsd_pixels(row, depth_gt[i], depth_est[i], zt, delta, taus)
        out[i] = vsd_from_counts(counts[i])
    return out, counts


def render_depths(pairs, vertices, faces, face_start, H, W):
    """(depth_gt, depth_est) float32 [n,H,W] of a pair table through tests/_render.py: one pose per image, mask value 1."""
    pairs = np.asarray(pairs, np.float64)
    n = len(pairs)
    cam = np.concatenate([pairs[:, 28:32], np.ones((n, 1))], axis=1)
    out = []
    for o in (4, 16):
        poses = np.zeros((n, 1, 16))
        poses[:, 0, 0], poses[:, 0, 1], poses[:, 0, 2] = pairs[:, 0], pairs[:, 1], 1.0
        poses[:, 0, 4:16] = pairs[:, o:o + 12]
        out.append(R.render_models(poses, cam, vertices, faces, face_start, H, W)["depth"])
    return out[0], out[1]


# ---- the host tail: average recall ---------------------------------------------------------------------------------------------
FRACTIONS = np.arange(0.05, 0.51, 0.05)


def recall(errors, num_annotations, thresholds):
    """Mean over ``thresholds`` of (errors < threshold).sum() / num_annotations; a NaN error is a miss; NaN without annotations."""
    if num_annotations == 0:
        return NAN
    e = np.asarray(errors, np.float64).reshape(-1)
    return float(np.mean([np.count_nonzero(e < th) / num_annotations for th in thresholds]))


def average_recall(mssd, mspd, vsd_errors, num_annotations, diameter, width):
    """dict(AR_VSD, AR_MSSD, AR_MSPD, AR) of one label: ``mssd``, ``mspd`` [m] and ``vsd_errors`` [m,T] (one column per tau) of its
    matched annotations, ``num_annotations`` its valid ones."""
    if num_annotations == 0:
        return dict(AR_VSD=NAN, AR_MSSD=NAN, AR_MSPD=NAN, AR=NAN)
    v = np.asarray(vsd_errors, np.float64)
    assert v.ndim == 2
    ar_vsd = float(np.mean([np.count_nonzero(v[:, j] < th) / num_annotations for j in range(v.shape[1]) for th in FRACTIONS]))
    ar_mssd = recall(mssd, num_annotations, FRACTIONS * diameter)
    ar_mspd = recall(mspd, num_annotations, np.arange(5, 51, 5) * (width / 640.0))
    return dict(AR_VSD=ar_vsd, AR_MSSD=ar_mssd, AR_MSPD=ar_mspd, AR=(ar_vsd + ar_mssd + ar_mspd) / 3.0)
