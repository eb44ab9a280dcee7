"""hep_draw_poses_device stated in numpy (float64 projection, int64 coverage): THE definition of the pose overlays - the kernel
(csrc/k_draw.hip) reproduces it byte for byte.  include/hep.h states the same in words.  Shared by tests/test_draw_cpu.py and
tests/test_gpu_draw.py.

The drawing is the project's own: cv2's line / circle rasterisers are not restated (the reference draws with cv2.line and cv2.circle,
generators/utils/visualization.py:85-117, 234-290; cv2 is absent from the build image)."""
import math

import numpy as np

BOX2D, CUBOID, HAND = 1, 2, 4
SAT_LO, SAT_HI = -8192.0, 8191.0
# primitives of a shape over its 34 points (0-3 box corners, 4-11 cuboid corners, 12 centre, 13-33 joints), in drawing order
BOX_SEGMENTS = [(0, 1), (1, 2), (2, 3), (3, 0)]
CUBOID_EDGES = [(0, 1), (1, 2), (2, 3), (0, 3), (4, 5), (5, 6), (6, 7), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)]      # visualization.py:99-112
HAND_SEGMENTS = [(0 if k == 0 else 4 * f + k, 4 * f + k + 1) for f in range(5) for k in range(4)]
ANN_CUBOID, ANN_BOX, ANN_HAND, DET_BOX = (0, 255, 0), (0, 127, 0), (0, 178, 0), (255, 0, 255)


def rodrigues(rv):
    """rodrigues_f64 of csrc/eval_dev.h statement by statement; ``rv`` float32 or float64 [3].  Returns (R [9], angle)."""
    x, y, z = (float(v) for v in rv)
    th = math.sqrt((x * x + y * y) + z * z)
    if th < 1e-12:
        return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], th
    kx, ky, kz, c, s = x / th, y / th, z / th, math.cos(th), math.sin(th)
    v = 1.0 - c
    return [c + v * kx * kx, v * kx * ky - s * kz, v * kx * kz + s * ky,
            v * ky * kx + s * kz, c + v * ky * ky, v * ky * kz - s * kx,
            v * kz * kx - s * ky, v * kz * ky + s * kx, c + v * kz * kz], th


def sat_trunc(v):
    v = SAT_LO if v < SAT_LO else (SAT_HI if v > SAT_HI else v)
    return int(v)                                   # toward zero


def _div(a, b):
    """IEEE float64 a / b, b > 0 or NaN handled by the caller (no Python ZeroDivisionError: b > 0 here)."""
    return float(np.float64(a) / np.float64(b))


class Shape:
    """One annotation or kept detection: ``pts`` 34 integer points or None (invalid), the colours, whether it has joints, and - for
    the input condition of the bit-exact tests - ``raw`` (every projected float coordinate before saturation), ``depths`` (of the rotated
    cuboid corners: computed through sin / cos), ``given_depths`` (of the centre and the joints: inputs, used as they are) and ``angle``."""

    def __init__(self):
        self.pts, self.raw, self.depths, self.given_depths, self.angle = [None] * 34, [], [], [], None
        self.annotation, self.colour = True, ANN_CUBOID


def _put(shape, p, u, v, projected=True):
    if u != u or v != v:
        return
    if projected:                                   # the box corners are no projections: IEEE-exact on both sides, often integers
        shape.raw += [u, v]
    shape.pts[p] = (sat_trunc(u), sat_trunc(v))


def _project(shape, p, X, Y, Z, cam, given=True):
    (shape.given_depths if given else shape.depths).append(Z)
    if not Z > 0.0:
        return
    fx, fy, cx, cy = cam[:4]
    _put(shape, p, _div(fx * X, Z) + cx, _div(fy * Y, Z) + cy)


def _pose_points(shape, rv, t, cuboid, cam):
    R, shape.angle = rodrigues(rv)
    t = [float(v) for v in t]
    for k in range(8):
        c0, c1, c2 = (float(v) for v in cuboid[k])
        P = [((R[3 * r] * c0 + R[3 * r + 1] * c1) + R[3 * r + 2] * c2) + t[r] for r in range(3)]
        _project(shape, 4 + k, P[0], P[1], P[2], cam, given=False)
    _project(shape, 12, t[0], t[1], t[2], cam)


def image_shapes(cam, gt, det, cuboids, colours, score_threshold, max_detections):
    """The shapes of ONE image in drawing order.  ``cam``: 5 float64 (fx, fy, cx, cy, scale); ``gt`` [amax,88] float64 or None; ``det``:
    dict of boxes [rows,4], scores, labels, rotation, translation and optionally hand (float32 / int32), or None."""
    num_labels = len(cuboids)
    cam = [float(v) for v in cam]
    shapes = []
    if gt is not None:
        for g in np.asarray(gt, np.float64):
            lab = g[83]
            if g[0] == 0.0 or not (lab >= 0.0 and lab < num_labels):
                continue
            s = Shape()
            lab = int(lab)
            for p, (ix, iy) in enumerate(((0, 1), (2, 1), (2, 3), (0, 3))):
                _put(s, p, float(g[1 + ix]), float(g[1 + iy]), projected=False)
            _pose_points(s, g[5:8], g[8:11], cuboids[lab], cam)
            if g[19] != 0.0:
                for j in range(21):
                    _project(s, 13 + j, float(g[20 + 3 * j]), float(g[21 + 3 * j]), float(g[22 + 3 * j]), cam)
            shapes.append(s)
    if det is not None:
        scores = np.asarray(det["scores"], np.float32)
        kept = np.nonzero(scores > np.float32(score_threshold))[0][:max_detections]
        scale = np.float32(cam[4])
        for r in kept:
            lab = int(det["labels"][r])
            if not 0 <= lab < num_labels:
                continue
            s = Shape()
            s.annotation, s.colour = False, tuple(int(v) for v in colours[lab])
            box = np.asarray(det["boxes"][r], np.float32) / scale                     # float32
            for p, (ix, iy) in enumerate(((0, 1), (2, 1), (2, 3), (0, 3))):
                _put(s, p, float(box[ix]), float(box[iy]), projected=False)
            rv = np.asarray(det["rotation"][r], np.float32) * np.float32(math.pi)      # float32
            _pose_points(s, rv, np.asarray(det["translation"][r], np.float32), cuboids[lab], cam)
            if det.get("hand") is not None:
                h = np.asarray(det["hand"][r], np.float32)
                for j in range(21):
                    _project(s, 13 + j, float(h[3 * j]), float(h[3 * j + 1]), float(h[3 * j + 2]), cam)
            shapes.append(s)
    return shapes


def segment_mask(xs, ys, a, b, t):
    """Coverage of the pixels (xs, ys) (int64 arrays) by the segment a-b of thickness t: exact integers."""
    ax, ay, bx, by = (int(v) for v in (*a, *b))
    dx, dy = bx - ax, by - ay
    qx, qy = xs - ax, ys - ay
    L, s = dx * dx + dy * dy, qx * dx + qy * dy
    tt = t * t
    c = qx * dy - qy * dx
    rx, ry = xs - bx, ys - by
    return np.where(s <= 0, 4 * (qx * qx + qy * qy) <= tt, np.where(s >= L, 4 * (rx * rx + ry * ry) <= tt, 4 * (c * c) <= tt * L))


def disc_mask(xs, ys, c, r2=9):
    qx, qy = xs - int(c[0]), ys - int(c[1])
    return qx * qx + qy * qy <= r2


def primitives(shape, layers):
    """[(kind, a, b, colour)] of one shape in drawing order; kind 'seg' or 'disc'."""
    out = []
    ann = shape.annotation
    P = shape.pts
    if layers & BOX2D:
        out += [("seg", P[a], P[b], ANN_BOX if ann else DET_BOX) for a, b in BOX_SEGMENTS]
    if layers & CUBOID:
        out += [("seg", P[4 + a], P[4 + b], shape.colour) for a, b in CUBOID_EDGES]
        out.append(("disc", P[12], P[12], shape.colour))
    if layers & HAND:
        out += [("seg", P[13 + a], P[13 + b], ANN_HAND if ann else shape.colour) for a, b in HAND_SEGMENTS]
    return [q for q in out if q[1] is not None and q[2] is not None]


def paint(image, prims, thickness):
    """The primitives into ``image`` uint8 [H,W,3] in place, later over earlier."""
    H, W = image.shape[:2]
    for kind, a, b, colour in prims:
        pad = 3 if kind == "disc" else (thickness + 1) // 2
        xa, xb = max(min(a[0], b[0]) - pad, 0), min(max(a[0], b[0]) + pad, W - 1)
        ya, yb = max(min(a[1], b[1]) - pad, 0), min(max(a[1], b[1]) + pad, H - 1)
        if xa > xb or ya > yb:
            continue
        ys, xs = np.meshgrid(np.arange(ya, yb + 1, dtype=np.int64), np.arange(xa, xb + 1, dtype=np.int64), indexing="ij")
        m = disc_mask(xs, ys, a) if kind == "disc" else segment_mask(xs, ys, a, b, thickness)
        image[ya:yb + 1, xa:xb + 1][m] = np.array(colour, np.uint8)


def draw_poses(frames, cuboids, colours, gt=None, camera=None, det=None, score_threshold=0.5, max_detections=10, ann_layers=CUBOID,
               det_layers=CUBOID, thickness=2, shapes_out=None):
    """hep_draw_poses_device on host arrays: returns a drawn COPY of ``frames`` uint8 [B,H,W,3].  ``gt`` [B,amax,88] float64 or None,
    ``camera`` [B,5] float64 or None (then slots 14-18 of gt row 0), ``det``: dict of [B,rows,...] arrays or None, ``cuboids``
    float32 [L,8,3], ``colours`` uint8 [L,3].  ``shapes_out``: a list that receives every image's Shape list."""
    out = np.array(frames, dtype=np.uint8, copy=True)
    cuboids = np.asarray(cuboids, np.float32)
    for b in range(out.shape[0]):
        cam = camera[b] if camera is not None else gt[b, 0, 14:19]
        d = None if det is None else {k: (None if v is None else v[b]) for k, v in det.items()}
        shapes = image_shapes(cam, None if gt is None else gt[b], d, cuboids, colours, score_threshold, max_detections)
        if shapes_out is not None:
            shapes_out.append(shapes)
        prims = [q for s in shapes for q in primitives(s, ann_layers if s.annotation else det_layers)]
        paint(out[b], prims, thickness)
    return out


def input_margins(shapes_per_image):
    """The input condition of the bit-exact tests (the device's sin / cos may differ from libm's in the last bits), measured on the
    oracle alone: (smallest distance of a projected coordinate that is not saturated from an integer, smallest distance of any
    coordinate from a saturation bound, smallest |depth| of a rotated corner, smallest distance of a non-zero rotation angle from the
    1e-12 switch, smallest |depth| of a centre or joint).  An angle that is exactly 0 is exact on both sides (sqrt(0)) and is left out.
    The depth of a centre or a joint is an input that both sides use as it is, bit for bit: ``Z > 0`` decides alike whatever its size."""
    d_int, d_sat, d_z, d_th, d_given = math.inf, math.inf, math.inf, math.inf, math.inf
    for shapes in shapes_per_image:
        for s in shapes:
            for v in s.raw:
                d_sat = min(d_sat, abs(v - SAT_LO), abs(v - SAT_HI))
                if SAT_LO < v < SAT_HI:
                    d_int = min(d_int, abs(v - round(v)))
            for z in s.depths:
                d_z = min(d_z, abs(z))
            for z in s.given_depths:
                d_given = min(d_given, abs(z))
            if s.angle is not None and s.angle != 0.0:
                d_th = min(d_th, abs(s.angle - 1e-12))
    return d_int, d_sat, d_z, d_th, d_given


def assert_input_condition(shapes_per_image, given_depths=True):
    """``given_depths=False`` for poses a model produced (a seeded model's joints lie around depth 0): the depths that no sin / cos
    enters are then left out - they are the same bits on both sides; every seeded case of this file is checked with them."""
    d_int, d_sat, d_z, d_th, d_given = input_margins(shapes_per_image)
    assert d_int >= 1e-7 and d_sat >= 1e-7 and d_z >= 1e-3 and d_th >= 1e-9, (d_int, d_sat, d_z, d_th)
    assert not given_depths or d_given >= 1e-3, d_given


# ---- seeded cases shared by the CPU and the GPU tests ----------------------------------------------------------------------------
def corners(min_xyz, size_xyz):
    """The cuboid corner order of generators/colibri.py:121-151 (lower level first), float32 [8,3]."""
    m, s = np.asarray(min_xyz, np.float64), np.asarray(size_xyz, np.float64)
    return np.array([[m[0] + s[0] * (k % 4 in (1, 2)), m[1] + s[1] * (k % 4 in (2, 3)), m[2] + s[2] * (k >= 4)] for k in range(8)], np.float32)


def case_cuboids(n):
    return np.stack([corners([-40.0 - 6 * l, -30.0 - 4 * l, -50.0 - 5 * l], [80.0 + 12 * l, 60.0 + 8 * l, 100.0 + 10 * l]) for l in range(n)])


def case_colours(n):
    return np.array([[(37 * l + 11) % 256, (91 * l + 200) % 256, (53 * l + 90) % 256] for l in range(n)], np.uint8)


def _gt_row(rng, cam, label, t, rv=None, hand=False, box=None):
    g = np.zeros(88, np.float64)
    g[0] = 1.0
    g[1:5] = box if box is not None else rng.uniform(-5, 60, 4)
    g[5:8] = rng.standard_normal(3) if rv is None else rv
    g[8:11] = t
    g[14:19] = cam
    if hand:
        g[19] = 1.0
        g[20:83] = (np.array([0.0, 0.0, 0.5]) + rng.standard_normal((21, 3)) * 0.03).reshape(-1)
    g[83] = label
    return g


def case_main(seed=3):
    """Frames 48 x 64, batch 3, three labels, amax 4, six detection rows, cap 3 (the GPU test's first case; what each image holds is
    asserted on the oracle in tests/test_draw_cpu.py).  Returns a dict of host arrays."""
    rng = np.random.Generator(np.random.PCG64([seed, 0xD2A3]))
    B, H, W, A, R, L = 3, 48, 64, 4, 6, 3
    cam = np.array([300.5, 298.25, 31.7, 23.3, 0.5])
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    gt = np.zeros((B, A, 88))
    gt[:, :, 14:19] = cam
    near = lambda: np.array([rng.normal(0, 20), rng.normal(0, 15), 520 + rng.normal(0, 30)])
    # image 0: two annotations (one with joints), slot 1 is padding and slot 3 has a label out of range
    gt[0, 0] = _gt_row(rng, cam, 1, near(), hand=True)
    gt[0, 2] = _gt_row(rng, cam, 0, near())
    gt[0, 3] = _gt_row(rng, cam, 3, near())
    # image 1: nothing valid (slot 0 == 0 everywhere; one row filled in but switched off)
    gt[1, 1] = _gt_row(rng, cam, 0, near())
    gt[1, 1, 0] = 0.0
    # image 2: partly outside the frame; a corner behind the camera and projections that saturate; a zero rotation with a degenerate
    # box (one point) and two joints that coincide
    gt[2, 0] = _gt_row(rng, cam, 2, np.array([95.0, -60.0, 400.0]))
    gt[2, 1] = _gt_row(rng, cam, 0, np.array([12.0, 7.0, 41.0]))
    gt[2, 2] = _gt_row(rng, cam, 1, near(), rv=np.zeros(3), hand=True, box=np.array([20.0, 30.0, 20.0, 30.0]))
    gt[2, 2, 20 + 3 * 6:23 + 3 * 6] = gt[2, 2, 20 + 3 * 5:23 + 3 * 5]
    det = dict(boxes=rng.uniform(0, 30, (B, R, 4)).astype(np.float32), scores=rng.uniform(0.55, 0.99, (B, R)).astype(np.float32),
               labels=rng.integers(0, L, (B, R)).astype(np.int32), rotation=rng.uniform(-1, 1, (B, R, 3)).astype(np.float32),
               translation=np.stack([[near() for _ in range(R)] for _ in range(B)]).astype(np.float32),
               hand=(np.array([0.0, 0.0, 0.5]) + rng.standard_normal((B, R, 21, 3)) * 0.03).reshape(B, R, 63).astype(np.float32))
    # image 0: row 1 exactly at the threshold (no candidate), row 2 padding, row 3 a label out of range (kept, then skipped), row 5 beyond the cap
    det["scores"][0, 1] = 0.5
    for k in det:
        det[k][0, 2] = -1
    det["labels"][0, 3] = 5
    det["scores"][1] = [0.5, 0.1, -1.0, 0.49, 0.0, float("nan")]       # image 1: no candidate
    det["rotation"][2, 0] = 0.0                                          # image 2: a zero rotation, a pose far off the frame, one behind the camera
    det["translation"][2, 1] = [-400.0, 300.0, 450.0]
    det["translation"][2, 2] = [5.0, 5.0, -300.0]
    return dict(frames=frames, gt=gt, det=det, cuboids=case_cuboids(L), colours=case_colours(L), score_threshold=0.5, max_detections=3)


def case_caps(seed=5):
    """Frames 37 x 50, batch 1, at the caps: 16 annotations, 256 rows with more than 64 candidates and max_detections 64; five labels."""
    rng = np.random.Generator(np.random.PCG64([seed, 0xCA95]))
    H, W, A, R, L = 37, 50, 16, 256, 5
    cam = np.array([150.25, 151.5, 24.6, 18.2, 1.0])
    frames = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    near = lambda: np.array([rng.normal(0, 320), rng.normal(0, 240), 900 + rng.normal(0, 60)])      # many shapes partly or wholly off the frame
    gt = np.stack([_gt_row(rng, cam, int(rng.integers(0, L)), near(), hand=bool(k % 2)) for k in range(A)])[None]
    det = dict(boxes=rng.uniform(0, 50, (1, R, 4)).astype(np.float32), scores=rng.uniform(0.0, 1.0, (1, R)).astype(np.float32),
               labels=rng.integers(0, L + 1, (1, R)).astype(np.int32), rotation=rng.uniform(-1, 1, (1, R, 3)).astype(np.float32),
               translation=np.stack([near() for _ in range(R)])[None].astype(np.float32),
               hand=(np.array([0.0, 0.0, 0.5]) + rng.standard_normal((1, R, 21, 3)) * 0.08).reshape(1, R, 63).astype(np.float32))
    return dict(frames=frames, gt=gt, det=det, cuboids=case_cuboids(L), colours=case_colours(L), score_threshold=0.5, max_detections=64)
