"""hep_render_models_device stated in numpy (float64 projection and depth, exact integer coverage): THE definition of the model
renderer - the kernels (csrc/k_render.hip) reproduce it bit for bit; include/hep.h states the same in words.  Plain loops over images,
pose slots and faces, vectorised over the pixels of a face's bounding box.  Shared by tests/test_render_cpu.py and
tests/test_gpu_render.py.

Every rounding, in order:
  projection   X = ((R0 v0 + R1 v1) + R2 v2) + t0 (rows 1, 2 alike for Y, Z) in float64, v the float32 vertex widened;
               u = (fx X) / Z + cx, v = (fy Y) / Z + cy; a vertex is valid when Z > 0 and neither u nor v is NaN;
               sx = floor(clip(16 u + 0.5, -8192*16, 8191*16)), sy alike (16 u is exact; the sum rounds once).
  coverage     integers only (Python ints / int64): see ``edge_setup`` and ``coverage``.
  depth        w_i = 1 / Z_i; invz = ((E0 w0 + E1 w1) + E2 w2) / A, E_i and A converted exactly (|.| < 2^53); z = 1 / invz.
  winner       z < best, or z == best and (slot << 24 | face) smaller; the start is (+inf, no key); a NaN z never wins.
  outputs      mask = uint8 of the winner's truncated mask value; depth = float32(z), round to nearest even;
               frame = (alpha colour + (256 - alpha) old + 128) >> 8 in integers."""
import numpy as np

SAT_LO, SAT_HI = -8192.0 * 16.0, 8191.0 * 16.0
NO_KEY = 0xFFFFFFFF
MAX_POSES = 16


def row_label(row, num_labels):
    """The label of a pose row, or None when the row is skipped."""
    valid, lab, mv = float(row[0]), float(row[1]), float(row[2])
    if not valid != 0.0 or not (lab >= 0.0 and lab < num_labels) or not (mv >= 1.0 and mv < 256.0):
        return None
    return int(lab)


def snap(u):
    t = 16.0 * u + 0.5
    return np.floor(np.clip(t, SAT_LO, SAT_HI)).astype(np.int64)


def project(row, cam, vertices):
    """(sx, sy int64 [V], w float64 [V], valid bool [V]) of float32 ``vertices`` [V,3] under one pose row and camera."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    P = np.asarray(row, np.float64)
    fx, fy, cx, cy = (np.float64(c) for c in cam[:4])
    with np.errstate(all="ignore"):
        X = ((P[4] * v[:, 0] + P[5] * v[:, 1]) + P[6] * v[:, 2]) + P[13]
        Y = ((P[7] * v[:, 0] + P[8] * v[:, 1]) + P[9] * v[:, 2]) + P[14]
        Z = ((P[10] * v[:, 0] + P[11] * v[:, 1]) + P[12] * v[:, 2]) + P[15]
        pu, pv = (fx * X) / Z + cx, (fy * Y) / Z + cy
        valid = (Z > 0.0) & (pu == pu) & (pv == pv)
        pu, pv = np.where(valid, pu, 0.0), np.where(valid, pv, 0.0)
        w = np.where(valid, 1.0 / np.where(valid, Z, 1.0), -1.0)
    return snap(pu), snap(pv), w, valid


def edge_setup(tri):
    """``tri``: three (sx, sy) integer pairs.  None when the doubled area A' = (x1-x0)(y2-y0) - (y1-y0)(x2-x0) is zero, else the three
    edges (ax, ay, dx, dy, top_left) for (a, b) = (v1, v2), (v2, v0), (v0, v1) with (dx, dy) = sign(A') (b - a), so that the edge
    functions E_i(p) = dx (py - ay) - dy (px - ax) sum to |A'|.  top_left: dy < 0, or dy == 0 and dx > 0."""
    (x0, y0), (x1, y1), (x2, y2) = [(int(p[0]), int(p[1])) for p in tri]
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    if area == 0:
        return None
    s = 1 if area > 0 else -1
    out = []
    for (ax, ay), (bx, by) in (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1))):
        dx, dy = s * (bx - ax), s * (by - ay)
        out.append((ax, ay, dx, dy, dy < 0 or (dy == 0 and dx > 0)))
    return out


def coverage(tri, xs, ys):
    """(inside bool, [E0, E1, E2] int64) at the pixels (xs, ys) (int64 arrays of pixel indices); None for a face of zero area."""
    edges = edge_setup(tri)
    if edges is None:
        return None
    px, py = 16 * np.asarray(xs, np.int64) + 8, 16 * np.asarray(ys, np.int64) + 8
    inside, E = np.ones(px.shape, bool), []
    for ax, ay, dx, dy, tl in edges:
        e = dx * (py - ay) - dy * (px - ax)               # |.| < 2^37: exact in int64
        inside &= (e > 0) | ((e == 0) & tl)
        E.append(e)
    return inside, E


def face_depth(E, w):
    """float64 z of the fragments with edge functions ``E`` (three int64 arrays) and the vertices' 1 / Z ``w`` (three float64)."""
    with np.errstate(all="ignore"):
        A = (E[0] + E[1] + E[2]).astype(np.float64)
        invz = ((E[0].astype(np.float64) * w[0] + E[1].astype(np.float64) * w[1]) + E[2].astype(np.float64) * w[2]) / A
        return 1.0 / invz


def render_image(poses, cam, vertices, faces, face_start, H, W):
    """(best z float64 [H,W], key uint32 [H,W]) of one image: key = slot << 24 | face of the winner, NO_KEY where nothing is rendered."""
    num_labels, V = len(face_start) - 1, len(vertices)
    bz, bkey = np.full((H, W), np.inf), np.full((H, W), NO_KEY, np.int64)
    faces = np.asarray(faces, np.int64)
    for slot, row in enumerate(np.asarray(poses, np.float64)):
        lab = row_label(row, num_labels)
        if lab is None:
            continue
        sx, sy, w, valid = project(row, cam, vertices)
        for f in range(int(face_start[lab]), int(face_start[lab + 1])):
            idx = faces[f]
            if (idx < 0).any() or (idx >= V).any() or not valid[idx].all():
                continue
            tri = [(int(sx[i]), int(sy[i])) for i in idx]
            # the pixels whose centres lie in the sub-pixel bounding box (inclusive), clipped to the frame
            xa, xb = max(0, -(-(min(p[0] for p in tri) - 8) // 16)), min(W - 1, (max(p[0] for p in tri) - 8) // 16)
            ya, yb = max(0, -(-(min(p[1] for p in tri) - 8) // 16)), min(H - 1, (max(p[1] for p in tri) - 8) // 16)
            if xa > xb or ya > yb:
                continue
            ys, xs = np.mgrid[ya:yb + 1, xa:xb + 1]
            cov = coverage(tri, xs, ys)
            if cov is None:
                continue
            inside, E = cov
            if not inside.any():
                continue
            z = face_depth(E, [w[i] for i in idx])
            key = (slot << 24) | f
            sub_z, sub_k = bz[ya:yb + 1, xa:xb + 1], bkey[ya:yb + 1, xa:xb + 1]
            win = inside & ((z < sub_z) | ((z == sub_z) & (key < sub_k)))
            sub_z[win] = z[win]
            sub_k[win] = key
    return bz, bkey


def blend(old, colour, alpha):
    """(alpha colour + (256 - alpha) old + 128) >> 8 per channel, integers."""
    return ((int(alpha) * np.asarray(colour, np.int64) + (256 - int(alpha)) * np.asarray(old, np.int64) + 128) >> 8).astype(np.uint8)


def render_models(poses, camera, vertices, faces, face_start, H, W, frames=None, colours=None, alpha=128):
    """dict(mask uint8 [B,H,W], depth float32 [B,H,W], key int64 [B,H,W], z float64 [B,H,W], frames: a blended copy or None)."""
    poses = np.asarray(poses, np.float64)
    B = poses.shape[0]
    assert poses.ndim == 3 and poses.shape[2] == 16 and 1 <= poses.shape[1] <= MAX_POSES
    mask, depth = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.float32)
    keys, zs = np.zeros((B, H, W), np.int64), np.zeros((B, H, W), np.float64)
    out = None if frames is None else np.array(frames, np.uint8, copy=True)
    for b in range(B):
        bz, bkey = render_image(poses[b], camera[b], vertices, faces, face_start, H, W)
        keys[b], zs[b] = bkey, bz
        hit = bkey != NO_KEY
        slot = np.where(hit, bkey >> 24, 0)
        mask[b] = np.where(hit, poses[b, slot, 2].astype(np.int64), 0).astype(np.uint8)
        with np.errstate(over="ignore"):
            depth[b] = np.where(hit, bz, 0.0).astype(np.float32)
        if out is not None and hit.any():
            lab = poses[b, slot, 1].astype(np.int64)[hit]
            out[b][hit] = blend(out[b][hit], np.asarray(colours, np.uint8)[lab], alpha)
    return dict(mask=mask, depth=depth, key=keys, z=zs, frames=out)


# ---- shared cases -------------------------------------------------------------------------------------------------------------
def pose_row(label, mask_value, R=None, t=(0.0, 0.0, 1.0), valid=1.0):
    row = np.zeros(16)
    row[0], row[1], row[2] = valid, label, mask_value
    row[4:13] = np.eye(3).reshape(9) if R is None else np.asarray(R, np.float64).reshape(9)
    row[13:16] = t
    return row


def rotation(axis, angle):
    """A rotation matrix in float64 (numpy's sin / cos: the tables are INPUTS of both sides, their last bits do not matter)."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def cube(h=0.05):
    v = np.array([[x, y, z] for z in (-h, h) for y in (-h, h) for x in (-h, h)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def tetrahedron(h=0.06):
    v = np.array([[h, h, h], [h, -h, -h], [-h, h, -h], [-h, -h, h]], np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, f


def concat(meshes):
    """(vertices, faces, face_start) of a list of (vertices, faces), one per label."""
    vs, fs, start, off = [], [], [0], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32))
        fs.append(np.asarray(f, np.int32) + off)
        off += len(v)
        start.append(start[-1] + len(f))
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32), np.asarray(start, np.int32)


def case_scene(H=48, W=80, seed=7):
    """Batch 3 of H x W over a cube (label 0) and a tetrahedron (label 1): image 0 three poses at different depths that overlap, image 1
    no valid row (a zero valid slot, a bad label, mask values 0 and 256, a NaN label), image 2 a cube partly behind the camera (skipped
    faces), one cut by the frame's right side, one on screen and one entirely off screen; pmax 4."""
    rng = np.random.Generator(np.random.PCG64(seed))
    vertices, faces, face_start = concat([cube(), tetrahedron()])
    cam = np.array([[90.3, 88.1, W / 2 + 0.37, H / 2 - 0.21, 1.0], [85.0, 85.0, W / 2, H / 2, 0.5], [70.2, 71.9, W / 2 - 3.3, H / 2 + 2.1, 1.0]])
    poses = np.zeros((3, 4, 16))
    poses[0, 0] = pose_row(0, 7, rotation((1, 2, 3), 0.7), (0.02, 0.01, 0.30))
    poses[0, 1] = pose_row(1, 200, rotation((3, -1, 2), 1.9), (-0.03, 0.0, 0.26))
    poses[0, 2] = pose_row(0, 255, rotation((0, 1, 0), 0.4), (0.06, -0.02, 0.42))
    poses[1, 0] = pose_row(0, 9, None, (0, 0, 0.3), valid=0.0)
    poses[1, 1] = pose_row(2, 9, None, (0, 0, 0.3))
    poses[1, 2] = pose_row(0, 0, None, (0, 0, 0.3))
    poses[1, 3] = pose_row(float("nan"), 256, None, (0, 0, 0.3))
    poses[2, 0] = pose_row(0, 3, rotation((1, 1, 0), 0.5), (-0.05, 0.0, 0.03))          # corners behind the camera: those faces are skipped
    poses[2, 1] = pose_row(1, 4, rotation((1, 0, 1), 2.5), (0.16, -0.01, 0.2))         # cut by the right side of the frame
    poses[2, 2] = pose_row(1, 5, rotation((0, 0, 1), 0.3), (0.04, -0.07, 0.33))
    poses[2, 3] = pose_row(0, 6, rotation((1, 0, 0), 0.3), (-9.0, 0.0, 0.4))           # entirely off screen
    frames = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    colours = np.array([[255, 40, 0], [0, 90, 255]], np.uint8)
    return dict(poses=poses, camera=cam, vertices=vertices, faces=faces, face_start=face_start, H=H, W=W, frames=frames, colours=colours)
