"""hep_synth_frames_device stated in numpy: THE definition of the synthetic-frame generator - the kernels (csrc/k_render.hip, the shaded
variant of the rasteriser) reproduce it bit for bit; include/hep.h states the same in words.  Built on the primitives of tests/_render.py:
projection, coverage, depth and the winner per pixel are ``render_image``'s, unchanged.  Shared by tests/test_synth_cpu.py and
tests/test_gpu_synth.py.

Every rounding of the shading, in order (float64, one rounding per operation, no contraction), for a pixel whose winner is face f of a slot
with vertices v0, v1, v2, edge values E0, E1, E2 at the pixel centre (exact integers) and w_i = 1 / Z_i as ``project`` returns them:
  weights      q_i = float64(E_i) * w_i; den = (q0 + q1) + q2; b_i = q_i / den.
  colour       c_k = (b0 C0k + b1 C1k) + b2 C2k, Cik the uint8 colour of vertex i widened, k = 0, 1, 2.
  light        m_r = (R[r][0] n0 + R[r][1] n1) + R[r][2] n2 with R the pose row's matrix and n the face's normal (plain data; zeros are legal);
               d = (m_0 lx + m_1 ly) + m_2 lz; d = -d when d < 0 (two-sided); s = ambient + diffuse * d.
  byte         v_k = (c_k * s) * gain_k; t = v_k + 0.5; 0 when not t >= 0 (a NaN gives 0), 255 when t >= 256, else floor(t).
  frame        ``_render.blend``: (alpha byte + (256 - alpha) old + 128) >> 8 in integers.
visible is the box-from-mask rule per SLOT: inclusive minimum and maximum of the pixel indices a slot won, and their count.
The annotation tensors: per image the slots in order; a slot is kept when its row is rendered (``_render.row_label``) and count >=
min_pixels; the n-th kept slot becomes row n; padding is zeros, -1 in slot_of."""
import numpy as np

from tests import _render as R

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
EMPTY = (INT_MAX, INT_MAX, INT_MIN, INT_MIN, 0)


def shade_bytes(E, w, colours3, R9, normal, light):
    """int64 [n,3] bytes of n fragments of ONE face: ``E`` three int64 arrays [n], ``w`` three float64, ``colours3`` uint8 [3,3] (vertex,
    channel), ``R9`` the nine doubles of the pose row's matrix, ``normal`` float64 [3], ``light`` float64 [8]."""
    with np.errstate(all="ignore"):
        q = [E[i].astype(np.float64) * np.float64(w[i]) for i in range(3)]
        den = (q[0] + q[1]) + q[2]
        b = [q[i] / den for i in range(3)]
        C = np.asarray(colours3, np.uint8).astype(np.float64)
        Rm, n, L = np.asarray(R9, np.float64).reshape(3, 3), np.asarray(normal, np.float64), np.asarray(light, np.float64)
        m = [(Rm[r, 0] * n[0] + Rm[r, 1] * n[1]) + Rm[r, 2] * n[2] for r in range(3)]
        d = (m[0] * L[0] + m[1] * L[1]) + m[2] * L[2]
        d = -d if d < 0 else d
        s = L[3] + L[4] * d
        out = np.zeros((len(E[0]), 3), np.int64)
        for k in range(3):
            c = (b[0] * C[0, k] + b[1] * C[1, k]) + b[2] * C[2, k]
            t = (c * s) * L[5 + k] + 0.5
            ok = t >= 0                                                        # NaN fails
            out[:, k] = np.where(ok, np.where(t >= 256, 255, np.floor(np.where(ok & (t < 256), t, 0.0))), 0).astype(np.int64)
    return out


def synth_image(poses, cam, vertices, vertex_colours, faces, face_normals, face_start, light, H, W, frame, alpha):
    """One image: (bz, bkey, visible int64 [pmax,5]); ``frame`` uint8 [H,W,3] is composited in place."""
    poses = np.asarray(poses, np.float64)
    bz, bkey = R.render_image(poses, cam, vertices, faces, face_start, H, W)
    visible = np.array([EMPTY] * len(poses), np.int64)
    faces = np.asarray(faces, np.int64)
    for key in np.unique(bkey[bkey != R.NO_KEY]):
        slot, f = int(key) >> 24, int(key) & 0xFFFFFF
        ys, xs = np.nonzero(bkey == key)
        sx, sy, w, _ = R.project(poses[slot], cam, vertices)
        idx = faces[f]
        _, E = R.coverage([(int(sx[i]), int(sy[i])) for i in idx], xs, ys)
        byte = shade_bytes(E, [w[i] for i in idx], np.asarray(vertex_colours, np.uint8)[idx], poses[slot, 4:13], np.asarray(face_normals, np.float64)[f], light)
        frame[ys, xs] = R.blend(frame[ys, xs], byte, alpha)
    slots = np.where(bkey != R.NO_KEY, bkey >> 24, -1)
    for k in range(len(poses)):
        ys, xs = np.nonzero(slots == k)
        if len(ys):
            visible[k] = (xs.min(), ys.min(), xs.max(), ys.max(), len(ys))
    return bz, bkey, visible


def compact(poses, visible, num_labels, min_pixels, rvec, tvec, extra):
    """The padded annotation tensors of a batch from ``visible`` int [B,pmax,5] and the caller's padded rvec, tvec [B,pmax,3], extra [B,pmax,2]."""
    poses = np.asarray(poses, np.float64)
    B, K = poses.shape[:2]
    out = dict(boxes=np.zeros((B, K, 4), np.float64), labels=np.zeros((B, K), np.int32), mask_values=np.zeros((B, K), np.int32),
               rvec=np.zeros((B, K, 3), np.float32), tvec=np.zeros((B, K, 3), np.float32), extra=np.zeros((B, K, 2), np.float32),
               num_gt=np.zeros(B, np.int32), slot_of=np.full((B, K), -1, np.int32))
    for b in range(B):
        n = 0
        for k in range(K):
            lab = R.row_label(poses[b, k], num_labels)
            if lab is None or visible[b, k, 4] < min_pixels:
                continue
            out["boxes"][b, n] = visible[b, k, :4]
            out["labels"][b, n], out["mask_values"][b, n] = lab, int(poses[b, k, 2])
            out["rvec"][b, n], out["tvec"][b, n], out["extra"][b, n] = rvec[b, k], tvec[b, k], extra[b, k]
            out["slot_of"][b, n] = k
            n += 1
        out["num_gt"][b] = n
    return out


def synth_frames(poses, camera, vertices, vertex_colours, faces, face_normals, face_start, lights, frames, alpha=256, min_pixels=16,
                 rvec=None, tvec=None, extra=None):
    """dict(frames: a composited copy, mask uint8 [B,H,W], depth float32 [B,H,W], key int64, visible int32 [B,pmax,5], annotations: the
    dict of ``compact`` - None without rvec / tvec / extra)."""
    poses = np.asarray(poses, np.float64)
    B, K = poses.shape[:2]
    assert poses.ndim == 3 and poses.shape[2] == 16 and 1 <= K <= R.MAX_POSES and min_pixels >= 1 and 0 <= alpha <= 256
    out = np.array(frames, np.uint8, copy=True)
    H, W = out.shape[1:3]
    mask, depth = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.float32)
    keys, visible = np.zeros((B, H, W), np.int64), np.zeros((B, K, 5), np.int32)
    for b in range(B):
        bz, bkey, vis = synth_image(poses[b], camera[b], vertices, vertex_colours, faces, face_normals, face_start, np.asarray(lights, np.float64)[b], H, W, out[b], alpha)
        keys[b], visible[b] = bkey, vis
        hit = bkey != R.NO_KEY
        slot = np.where(hit, bkey >> 24, 0)
        mask[b] = np.where(hit, poses[b, slot, 2].astype(np.int64), 0).astype(np.uint8)
        with np.errstate(over="ignore"):
            depth[b] = np.where(hit, bz, 0.0).astype(np.float32)
    ann = None if rvec is None else compact(poses, visible, len(face_start) - 1, min_pixels, np.asarray(rvec, np.float32), np.asarray(tvec, np.float32), np.asarray(extra, np.float32))
    return dict(frames=out, mask=mask, depth=depth, key=keys, visible=visible, annotations=ann)


# ---- shared cases -------------------------------------------------------------------------------------------------------------
def face_normals(vertices, faces):
    """float64 [F,3]: cross(v1 - v0, v2 - v0) / length of the widened float32 vertices; zeros for a zero-length cross product - the
    statement ``ShadedMeshSet`` is tested against."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.sqrt((c * c).sum(axis=1))
    return np.where(n[:, None] > 0, c / np.where(n > 0, n, 1.0)[:, None], 0.0)


def sphere(radius=0.05, rings=18, sectors=32):
    """A latitude-longitude sphere: (vertices float32, faces int32) with 2 * sectors * (rings - 1) faces."""
    v = [[0.0, 0.0, radius]]
    for i in range(1, rings):
        th = np.pi * i / rings
        for j in range(sectors):
            ph = 2 * np.pi * j / sectors
            v.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
    v.append([0.0, 0.0, -radius])
    f, last = [], len(v) - 1
    ring = lambda i, j: 1 + (i - 1) * sectors + j % sectors
    for j in range(sectors):
        f.append([0, ring(1, j), ring(1, j + 1)])
        f.append([last, ring(rings - 1, j + 1), ring(rings - 1, j)])
    for i in range(1, rings - 1):
        for j in range(sectors):
            f.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            f.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def colours_for(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (n, 3), dtype=np.uint8)


def light_row(direction=(0.0, 0.0, -1.0), ambient=0.3, diffuse=0.7, gain=(1.0, 1.0, 1.0)):
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    return np.array([d[0], d[1], d[2], ambient, diffuse, gain[0], gain[1], gain[2]], np.float64)


def padded_inputs(B, K, seed=3):
    """rvec, tvec, extra float32 of arbitrary distinct values: the gather only copies them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal((B, K, 3)).astype(np.float32), rng.standard_normal((B, K, 3)).astype(np.float32), rng.standard_normal((B, K, 2)).astype(np.float32))


def case_overlap(H=44, W=72, seed=5):
    """Three images of 44 x 72 (partial tiles at both edges), pmax 3, each with its own light: a cube and a tetrahedron that overlap (the
    visible boxes differ from the projected ones) and one slot wholly behind another (image 0, slot 2 behind slot 0)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    vertices, faces, face_start = R.concat([R.cube(), R.tetrahedron()])
    cam = np.array([[90.3, 88.1, W / 2 + 0.37, H / 2 - 0.21, 1.0], [85.0, 85.0, W / 2, H / 2, 0.5], [70.2, 71.9, W / 2 - 3.3, H / 2 + 2.1, 1.0]])
    poses = np.zeros((3, 3, 16))
    poses[0, 0] = R.pose_row(0, 7, R.rotation((1, 2, 3), 0.7), (0.02, 0.01, 0.30))
    poses[0, 1] = R.pose_row(1, 200, R.rotation((3, -1, 2), 1.9), (-0.03, 0.0, 0.26))
    poses[0, 2] = R.pose_row(1, 255, R.rotation((0, 1, 0), 0.4), (0.02, 0.01, 0.95))           # small and far: wholly behind the cube of slot 0
    poses[1, 0] = R.pose_row(1, 9, R.rotation((1, 0, 0), 1.0), (0.0, 0.0, 0.25))
    poses[1, 1] = R.pose_row(0, 10, R.rotation((0, 1, 1), 0.5), (0.03, 0.01, 0.3))
    poses[1, 2] = R.pose_row(0, 11, None, (0, 0, 0.3), valid=0.0)
    poses[2, 0] = R.pose_row(0, 3, R.rotation((1, 1, 0), 0.5), (0.10, 0.0, 0.25))              # cut by the frame's right side
    poses[2, 1] = R.pose_row(1, 4, R.rotation((1, 0, 1), 2.5), (-0.05, -0.01, 0.2))
    poses[2, 2] = R.pose_row(0, 5, R.rotation((0, 0, 1), 0.3), (-0.02, 0.02, 0.33))
    lights = np.stack([light_row((0.2, -0.3, -1.0), 0.35, 0.6, (1.0, 0.95, 1.05)), light_row((-1.0, 0.1, -0.4), 0.5, 0.45, (0.9, 1.1, 1.0)),
                       light_row((0.0, 1.0, -0.2), 0.3, 0.8, (1.1, 1.0, 0.9))])
    rvec, tvec, extra = padded_inputs(3, 3)
    return dict(poses=poses, camera=cam, vertices=vertices, vertex_colours=colours_for(len(vertices), seed + 1), faces=faces,
                face_normals=face_normals(vertices, faces), face_start=face_start, lights=lights, H=H, W=W,
                frames=rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8), rvec=rvec, tvec=tvec, extra=extra)


def run(c, alpha=256, min_pixels=16, annotations=True):
    """``synth_frames`` on a case dict."""
    kw = dict(rvec=c["rvec"], tvec=c["tvec"], extra=c["extra"]) if annotations else {}
    return synth_frames(c["poses"], c["camera"], c["vertices"], c["vertex_colours"], c["faces"], c["face_normals"], c["face_start"], c["lights"], c["frames"],
                        alpha=alpha, min_pixels=min_pixels, **kw)
