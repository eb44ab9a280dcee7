"""CPU (no GPU): the rectified windows of the whole-frame search.  1: the host arithmetic (hep_rectify_windows, hep_rectified_point_to_frame,
hep_window_from_box_rectified) equals the numpy definition of tests/_rectify.py bit for bit and refuses bad arguments with the named reason.
2: the geometry of that definition is exact - the rectified window is a rotated camera, and a back-rotated pose lands on the same frame pixels.
3: the rectified window IS the rotated camera's picture of a rendered mesh to within one pixel of its silhouette, and the plain window is not."""
import ctypes
import os

import numpy as np
import pytest

import hmd_ego_pose_amd as H
from hmd_ego_pose_amd import _capi
from tests import _rectify as R
from tests import _render as RD
from tests import _windows as W

NEW = ("hep_rectify_windows", "hep_rectified_point_to_frame", "hep_window_from_box_rectified", "hep_preprocess_i420_rectified_device",
       "hep_derotate_records_device", "hep_pose_from_i420_windows_rectified", "hep_poses_from_i420_windows_rectified",
       "hep_pose_from_i420_tiled_rectified", "hep_poses_from_i420_tiled_rectified")
H50, W66, CROP, RS, SIZE = 50, 66, 32, 48, 128
# a short focal length (pixels of the resized window), principal point off the centre 23.5: border windows sit about 30 degrees off axis
CAM = np.array([[40.25, 43.5, 25.75, 21.5, 1000.0, 0.375], [39.5, 42.75, 22.25, 26.0, 1000.0, 0.375]], np.float32)
TABLE = np.array([[1, 34, 18], [1, 5, 7], [0, 17, 0], [0, 17, 0], [0, 1, 17]], np.int32)      # odd offsets, frames out of order, one window twice


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_the_nine_symbols_are_declared_bound_and_exported():
    l = _capi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hep.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name
        assert name in _capi.SYMBOLS and hasattr(l, name), name
    assert f"#define HEP_RECTIFY_ROW_DOUBLES {R.TABLE_DOUBLES}" in header and _capi.RECTIFY_ROW_DOUBLES == R.TABLE_DOUBLES
    assert l.hep_abi_version() == 1                                 # additive: the ABI version stays


@pytest.mark.parametrize("geom", [(H50, W66, CROP, RS), (48, 64, 32, 48), (504, 896, 256, 512), (300, 402, 201, 333)])
def test_rectify_windows_equals_the_definition_bit_for_bit(geom):
    h, w, crop, rs = geom
    scale = rs / RS                                                 # the same field of view at every geometry
    cam = CAM.copy()
    cam[:, :4] *= np.float32(scale)
    grid = W.tile_windows(h, w, crop, 3, 2, 2)
    table = TABLE if geom == (H50, W66, CROP, RS) else np.array([[1, w - crop, h - crop], [1, 5, 7], [0, 17, 0], [0, 1, 15]], np.int32)
    for windows in (grid, table):
        got = H.rectify_windows(cam, windows, h, w, crop, rs)
        want = R.rectify_windows(cam, windows, h, w, crop, rs)
        assert got.dtype == np.float64 and got.shape == (len(windows), 13) and np.array_equal(bits(got), bits(want)), geom
        for row in got:                                             # a rotation: orthonormal, determinant +1
            Rw = row[:9].reshape(3, 3)
            assert np.abs(Rw @ Rw.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(Rw) - 1.0) < 1e-15
    # the corner window of the small geometries looks about 30 degrees off axis
    if rs == RS:
        off = np.degrees(np.arccos(H.rectify_windows(cam, grid, h, w, crop, rs)[:, 8]))
        assert 25.0 < off.max() < 40.0, off
    # the centre window: the identity bit for bit (+0.0 everywhere), whichever frame
    centre = np.array([[f, (w - crop) // 2, (h - crop) // 2] for f in (1, 0)], np.int32)
    got = H.rectify_windows(cam, centre, h, w, crop, rs)
    assert np.array_equal(bits(got[:, :9]), bits(np.tile(np.eye(3).reshape(9), (2, 1))))
    assert np.array_equal(got[:, 9:], cam[[1, 0], :4].astype(np.float64))


def test_point_to_frame_and_window_from_box_equal_the_definition():
    h, w, crop, rs, size = 504, 896, 256, 512, 512
    cam = np.array([[840.0, 851.5, 262.25, 249.5, 1000.0, 1.0]], np.float32)       # the border windows look 37 degrees off axis
    rng = np.random.Generator(np.random.PCG64(13))
    grid = W.tile_windows(h, w, crop, 4, 2, 1)
    table = H.rectify_windows(cam, grid, h, w, crop, rs)
    for i, row in enumerate(table):
        for _ in range(40):
            x, y = rng.uniform(-30, size + 30, 2)
            got, want = H.rectified_point_to_frame(row, x, y, h, w, crop, rs, size), R.rectified_point_to_frame(row, x, y, h, w, crop, rs, size)
            assert np.array_equal(bits(got), bits(want)), (i, x, y)
            c, half = rng.uniform(-40, size + 40, 2), rng.uniform(1, 120, 2)
            box = np.concatenate([c - half, c + half]).astype(np.float32)
            g = H.window_from_box_rectified(row, box, h, w, crop, rs, size)
            assert g == R.window_from_box_rectified(row, box, h, w, crop, rs, size) and 0 <= g[0] <= w - crop and 0 <= g[1] <= h - crop
        # the centre of the network input looks (almost: the principal point sits 6.75 and 6 resized pixels off it) along the window's ray, so a
        # box there keeps the window: 3.4 frame pixels, stretched by at most 1 / cos^2 = 1.6 off axis, and the rounding
        mid = np.array([size / 2 - 10.5, size / 2 - 10.5, size / 2 + 9.5, size / 2 + 9.5], np.float32)
        gx, gy = H.window_from_box_rectified(row, mid, h, w, crop, rs, size)
        assert abs(gx - grid[i, 1]) <= 7 and abs(gy - grid[i, 2]) <= 7, (i, gx, gy, grid[i])
    # a ray that points backwards: NaN from the point map, the window clamps to 0
    back = table[0].copy()
    back[:9] = [1, 0, 0, 0, -1, 0, 0, 0, -1]
    assert all(np.isnan(v) for v in H.rectified_point_to_frame(back, 10.0, 10.0, h, w, crop, rs, size))
    assert H.window_from_box_rectified(back, mid, h, w, crop, rs, size) == (0, 0) == R.window_from_box_rectified(back, mid, h, w, crop, rs, size)


def test_every_refusal_of_the_host_arithmetic_and_of_the_device_entry_points():
    """No device exists here: a call that reached HIP would fail with another code and another text (see tests/test_windows_cpu.py)."""
    l = _capi.lib()
    buf = np.zeros(4096, np.float32)
    a = buf.ctypes.data
    fake = np.zeros(1 << 16, np.uint8).ctypes.data
    cam = np.array([[400, 400, 255, 255, 1000, 1], [400, 400, 255, 255, 1000, 1]], np.float32)
    cp = cam.ctypes.data
    inside = np.array([[0, 10, 10]], np.int32)
    iw = inside.ctypes.data
    out = np.zeros(26, np.float64)
    op = out.ctypes.data
    row = R.rectify_windows(cam, inside, 480, 640, 256, 512)[0].copy()
    rp = row.ctypes.data
    x, y = ctypes.c_int32(), ctypes.c_int32()
    bad_rows = []
    for k, v in ((9, 0.0), (9, -1.0), (10, float("nan")), (10, float("inf"))):
        r = row.copy(); r[k] = v
        bad_rows.append(r)
    bad_cams = []
    for k, v in ((0, 0.0), (1, -3.0), (0, float("nan")), (1, float("inf"))):
        c = cam.copy(); c[0, k] = v
        bad_cams.append(c)
    outside = [np.array([[0, 385, 0]], np.int32), np.array([[0, 0, 225]], np.int32), np.array([[0, -1, 0]], np.int32), np.array([[-1, 0, 0]], np.int32)]
    no_row = np.array([[2, 0, 0]], np.int32)                          # two camera rows: frame 2 has none

    def rect(camera=cp, frames=2, win=iw, n=1, hh=480, ww=640, crop=256, rs=512, o=op):
        return l.hep_rectify_windows(camera, frames, win, n, hh, ww, crop, rs, o)

    def point(r=rp, hh=480, ww=640, crop=256, rs=512, size=512, o=op):
        return l.hep_rectified_point_to_frame(r, 1.0, 2.0, hh, ww, crop, rs, size, o)

    def from_box(r=rp, box=a, hh=480, ww=640, crop=256, rs=512, size=512, xo=ctypes.byref(x), yo=ctypes.byref(y)):
        return l.hep_window_from_box_rectified(r, box, hh, ww, crop, rs, size, xo, yo)

    def pre(h_, yuv=a, frames=1, hh=480, ww=640, win=a, table=a, n=1, crop=256, o=a):
        return l.hep_preprocess_i420_rectified_device(h_, yuv, frames, hh, ww, win, table, n, crop, 512, o, None)

    rest8, rest7 = [None] * 7, [None] * 6

    def windows(h_, yuv=a, frames=1, hh=480, ww=640, win=iw, n=1, crop=256, camera=cp, found=a, per_label=False):
        if per_label:
            return l.hep_poses_from_i420_windows_rectified(h_, yuv, frames, hh, ww, win, n, crop, 512, camera, 0.5, found, *rest7)
        return l.hep_pose_from_i420_windows_rectified(h_, yuv, frames, hh, ww, win, n, crop, 512, camera, 0.5, found, *rest8)

    def tiled(h_, yuv=a, frames=1, hh=480, ww=640, crop=256, nx=2, ny=2, camera=cp, found=a, window=a, per_label=False):
        if per_label:
            return l.hep_poses_from_i420_tiled_rectified(h_, yuv, frames, hh, ww, crop, 512, nx, ny, camera, 0.5, found, *rest7, window)
        return l.hep_pose_from_i420_tiled_rectified(h_, yuv, frames, hh, ww, crop, 512, nx, ny, camera, 0.5, found, *rest8, window)

    cases = [
        (lambda: rect(camera=None), b"hep_rectify_windows: camera is NULL"),
        (lambda: rect(win=None), b"windows is NULL"),
        (lambda: rect(o=None), b"table_out is NULL"),
        (lambda: rect(n=0), b"n must be >= 1"),
        (lambda: rect(frames=0), b"frames must be >= 1"),
        (lambda: rect(hh=481), b"even"),
        (lambda: rect(ww=641), b"even"),
        (lambda: rect(crop=482), b"crop"),
        (lambda: rect(rs=0), b"resized"),
        (lambda: rect(win=no_row.ctypes.data), b"outside the frame (frame index"),
        (lambda: point(r=None), b"hep_rectified_point_to_frame: row is NULL"),
        (lambda: point(o=None), b"xy_out is NULL"),
        (lambda: point(size=0), b"size must be >= 1"),
        (lambda: point(hh=481), b"even"),
        (lambda: point(crop=482), b"crop"),
        (lambda: from_box(r=None), b"hep_window_from_box_rectified: row is NULL"),
        (lambda: from_box(box=None), b"box is NULL"),
        (lambda: from_box(xo=None), b"ox_out is NULL"),
        (lambda: from_box(yo=None), b"oy_out is NULL"),
        (lambda: from_box(size=0), b"size must be >= 1"),
        (lambda: from_box(ww=641), b"even"),
        (lambda: pre(None), b"hep_preprocess_i420_rectified_device: handle is NULL"),
        (lambda: pre(fake, yuv=None), b"yuv is NULL"),
        (lambda: pre(fake, win=None), b"windows is NULL"),
        (lambda: pre(fake, table=None), b"table is NULL"),
        (lambda: pre(fake, o=None), b"out_hwc is NULL"),
        (lambda: pre(fake, frames=0), b"frames must be >= 1"),
        (lambda: pre(fake, hh=481), b"even"),
        (lambda: pre(fake, crop=482), b"crop"),
        (lambda: pre(fake, n=0), b"n outside 1..max_batch"),
        (lambda: l.hep_derotate_records_device(None, 1, a, 1, None), b"hep_derotate_records_device: records is NULL"),
        (lambda: l.hep_derotate_records_device(a, 1, None, 1, None), b"table is NULL"),
        (lambda: l.hep_derotate_records_device(a, 0, a, 1, None), b"slots outside 1..63"),
        (lambda: l.hep_derotate_records_device(a, 64, a, 1, None), b"slots outside 1..63"),
        (lambda: l.hep_derotate_records_device(a, 1, a, 0, None), b"n outside 1.."),
    ]
    cases += [(lambda o=o: rect(win=o.ctypes.data), b"outside the frame") for o in outside]
    cases += [(lambda c=c: rect(camera=c.ctypes.data), b"fx and fy must be finite and positive") for c in bad_cams]
    cases += [(lambda r=r: point(r=r.ctypes.data), b"fx and fy must be finite and positive") for r in bad_rows]
    cases += [(lambda r=r: from_box(r=r.ctypes.data), b"fx and fy must be finite and positive") for r in bad_rows]
    for per_label in (False, True):
        pre_w = b"hep_poses_from_i420_windows_rectified: " if per_label else b"hep_pose_from_i420_windows_rectified: "
        pre_t = b"hep_poses_from_i420_tiled_rectified: " if per_label else b"hep_pose_from_i420_tiled_rectified: "
        k = dict(per_label=per_label)
        cases += [
            (lambda k=k: windows(None, **k), pre_w + b"handle is NULL"),
            (lambda k=k: windows(fake, yuv=None, **k), pre_w + b"yuv is NULL"),
            (lambda k=k: windows(fake, win=None, **k), b"windows is NULL"),
            (lambda k=k: windows(fake, camera=None, **k), b"camera is NULL"),
            (lambda k=k: windows(fake, found=None, **k), b"found is NULL"),
            (lambda k=k: windows(fake, n=0, **k), b"n outside 1..max_batch"),
            (lambda k=k: windows(fake, frames=0, **k), b"frames must be >= 1"),
            (lambda k=k: windows(fake, hh=481, **k), b"even"),
            (lambda k=k: windows(fake, crop=482, **k), b"crop"),
            (lambda k=k: windows(fake, win=outside[0].ctypes.data, **k), b"outside the frame"),
            (lambda k=k: windows(fake, win=no_row.ctypes.data, frames=2, **k), b"outside the frame"),
            (lambda k=k: windows(fake, camera=bad_cams[0].ctypes.data, **k), pre_w + b"camera row 0: fx and fy must be finite and positive"),
            (lambda k=k: windows(fake, camera=bad_cams[3].ctypes.data, **k), b"fx and fy must be finite and positive"),
            (lambda k=k: tiled(None, **k), pre_t + b"handle is NULL"),
            (lambda k=k: tiled(fake, yuv=None, **k), pre_t + b"yuv is NULL"),
            (lambda k=k: tiled(fake, camera=None, **k), b"camera is NULL"),
            (lambda k=k: tiled(fake, found=None, **k), b"found is NULL"),
            (lambda k=k: tiled(fake, window=None, **k), b"window is NULL"),
            (lambda k=k: tiled(fake, nx=0, **k), b"nx must be >= 1"),
            (lambda k=k: tiled(fake, ny=0, **k), b"ny must be >= 1"),
            (lambda k=k: tiled(fake, frames=0, **k), b"frames must be >= 1"),
            (lambda k=k: tiled(fake, ww=641, **k), b"even"),
            (lambda k=k: tiled(fake, crop=482, **k), b"crop"),
        ]
    for call, reason in cases:
        assert l.hep_anchors(100, None, None) < 0                   # another message in between: the text below is never a stale one
        assert call() == -1, reason                                 # HEP_ERR_INVALID
        assert reason in l.hep_last_error(), (reason, l.hep_last_error())
    # the Python face
    with pytest.raises(ValueError):
        H.rectify_windows(cam, inside.astype(np.int64), 480, 640, 256, 512)
    with pytest.raises(ValueError):
        H.rectify_windows(cam[:, :5], inside, 480, 640, 256, 512)
    with pytest.raises(_capi.HepError):
        H.rectify_windows(cam[:1], np.array([[1, 0, 0]], np.int32), 480, 640, 256, 512)      # no camera row for frame 1
    with pytest.raises(_capi.HepError):
        H.rectify_windows(bad_cams[0], inside, 480, 640, 256, 512)
    with pytest.raises(ValueError):
        H.rectified_point_to_frame(row[:12], 0.0, 0.0, 480, 640, 256, 512, 512)
    with pytest.raises(ValueError):
        H.window_from_box_rectified(row, [1, 2, 3], 480, 640, 256, 512, 512)


# ---- 2. the geometry is exact ----
def test_the_rectified_window_is_a_rotated_camera_and_back_rotated_poses_land_on_the_same_frame_pixels():
    h, w, crop, rs = H50, W66, CROP, RS
    rng = np.random.Generator(np.random.PCG64(2))
    grid = W.tile_windows(h, w, crop, 3, 2, 2)
    table = R.rectify_windows(CAM, grid, h, w, crop, rs)
    model = rng.uniform(-0.05, 0.05, (12, 3))
    worst = [0.0, 0.0, 0.0]
    for (f, _ox, _oy), row in zip(grid, table):
        Rw, cam4 = row[:9].reshape(3, 3), CAM[f, :4]
        # random points in front of BOTH cameras (the rectified view of a point behind the virtual camera does not exist)
        d = Rw[:, 2]
        for _ in range(25):
            Xc = d * rng.uniform(0.3, 2.0) + rng.uniform(-0.08, 0.08, 3)
            Xf, Yf = R.project_to_frame(cam4, Xc, h, w, crop, rs)
            for side in (crop, 128):
                got = R.frame_to_rectified_point(row, Xf, Yf, h, w, crop, rs, side)
                want = R.project_to_side(cam4, Rw.T @ Xc, rs, side)
                worst[0] = max(worst[0], abs(got[0] - want[0]), abs(got[1] - want[1]))
                back = R.rectified_point_to_frame(row, want[0], want[1], h, w, crop, rs, side)      # and the definition's forward map returns
                worst[1] = max(worst[1], abs(back[0] - Xf), abs(back[1] - Yf))
        # a pose of the virtual camera, back-rotated by the definition: the model's points project to the same frame pixels
        R_v, t_v = RD.rotation(rng.standard_normal(3), rng.uniform(0.1, 3.0)), np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 1.5)])
        R_c, t_c = R.derotate_pose(list(row[:9]), R_v, t_v)
        for p in model:
            pv = R.project_to_side(cam4, R_v @ p + t_v, rs, crop)                                  # the pixel of the rectified crop ...
            via_window = R.rectified_point_to_frame(row, pv[0], pv[1], h, w, crop, rs, crop)         # ... carried to the frame
            direct = R.project_to_frame(cam4, R_c @ p + t_c, h, w, crop, rs)                       # the back-rotated pose under the frame camera
            worst[2] = max(worst[2], abs(via_window[0] - direct[0]), abs(via_window[1] - direct[1]))
    print(f"frame -> rectified {worst[0]:.2e} px, rectified -> frame {worst[1]:.2e} px, back-rotated pose {worst[2]:.2e} px")
    assert max(worst) <= 1e-9, worst


def test_derotate_records_of_the_definition_leaves_what_it_must():
    rng = np.random.Generator(np.random.PCG64(3))
    rec = rng.integers(-2 ** 31, 2 ** 31, (3, 2, R.RECORD_WORDS), dtype=np.int64).astype(np.int32)
    rec.view(np.float32)[..., 9:78] = rng.uniform(-0.9, 0.9, (3, 2, 69)).astype(np.float32)
    rec[..., 0] = [[1, 0], [1, 2], [1, 1]]
    grid = np.array([[0, 34, 18], [0, 0, 0], [1, 17, 9]], np.int32)      # the last one: the centre window
    table = R.rectify_windows(CAM, grid, H50, W66, CROP, RS)
    out = R.derotate_records(rec, table)
    keep = np.r_[0:9, 78:80]
    assert np.array_equal(out[..., keep], rec[..., keep])
    assert np.array_equal(out[0, 1], rec[0, 1]) and np.array_equal(out[1, 1], rec[1, 1]) and np.array_equal(out[2], rec[2])      # found 0, found 2, the identity
    assert not np.array_equal(out[0, 0, 9:78], rec[0, 0, 9:78])
    # lengths are kept, and the rotation is R_w applied on the left
    f, g = rec.view(np.float32), out.view(np.float32)
    for i in (0, 1):
        Rw = table[i, :9].reshape(3, 3)
        assert np.allclose(g[i, 0, 12:15], Rw @ f[i, 0, 12:15].astype(np.float64), rtol=0, atol=1e-7)
        A = R.axis_angle_to_matrix(np.pi * g[i, 0, 9:12].astype(np.float64))
        B = Rw @ R.axis_angle_to_matrix(np.pi * f[i, 0, 9:12].astype(np.float64))
        assert np.abs(A - B).max() < 1e-6
    assert R.rotation_error(R.derotate_records(rec, table, np.float32), out) < 1e-5


# ---- 3. the rectified window is the rotated camera's picture ----
def grey_i420(mask):
    """a binary mask as a grey I420 frame: Y 235 inside, 16 outside, neutral chroma"""
    h, w = mask.shape
    return np.concatenate([np.where(mask, 235, 16).astype(np.uint8).ravel(), np.full(h * w // 2, 128, np.uint8)])


def render_mask(pose_R, pose_t, fx, fy, cx, cy, h, w):
    """tests/_render.py's rasteriser; ITS convention: pixel index i covers [i, i + 1) and is sampled at i + 0.5, so a principal point stated
    in pixel-index coordinates (index i sits AT coordinate i, this project's camera rows and the chain of tests/_rectify.py) is passed + 0.5"""
    v, f = RD.cube(0.085)
    verts, faces, start = RD.concat([(v, f)])
    poses = np.zeros((1, 1, 16))
    poses[0, 0] = RD.pose_row(0, 255, pose_R, pose_t)
    out = RD.render_models(poses, np.array([[fx, fy, cx + 0.5, cy + 0.5, 1.0]]), verts, faces, start, h, w)
    return out["mask"][0] != 0


def band_of(mask):
    """within one pixel of the silhouette's edge: the 3 x 3 neighbourhood holds both inside and outside (the frame's border replicated)"""
    p = np.pad(mask, 1, mode="edge")
    stack = np.stack([p[1 + dy: p.shape[0] - 1 + dy, 1 + dx: p.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    return stack.any(axis=0) & ~stack.all(axis=0)


def test_the_rectified_window_is_the_rotated_cameras_picture_and_the_plain_window_is_not():
    h, w, crop, rs = 96, 128, 48, 96
    cam = np.array([[100.0, 99.0, 47.0, 48.25, 1000.0, 1.0]], np.float32)        # resized-window pixels: 50 frame pixels of focal length
    window = np.array([[0, 70, 34]], np.int32)                                   # ox_c = 40, oy_c = 24: about 30 degrees off axis
    row = R.rectify_windows(cam, window, h, w, crop, rs)[0]
    Rw = row[:9].reshape(3, 3)
    assert 28.0 < np.degrees(np.arccos(Rw[2, 2])) < 35.0
    fx, fy, px, py = (float(v) for v in cam[0, :4])
    s = rs / crop
    pose_R, pose_t = RD.rotation((1, 2, 3), 0.9), Rw[:, 2] * 0.5 + np.array([0.004, -0.003, 0.0])      # on the window's ray, half a unit away
    # the frame camera in frame pixel-index coordinates: X_f = (u' + 0.5) / s - 0.5 + ox_c
    frame_mask = render_mask(pose_R, pose_t, fx / s, fy / s, (px + 0.5) / s - 0.5 + (w - crop) // 2, (py + 0.5) / s - 0.5 + (h - crop) // 2, h, w)
    assert 200 < frame_mask.sum() and not frame_mask[0].any() and not frame_mask[-1].any() and not frame_mask[:, 0].any() and not frame_mask[:, -1].any()
    frame = grey_i420(frame_mask)[None]
    # the direct render: the rotated camera, the centre intrinsics at crop resolution, x = (u + 0.5) / s - 0.5
    direct = render_mask(Rw.T @ pose_R, Rw.T @ pose_t, fx / s, fy / s, (px + 0.5) / s - 0.5, (py + 0.5) / s - 0.5, crop, crop)
    band = band_of(direct)
    rectified = R.rectified_crops(frame, h, w, window, row[None], crop, rs)[0][..., 0] >= 128
    plain = W.D.yv12_to_bgr(frame[0], h, w)[34:34 + crop, 70:70 + crop, 0] >= 128
    diff_r, diff_p = rectified != direct, plain != direct
    print(f"silhouette {int(direct.sum())} px, band {int(band.sum())} px; rectified differs at {int(diff_r.sum())} px, outside the band {int((diff_r & ~band).sum())}; "
          f"plain differs at {int(diff_p.sum())} px, outside the band {int((diff_p & ~band).sum())}")
    assert 200 < direct.sum() < crop * crop // 2
    assert not (diff_r & ~band).any()
    assert (diff_p & ~band).sum() >= 20                               # the effect the rectification removes
