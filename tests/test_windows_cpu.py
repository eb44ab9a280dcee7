"""CPU (no GPU): the whole-frame search's entry points exist, its host arithmetic (hep_tile_windows, hep_window_cameras, hep_window_from_box)
equals the numpy definitions of tests/_windows.py, and every entry point refuses bad arguments before any HIP call with the named reason."""
import ctypes

import numpy as np
import pytest

import hmd_ego_pose_amd as H
from hmd_ego_pose_amd import _capi
from tests import _windows as W

NEW = ("hep_tile_windows", "hep_window_cameras", "hep_window_from_box", "hep_preprocess_i420_windows_device", "hep_best_window_device",
       "hep_pose_from_i420_windows", "hep_poses_from_i420_windows", "hep_pose_from_i420_tiled", "hep_poses_from_i420_tiled")
GEOMS = [(480, 640, 256), (504, 896, 256)]
GRIDS = [(1, 1), (3, 2), (4, 2), (6, 3)]


def test_the_nine_symbols_are_declared_bound_and_exported():
    import os
    l = _capi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hep.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name
        assert name in _capi.SYMBOLS and hasattr(l, name), name
    assert l.hep_abi_version() == 1                                 # additive: the ABI version stays


@pytest.mark.parametrize("geom", GEOMS + [(300, 256, 256), (50, 66, 32)])
@pytest.mark.parametrize("grid", GRIDS + [(1, 3)])
def test_tile_windows_equals_the_formula(geom, grid):
    (h, w, crop), (nx, ny) = geom, grid
    for frames in (1, 2):
        got = H.tile_windows(h, w, crop, nx, ny, frames)
        want = W.tile_windows(h, w, crop, nx, ny, frames)
        assert got.dtype == np.int32 and got.shape == (frames * ny * nx, 3) and np.array_equal(got, want), (geom, grid)
        g = got.reshape(frames, ny, nx, 3)
        assert (g[..., 0] == np.arange(frames)[:, None, None]).all()
        if nx > 1:                                                  # the outer cells touch the borders
            assert (g[:, :, 0, 1] == 0).all() and (g[:, :, -1, 1] == w - crop).all()
        else:
            assert (g[..., 1] == (w - crop) // 2).all()
        if ny > 1:
            assert (g[:, 0, :, 2] == 0).all() and (g[:, -1, :, 2] == h - crop).all()
        else:
            assert (g[..., 2] == (h - crop) // 2).all()
        assert (g[..., 1] >= 0).all() and (g[..., 1] <= w - crop).all() and (g[..., 2] >= 0).all() and (g[..., 2] <= h - crop).all()
    if grid == (1, 1):
        assert got[0].tolist() == [0, (w - crop) // 2, (h - crop) // 2]


def test_tile_windows_of_the_issue_offsets():
    assert sorted(set(H.tile_windows(50, 66, 32, 3, 2, 2)[:, 1].tolist())) == [0, 17, 34]
    assert sorted(set(H.tile_windows(50, 66, 32, 3, 2, 2)[:, 2].tolist())) == [0, 18]


@pytest.mark.parametrize("geom", [(480, 640, 256, 512), (504, 896, 256, 512), (50, 66, 32, 48), (300, 402, 201, 333), (48, 64, 32, 48)])
def test_window_cameras_equal_the_float64_statement_bit_for_bit(geom):
    h, w, crop, rs = geom                                          # (402 - 201 and 300 - 201 are odd: the centre is their floor)
    rng = np.random.Generator(np.random.PCG64(h + w))
    cam = np.stack([rng.uniform(300, 900, 3), rng.uniform(300, 900, 3), rng.uniform(-50, 700, 3), rng.uniform(-50, 700, 3),
                    np.full(3, 1000.0), rng.uniform(0.2, 2.0, 3)], axis=1).astype(np.float32)
    grid = W.tile_windows(h, w, crop, 4, 3, 3)
    rand = np.stack([rng.integers(0, 3, 40), rng.integers(0, w - crop + 1, 40), rng.integers(0, h - crop + 1, 40)], axis=1).astype(np.int32)
    centre = np.array([[f, (w - crop) // 2, (h - crop) // 2] for f in (2, 0, 1)], np.int32)
    for windows in (grid, rand, centre):
        got = H.window_cameras(cam, windows, h, w, crop, rs)
        want = W.window_cameras(cam, windows, h, w, crop, rs)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), geom
        assert np.array_equal(got[:, [0, 1, 4, 5]].view(np.int32), cam[windows[:, 0]][:, [0, 1, 4, 5]].view(np.int32))
    assert np.array_equal(H.window_cameras(cam, centre, h, w, crop, rs).view(np.int32), cam[[2, 0, 1]].view(np.int32))      # the centre window: unchanged
    assert len(np.unique(H.window_cameras(cam, grid, h, w, crop, rs)[:12, 2])) == 4                                          # ... the others move


def test_window_from_box_equals_numpy_and_clamps_at_all_four_borders():
    h, w, crop, size = 504, 896, 256, 512
    rng = np.random.Generator(np.random.PCG64(12))
    cases = []
    for _ in range(300):
        ox, oy = int(rng.integers(0, w - crop + 1)), int(rng.integers(0, h - crop + 1))
        c, half = rng.uniform(-40, size + 40, 2), rng.uniform(1, 120, 2)
        cases.append((np.concatenate([c - half, c + half]).astype(np.float32), ox, oy))
    # a box at each corner of the network input of a window at each corner of the frame: both clamps on both axes
    cases += [(np.array([0, 0, 8, 8], np.float32), 0, 0), (np.array([504, 504, 511, 511], np.float32), w - crop, h - crop),
              (np.array([0, 504, 8, 511], np.float32), 0, h - crop), (np.array([504, 0, 511, 8], np.float32), w - crop, 0),
              (np.array([255.5, 255.5, 256.5, 256.5], np.float32), 321, 123)]      # a box at the window's centre: the window stays
    for box, ox, oy in cases:
        got = H.window_from_box(box, ox, oy, h, w, crop, size)
        assert got == W.window_from_box(box, ox, oy, h, w, crop, size), (box, ox, oy)
        assert 0 <= got[0] <= w - crop and 0 <= got[1] <= h - crop
    assert H.window_from_box(cases[-1][0], 321, 123, h, w, crop, size) == (321, 123)
    assert H.window_from_box(cases[-5][0], 0, 0, h, w, crop, size) == (0, 0)
    assert H.window_from_box(cases[-4][0], w - crop, h - crop, h, w, crop, size) == (w - crop, h - crop)
    assert H.window_from_box(cases[-3][0], 0, h - crop, h, w, crop, size) == (0, h - crop)
    assert H.window_from_box(cases[-2][0], w - crop, 0, h, w, crop, size) == (w - crop, 0)
    # a detection right of the centre pulls the window right by its distance in frame pixels: (384 - 256) * 256 / 512 = 64
    assert H.window_from_box(np.array([374, 246, 394, 266], np.float32), 100, 100, h, w, crop, size) == (164, 100)


def test_every_entry_point_refuses_before_any_hip_call():
    """No device exists here: a call that reached HIP would fail with another code and another text.  Checks that do not read the handle come
    first, so a zeroed block stands in for one where a case needs a non-NULL handle (zeroed: max_batch reads as 0 and refuses, should the order
    ever change)."""
    l = _capi.lib()
    buf = np.zeros(4096, np.float32)
    a = buf.ctypes.data
    fake = np.zeros(1 << 16, np.uint8).ctypes.data
    inside = np.array([[0, 10, 10]], np.int32)
    outside = [np.array([[0, 385, 0]], np.int32), np.array([[0, 0, 225]], np.int32), np.array([[0, -1, 0]], np.int32), np.array([[1, 0, 0]], np.int32),
               np.array([[-1, 0, 0]], np.int32)]
    iw = inside.ctypes.data
    x, y = ctypes.c_int32(), ctypes.c_int32()
    rest8, rest7 = [None] * 7, [None] * 6

    def windows(h_, yuv=a, frames=1, hh=480, ww=640, win=iw, n=1, crop=256, cam=a, found=a, per_label=False):
        if per_label:
            return l.hep_poses_from_i420_windows(h_, yuv, frames, hh, ww, win, n, crop, 512, cam, 0.5, found, *rest7)
        return l.hep_pose_from_i420_windows(h_, yuv, frames, hh, ww, win, n, crop, 512, cam, 0.5, found, *rest8)

    def tiled(h_, yuv=a, frames=1, hh=480, ww=640, crop=256, nx=2, ny=2, cam=a, found=a, window=a, per_label=False):
        if per_label:
            return l.hep_poses_from_i420_tiled(h_, yuv, frames, hh, ww, crop, 512, nx, ny, cam, 0.5, found, *rest7, window)
        return l.hep_pose_from_i420_tiled(h_, yuv, frames, hh, ww, crop, 512, nx, ny, cam, 0.5, found, *rest8, window)

    def pre(h_, yuv=a, frames=1, hh=480, ww=640, win=a, n=1, crop=256, out=a):
        return l.hep_preprocess_i420_windows_device(h_, yuv, frames, hh, ww, win, n, crop, 512, out, None)

    cases = [
        # host arithmetic
        (lambda: l.hep_tile_windows(480, 640, 256, 2, 2, 1, None), b"hep_tile_windows: windows_out is NULL"),
        (lambda: l.hep_tile_windows(480, 640, 256, 0, 2, 1, a), b"nx must be >= 1"),
        (lambda: l.hep_tile_windows(480, 640, 256, 2, 0, 1, a), b"ny must be >= 1"),
        (lambda: l.hep_tile_windows(480, 640, 256, 2, 2, 0, a), b"frames must be >= 1"),
        (lambda: l.hep_tile_windows(481, 640, 256, 2, 2, 1, a), b"even"),
        (lambda: l.hep_tile_windows(480, 641, 256, 2, 2, 1, a), b"even"),
        (lambda: l.hep_tile_windows(480, 640, 482, 2, 2, 1, a), b"crop"),
        (lambda: l.hep_window_cameras(None, iw, 1, 480, 640, 256, 512, a), b"hep_window_cameras: camera is NULL"),
        (lambda: l.hep_window_cameras(a, None, 1, 480, 640, 256, 512, a), b"windows is NULL"),
        (lambda: l.hep_window_cameras(a, iw, 1, 480, 640, 256, 512, None), b"camera_out is NULL"),
        (lambda: l.hep_window_cameras(a, iw, 0, 480, 640, 256, 512, a), b"n must be >= 1"),
        (lambda: l.hep_window_cameras(a, iw, 1, 480, 642 - 1, 256, 512, a), b"even"),
        (lambda: l.hep_window_cameras(a, iw, 1, 480, 640, 642, 512, a), b"crop"),
        (lambda: l.hep_window_cameras(a, outside[0].ctypes.data, 1, 480, 640, 256, 512, a), b"outside the frame"),
        (lambda: l.hep_window_cameras(a, outside[4].ctypes.data, 1, 480, 640, 256, 512, a), b"outside the frame"),
        (lambda: l.hep_window_from_box(None, 0, 0, 480, 640, 256, 512, ctypes.byref(x), ctypes.byref(y)), b"hep_window_from_box: box is NULL"),
        (lambda: l.hep_window_from_box(a, 0, 0, 480, 640, 256, 512, None, ctypes.byref(y)), b"ox_out is NULL"),
        (lambda: l.hep_window_from_box(a, 0, 0, 480, 640, 256, 0, ctypes.byref(x), ctypes.byref(y)), b"size must be >= 1"),
        (lambda: l.hep_window_from_box(a, 0, 0, 481, 640, 256, 512, ctypes.byref(x), ctypes.byref(y)), b"even"),
        (lambda: l.hep_window_from_box(a, 0, 0, 480, 640, 482, 512, ctypes.byref(x), ctypes.byref(y)), b"crop"),
        (lambda: l.hep_window_from_box(a, 385, 0, 480, 640, 256, 512, ctypes.byref(x), ctypes.byref(y)), b"outside the frame"),
        # the device entry points
        (lambda: pre(None), b"hep_preprocess_i420_windows_device: handle is NULL"),
        (lambda: pre(fake, yuv=None), b"yuv is NULL"),
        (lambda: pre(fake, win=None), b"windows is NULL"),
        (lambda: pre(fake, out=None), b"out_hwc is NULL"),
        (lambda: pre(fake, frames=0), b"frames must be >= 1"),
        (lambda: pre(fake, hh=481), b"even"),
        (lambda: pre(fake, ww=641), b"even"),
        (lambda: pre(fake, crop=482), b"crop"),
        (lambda: l.hep_best_window_device(None, 1, a, 1, 1, a, a, None), b"hep_best_window_device: records is NULL"),
        (lambda: l.hep_best_window_device(a, 1, None, 1, 1, a, a, None), b"windows is NULL"),
        (lambda: l.hep_best_window_device(a, 1, a, 1, 1, None, a, None), b"out_records is NULL"),
        (lambda: l.hep_best_window_device(a, 1, a, 1, 1, a, None, None), b"out_window is NULL"),
        (lambda: l.hep_best_window_device(a, 0, a, 1, 1, a, a, None), b"slots outside 1..63"),
        (lambda: l.hep_best_window_device(a, 64, a, 1, 1, a, a, None), b"slots outside 1..63"),
        (lambda: l.hep_best_window_device(a, 1, a, 0, 1, a, a, None), b"n must be >= 1"),
        (lambda: l.hep_best_window_device(a, 1, a, 1, 0, a, a, None), b"frames outside"),
    ]
    for per_label in (False, True):
        pre_w = b"hep_poses_from_i420_windows: " if per_label else b"hep_pose_from_i420_windows: "
        pre_t = b"hep_poses_from_i420_tiled: " if per_label else b"hep_pose_from_i420_tiled: "
        k = dict(per_label=per_label)
        cases += [
            (lambda k=k: windows(None, **k), pre_w + b"handle is NULL"),
            (lambda k=k: windows(fake, yuv=None, **k), pre_w + b"yuv is NULL"),
            (lambda k=k: windows(fake, win=None, **k), b"windows is NULL"),
            (lambda k=k: windows(fake, cam=None, **k), b"camera is NULL"),
            (lambda k=k: windows(fake, found=None, **k), b"found is NULL"),
            (lambda k=k: windows(fake, n=0, **k), b"n outside 1..max_batch"),
            (lambda k=k: windows(fake, frames=0, **k), b"frames must be >= 1"),
            (lambda k=k: windows(fake, hh=481, **k), b"even"),
            (lambda k=k: windows(fake, ww=641, **k), b"even"),
            (lambda k=k: windows(fake, crop=482, **k), b"crop"),
            (lambda k=k: tiled(None, **k), pre_t + b"handle is NULL"),
            (lambda k=k: tiled(fake, yuv=None, **k), pre_t + b"yuv is NULL"),
            (lambda k=k: tiled(fake, cam=None, **k), b"camera is NULL"),
            (lambda k=k: tiled(fake, found=None, **k), b"found is NULL"),
            (lambda k=k: tiled(fake, window=None, **k), b"window is NULL"),
            (lambda k=k: tiled(fake, nx=0, **k), b"nx must be >= 1"),
            (lambda k=k: tiled(fake, ny=0, **k), b"ny must be >= 1"),
            (lambda k=k: tiled(fake, frames=0, **k), b"frames must be >= 1"),
            (lambda k=k: tiled(fake, hh=481, **k), b"even"),
            (lambda k=k: tiled(fake, ww=641, **k), b"even"),
            (lambda k=k: tiled(fake, crop=482, **k), b"crop"),
        ]
        cases += [(lambda k=k, o=o: windows(fake, win=o.ctypes.data, **k), b"outside the frame") for o in outside]
    for call, reason in cases:
        assert l.hep_anchors(100, None, None) < 0                   # another message in between: the text below is never a stale one
        assert call() == -1, reason                                 # HEP_ERR_INVALID
        assert reason in l.hep_last_error(), (reason, l.hep_last_error())
    # the Python face of the host arithmetic
    with pytest.raises(ValueError):
        H.tile_windows(480, 640, 256, 0, 1)
    with pytest.raises(_capi.HepError):
        H.tile_windows(480, 640, 700, 1, 1)
    with pytest.raises(ValueError):
        H.window_cameras(np.zeros((1, 6), np.float32), np.array([[1, 0, 0]], np.int32), 480, 640, 256, 512)      # no camera row for frame 1
    with pytest.raises(ValueError):
        H.window_cameras(np.zeros((1, 6), np.float32), np.array([[0, 0, 0]], np.int64), 480, 640, 256, 512)
    with pytest.raises(ValueError):
        H.window_from_box([1, 2, 3], 0, 0, 480, 640, 256, 512)


def test_best_window_rule_on_a_hand_made_table():
    """the numpy rule the GPU tests hold the launch to, on a case small enough to check by eye"""
    rec = np.tile(W.not_found_record(), (4, 1, 1))
    sc = rec.view(np.float32)
    for i, s in ((0, 0.5), (2, 0.75), (3, 0.75)):
        rec[i, 0, 0], rec[i, 0, 1], rec[i, 0, 2] = 1, 0, 100 + i
        sc[i, 0, 4] = s
    windows = np.array([[1, 0, 0], [0, 0, 0], [1, 2, 0], [1, 4, 0]], np.int32)
    out, win = W.best_window_rule(rec, windows, 3)
    assert win[:, 0].tolist() == [-1, 2, -1]                        # frame 0: its window found nothing; frame 1: the tie goes to window 2; frame 2: no window
    assert np.array_equal(out[1, 0], rec[2, 0]) and np.array_equal(out[0, 0], W.not_found_record()) and np.array_equal(out[2, 0], W.not_found_record())
