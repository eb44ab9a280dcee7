"""Whole-frame search on the device (hep_preprocess_i420_windows_device, hep_best_window_device, hep_pose_from_i420_windows,
hep_pose_from_i420_tiled, hep_poses_from_i420_tiled) against the numpy definitions of tests/_windows.py and against the calls they compose,
bit for bit: no tolerances anywhere.  Sessions: phi 0 at size 128, fp32, max_batch 12; one with seeded 3-class weights for the per-label calls."""
import numpy as np
import pytest
import torch

from tests import _windows as W

pytestmark = pytest.mark.gpu

KEYS = ("found", "score", "label", "index", "box", "rotation", "translation", "hand")
CAM = [480.0, 470.0, 61.0, 66.0, 1000.0, 0.5]
H48, W64, CROP, RS = 48, 64, 32, 48              # the small geometry of tests 3, 4 and 6: a 3 x 2 grid has the even offsets {0, 16, 32} x {0, 16}


def cam_rows(B):
    return np.array([[CAM[0] + b, CAM[1], CAM[2], CAM[3] - b, CAM[4], CAM[5]] for b in range(B)], np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def thr_for_about_five(cls_image):
    """the sixth largest distinct score: the five values above it pass (more anchors where scores tie)"""
    return float(np.unique(cls_image.reshape(-1))[-6])


@pytest.fixture(scope="module")
def env():
    import hmd_ego_pose_amd as H
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd.model import Session
    from hmd_ego_pose_amd.weights import seeded_state_dict
    assert torch.cuda.is_available()
    return H, Session, seeded_state_dict, _capi


@pytest.fixture(scope="module")
def sess(env):
    _H, Session, sd_of, _capi = env
    s = Session(sd_of(0, 0), 0, 128, 12, "fp32")
    yield s
    s.close()


@pytest.fixture(scope="module")
def sess3(env):
    _H, Session, sd_of, _capi = env
    s = Session(sd_of(0, 0, num_classes=3), 0, 128, 12, "fp32")
    yield s
    s.close()


def make_scene(H, s, per_label):
    """2 frames of 48 x 64, the 3 x 2 grid, its cameras, and the records of hep_pose(s)_from_i420_windows at the thresholds of tests 3 and 4
    (computed once per session, never modified)"""
    rng = np.random.Generator(np.random.PCG64(48 + 64))
    frames = rng.integers(0, 256, (2, H48 * W64 * 3 // 2), dtype=np.uint8)
    cam = cam_rows(2)
    grid = H.tile_windows(H48, W64, CROP, 3, 2, 2)
    assert sorted(set(grid[:, 1].tolist())) == [0, 16, 32] and sorted(set(grid[:, 2].tolist())) == [0, 16]
    wcam = H.window_cameras(cam, grid, H48, W64, CROP, RS)
    xin = s.preprocess_i420_windows(torch.from_numpy(frames).cuda(), H48, W64, torch.from_numpy(grid).cuda(), CROP, RS)
    cls = s.forward(xin, want_features=False)[2].cpu().numpy()                      # [12, N, K]
    top = cls[:, :, 0].max(axis=1)                                                  # per-window top score (of label 0)
    order = np.sort(top[:6])[::-1]
    assert order[1] > order[2], "two windows of frame 0 tie for the second place: choose another seed"
    thr = {"five": thr_for_about_five(cls[0]), "zero": 0.0, "two": float(order[2]), "none": 2.0}
    assert int((top[:6] > np.float32(thr["two"])).sum()) == 2
    recs = {k: W.records_of(s.pose_from_i420_windows(frames, H48, W64, grid, wcam, CROP, RS, t, per_label=per_label)) for k, t in thr.items()}
    return dict(frames=frames, cam=cam, grid=grid, wcam=wcam, thr=thr, recs=recs)


@pytest.fixture(scope="module")
def scene(env, sess):
    return make_scene(env[0], sess, False)


@pytest.fixture(scope="module")
def scene3(env, sess3):
    return make_scene(env[0], sess3, True)


# ---- 1. the windowed preprocess, bit for bit against numpy ----
def preprocess_case(s, frames, h, w, windows, crop, rs):
    got = s.preprocess_i420_windows(torch.from_numpy(frames).cuda(), h, w, torch.from_numpy(windows).cuda(), crop, rs)
    assert tuple(got.shape) == (len(windows), 3, s.size, s.size)
    got = got.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    want = W.window_blobs(frames, h, w, windows, s.size, crop, rs)
    assert np.array_equal(bits(got), bits(want)), np.nonzero((bits(got) != bits(want)).reshape(len(windows), -1).any(axis=1))
    return got


def test_windowed_preprocess_small_frames_odd_offsets_and_a_hand_written_table(env, sess):
    H = env[0]
    h, w, crop, rs = 50, 66, 32, 48
    rng = np.random.Generator(np.random.PCG64(50 + 66))
    frames = rng.integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    # a: the 3 x 2 grid of both frames - an odd offset (17), both far edges (34, 18), both frames, n = max_batch
    grid = H.tile_windows(h, w, crop, 3, 2, 2)
    assert len(grid) == 12 and sorted(set(grid[:, 1].tolist())) == [0, 17, 34] and sorted(set(grid[:, 2].tolist())) == [0, 18]
    a = preprocess_case(sess, frames, h, w, grid, crop, rs)
    assert len({x.tobytes() for x in a}) == 12                                      # twelve different images: a mixed-up table would show
    # b: five windows, frames in reversed order, odd offsets on both axes, one window twice
    table = np.array([[1, 34, 18], [1, 5, 7], [0, 17, 0], [0, 17, 0], [0, 1, 17]], np.int32)
    b = preprocess_case(sess, frames, h, w, table, crop, rs)
    assert np.array_equal(b[2], b[3]) and np.array_equal(b[2], a[1]) and np.array_equal(b[0], a[11])
    # the centre window is the frame path
    centre = np.array([[0, (w - crop) // 2, (h - crop) // 2], [1, (w - crop) // 2, (h - crop) // 2]], np.int32)
    c = sess.preprocess_i420_windows(torch.from_numpy(frames).cuda(), h, w, torch.from_numpy(centre).cuda(), crop, rs)
    assert torch.equal(c, sess.preprocess_i420(torch.from_numpy(frames).cuda(), h, w, crop, rs))
    # the Python face checks what the ABI only sees as pointers
    with pytest.raises(ValueError):
        sess.preprocess_i420_windows(torch.from_numpy(frames).cuda(), h, w, torch.from_numpy(table), crop, rs)                 # table on the host
    with pytest.raises(ValueError):
        sess.preprocess_i420_windows(torch.from_numpy(frames).cuda(), h, w, torch.from_numpy(table).cuda().long(), crop, rs)
    with pytest.raises(ValueError):
        sess.preprocess_i420_windows(torch.from_numpy(frames).cuda(), h, w, torch.from_numpy(np.tile(table, (3, 1))).cuda(), crop, rs)   # 15 > max_batch


def test_windowed_preprocess_the_apps_geometry(env, sess):
    H = env[0]
    h, w, crop, rs = 504, 896, 256, 512
    frames = np.random.Generator(np.random.PCG64(504 + 896)).integers(0, 256, (1, h * w * 3 // 2), dtype=np.uint8)
    grid = H.tile_windows(h, w, crop, 4, 2, 1)
    assert grid[:, 1].tolist() == [0, 213, 426, 640] * 2 and grid[:, 2].tolist() == [0] * 4 + [248] * 4
    preprocess_case(sess, frames, h, w, grid, crop, rs)


# ---- 2. a 1 x 1 grid is today's call ----
@pytest.mark.parametrize("geom", [(48, 64, 32, 48), (300, 402, 200, 333)])
def test_a_1x1_grid_is_pose_from_i420(env, sess, geom):
    h, w, crop, rs = geom
    rng = np.random.Generator(np.random.PCG64(h + w))
    frames = rng.integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    cam = cam_rows(2)
    xin = sess.preprocess_i420(torch.from_numpy(frames).cuda(), h, w, crop, rs)
    thr = thr_for_about_five(sess.forward(xin, want_features=False)[2][0].cpu().numpy())
    for B in (1, 2):
        for t in (thr, 0.0, 2.0):
            p = sess.pose_from_i420(frames[:B], h, w, cam[:B], crop, rs, t)
            q = sess.pose_from_i420_tiled(frames[:B], h, w, cam[:B], crop, rs, 1, 1, t)
            for k in KEYS:
                assert q[k].dtype == p[k].dtype and q[k].shape == p[k].shape and np.array_equal(bits(q[k]), bits(p[k])), (geom, B, t, k)
            assert p["found"][0] == (t != 2.0)
            assert np.array_equal(q["window"], np.where(p["found"] == 1, np.arange(B), -1)), (geom, B, t)      # one frame: window == 0


# ---- 3. windows equal the composed path ----
@pytest.mark.parametrize("which", ["five", "zero"])
def test_windows_equal_pose_from_i420_on_host_cut_sub_frames(env, sess, scene, which):
    sc, t = scene, scene["thr"][which]
    subs = np.stack([W.cut_window_i420(sc["frames"][f], H48, W64, ox, oy, CROP) for f, ox, oy in sc["grid"]])
    want = W.records_of(sess.pose_from_i420(subs, CROP, CROP, sc["wcam"], CROP, RS, t))      # a crop x crop frame: its centre crop is all of it
    got = sc["recs"][which]
    assert got.shape == (12, W.RECORD_WORDS) and np.array_equal(got, want), np.nonzero((got != want).any(axis=1))
    assert got[0, 0] == 1 and (which != "zero" or (got[:, 0] == 1).all())


# ---- 4. the tiled call equals the rule ----
def tiled_case(s, sc, which, per_label):
    t = sc["thr"][which]
    call = s.poses_from_i420_tiled if per_label else s.pose_from_i420_tiled
    got = call(sc["frames"], H48, W64, sc["cam"], CROP, RS, 3, 2, t)
    recs = sc["recs"][which]
    want, win = W.best_window_rule(recs if per_label else recs[:, None, :], sc["grid"], 2)
    if not per_label:
        want, win = want[:, 0], win[:, 0]
    assert got["window"].dtype == np.int32 and np.array_equal(got["window"], win), (which, got["window"], win)
    assert np.array_equal(W.records_of(got), want), which
    return got


@pytest.mark.parametrize("which", ["two", "none", "zero"])
def test_tiled_equals_the_best_of_rule(env, sess, scene, which):
    got = tiled_case(sess, scene, which, False)
    top = scene["recs"]["zero"].view(np.float32)[:, 4]
    if which == "none":
        assert (got["found"] == 0).all() and (got["window"] == -1).all() and (got["index"] == -1).all() and (got["label"] == -1).all()
        assert all((got[k] == -1).all() for k in ("score", "box", "rotation", "translation", "hand"))
    else:
        assert int((scene["recs"][which][:6, 0] == 1).sum()) == (2 if which == "two" else 6)      # exactly two windows of frame 0 have a candidate
        assert got["found"][0] == 1 and got["window"][0] == int(np.argmax(top[:6]))
        if which == "zero":
            assert got["found"][1] == 1 and got["window"][1] == 6 + int(np.argmax(top[6:]))


@pytest.mark.parametrize("which", ["two", "none", "zero"])
def test_tiled_per_label_equals_the_best_of_rule_per_slot(env, sess3, scene3, which):
    got = tiled_case(sess3, scene3, which, True)
    assert got["found"].shape == (2, 3) and got["window"].shape == (2, 3) and got["hand"].shape == (2, 3, 63)
    if which == "none":
        assert (got["found"] == 0).all() and (got["window"] == -1).all()
    if which == "zero":
        assert (got["found"] == 1).all() and (got["window"][0] < 6).all() and (got["window"][1] >= 6).all()


# ---- 5. the reduction alone, on fabricated records ----
def fabricated(rng, n, slots, frame_of, levels):
    """random bit patterns in every word, found 0 / 1, scores from a few levels (ties everywhere)"""
    rec = rng.integers(-2 ** 31, 2 ** 31, (n, slots, W.RECORD_WORDS), dtype=np.int64).astype(np.int32)
    rec[..., 0] = rng.integers(0, 2, (n, slots))
    rec.view(np.float32)[..., 4] = rng.choice(np.asarray(levels, np.float32), (n, slots))
    windows = np.stack([np.asarray(frame_of), rng.integers(0, 100, n), rng.integers(0, 100, n)], axis=1).astype(np.int32)
    return rec, windows


def best_window_guarded(_capi, rec, windows, frames):
    """hep_best_window_device into the middle of guarded buffers -> (records, window); the guard words around both outputs stay intact"""
    n, slots = rec.shape[0], rec.shape[1]
    G, rows = 64, frames * slots
    out = torch.full((G + rows * W.RECORD_WORDS + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    win = torch.full((G + rows + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    r, w = torch.from_numpy(rec).cuda(), torch.from_numpy(windows).cuda()
    _capi.check(_capi.lib().hep_best_window_device(r.data_ptr(), slots, w.data_ptr(), n, frames, out.data_ptr() + 4 * G, win.data_ptr() + 4 * G,
                                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out, win = out.cpu().numpy(), win.cpu().numpy()
    for a in (out, win):
        assert (a[:G] == 0x5A5A5A5A).all() and (a[-G:] == 0x5A5A5A5A).all()
    return out[G:-G].reshape(frames, slots, W.RECORD_WORDS), win[G:-G].reshape(frames, slots)


def test_best_window_on_fabricated_records(env):
    _H, Session, _sd, _capi = env
    rng = np.random.Generator(np.random.PCG64(7))
    # 7 windows of the frames 0, 1 and 3, interleaved; frame 2 has no window at all
    rec, windows = fabricated(rng, 7, 3, [0, 1, 3, 0, 1, 3, 1], [0.25, 0.5, 0.75])
    f = rec.view(np.float32)
    rec[[1, 4, 6], 0, 0] = 1; f[1, 0, 4] = f[4, 0, 4] = 0.875; f[6, 0, 4] = 0.5       # frame 1, slot 0: windows 1 and 4 share the best score
    rec[[2, 5], 1, 0] = 0                                                             # frame 3, slot 1: nothing found
    rec[0, 2, 0], rec[3, 2, 0] = 1, 1; f[0, 2, 4], f[3, 2, 4] = 0.25, 0.75            # frame 0, slot 2: the later window is better
    want, wwin = W.best_window_rule(rec, windows, 4)
    assert wwin[1, 0] == 1 and wwin[3, 1] == -1 and wwin[0, 2] == 3 and (wwin[2] == -1).all()
    got, gwin = best_window_guarded(_capi, rec, windows, 4)
    assert np.array_equal(gwin, wwin) and np.array_equal(got, want)
    assert np.array_equal(got[1, 0], rec[1, 0]) and np.array_equal(got[2, 1], W.not_found_record())
    # the Python face: [n,K,80] and [n,80] records
    r, w = torch.from_numpy(rec).cuda(), torch.from_numpy(windows).cuda()
    o, wi = Session.best_window(r, w, 4)
    assert np.array_equal(o.cpu().numpy(), want) and np.array_equal(wi.cpu().numpy(), wwin)
    o1, wi1 = Session.best_window(r[:, 1].contiguous(), w, 4)
    assert tuple(o1.shape) == (4, W.RECORD_WORDS) and np.array_equal(o1.cpu().numpy(), want[:, 1]) and np.array_equal(wi1.cpu().numpy(), wwin[:, 1])
    with pytest.raises(ValueError):
        Session.best_window(r, w[:6], 4)
    with pytest.raises(ValueError):
        Session.best_window(r.float(), w, 4)
    # more windows than a wave has lanes (a lane then holds several), negative scores, signed zeros, ties across lanes
    rec, windows = fabricated(rng, 150, 2, rng.integers(0, 5, 150), [-0.5, -0.0, 0.0, 0.25, 0.75])
    want, wwin = W.best_window_rule(rec, windows, 6)
    got, gwin = best_window_guarded(_capi, rec, windows, 6)
    assert np.array_equal(gwin, wwin) and np.array_equal(got, want) and (wwin[5] == -1).all() and (wwin[:5] >= 0).all()


# ---- 6. steady state and recovery ----
def test_steady_state_allocates_nothing_and_a_refused_call_is_followed_by_a_good_one(env, sess, sess3, scene, scene3):
    _H, _S, _sd, _capi = env
    l = _capi.lib()

    def all_calls():
        for s, sc, pl in ((sess, scene, False), (sess3, scene3, True)):
            s.pose_from_i420_windows(sc["frames"], H48, W64, sc["grid"], sc["wcam"], CROP, RS, 0.5, per_label=pl)
            (s.poses_from_i420_tiled if pl else s.pose_from_i420_tiled)(sc["frames"], H48, W64, sc["cam"], CROP, RS, 3, 2, 0.5)
    all_calls()                                                                       # warm: every buffer exists
    torch.cuda.synchronize()
    before, free = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
    for _ in range(3):
        all_calls()
    assert torch.cuda.memory_allocated() == before and torch.cuda.mem_get_info()[0] == free
    # refused: 2 frames x 4 x 2 = 16 windows > max_batch 12, before any HIP call
    fr, cam = scene["frames"], scene["cam"]
    found, window = np.zeros(2, np.int32), np.zeros(2, np.int32)
    for fn, rest in ((l.hep_pose_from_i420_tiled, 7), (l.hep_poses_from_i420_tiled, 6)):
        assert l.hep_anchors(100, None, None) < 0                                     # another message in between
        assert fn(sess.handle, fr.ctypes.data, 2, H48, W64, CROP, RS, 4, 2, cam.ctypes.data, 0.5, found.ctypes.data, *([None] * rest), window.ctypes.data) == -1
        assert b"frames * nx * ny outside 1..max_batch" in l.hep_last_error(), l.hep_last_error()
    big = np.zeros((13, 3), np.int32)
    assert l.hep_pose_from_i420_windows(sess.handle, fr.ctypes.data, 2, H48, W64, big.ctypes.data, 13, CROP, RS, cam.ctypes.data, 0.5, found.ctypes.data,
                                        *([None] * 7)) == -1 and b"n outside 1..max_batch" in l.hep_last_error()
    with pytest.raises(ValueError):
        sess.pose_from_i420_tiled(fr, H48, W64, cam, CROP, RS, 4, 2, 0.5)
    with pytest.raises(ValueError):
        sess.pose_from_i420_windows(fr, H48, W64, np.array([[0, 33, 0]], np.int32), scene["wcam"][:1], CROP, RS, 0.5)      # ox past width - crop
    with pytest.raises(ValueError):
        sess.pose_from_i420_windows(fr, H48, W64, scene["grid"], scene["wcam"][:11], CROP, RS, 0.5)                        # a camera row per window
    tiled_case(sess, scene, "two", False)                                             # a good call still equals test 4's result
    tiled_case(sess3, scene3, "zero", True)
