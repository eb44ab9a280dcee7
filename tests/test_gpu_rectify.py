"""Rectified windows of the whole-frame search on the device (hep_preprocess_i420_rectified_device, hep_derotate_records_device and the four
*_rectified one-call forms) against the numpy definition of tests/_rectify.py and against the calls they compose.  Everything is compared bit
for bit except the rotation words of the back-rotation, whose two Rodrigues conversions go through sin / cos / atan2: those are compared as
matrices, GPU error against the float64 definition <= 4 x the error of the same definition evaluated in float32 numpy (the rule of
tests/test_gpu_augment.py).  Measured on the MI355X: GPU 0.0 (every rotation word equals the definition's), float32 4.5e-07 and 2.2e-06 on generic
rows, 1.4e-01 with the rows near pi (NOTEBOOK section 41).
Sessions: phi 0 at size 128, fp32, max_batch 12, as tests/test_gpu_windows.py; a short focal length puts the border windows about 30 degrees
off axis, where their footprints leave the frame."""
import numpy as np
import pytest
import torch

from tests import _rectify as R
from tests import _windows as W

pytestmark = pytest.mark.gpu

KEYS = ("found", "score", "label", "index", "box", "rotation", "translation", "hand")
H50, W66, H48, W64, CROP, RS = 50, 66, 48, 64, 32, 48
CAM = np.array([[40.25, 43.5, 25.75, 21.5, 1000.0, 0.375], [39.5, 42.75, 22.25, 26.0, 1000.0, 0.375]], np.float32)
TABLE = np.array([[1, 34, 18], [1, 5, 7], [0, 17, 0], [0, 17, 0], [0, 1, 17]], np.int32)      # odd offsets, frames out of order, one window twice


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


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


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 4. the rectified preprocess, bit for bit against numpy ----
def preprocess_case(s, frames, h, w, windows, table, crop, rs):
    got = s.preprocess_i420_rectified(cuda(frames), h, w, cuda(windows), cuda(table), crop, rs)
    assert tuple(got.shape) == (len(windows), 3, s.size, s.size)
    got = got.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    want = R.rectified_blobs(frames, h, w, windows, table, s.size, crop, rs)
    assert np.array_equal(bits(got), bits(want)), np.nonzero((bits(got) != bits(want)).reshape(len(windows), -1).any(axis=1))
    return got


def test_rectified_preprocess_equals_the_definition_bit_for_bit(env, sess):
    H = env[0]
    h, w, crop, rs = H50, W66, CROP, RS
    rng = np.random.Generator(np.random.PCG64(50 + 66))
    frames = rng.integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    # a: the 3 x 2 grid of both frames (n = max_batch); the footprints of the border windows leave the frame: clamped taps
    grid = H.tile_windows(h, w, crop, 3, 2, 2)
    table = H.rectify_windows(CAM, grid, h, w, crop, rs)
    Xf, Yf, _ = R.source_points(table[0], np.arange(crop, dtype=np.float64), np.arange(crop, dtype=np.float64), h, w, crop, rs, crop)
    assert Xf.min() < -1 and Yf.min() < -1                          # the top-left window looks past the frame's corner
    a = preprocess_case(sess, frames, h, w, grid, table, crop, rs)
    assert len({x.tobytes() for x in a}) == 12
    # ... and differs from the plain windows everywhere but at the centre column's middle (there is none in a 3 x 2 grid: all differ)
    plain = W.window_blobs(frames, h, w, grid, sess.size, crop, rs)
    assert all(not np.array_equal(a[i], plain[i]) for i in range(12))
    # b: the hand-written table
    tb = H.rectify_windows(CAM, TABLE, h, w, crop, rs)
    b = preprocess_case(sess, frames, h, w, TABLE, tb, crop, rs)
    assert np.array_equal(b[2], b[3]) and np.array_equal(b[0], a[11])
    # c: fabricated rows - a 120 degree rotation about (1, 1, 1) (x -> y -> z -> x: p_z = q_y, so the rows above the principal point are
    #    black and every other pixel takes clamped taps), a row of NaNs (all black), an infinite focal length; none reads outside the frame
    rows = np.stack([tb[0], tb[0], tb[0]])
    rows[0, :9] = [0, 0, 1, 1, 0, 0, 0, 1, 0]
    rows[1, :] = np.nan
    rows[2, 9] = np.inf
    fab = np.array([[0, 0, 0], [1, 3, 3], [1, 34, 18]], np.int32)
    crops = R.rectified_crops(frames, h, w, fab, rows, crop, rs)
    black = (crops[0] == 0).all(axis=2)
    assert black[:14].all() and not black[16:].all() and (crops[1] == 0).all()
    c = preprocess_case(sess, frames, h, w, fab, rows, crop, rs)
    assert np.isfinite(c).all()
    zero = ((np.float32(0) / np.float32(255) - np.array([0.485, 0.456, 0.406], np.float32)) / np.array([0.229, 0.224, 0.225], np.float32)).astype(np.float32)
    assert np.array_equal(c[1][:100, :100], np.broadcast_to(zero, (100, 100, 3)))
    torch.cuda.synchronize()
    # d: the centre windows are the frame path
    centre = np.array([[0, (w - crop) // 2, (h - crop) // 2], [1, (w - crop) // 2, (h - crop) // 2]], np.int32)
    tc = H.rectify_windows(CAM, centre, h, w, crop, rs)
    d = sess.preprocess_i420_rectified(cuda(frames), h, w, cuda(centre), cuda(tc), crop, rs)
    assert torch.equal(d, sess.preprocess_i420(cuda(frames), h, w, crop, rs))
    # the Python face checks what the ABI only sees as pointers
    with pytest.raises(ValueError):
        sess.preprocess_i420_rectified(cuda(frames), h, w, cuda(TABLE), torch.from_numpy(tb), crop, rs)               # table on the host
    with pytest.raises(ValueError):
        sess.preprocess_i420_rectified(cuda(frames), h, w, cuda(TABLE), cuda(tb).float(), crop, rs)
    with pytest.raises(ValueError):
        sess.preprocess_i420_rectified(cuda(frames), h, w, cuda(TABLE), cuda(tb[:4]), crop, rs)


def test_rectified_preprocess_second_geometry_with_an_upscale_and_equal_sides(env, sess):
    """48 x 64 (even offsets, resized / crop = 1.5) and a geometry whose resize is the identity (resized == crop)"""
    H = env[0]
    rng = np.random.Generator(np.random.PCG64(48 + 64))
    frames = rng.integers(0, 256, (2, H48 * W64 * 3 // 2), dtype=np.uint8)
    grid = H.tile_windows(H48, W64, CROP, 3, 2, 2)
    preprocess_case(sess, frames, H48, W64, grid, H.rectify_windows(CAM, grid, H48, W64, CROP, RS), CROP, RS)
    cam = CAM.copy()
    cam[:, :4] *= np.float32(40 / 48)
    odd = np.array([[1, 23, 7], [0, 0, 8], [0, 12, 4]], np.int32)
    preprocess_case(sess, frames, H48, W64, odd, H.rectify_windows(cam, odd, H48, W64, 40, 40), 40, 40)


# ---- 5. the back-rotation alone, on fabricated records ----
def test_derotate_records_on_fabricated_records(env):
    H, Session, _sd, _capi = env
    rng = np.random.Generator(np.random.PCG64(5))
    n = 70                                                            # not a multiple of 64
    windows = np.stack([rng.integers(0, 2, n), rng.integers(0, W66 - CROP + 1, n), rng.integers(0, H50 - CROP + 1, n)], axis=1).astype(np.int32)
    windows[3, 1:] = [17, 9]                                          # a centre window among them: the identity row
    table = R.rectify_windows(CAM, windows, H50, W66, CROP, RS)
    table[6, :9] = [1, 0, 0, 0, -1, 0, 0, 0, -1]                      # fabricated rows: a half turn about x and a turn by 1e-11 about z - with a zero
    table[7, :9] = [1, -1e-11, 0, 1e-11, 1, 0, 0, 0, 1]              # rotation in the record they reach the conversion's branches at pi and at 0
    errs = {}
    for slots in (1, 3):
        rec = rng.integers(-2 ** 31, 2 ** 31, (n, slots, R.RECORD_WORDS), dtype=np.int64).astype(np.int32)
        f = rec.view(np.float32)
        f[..., 12:78] = rng.uniform(-2.0, 2.0, (n, slots, 66)).astype(np.float32)
        rec[..., 0] = rng.choice(np.array([1, 1, 1, 0, 2, -1], np.int32), (n, slots))
        rec[:8, :, 0] = 1
        axis = rng.standard_normal((n, slots, 3))
        axis /= np.linalg.norm(axis, axis=2, keepdims=True)
        angle = rng.uniform(0.05, 3.0, (n, slots))                    # generic ...
        angle[0] = 0.0                                                # ... exactly 0,
        angle[1] = 1e-7                                               # near 0,
        angle[2] = np.pi - 5e-7                                       # within 1e-6 of pi as the record holds it,
        f[..., 9:12] = (axis * angle[..., None] / np.pi).astype(np.float32)
        f[3, :, 9:12] = [1.0, 0.0, 0.0]                               # the identity row: untouched whatever it holds
        f[4, :, 9:12] = [0.0, 1.0, 0.0]                               # exactly pi about y under a real R_w
        f[6:8, :, 9:12] = 0.0
        for c in range(slots):                                        # and a result within 1e-6 of pi: R_w^T applied to a rotation by pi - 4e-7
            Rw = table[5, :9].reshape(3, 3)
            f[5, c, 9:12] = (R.matrix_to_axis_angle(Rw.T @ R.axis_angle_to_matrix(axis[5, c] * (np.pi - 4e-7))) / np.pi).astype(np.float32)
        want, want32 = R.derotate_records(rec, table), R.derotate_records(rec, table, np.float32)
        r = cuda(rec if slots > 1 else rec[:, 0])
        out = Session.derotate_records(r, cuda(table))
        assert out.data_ptr() == r.data_ptr()                         # in place
        got = out.cpu().numpy().reshape(n, slots, R.RECORD_WORDS)
        other = np.r_[0:9, 12:80]
        assert np.array_equal(got[..., other], want[..., other]), np.nonzero((got[..., other] != want[..., other]).any(axis=2))
        untouched = (rec[..., 0] != 1)
        untouched[(table[:, :9] == np.eye(3).reshape(9)).all(axis=1)] = True      # row 3, and any other draw of the centre window
        assert np.array_equal(got[untouched], rec[untouched]) and untouched.sum() > 10 and (~untouched).sum() > 30
        assert not np.array_equal(got[~untouched][:, 12:78], rec[~untouched][:, 12:78])
        moved = ~untouched
        moved[[0, 6, 7]] = False                                      # (a zero rotation under a real R_w moves too, but rows 6 and 7 barely)
        assert (got[moved][:, 9:12] != rec[moved][:, 9:12]).any(axis=1).all()
        # the rule, on the generic rows alone (angles in 0.05..3.0) and on all rows: the float32 evaluation loses the axis near pi, which
        # makes its error - the yardstick - large there; the generic rows keep the bound meaningful
        for name, rows in (("generic", slice(8, None)), ("all", slice(None))):
            e, b = R.rotation_error(got[rows], want[rows]), R.rotation_error(want32[rows], want[rows])
            errs[(slots, name)] = (e, b)
            print(f"derotate slots {slots}, {name} rows: rotation as matrices, GPU vs float64 definition {e:.3e}; float32 definition {b:.3e}")
    for key, (e, b) in errs.items():
        assert e <= 4 * b, (key, e, b)
    # the Python face
    with pytest.raises(ValueError):
        Session.derotate_records(cuda(rec), cuda(table[:-1]))
    with pytest.raises(ValueError):
        Session.derotate_records(cuda(rec).float(), cuda(table))
    with pytest.raises(ValueError):
        Session.derotate_records(cuda(rec), cuda(table).float())


# ---- 6. a rectified 1 x 1 grid is today's call ----
@pytest.mark.parametrize("geom", [(48, 64, 32, 48), (300, 402, 200, 333)])
def test_a_rectified_1x1_grid_is_pose_from_i420(env, sess, geom):
    h, w, crop, rs = geom
    rng = np.random.Generator(np.random.PCG64(h + w))
    frames = rng.integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    cam = CAM.copy()
    cam[:, :4] *= np.float32(rs / RS)
    xin = sess.preprocess_i420(cuda(frames), h, w, crop, rs)
    thr = float(np.unique(sess.forward(xin, want_features=False)[2][0].cpu().numpy().reshape(-1))[-6])
    for B in (1, 2):
        for t in (thr, 0.0, 2.0):
            p = sess.pose_from_i420(frames[:B], h, w, cam[:B], crop, rs, t)
            q = sess.pose_from_i420_tiled(frames[:B], h, w, cam[:B], crop, rs, 1, 1, t, rectified=True)
            for k in KEYS:
                assert q[k].dtype == p[k].dtype and q[k].shape == p[k].shape and np.array_equal(bits(q[k]), bits(p[k])), (geom, B, t, k)
            assert p["found"][0] == (t != 2.0)
            assert np.array_equal(q["window"], np.where(p["found"] == 1, np.arange(B), -1)), (geom, B, t)


# ---- 7. the one-call forms equal their own composition ----
def make_scene(H, s, per_label):
    """2 frames of 48 x 64, the 3 x 2 grid, its table and the thresholds that leave five, two and no windows with a detection"""
    rng = np.random.Generator(np.random.PCG64(48 + 64 + 1))
    frames = rng.integers(0, 256, (2, H48 * W64 * 3 // 2), dtype=np.uint8)
    grid = H.tile_windows(H48, W64, CROP, 3, 2, 2)
    table = H.rectify_windows(CAM, grid, H48, W64, CROP, RS)
    xin = s.preprocess_i420_rectified(cuda(frames), H48, W64, cuda(grid), cuda(table), CROP, RS)
    heads = tuple(t.clone() for t in s.forward(xin, want_features=False)[1:6])
    top = np.sort(heads[1].cpu().numpy()[:, :, 0].max(axis=1))[::-1]              # per-window top score (of label 0), descending
    assert top[1] > top[2] and top[4] > top[5], "two windows tie at a threshold: choose another seed"
    thr = {"five": float(top[5]), "two": float(top[2]), "none": 2.0}
    return dict(frames=frames, grid=grid, table=table, heads=heads, thr=thr)


@pytest.fixture(scope="module")
def scene(env, sess):
    return make_scene(env[0], sess, False)


@pytest.fixture(scope="module")
def scene3(env, sess3):
    return make_scene(env[0], sess3, True)


def composed(Session, s, sc, t, per_label):
    """rectify_windows -> preprocess_i420_rectified -> forward (the scene's heads) -> top1 / top_labels with the CENTRE rows -> derotate_records
    -> best_window"""
    centre_rows = cuda(CAM[sc["grid"][:, 0]])
    top = (s.top_labels if per_label else s.top1)(centre_rows, t, heads=sc["heads"])
    before = top["record"].clone()
    rec = Session.derotate_records(top["record"], cuda(sc["table"]))
    best, win = Session.best_window(rec, cuda(sc["grid"]), 2)
    return before.cpu().numpy(), rec.cpu().numpy(), best.cpu().numpy(), win.cpu().numpy()


def one_call_case(env, s, sc, which, per_label):
    H, Session, _sd, _capi = env
    t = sc["thr"][which]
    before, rec, best, win = composed(Session, s, sc, t, per_label)
    found = before[..., 0].reshape(12, -1)[:, 0] == 1
    assert int(found.sum()) == {"five": 5, "two": 2, "none": 0}[which]
    if which != "none":                                               # the back-rotation did something, and only to rotation, translation and hand
        assert not np.array_equal(rec, before) and np.array_equal(rec[..., :9], before[..., :9])
    got = s.pose_from_i420_windows(sc["frames"], H48, W64, sc["grid"], CAM, CROP, RS, t, per_label=per_label, rectified=True)
    assert np.array_equal(W.records_of(got), rec), which
    tiled = (s.poses_from_i420_tiled if per_label else s.pose_from_i420_tiled)(sc["frames"], H48, W64, CAM, CROP, RS, 3, 2, t, rectified=True)
    assert tiled["window"].dtype == np.int32 and np.array_equal(tiled["window"], win), (which, tiled["window"], win)
    assert np.array_equal(W.records_of(tiled), best), which
    # the definition agrees: bit for bit outside the rotation words, the rotation by the matrix rule
    want = R.derotate_records(before, sc["table"])
    other = np.r_[0:9, 12:80]
    assert np.array_equal(rec[..., other], want[..., other])
    assert R.rotation_error(rec, want) <= 4 * R.rotation_error(R.derotate_records(before, sc["table"], np.float32), want)
    return tiled


@pytest.mark.parametrize("which", ["five", "two", "none"])
def test_one_call_forms_equal_their_composition(env, sess, scene, which):
    tiled = one_call_case(env, sess, scene, which, False)
    if which == "none":
        assert (tiled["found"] == 0).all() and (tiled["window"] == -1).all() and all((tiled[k] == -1).all() for k in ("score", "box", "rotation", "translation", "hand"))
    else:
        assert tiled["found"].sum() >= 1


@pytest.mark.parametrize("which", ["five", "two", "none"])
def test_one_call_forms_per_label_equal_their_composition(env, sess3, scene3, which):
    tiled = one_call_case(env, sess3, scene3, which, True)
    assert tiled["found"].shape == (2, 3) and tiled["window"].shape == (2, 3) and tiled["hand"].shape == (2, 3, 63)


def test_rectified_and_plain_calls_differ_off_axis_and_share_the_centre_column(env, sess, scene):
    """what the rectification changes, shown: at threshold 0 every window finds something; the plain call's poses of the border windows differ
    from the rectified call's (another picture went in), and the default rectified=False is the plain call"""
    sc = scene
    wcam = env[0].window_cameras(CAM, sc["grid"], H48, W64, CROP, RS)
    plain = sess.pose_from_i420_windows(sc["frames"], H48, W64, sc["grid"], wcam, CROP, RS, 0.0)
    again = sess.pose_from_i420_windows(sc["frames"], H48, W64, sc["grid"], wcam, CROP, RS, 0.0, rectified=False)
    rect = sess.pose_from_i420_windows(sc["frames"], H48, W64, sc["grid"], CAM, CROP, RS, 0.0, rectified=True)
    assert all(np.array_equal(bits(plain[k]), bits(again[k])) for k in KEYS)
    assert (plain["found"] == 1).all() and (rect["found"] == 1).all()
    assert not np.array_equal(plain["rotation"], rect["rotation"]) and not np.array_equal(plain["score"], rect["score"])


# ---- 8. steady state and recovery ----
def test_steady_state_allocates_nothing_and_a_refused_call_is_followed_by_a_good_one(env, sess, sess3, scene, scene3):
    H, _S, _sd, _capi = env
    l = _capi.lib()

    def all_calls():
        for s, sc, pl in ((sess, scene, False), (sess3, scene3, True)):
            s.pose_from_i420_windows(sc["frames"], H48, W64, sc["grid"], CAM, CROP, RS, 0.5, per_label=pl, rectified=True)
            (s.poses_from_i420_tiled if pl else s.pose_from_i420_tiled)(sc["frames"], H48, W64, CAM, CROP, RS, 3, 2, 0.5, rectified=True)
            s.pose_from_i420_windows(sc["frames"], H48, W64, sc["grid"], H.window_cameras(CAM, sc["grid"], H48, W64, CROP, RS), CROP, RS, 0.5, per_label=pl)
    all_calls()                                                                       # warm: every buffer exists
    torch.cuda.synchronize()
    before, free = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
    for _ in range(3):
        all_calls()
    assert torch.cuda.memory_allocated() == before and torch.cuda.mem_get_info()[0] == free
    fr = scene["frames"]
    # refused before any HIP call: ox past width - crop, fx = 0, too many windows
    with pytest.raises(ValueError):
        sess.pose_from_i420_windows(fr, H48, W64, np.array([[0, 33, 0]], np.int32), CAM, CROP, RS, 0.5, rectified=True)
    found = np.zeros(12, np.int32)
    past = np.array([[0, 33, 0]], np.int32)
    assert l.hep_pose_from_i420_windows_rectified(sess.handle, fr.ctypes.data, 2, H48, W64, past.ctypes.data, 1, CROP, RS, CAM.ctypes.data, 0.5,
                                                  found.ctypes.data, *([None] * 7)) == -1 and b"outside the frame" in l.hep_last_error()
    bad = CAM.copy()
    bad[1, 0] = 0.0
    with pytest.raises(_capi.HepError, match="camera row 1: fx and fy must be finite and positive"):
        sess.pose_from_i420_windows(fr, H48, W64, scene["grid"], bad, CROP, RS, 0.5, rectified=True)
    with pytest.raises(_capi.HepError, match="camera row 1: fx and fy must be finite and positive"):
        sess.pose_from_i420_tiled(fr, H48, W64, bad, CROP, RS, 3, 2, 0.5, rectified=True)
    with pytest.raises(ValueError):
        sess.pose_from_i420_tiled(fr, H48, W64, CAM, CROP, RS, 4, 2, 0.5, rectified=True)                    # 16 windows > max_batch
    with pytest.raises(ValueError):
        sess.pose_from_i420_windows(fr, H48, W64, scene["grid"], CAM[:1], CROP, RS, 0.5, rectified=True)     # a camera row per FRAME
    with pytest.raises(ValueError):                                                                          # the table on the wrong device
        sess.preprocess_i420_rectified(cuda(fr), H48, W64, cuda(scene["grid"]), torch.from_numpy(scene["table"]), CROP, RS)
    one_call_case(env, sess, scene, "two", False)                                     # a good call still equals test 7's result
    one_call_case(env, sess3, scene3, "five", True)
