"""The top detection of every label (hep_top_labels_device, hep_poses_from_input, hep_poses_from_i420) against the chain it
replaces - decode + class-specific filter row 0 on the classification with every column but c masked out - and against the
numpy rule of tests/_top_labels.py, bit for bit: no tolerances anywhere.  Shapes: phi 0 at size 128 (N = 3069, no multiple of
the workgroup), max_batch 3, K = 1 / 3 / 63, one K = 3 session at size 256 (N = 12 276)."""
import threading

import numpy as np
import pytest
import torch

from tests._top1 import RECORD_WORDS, random_scores, record_of_row0
from tests._top_labels import best_over_labels, masked, rule_records

pytestmark = pytest.mark.gpu

KEYS = ("boxes", "scores", "labels", "rotation", "translation", "hand", "index")
CAM = [480.0, 470.0, 61.0, 66.0, 1000.0, 0.5]


@pytest.fixture(scope="module")
def env():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd.model import Session
    from hmd_ego_pose_amd.weights import seeded_state_dict
    assert torch.cuda.is_available()
    return Session, seeded_state_dict, _capi


@pytest.fixture(scope="module")
def sess(env):
    """fp32, phi 0 @ 128, three classes, max_batch 3, with one forward's scores of three frames (shared, never modified)."""
    Session, sd_of, _capi = env
    s = Session(sd_of(0, 0, num_classes=3), 0, 128, 3, "fp32")
    rng = np.random.Generator(np.random.PCG64(78))
    x = rng.standard_normal((3, 3, 128, 128)).astype(np.float32)
    cls = s.forward(torch.from_numpy(x).cuda(), want_features=False)[2].cpu().numpy()
    yield s, x, cls
    s.close()


def cam_rows(B):
    return np.array([[CAM[0] + b, CAM[1], CAM[2], CAM[3] - b, CAM[4], CAM[5]] for b in range(B)], np.float32)


def thr_for_about_five(cls_image):
    """the sixth largest distinct score of the image (all classes): the five values above it pass (more pairs where scores tie)"""
    return float(np.unique(cls_image.reshape(-1))[-6])


def masked_chain(s, heads, cam, thr, nms=0.5, M=100):
    """decode + class-specific filter on device tensors, once per class on the masked classification -> [B, K, 80] records of row 0"""
    reg, cls, rot, trn, hand = heads
    B, K = cls.shape[0], cls.shape[2]
    boxes, trans = s.decode(reg, trn, cam)
    out = np.zeros((B, K, RECORD_WORDS), np.int32)
    for c in range(K):
        m = torch.full_like(cls, -1.0)
        m[..., c] = cls[..., c]
        det = s.filter(boxes, m, rot, trans, hand, thr, nms, M, class_specific_filter=True)
        torch.cuda.synchronize()
        d = {k: v.cpu().numpy() for k, v in det.items()}
        for b in range(B):
            out[b, c] = record_of_row0(int(d["count"][b]), *[d[k][b] for k in KEYS])
    return out


def rule_chain(s, heads, cam, thr):
    """the numpy rule on the device decode's boxes and translations -> [B, K, 80] records"""
    reg, cls, rot, trn, hand = heads
    boxes, trans = s.decode(reg, trn, cam)
    torch.cuda.synchronize()
    a = [t.cpu().numpy() for t in (cls, boxes, rot, trans, hand)]
    return np.stack([rule_records(a[0][b], thr, a[1][b], a[2][b], a[3][b], a[4][b]) for b in range(cls.shape[0])])


def random_heads(rng, B, N, K, ncand, thr, drop=()):
    """random head outputs; image 0 loses every candidate of the classes in `drop` (some labels found, some not)"""
    cls = np.stack([random_scores(rng, N, K, ncand, thr, ties=True) for _ in range(B)])
    for c in drop:
        cls[0, :, c] = np.minimum(cls[0, :, c], np.float32(thr))                  # at or below the threshold: no candidate
    reg = (rng.standard_normal((B, N, 4)) * 0.4).astype(np.float32)
    trn = rng.standard_normal((B, N, 3)).astype(np.float32)
    rot = rng.standard_normal((B, N, 3)).astype(np.float32)
    hand = rng.standard_normal((B, N, 63)).astype(np.float32)
    return reg, cls, rot, trn, hand


@pytest.mark.parametrize("size,K", [(128, 1), (128, 3), (256, 3), (128, 63)])
def test_top_labels_fuzz_equals_masked_decode_and_filter_and_the_rule(env, size, K):
    Session, sd_of, _capi = env
    s = Session(sd_of(0, 0, num_classes=K), 0, size, 3, "fp32")
    N = s.num_anchors
    assert N % 1024 != 0 and s.num_classes == K
    rng = np.random.Generator(np.random.PCG64(2000 + size + K))
    t = lambda a: torch.from_numpy(a).cuda()
    counts = [50] if K == 63 else [0, 1, 2, 7, 50, N] if size == 128 else [7, N]
    mixed = False
    for case, ncand in enumerate(counts):
        B = 2 if K == 63 else case % 3 + 1
        thr = 0.5 if case % 2 else 0.05
        drop = tuple(range(5, 21)) if K == 63 else (1,) if K == 3 and case % 2 == 0 else ()
        np_heads = random_heads(rng, B, N, K, ncand, thr, drop)
        heads = tuple(t(a) for a in np_heads)
        cam = t(cam_rows(B))
        got = s.top_labels(cam, thr, heads=heads)
        torch.cuda.synchronize()
        rec = got["record"].cpu().numpy()
        assert rec.shape == (B, K, RECORD_WORDS)
        want = rule_chain(s, heads, cam, thr)
        assert np.array_equal(rec, want), (size, K, ncand, B, np.nonzero(rec != want))
        chain_on = slice(0, 1) if K == 63 else slice(0, B)                        # K = 63: the masked chain for image 0 only
        sub = tuple(h[chain_on] for h in heads)
        for M in (1, 100):
            for nms in (0.3, 0.9):
                want = masked_chain(s, sub, cam[chain_on], thr, nms, M)
                assert np.array_equal(rec[chain_on], want), (size, K, ncand, B, M, nms, np.nonzero(rec[chain_on] != want))
        found = rec[..., 0]
        assert set(np.unique(found)) <= {0, 1}
        assert np.array_equal(found == 1, (np_heads[1] > np.float32(thr)).any(axis=1))
        mixed |= bool(any(0 < found[b].sum() < K for b in range(B)))
        # the views of the record
        assert np.array_equal(got["found"].cpu().numpy(), rec[..., 0]) and np.array_equal(got["index"].cpu().numpy(), rec[..., 2])
        assert np.array_equal(got["score"].cpu().numpy().view(np.int32), rec[..., 4])
        assert np.array_equal(got["box"].cpu().numpy().view(np.int32), rec[..., 5:9])
        assert np.array_equal(got["rotation"].cpu().numpy().view(np.int32), rec[..., 9:12])
        assert np.array_equal(got["translation"].cpu().numpy().view(np.int32), rec[..., 12:15])
        assert np.array_equal(got["hand"].cpu().numpy().view(np.int32), rec[..., 15:78])
        assert (rec[..., 3] == 0).all() and (rec[..., 78:] == 0).all()
        assert np.array_equal(rec[..., 1], np.where(found == 1, np.arange(K)[None, :], -1))      # the label word is the slot
    assert K == 1 or mixed                                                         # an image with some labels found and some not
    s.close()


def test_one_class_equals_top1(env):
    Session, sd_of, _capi = env
    s = Session(sd_of(0, 0), 0, 128, 3, "fp32")
    rng = np.random.Generator(np.random.PCG64(31))
    for ncand, thr in ((0, 0.5), (7, 0.05), (s.num_anchors, 0.5)):
        heads = tuple(torch.from_numpy(a).cuda() for a in random_heads(rng, 3, s.num_anchors, 1, ncand, thr))
        cam = torch.from_numpy(cam_rows(3)).cuda()
        rec = s.top_labels(cam, thr, heads=heads)["record"]
        assert torch.equal(rec[:, 0], s.top1(cam, thr, heads=heads)["record"]), ncand
    s.close()


def test_three_classes_best_over_labels_is_top1_and_the_filter_mode_is_not_read(env, sess):
    _S, _sd, _capi = env
    s, _x, _cls = sess
    rng = np.random.Generator(np.random.PCG64(32))
    cam = torch.from_numpy(cam_rows(3)).cuda()
    try:
        for ncand, thr in ((0, 0.5), (2, 0.05), (50, 0.5), (s.num_anchors, 0.05)):
            heads = tuple(torch.from_numpy(a).cuda() for a in random_heads(rng, 3, s.num_anchors, 3, ncand, thr))
            rec = s.top_labels(cam, thr, heads=heads)["record"].cpu().numpy()
            top = s.top1(cam, thr, heads=heads, class_specific_filter=True)["record"].cpu().numpy()
            assert np.array_equal(np.stack([best_over_labels(rec[b]) for b in range(3)]), top), ncand
            # hep_set_class_specific_filter(h, 0): top1 changes its rule, the per-label records do not
            _capi.check(_capi.lib().hep_set_class_specific_filter(s.handle, 0))
            again = s.top_labels(cam, thr, heads=heads)["record"].cpu().numpy()
            _capi.check(_capi.lib().hep_set_class_specific_filter(s.handle, 1))
            assert np.array_equal(again, rec), ncand
    finally:
        _capi.check(_capi.lib().hep_set_class_specific_filter(s.handle, 1))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_top_labels_on_the_handles_own_outputs_after_a_forward(env, precision):
    Session, sd_of, _capi = env
    s = Session(sd_of(0, 0, num_classes=3), 0, 128, 3, precision)
    rng = np.random.Generator(np.random.PCG64(6))
    x = torch.from_numpy(rng.standard_normal((3, 3, 128, 128)).astype(np.float32)).cuda()
    for B in (3, 2):
        outs = s.forward(x[:B], want_features=False)[1:]
        cam = torch.from_numpy(cam_rows(B)).cuda()
        own = [v[:B] for v in s.output_views()]
        for a, b in zip(outs, own):
            assert torch.equal(a, b)
        for thr in (thr_for_about_five(outs[1][0].cpu().numpy()), 2.0):
            rec = s.top_labels(cam, thr)["record"].cpu().numpy()                  # NULL head pointers: the handle's buffers
            assert np.array_equal(rec, masked_chain(s, own, cam, thr)), (precision, B, thr)
            assert np.array_equal(rec, rule_chain(s, own, cam, thr)), (precision, B, thr)
            assert (rec[..., 0] == 0).all() == (thr == 2.0)
    s.close()


def records_of_poses(p):
    """the dict of numpy arrays of Session.poses_from_* as [B, K, 80] records"""
    B, K = p["found"].shape
    return np.stack([np.stack([record_of_row0(int(p["found"][b, c]), p["box"][b, c:c + 1], p["score"][b, c:c + 1],
                                              [c if p["found"][b, c] else -1], p["rotation"][b, c:c + 1], p["translation"][b, c:c + 1],
                                              p["hand"][b, c:c + 1], p["index"][b, c:c + 1]) for c in range(K)]) for b in range(B)])


def host_chain(s, _capi, x, cam, thr, M=100, nms=0.5):
    """hep_run -> hep_decode -> hep_filter per class on the masked classification, all on host arrays: [B, K, 80] records of row 0"""
    l = _capi.lib()
    B, N, K = x.shape[0], s.num_anchors, s.num_classes
    ho = [np.empty((B, N, k), np.float32) for k in s.out_width]
    hb, ht = np.empty((B, N, 4), np.float32), np.empty((B, N, 3), np.float32)
    det = [np.empty((B, M, 4), np.float32), np.empty((B, M), np.float32), np.empty((B, M), np.int32), np.empty((B, M, 3), np.float32),
           np.empty((B, M, 3), np.float32), np.empty((B, M, 63), np.float32), np.empty((B, M), np.int32), np.empty((B,), np.int32)]
    _capi.check(l.hep_run(s.handle, x.ctypes.data, B, None, *[o.ctypes.data for o in ho]))
    _capi.check(l.hep_decode(s.handle, ho[0].ctypes.data, ho[3].ctypes.data, cam.ctypes.data, B, hb.ctypes.data, ht.ctypes.data))
    out = np.zeros((B, K, RECORD_WORDS), np.int32)
    for c in range(K):
        m = np.ascontiguousarray(masked(ho[1], c))
        _capi.check(l.hep_filter(s.handle, hb.ctypes.data, m.ctypes.data, ho[2].ctypes.data, ht.ctypes.data, ho[4].ctypes.data, B, thr, nms, M,
                                 *[a.ctypes.data for a in det]))
        for b in range(B):
            out[b, c] = record_of_row0(int(det[7][b]), *[det[i][b] for i in range(7)])
    return out


@pytest.mark.parametrize("B", [1, 3])
def test_poses_from_input_equals_the_host_chain(env, sess, B):
    _S, _sd, _capi = env
    s, x, cls = sess
    cam = cam_rows(B)
    thr = thr_for_about_five(cls[0])
    assert 5 <= int((cls[0] > np.float32(thr)).sum()) <= 50
    xb = np.ascontiguousarray(x[:B])
    p = s.poses_from_input(xb, cam, thr)
    assert p["found"].shape == (B, 3) and p["hand"].shape == (B, 3, 63) and "label" not in p
    want = host_chain(s, _capi, xb, cam, thr)
    assert p["found"][0].any() and np.array_equal(records_of_poses(p), want), (B, p["index"], want[..., :3])
    # a threshold no score reaches: found 0 and the filter's padding in place
    q = s.poses_from_input(xb, cam, 2.0)
    assert (q["found"] == 0).all() and (q["index"] == -1).all() and (q["score"] == -1).all()
    assert all((q[k] == -1).all() for k in ("box", "rotation", "translation", "hand"))
    assert np.array_equal(records_of_poses(q), host_chain(s, _capi, xb, cam, 2.0))
    # outputs other than found may be NULL
    found = np.full((B, 3), 7, np.int32)
    assert _capi.lib().hep_poses_from_input(s.handle, xb.ctypes.data, B, cam.ctypes.data, thr, found.ctypes.data, *([None] * 6)) == 0
    assert np.array_equal(found, p["found"])


def frame_chain(s, frames, h, w, crop, rs, cam, thr):
    """preprocess_i420 -> forward -> decode -> masked filter on the device: [B, K, 80] records of row 0"""
    xin = s.preprocess_i420(torch.from_numpy(frames).cuda(), h, w, crop, rs)
    heads = s.forward(xin, want_features=False)[1:]
    return masked_chain(s, heads, torch.from_numpy(cam).cuda(), thr)


@pytest.mark.parametrize("geom", [(480, 640, 256, 512), (300, 402, 200, 333)])
def test_poses_from_i420_equals_the_frame_chain(env, sess, geom):
    _S, _sd, _capi = env
    s, _x, _cls = sess
    h, w, crop, rs = geom
    rng = np.random.Generator(np.random.PCG64(h + w + 1))
    frames = rng.integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    cam = cam_rows(2)
    xin = s.preprocess_i420(torch.from_numpy(frames).cuda(), h, w, crop, rs)
    thr = thr_for_about_five(s.forward(xin, want_features=False)[2][0].cpu().numpy())
    for t in (thr, 0.0):                                                          # about five candidates in frame 0; every anchor
        p = s.poses_from_i420(frames, h, w, cam, crop, rs, t)
        assert np.array_equal(records_of_poses(p), frame_chain(s, frames, h, w, crop, rs, cam, t)), (geom, t)
        assert p["found"][0].any()
    found = np.full((2, 3), 7, np.int32)
    assert _capi.lib().hep_poses_from_i420(s.handle, frames.ctypes.data, 2, h, w, crop, rs, cam.ctypes.data, 0.0, found.ctypes.data, *([None] * 6)) == 0
    assert (found == 1).all()


def test_poses_from_i420_reentered_from_four_threads(env, sess):
    s, _x, _cls = sess
    h, w = 480, 640
    rng = np.random.Generator(np.random.PCG64(10))
    frames = [rng.integers(0, 256, (1, h * w * 3 // 2), dtype=np.uint8) for _ in range(4)]
    cams = [cam_rows(2)[i % 2:i % 2 + 1] for i in range(4)]
    serial = [records_of_poses(s.poses_from_i420(f, h, w, c, 256, 512, 0.0)) for f, c in zip(frames, cams)]
    assert len({r.tobytes() for r in serial}) == 4                                # four different answers: a mix-up would show
    results = [[] for _ in range(4)]

    def worker(i):
        for _ in range(4):
            results[i].append(records_of_poses(s.poses_from_i420(frames[i], h, w, cams[i], 256, 512, 0.0)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i in range(4):
        assert len(results[i]) == 4 and all(np.array_equal(r, serial[i]) for r in results[i]), i


def test_poses_calls_allocate_nothing_in_steady_state(env, sess):
    s, x, _cls = sess
    h, w = 480, 640
    frames = np.random.Generator(np.random.PCG64(3)).integers(0, 256, (3, h * w * 3 // 2), dtype=np.uint8)
    cam = cam_rows(3)
    for _ in range(2):
        s.poses_from_i420(frames, h, w, cam, 256, 512, 0.5)
        s.pose_from_i420(frames, h, w, cam, 256, 512, 0.5)
        s.poses_from_input(x, cam, 0.5)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        s.poses_from_i420(frames, h, w, cam, 256, 512, 0.5)
        s.pose_from_i420(frames, h, w, cam, 256, 512, 0.5)
        s.poses_from_input(x, cam, 0.5)
    assert torch.cuda.mem_get_info()[0] == before


def test_poses_calls_refuse_bad_arguments_and_work_afterwards(env, sess):
    _S, _sd, _capi = env
    s, x, _cls = sess
    l = _capi.lib()
    h, w = 480, 640
    frames = np.random.Generator(np.random.PCG64(4)).integers(0, 256, (3, h * w * 3 // 2), dtype=np.uint8)
    cam = cam_rows(3)
    found = np.zeros(16, np.int32)
    i420 = lambda B, hh, ww, crop, c: l.hep_poses_from_i420(s.handle, frames.ctypes.data, B, hh, ww, crop, 512, c, 0.5, found.ctypes.data, *([None] * 6))
    blob = lambda B, c: l.hep_poses_from_input(s.handle, x.ctypes.data, B, c, 0.5, found.ctypes.data, *([None] * 6))
    for call, reason in ((lambda: i420(1, 481, w, 256, cam.ctypes.data), b"even"),
                         (lambda: i420(1, h, 641, 256, cam.ctypes.data), b"even"),
                         (lambda: i420(4, h, w, 256, cam.ctypes.data), b"hep_poses_from_i420: batch"),
                         (lambda: i420(0, h, w, 256, cam.ctypes.data), b"hep_poses_from_i420: batch"),
                         (lambda: i420(1, h, w, 482, cam.ctypes.data), b"crop"),
                         (lambda: i420(1, h, w, 256, None), b"hep_poses_from_i420: camera is NULL"),
                         (lambda: l.hep_poses_from_i420(s.handle, None, 1, h, w, 256, 512, cam.ctypes.data, 0.5, found.ctypes.data, *([None] * 6)), b"yuv is NULL"),
                         (lambda: blob(4, cam.ctypes.data), b"hep_poses_from_input: batch"),
                         (lambda: blob(1, None), b"hep_poses_from_input: camera is NULL"),
                         (lambda: l.hep_poses_from_input(s.handle, x.ctypes.data, 1, cam.ctypes.data, 0.5, None, *([None] * 6)), b"hep_poses_from_input: found is NULL"),
                         (lambda: l.hep_top_labels_device(s.handle, None, None, None, None, None, None, 1, 0.5, found.ctypes.data, None), b"hep_top_labels_device: camera is NULL"),
                         (lambda: l.hep_top_labels_device(s.handle, None, None, None, None, None, found.ctypes.data, 1, 0.5, None, None), b"hep_top_labels_device: records is NULL"),
                         (lambda: l.hep_top_labels_device(s.handle, None, None, None, None, None, found.ctypes.data, 4, 0.5, found.ctypes.data, None), b"hep_top_labels_device: batch"),
                         (lambda: l.hep_top_labels_device(s.handle, None, None, None, None, None, found.ctypes.data, 0, 0.5, found.ctypes.data, None), b"hep_top_labels_device: batch")):
        assert l.hep_anchors(100, None, None) < 0                   # another message in between
        assert call() == -1                                         # HEP_ERR_INVALID
        assert reason in l.hep_last_error(), (reason, l.hep_last_error())
    # the Python face refuses before a pointer reaches the ABI
    with pytest.raises(ValueError):
        s.poses_from_i420(frames[:, :-1], h, w, cam)
    with pytest.raises(ValueError):
        s.poses_from_i420(torch.from_numpy(frames).cuda(), h, w, cam)
    with pytest.raises(ValueError):
        s.poses_from_input(x[:, :, :64], cam)
    with pytest.raises(ValueError):
        s.poses_from_input(x, cam[:2])
    with pytest.raises(ValueError):
        s.top_labels(torch.from_numpy(cam), 0.5)                    # camera on the host
    with pytest.raises(ValueError):
        s.top_labels(torch.from_numpy(np.concatenate([cam, cam])).cuda(), 0.5)      # batch above max_batch
    with pytest.raises(ValueError):
        s.top_labels(torch.from_numpy(cam).cuda(), 0.5, heads=[torch.zeros(3, 5, 4).cuda()] * 5)
    with pytest.raises(ValueError):                                 # a one-class classification for a three-class session
        N = s.num_anchors
        s.top_labels(torch.from_numpy(cam).cuda(), 0.5, heads=[torch.zeros(3, N, k).cuda() for k in (4, 1, 3, 3, 63)])
    # a correct call still works
    p = s.poses_from_i420(frames, h, w, cam, 256, 512, 0.5)
    assert np.array_equal(records_of_poses(p), frame_chain(s, frames, h, w, 256, 512, cam, 0.5))
