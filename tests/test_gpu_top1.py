"""Top detection per image and the frame-to-pose host calls (hep_top1_device, hep_pose_from_input, hep_pose_from_i420) against
the chain they replace - decode + filter row 0 - bit for bit: no tolerances anywhere.  Shapes: phi 0 at size 128 (N = 3069, no
multiple of the workgroup), max_batch 3, one session at size 256 (N = 12 276)."""
import threading

import numpy as np
import pytest
import torch

from tests._top1 import RECORD_WORDS, random_scores, record_of_row0, top1_rule

pytestmark = pytest.mark.gpu

KEYS = ("boxes", "scores", "labels", "rotation", "translation", "hand", "index")
CAM = [480.0, 470.0, 61.0, 66.0, 1000.0, 0.5]


@pytest.fixture(scope="module")
def env():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd.model import Session
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from oracle import decode_ref
    assert torch.cuda.is_available()
    return Session, seeded_state_dict, decode_ref, _capi


@pytest.fixture(scope="module")
def sess(env):
    """fp32, phi 0 @ 128, max_batch 3, with one forward's scores of three frames (shared, never modified)."""
    Session, sd_of, _D, _capi = env
    s = Session(sd_of(0, 0), 0, 128, 3, "fp32")
    rng = np.random.Generator(np.random.PCG64(77))
    x = rng.standard_normal((3, 3, 128, 128)).astype(np.float32)
    cls = s.forward(torch.from_numpy(x).cuda(), want_features=False)[2].cpu().numpy()
    yield s, x, cls
    s.close()


def cam_rows(B):
    return np.array([[CAM[0] + b, CAM[1], CAM[2], CAM[3] - b, CAM[4], CAM[5]] for b in range(B)], np.float32)


def chain_records(s, heads, cam, thr, nms, M, mode):
    """decode + filter on device tensors -> [B, 80] int32 records of row 0, and the filter's dict."""
    reg, cls, rot, trn, hand = heads
    boxes, trans = s.decode(reg, trn, cam)
    det = s.filter(boxes, cls, rot, trans, hand, thr, nms, M, class_specific_filter=mode)
    torch.cuda.synchronize()
    d = {k: v.cpu().numpy() for k, v in det.items()}
    recs = np.stack([record_of_row0(int(d["count"][b]), *[d[k][b] for k in KEYS]) for b in range(reg.shape[0])])
    return recs, boxes, trans


def thr_for_about_five(cls_image):
    """the sixth largest distinct score: the five values above it pass (more anchors where scores tie)"""
    return float(np.unique(cls_image.reshape(-1))[-6])


@pytest.mark.parametrize("size,K", [(128, 1), (128, 3), (256, 1)])
def test_top1_fuzz_equals_row_0_of_decode_and_filter(env, size, K):
    Session, sd_of, D, _capi = env
    s = Session(sd_of(0, 0, num_classes=K), 0, size, 3, "fp32")
    N = s.num_anchors
    assert N % 1024 != 0
    rng = np.random.Generator(np.random.PCG64(1000 + size + K))
    t = lambda a: torch.from_numpy(a).cuda()
    counts = [0, 1, 2, 7, 50, N] if size == 128 else [7, N]
    case = 0
    for ncand in counts:
        for mode in (True, False):
            B = case % 3 + 1
            thr = 0.5 if case % 2 else 0.05
            cls = np.stack([random_scores(rng, N, K, ncand, thr, ties=True) for _ in range(B)])
            reg = (rng.standard_normal((B, N, 4)) * 0.4).astype(np.float32)
            trn = rng.standard_normal((B, N, 3)).astype(np.float32)
            rot = rng.standard_normal((B, N, 3)).astype(np.float32)
            hand = rng.standard_normal((B, N, 63)).astype(np.float32)
            heads = tuple(t(a) for a in (reg, cls, rot, trn, hand))
            cam = t(cam_rows(B))
            got = s.top1(cam, thr, heads=heads, class_specific_filter=mode)
            torch.cuda.synchronize()
            rec = got["record"].cpu().numpy()
            assert rec.shape == (B, RECORD_WORDS)
            for M in (1, 100):
                for nms in (0.3, 0.9):
                    want, boxes, trans = chain_records(s, heads, cam, thr, nms, M, mode)
                    assert np.array_equal(rec, want), (size, K, ncand, mode, B, M, nms, np.nonzero(rec != want))
            bx, tr = boxes.cpu().numpy(), trans.cpu().numpy()
            for b in range(B):
                ctx = (size, K, ncand, mode, b)
                ncands = int((cls[b] > np.float32(thr)).any(axis=1).sum())
                assert int(rec[b, 0]) == int(ncands > 0), ctx
                for M in ((1, 100) if ncand <= 50 else (1,)):                      # (the oracle's NMS is a Python loop)
                    o = D.filter_detections(bx[b], cls[b], rot[b], tr[b], hand[b], thr, M, 0.3, class_specific_filter=mode)
                    assert np.array_equal(rec[b], record_of_row0(int(o[6][0] >= 0), *o)), ctx
                assert (int(rec[b, 0]), int(rec[b, 1]), int(rec[b, 2])) == top1_rule(cls[b], thr, mode)[:3], ctx
                # the views of the record
                assert int(got["found"][b]) == rec[b, 0] and int(got["index"][b]) == rec[b, 2] and int(got["label"][b]) == rec[b, 1]
                assert np.array_equal(got["hand"][b].cpu().numpy().view(np.int32), rec[b, 15:78])
                assert np.array_equal(got["box"][b].cpu().numpy().view(np.int32), rec[b, 5:9])
            case += 1
    s.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_top1_on_the_handles_own_outputs_after_a_forward(env, precision):
    Session, sd_of, _D, _capi = env
    s = Session(sd_of(0, 0), 0, 128, 3, precision)
    rng = np.random.Generator(np.random.PCG64(5))
    x = torch.from_numpy(rng.standard_normal((3, 3, 128, 128)).astype(np.float32)).cuda()
    for B in (3, 2):
        outs = s.forward(x[:B], want_features=False)[1:]
        cam = torch.from_numpy(cam_rows(B)).cuda()
        own = [v[:B] for v in s.output_views()]
        for a, b in zip(outs, own):
            assert torch.equal(a, b)
        for thr in (0.5, thr_for_about_five(outs[1][0].cpu().numpy()), 2.0):
            rec = s.top1(cam, thr)["record"].cpu().numpy()                        # NULL head pointers: the handle's buffers
            want, _b, _t = chain_records(s, own, cam, thr, 0.5, 100, True)
            assert np.array_equal(rec, want), (precision, B, thr)
            assert (rec[:, 0] == 0).all() == (thr == 2.0)
    s.close()


def host_chain(s, _capi, x, cam, thr, M=100, nms=0.5):
    """hep_run -> hep_decode -> hep_filter on host arrays (what the C# binding could call before): records of row 0"""
    l = _capi.lib()
    B, N = x.shape[0], s.num_anchors
    ho = [np.empty((B, N, k), np.float32) for k in s.out_width]
    hb, ht = np.empty((B, N, 4), np.float32), np.empty((B, N, 3), np.float32)
    det = [np.empty((B, M, 4), np.float32), np.empty((B, M), np.float32), np.empty((B, M), np.int32), np.empty((B, M, 3), np.float32),
           np.empty((B, M, 3), np.float32), np.empty((B, M, 63), np.float32), np.empty((B, M), np.int32), np.empty((B,), np.int32)]
    _capi.check(l.hep_run(s.handle, x.ctypes.data, B, None, *[o.ctypes.data for o in ho]))
    _capi.check(l.hep_decode(s.handle, ho[0].ctypes.data, ho[3].ctypes.data, cam.ctypes.data, B, hb.ctypes.data, ht.ctypes.data))
    _capi.check(l.hep_filter(s.handle, hb.ctypes.data, ho[1].ctypes.data, ho[2].ctypes.data, ht.ctypes.data, ho[4].ctypes.data, B, thr, nms, M,
                             *[a.ctypes.data for a in det]))
    return np.stack([record_of_row0(int(det[7][b]), *[det[i][b] for i in range(7)]) for b in range(B)])


def records_of_pose(p):
    """the dict of numpy arrays of Session.pose_from_* as [B, 80] records"""
    B = len(p["found"])
    return np.stack([record_of_row0(int(p["found"][b]), p["box"][b:b + 1], p["score"][b:b + 1], p["label"][b:b + 1], p["rotation"][b:b + 1],
                                    p["translation"][b:b + 1], p["hand"][b:b + 1], p["index"][b:b + 1]) for b in range(B)])


@pytest.mark.parametrize("B", [1, 3])
def test_pose_from_input_equals_the_host_chain(env, sess, B):
    _S, _sd, _D, _capi = env
    s, x, cls = sess
    cam = cam_rows(B)
    thr = thr_for_about_five(cls[0])
    assert 5 <= int((cls[0] > np.float32(thr)).sum()) <= 50
    p = s.pose_from_input(x[:B], cam, thr)
    want = host_chain(s, _capi, np.ascontiguousarray(x[:B]), cam, thr)
    assert p["found"][0] == 1 and np.array_equal(records_of_pose(p), want), (B, p["index"], want[:, :3])
    # a threshold no score reaches: found 0 and the filter's padding in place
    q = s.pose_from_input(x[:B], cam, 2.0)
    assert (q["found"] == 0).all() and (q["index"] == -1).all() and (q["label"] == -1).all() and (q["score"] == -1).all()
    assert all((q[k] == -1).all() for k in ("box", "rotation", "translation", "hand"))
    assert np.array_equal(records_of_pose(q), host_chain(s, _capi, np.ascontiguousarray(x[:B]), cam, 2.0))
    # outputs other than found may be NULL
    found = np.full(B, 7, np.int32)
    assert _capi.lib().hep_pose_from_input(s.handle, x.ctypes.data, B, cam.ctypes.data, thr, found.ctypes.data, *([None] * 7)) == 0
    assert np.array_equal(found, p["found"])


def frame_chain(s, frames, h, w, crop, rs, cam, thr):
    """preprocess_i420 -> forward -> decode -> filter on the device: records of row 0"""
    xin = s.preprocess_i420(torch.from_numpy(frames).cuda(), h, w, crop, rs)
    heads = s.forward(xin, want_features=False)[1:]
    return chain_records(s, heads, torch.from_numpy(cam).cuda(), thr, 0.5, 100, True)[0]


@pytest.mark.parametrize("geom", [(480, 640, 256, 512), (300, 402, 200, 333)])
def test_pose_from_i420_equals_the_frame_chain(env, sess, geom):
    s, _x, _cls = sess
    h, w, crop, rs = geom
    rng = np.random.Generator(np.random.PCG64(h + w))
    frames = rng.integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    cam = cam_rows(2)
    xin = s.preprocess_i420(torch.from_numpy(frames).cuda(), h, w, crop, rs)
    thr = thr_for_about_five(s.forward(xin, want_features=False)[2][0].cpu().numpy())
    for t in (thr, 0.0):                                                          # about five candidates in frame 0; every anchor
        p = s.pose_from_i420(frames, h, w, cam, crop, rs, t)
        assert np.array_equal(records_of_pose(p), frame_chain(s, frames, h, w, crop, rs, cam, t)), (geom, t)
        assert p["found"][0] == 1


def test_pose_from_i420_reentered_from_four_threads(env, sess):
    s, _x, _cls = sess
    h, w = 480, 640
    rng = np.random.Generator(np.random.PCG64(9))
    frames = [rng.integers(0, 256, (1, h * w * 3 // 2), dtype=np.uint8) for _ in range(4)]
    cams = [cam_rows(2)[i % 2:i % 2 + 1] for i in range(4)]
    serial = [records_of_pose(s.pose_from_i420(f, h, w, c, 256, 512, 0.0)) for f, c in zip(frames, cams)]
    assert len({r.tobytes() for r in serial}) == 4                                # four different answers: a mix-up would show
    results = [[] for _ in range(4)]

    def worker(i):
        for _ in range(8):
            results[i].append(records_of_pose(s.pose_from_i420(frames[i], h, w, cams[i], 256, 512, 0.0)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i in range(4):
        assert len(results[i]) == 8 and all(np.array_equal(r, serial[i]) for r in results[i]), i


def test_pose_calls_allocate_nothing_in_steady_state(env, sess):
    s, x, _cls = sess
    h, w = 480, 640
    frames = np.random.Generator(np.random.PCG64(3)).integers(0, 256, (3, h * w * 3 // 2), dtype=np.uint8)
    cam = cam_rows(3)
    for _ in range(2):
        s.pose_from_i420(frames, h, w, cam, 256, 512, 0.5)
        s.pose_from_input(x, cam, 0.5)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        s.pose_from_i420(frames, h, w, cam, 256, 512, 0.5)
        s.pose_from_input(x, cam, 0.5)
    assert torch.cuda.mem_get_info()[0] == before


def test_pose_calls_refuse_bad_arguments_and_work_afterwards(env, sess):
    _S, _sd, _D, _capi = env
    s, x, _cls = sess
    l = _capi.lib()
    h, w = 480, 640
    frames = np.random.Generator(np.random.PCG64(4)).integers(0, 256, (3, h * w * 3 // 2), dtype=np.uint8)
    cam = cam_rows(3)
    found = np.zeros(4, np.int32)
    i420 = lambda B, hh, ww, crop, c: l.hep_pose_from_i420(s.handle, frames.ctypes.data, B, hh, ww, crop, 512, c, 0.5, found.ctypes.data, *([None] * 7))
    blob = lambda B, c: l.hep_pose_from_input(s.handle, x.ctypes.data, B, c, 0.5, found.ctypes.data, *([None] * 7))
    for call, reason in ((lambda: i420(1, 481, w, 256, cam.ctypes.data), b"even"),
                         (lambda: i420(1, h, 641, 256, cam.ctypes.data), b"even"),
                         (lambda: i420(4, h, w, 256, cam.ctypes.data), b"batch"),
                         (lambda: i420(0, h, w, 256, cam.ctypes.data), b"batch"),
                         (lambda: i420(1, h, w, 482, cam.ctypes.data), b"crop"),
                         (lambda: i420(1, h, w, 256, None), b"camera is NULL"),
                         (lambda: blob(4, cam.ctypes.data), b"batch"),
                         (lambda: blob(1, None), b"camera is NULL"),
                         (lambda: l.hep_pose_from_input(s.handle, x.ctypes.data, 1, cam.ctypes.data, 0.5, None, *([None] * 7)), b"found is NULL"),
                         (lambda: l.hep_top1_device(s.handle, None, None, None, None, None, None, 1, 0.5, found.ctypes.data, None), b"camera is NULL"),
                         (lambda: l.hep_top1_device(s.handle, None, None, None, None, None, found.ctypes.data, 4, 0.5, found.ctypes.data, None), b"batch")):
        assert l.hep_anchors(100, None, None) < 0                   # another message in between
        assert call() == -1                                         # HEP_ERR_INVALID
        assert reason in l.hep_last_error(), (reason, l.hep_last_error())
    # the Python face refuses before a pointer reaches the ABI
    with pytest.raises(ValueError):
        s.pose_from_i420(frames[:, :-1], h, w, cam)
    with pytest.raises(ValueError):
        s.pose_from_i420(torch.from_numpy(frames).cuda(), h, w, cam)
    with pytest.raises(ValueError):
        s.pose_from_input(x[:, :, :64], cam)
    with pytest.raises(ValueError):
        s.pose_from_input(x, cam[:2])
    with pytest.raises(ValueError):
        s.top1(torch.from_numpy(cam), 0.5)                          # camera on the host
    with pytest.raises(ValueError):
        s.top1(torch.from_numpy(cam).cuda(), 0.5, heads=[torch.zeros(3, 5, 4).cuda()] * 5)
    # a correct call still works
    p = s.pose_from_i420(frames, h, w, cam, 256, 512, 0.5)
    assert np.array_equal(records_of_pose(p), frame_chain(s, frames, h, w, 256, 512, cam, 0.5))
