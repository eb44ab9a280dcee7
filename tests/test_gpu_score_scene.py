"""hep_score_scene_device (every label and every annotation of a batch scored in one launch), SceneEvaluator and evaluate_scene_device
against hep_score_detections_device, hep_pose_errors_device and the numpy statement of tests/_score_scene.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import _score as S
from tests import _score_scene as SS

pytestmark = pytest.mark.gpu
GUARD = 8           # guard elements before and after every output


def _offsets(cl):
    return (ctypes.c_int32 * (len(cl) + 1))(*np.concatenate(([0], np.cumsum([len(c) for c in cl]))).tolist())


def _launch(det, gt, cl, M, iou_thr=0.5, thr=0.05, hand=True, max_points=1000):
    """One scoring launch; every output sits between guard words.  Returns the five outputs (host), the guards' state and the device inputs."""
    from hmd_ego_pose_amd import _capi
    B, rows = det["scores"].shape
    A = gt.shape[1]
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in det.items()}
    g, p = torch.from_numpy(np.ascontiguousarray(gt)).cuda(), torch.from_numpy(np.concatenate(cl)).cuda()
    outs = [torch.full((n + 2 * GUARD,), 7, dtype=dt, device="cuda") for n, dt in
            ((B * A * S.REC, torch.float64), (B * M, torch.float32), (B * M, torch.int32), (B * M, torch.int32), (B, torch.int32))]
    _capi.check(_capi.lib().hep_score_scene_device(
        d["boxes"].data_ptr(), d["scores"].data_ptr(), d["labels"].data_ptr(), d["rotation"].data_ptr(), d["translation"].data_ptr(),
        d["hand"].data_ptr() if hand else None, B, rows, g.data_ptr(), A, p.data_ptr(), _offsets(cl), len(cl), max_points, thr, M, iou_thr,
        *[o[GUARD:].data_ptr() for o in outs], torch.cuda.current_stream().cuda_stream))
    host = [o.cpu().numpy() for o in outs]
    intact = all((h[:GUARD] == 7).all() and (h[-GUARD:] == 7).all() for h in host)
    rec, out_s, out_tp, out_l, cnt = (h[GUARD:-GUARD] for h in host)
    return (rec.reshape(B, A, S.REC), out_s.reshape(B, M), out_tp.reshape(B, M), out_l.reshape(B, M), cnt), intact, (d, g, p)


def _pose_errors_by_label(rec, dev, cl):
    """ADD / ADD-S of every matched record through hep_pose_errors_device, label by label with that label's cloud: {(b, slot): (add, add_s)}."""
    from hmd_ego_pose_amd import _capi
    d, g, p = dev
    out, off = {}, np.concatenate(([0], np.cumsum([len(c) for c in cl])))
    for l in range(len(cl)):
        idx = np.argwhere((rec[..., 1] == 1.0) & (rec[..., 12] == l))
        if not len(idx):
            continue
        bi, si = torch.from_numpy(idx[:, 0]).cuda(), torch.from_numpy(idx[:, 1]).cuda()
        ri = torch.from_numpy(rec[idx[:, 0], idx[:, 1], 2].astype(np.int64)).cuda()
        rg, tg = g[bi, si, 5:8].float().contiguous(), g[bi, si, 8:11].float().contiguous()            # ground truth rounded to float32
        rp, tp = (d["rotation"][bi, ri] * np.float32(math.pi)).contiguous(), d["translation"][bi, ri].contiguous()
        add, add_s = torch.zeros(len(idx), dtype=torch.float64, device="cuda"), torch.zeros(len(idx), dtype=torch.float64, device="cuda")
        cloud = p[off[l]:off[l + 1]].contiguous()
        _capi.check(_capi.lib().hep_pose_errors_device(cloud.data_ptr(), len(cl[l]), rg.data_ptr(), tg.data_ptr(), rp.data_ptr(), tp.data_ptr(), len(idx), 1000,
                                                       add.data_ptr(), add_s.data_ptr(), torch.cuda.current_stream().cuda_stream))
        for (b, s), x, y in zip(idx.tolist(), add.cpu().tolist(), add_s.cpu().tolist()):
            out[(b, s)] = (x, y)
    return out


def _assert_outputs(got, want, gt, pairs, hand=True, name=""):
    """Flags, counts, labels, matched rows, score bits and IoU exact; ADD / ADD-S bit-identical to hep_pose_errors_device; the other slots
    within tests/_score.py::tolerance."""
    rec, out_s, out_tp, out_l, cnt = got
    w_rec, w_s, w_tp, w_l, w_cnt = want
    assert SS.margins_ok(w_rec)
    assert np.array_equal(cnt, w_cnt) and np.array_equal(out_tp, w_tp) and np.array_equal(out_l, w_l)
    assert np.array_equal(out_s.view(np.int32), w_s.view(np.int32))                            # the score bits
    assert np.array_equal(rec[..., :5], w_rec[..., :5], equal_nan=True)                         # valid, matched, row, score, IoU
    assert np.array_equal(rec[..., 12], w_rec[..., 12]) and not rec[..., 13:].any()
    matched = np.argwhere(w_rec[..., 1] == 1.0).tolist()
    assert np.isnan(rec[w_rec[..., 1] != 1.0][:, 3:12]).all()
    assert len(pairs) == len(matched)
    for b, s in matched:
        assert (rec[b, s, 5], rec[b, s, 6]) == pairs[(b, s)], (name, b, s, rec[b, s, 5:7], pairs[(b, s)])          # bit-identical
        for slot in (5, 6, 7, 8, 9, 10):
            assert abs(rec[b, s, slot] - w_rec[b, s, slot]) <= S.tolerance(slot, w_rec[b, s, slot]), (name, b, s, slot, rec[b, s, slot], w_rec[b, s, slot])
        if gt[b, s, 19] and hand:
            assert abs(rec[b, s, 11] - w_rec[b, s, 11]) <= S.tolerance(11, w_rec[b, s, 11]), (name, b, s, rec[b, s, 11], w_rec[b, s, 11])
        else:
            assert np.isnan(rec[b, s, 11])


@pytest.mark.parametrize("num_points", [1, 37, 1001])
@pytest.mark.parametrize("M", [10, 4])
def test_one_annotation_one_label_equals_the_single_object_entry(M, num_points):
    """synthetic(0) relabelled to label 0, one label, amax 1, slot 83 = 0: records slots 1-11, the score bits and the flags equal
    hep_score_detections_device's bit for bit; slot 0 is the valid mark here and the considered count there, which out_count carries."""
    from hmd_ego_pose_amd import _capi
    det, gt, pts = S.synthetic(0, num_points=num_points)
    det = dict(det, labels=np.where(det["labels"] >= 0, 0, det["labels"]).astype(np.int32))
    assert not gt[:, 83].any()
    (rec, out_s, out_tp, out_l, cnt), intact, (d, g, p) = _launch(det, gt[:, None, :], [pts], M)
    B = gt.shape[0]
    o_rec = torch.full((B, S.REC), 7.0, dtype=torch.float64, device="cuda")
    o_s, o_tp = torch.full((B, M), 7.0, dtype=torch.float32, device="cuda"), torch.full((B, M), 7, dtype=torch.int32, device="cuda")
    _capi.check(_capi.lib().hep_score_detections_device(
        d["boxes"].data_ptr(), d["scores"].data_ptr(), d["labels"].data_ptr(), d["rotation"].data_ptr(), d["translation"].data_ptr(), d["hand"].data_ptr(),
        B, det["scores"].shape[1], g.data_ptr(), p.data_ptr(), num_points, 1000, 0, 0.05, M, 0.5, o_rec.data_ptr(), o_s.data_ptr(), o_tp.data_ptr(),
        torch.cuda.current_stream().cuda_stream))
    o_rec, o_s, o_tp = o_rec.cpu().numpy(), o_s.cpu().numpy(), o_tp.cpu().numpy()
    assert intact and o_rec[:, 1].sum() >= 3
    assert np.array_equal(rec[:, 0, 1:12].view(np.int64), o_rec[:, 1:12].view(np.int64))         # bit for bit, NaNs included
    assert np.array_equal(rec[:, 0, 0], gt[:, 0]) and np.array_equal(cnt, o_rec[:, 0])
    assert np.array_equal(out_s.view(np.int32), o_s.view(np.int32)) and np.array_equal(out_tp, o_tp)
    assert np.array_equal(out_l, np.where(o_tp >= 0, 0, -1)) and (rec[:, 0, 12] == 0).all() and not rec[:, 0, 13:].any()


def test_special_scenes():
    """Batch 8 x 12 rows, amax 4, three labels with clouds of 1, 37 and 1001 points: the scenes (a) to (h) of tests/_score_scene.py SPECIAL
    (what each of them does is asserted on the oracle in tests/test_score_scene_cpu.py), then (i) the same launch without det_hand."""
    det, gt, cl, want, M = SS.case("special")
    got, intact, dev = _launch(det, gt, cl, M)
    assert intact
    _assert_outputs(got, want, gt, _pose_errors_by_label(want[0], dev, cl), name="special")
    assert want[0][0, 1, 1] == 1 and want[2][0, 1] == 0 and want[0][0, 3, 2] == 2                 # (a) is in there
    bare, intact, _ = _launch(det, gt, cl, M, hand=False)
    assert intact and np.isnan(bare[0][..., 11]).all() and not np.isnan(got[0][..., 11]).all()
    assert np.array_equal(bare[0][..., :11], got[0][..., :11], equal_nan=True) and all(np.array_equal(x, y) for x, y in zip(bare[1:], got[1:]))


@pytest.mark.parametrize("name", ["limits", "wide"])
def test_random_scenes(name):
    """Fixed-seed scenes: "limits" is batch 3 x 256 rows, amax 16, max_detections 256; "wide" is batch 64 x 12 rows, amax 4.  The asserts of
    the special scenes; the guard words around all five outputs stay intact; a second launch is bit-identical."""
    det, gt, cl, want, M = SS.case(name)
    assert (gt.shape[:2], det["scores"].shape[1], M) == (((3, 16), 256, 256) if name == "limits" else ((64, 4), 12, 10))
    got, intact, dev = _launch(det, gt, cl, M)
    assert intact
    _assert_outputs(got, want, gt, _pose_errors_by_label(want[0], dev, cl), name=name)
    again, intact, _ = _launch(det, gt, cl, M)
    assert intact
    for x, y in zip(got, again):
        assert x.tobytes() == y.tobytes()


def test_scene_evaluator_accumulates():
    """11 random scenes in batches of 4, 4 and 3 give the dictionaries of one oracle pass: fractions, AP and counts equal per label and in
    the mean, means and standard deviations within the slot tolerances.  Capacity, dtype, device and shape refusals change nothing."""
    from hmd_ego_pose_amd.evaluate import SceneEvaluator
    from tests.test_gpu_score import _Rows
    det, gt, cl, o, M = SS.case("evaluator")
    want = SS.oracle_scene_result(*o)
    assert SS.margins_ok(o[0]) and all(want["labels"][l]["num_matched"] >= 2 for l in range(3))
    models = list(zip(cl, SS.DIAMETERS, SS.SYMMETRIC))
    ev = SceneEvaluator(_Rows(det, (4, 4, 3)), models, 8, capacity=11, amax=SS.AMAX)
    img = lambda n: torch.zeros((n, 3, 8, 8), device="cuda")
    cam = lambda n: torch.zeros((n, 6), device="cuda")
    g = torch.from_numpy(gt).cuda()
    for o_, n in ((0, 4), (4, 4), (8, 3)):
        ev.add(img(n), cam(n), g[o_:o_ + n])
    got = ev.result()
    SS.assert_scene_results_close(got, want)
    assert got["mean"]["mixed_distance_mean"] == sum(got["labels"][l]["ADD-S_distance_mean" if SS.SYMMETRIC[l] else "ADD_distance_mean"] for l in range(3)) / 3
    same = lambda a, b: repr(a) == repr(b)                                                  # NaN-proof equality of the nested dictionaries
    with pytest.raises(ValueError, match="capacity"):
        ev.add(img(1), cam(1), g[:1])
    assert ev.count == 11 and same(ev.result(), got)                                         # the refused call changed nothing
    ev.reset()
    with pytest.raises(ValueError):
        ev.add(img(2), cam(2), g[:2].float())
    with pytest.raises(ValueError):
        ev.add(img(2), cam(2).cpu(), g[:2])
    with pytest.raises(ValueError):
        ev.add(img(2), cam(3), g[:2])
    with pytest.raises(ValueError):
        ev.add(img(2), cam(2), g[:2, :3])                                                    # amax 3 where the evaluator was built for 4
    with pytest.raises(ValueError):
        ev.add(img(2), cam(2), g[:2, 0])                                                     # the single-annotation table
    assert ev.count == 0 and ev.result()["mean"]["num_annotations"] == 0.0
    ev.model = _Rows(det, (4, 4, 3))                                                         # after reset the same images give the same dictionaries
    for o_, n in ((0, 4), (4, 4), (8, 3)):
        ev.add(img(n), cam(n), g[o_:o_ + n])
    assert same(ev.result(), got)


def _scene_folder_from_detections(root, frames, rows, cam_K, ids):
    """A scene folder whose ground truth is the model's own detections: per frame, the first row of every label becomes an annotation of
    that object (box, pose), written in the Linemod layout."""
    import os
    import yaml
    from PIL import Image
    from hmd_ego_pose_amd import evaluate as E
    obj = os.path.join(root, "data", f"{ids[0]:02}")
    os.makedirs(os.path.join(obj, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    info_models = {}
    for l, o in enumerate(ids):
        pts = SS.clouds()[l]
        with open(os.path.join(root, "models", f"obj_{o:02}.ply"), "wb") as f:
            f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(pts))
            f.write(pts.astype("<f4").tobytes())
        info_models[o] = {"diameter": SS.DIAMETERS[l]}
    with open(os.path.join(root, "models", "models_info.yml"), "w") as f:
        yaml.safe_dump(info_models, f)
    gt, info = {}, {}
    for i, frame in enumerate(frames):
        Image.fromarray(frame).save(os.path.join(obj, "rgb", f"{i:06d}.png"))
        gt[i] = []
        for l, o in enumerate(ids):
            r = np.nonzero((rows["labels"][i] == l) & (rows["scores"][i] > 0))[0]
            if not len(r):
                continue
            x1, y1, x2, y2 = (int(round(float(v))) for v in rows["boxes"][i, r[0]])
            R = E.axis_angle_to_matrix(rows["rotation"][i, r[0]].astype(np.float64) * math.pi)
            gt[i].append({"cam_R_m2c": [float(v) for v in R.reshape(-1)], "cam_t_m2c": [float(v) + 3.0 for v in rows["translation"][i, r[0]]],
                          "obj_bb": [x1, y1, x2 - x1, y2 - y1], "obj_id": o})
        info[i] = {"cam_K": [float(v) for v in cam_K.reshape(-1)], "depth_scale": 1.0}
    for name, d in (("gt_0.yml", gt), ("info_0.yml", info)):
        with open(os.path.join(obj, name), "w") as f:
            yaml.safe_dump(d, f)
    with open(os.path.join(obj, "test_0.txt"), "w") as f:
        f.write("".join(f"{i:06d}\n" for i in range(len(frames))))


def test_evaluate_scene_device_end_to_end(tmp_path):
    """phi 0, size 128, batch 2, seeded 3-class weights, a SceneFolder of 3 frames whose annotations are the model's own first detection of
    every label (boxes rounded to pixels, translations moved by 3): at least one frame matches two annotations, and
    evaluate_scene_device equals the scene oracle run over the same ``model.detect`` rows."""
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    size, ids, kw = 128, [1, 5, 6], dict(score_threshold=0.05, max_detections=100, iou_threshold=0.5)      # the cap at the filter's 100 rows: every label's first row is a candidate
    m = HMDEgoPose({"iter": 0}, num_classes=3, compound_coef=0, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(0, 0, num_classes=3), strict=True)
    model = TrainModelWithLoss(m.to("cuda").eval()).eval()
    rng = np.random.Generator(np.random.PCG64(17))
    frames = rng.integers(0, 256, (3, size, size, 3), dtype=np.uint8)
    K = np.array([[480.0, 0, 64.0], [0, 480.0, 64.0], [0, 0, 1.0]])
    cam_row = np.array([480.0, 480.0, 64.0, 64.0, 1000.0, 1.0], np.float32)

    def detect(idx):
        u8 = torch.from_numpy(frames[idx]).cuda()
        x = model.model.session(size, len(idx), torch.device("cuda", torch.cuda.current_device())).preprocess(u8)
        det = model.detect(x, torch.from_numpy(np.stack([cam_row] * len(idx))).cuda())
        return {k: det[k].cpu().numpy() for k in ("boxes", "scores", "labels", "rotation", "translation", "hand")}
    parts = [detect([0, 1]), detect([2])]                                                      # the batches evaluate_scene_device makes
    rows = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    _scene_folder_from_detections(str(tmp_path), frames, rows, K, ids)
    ds = E.SceneFolder(str(tmp_path), ids)
    gt = E.gt_scene_table(ds.annotations, ds.camera, 1.0, ds.amax)
    cl = [mdl[0] for mdl in ds.models]
    o = SS.score_scene_batch(rows, gt, cl, **kw)
    per_frame = (o[0][..., 1] == 1.0).sum(axis=1)
    print("annotations per frame", [len(a) for a in ds.annotations], "matched per frame", per_frame.tolist())
    assert per_frame.max() >= 2, per_frame                                                     # else the comparison below says little
    want = SS.oracle_scene_result(*o, diameters=SS.DIAMETERS, symmetric=(False,) * 3)
    got = E.evaluate_scene_device(ds, model, size, batch_size=2, **kw)
    print("oracle", want["mean"])
    print("device", got["mean"])
    print("matched records (label, ADD, ADD-S, t, r, tip, reproj)", [[r[12]] + r[5:11].tolist() for r in o[0].reshape(-1, 16) if r[1] == 1.0])
    assert SS.margins_ok(o[0])
    SS.assert_scene_results_close(got, want, symmetric=(False,) * 3)
