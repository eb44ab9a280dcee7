"""hep_score_detections_device (per-image matching and all pose metrics in one launch), DeviceEvaluator and evaluate_device against
the numpy statement of tests/_score.py, hep_pose_errors_device and evaluate()."""
import math

import numpy as np
import pytest
import torch

from tests import _score as S

pytestmark = pytest.mark.gpu


def _launch(det, gt, pts, M, iou_thr=0.5, thr=0.05, label=0, hand=True, max_points=1000):
    from hmd_ego_pose_amd import _capi
    B, rows = det["scores"].shape
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in det.items()}
    g, p = torch.from_numpy(gt).cuda(), torch.from_numpy(pts).cuda()
    rec = torch.full((B, S.REC), 7.0, dtype=torch.float64, device="cuda")
    out_s = torch.full((B, M), 7.0, dtype=torch.float32, device="cuda")
    out_tp = torch.full((B, M), 7, dtype=torch.int32, device="cuda")
    _capi.check(_capi.lib().hep_score_detections_device(
        d["boxes"].data_ptr(), d["scores"].data_ptr(), d["labels"].data_ptr(), d["rotation"].data_ptr(), d["translation"].data_ptr(),
        d["hand"].data_ptr() if hand else None, B, rows, g.data_ptr(), p.data_ptr(), pts.shape[0], max_points, label, thr, M, iou_thr,
        rec.data_ptr(), out_s.data_ptr(), out_tp.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return rec, out_s, out_tp, d, g, p


@pytest.mark.parametrize("num_points", [1, 37, 1001])
@pytest.mark.parametrize("M", [10, 4])
def test_records_of_synthetic_rows(M, num_points):
    """Batch 6 x 12 rows, the six images of tests/_score.py SPECIAL: flags, counts, matched rows and score bits exact; ADD and
    ADD-S bit-identical to hep_pose_errors_device on the same pairs; the float64 metrics within 1e-9 relative (floor 1), the rotation
    difference within 1e-5 degrees.  The oracle's thresholded quantities keep ten tolerances from their thresholds."""
    from hmd_ego_pose_amd import _capi
    det, gt, pts = S.synthetic(0, num_points=num_points)
    assert gt.shape == (6, S.GT) and det["scores"].shape == (6, S.ROWS)
    want, want_s, want_tp = S.score_batch(det, gt, pts, max_detections=M)
    assert S.margins_ok(want)
    assert want[:, 1].tolist() == [0, 1, 1, 1, 0, 1] and want[3, 4] == 0.5 and want[4, 0] == M and want[2, 2] == 1 and want[1, 2] == 1
    rec, out_s, out_tp, d, g, p = _launch(det, gt, pts, M)
    # the same pairs through hep_pose_errors_device, in the same test: ground truth rounded to float32, rotation x pi in float32
    rows_m = torch.from_numpy(np.maximum(want[:, 2], 0).astype(np.int64)).cuda()
    pick = lambda t: t[torch.arange(6, device="cuda"), rows_m].contiguous()
    rg, tg = g[:, 5:8].float().contiguous(), g[:, 8:11].float().contiguous()
    rp, tp = (pick(d["rotation"]) * np.float32(math.pi)).contiguous(), pick(d["translation"])
    add, add_s = torch.zeros(6, dtype=torch.float64, device="cuda"), torch.zeros(6, dtype=torch.float64, device="cuda")
    _capi.check(_capi.lib().hep_pose_errors_device(p.data_ptr(), num_points, rg.data_ptr(), tg.data_ptr(), rp.data_ptr(), tp.data_ptr(), 6, 1000,
                                                   add.data_ptr(), add_s.data_ptr(), torch.cuda.current_stream().cuda_stream))
    rec, out_s, out_tp, add, add_s = rec.cpu().numpy(), out_s.cpu().numpy(), out_tp.cpu().numpy(), add.cpu().numpy(), add_s.cpu().numpy()
    assert np.array_equal(out_tp, want_tp)
    assert np.array_equal(out_s.view(np.int32), want_s.view(np.int32))                      # the score bits
    assert np.array_equal(rec[:, :3], want[:, :3])                                          # considered, matched, matched row
    assert np.array_equal(rec[:, 3], want[:, 3], equal_nan=True) and np.array_equal(rec[:, 4], want[:, 4], equal_nan=True)
    assert not rec[:, 12:].any()
    for b in range(6):
        if not want[b, 1]:
            assert np.isnan(rec[b, 3:12]).all(), (b, rec[b])
            continue
        assert rec[b, 5] == add[b] and rec[b, 6] == add_s[b], (b, rec[b, 5:7], add[b], add_s[b])          # bit-identical
        for slot in (5, 6, 7, 8, 9, 10):
            print(f"M={M} P={num_points} image {b} slot {slot}: got {rec[b, slot]!r} want {want[b, slot]!r}")
            assert abs(rec[b, slot] - want[b, slot]) <= S.tolerance(slot, want[b, slot]), (b, slot, rec[b, slot], want[b, slot])
        if gt[b, 19]:
            assert abs(rec[b, 11] - want[b, 11]) <= S.tolerance(11, want[b, 11]), (b, rec[b, 11], want[b, 11])
        else:
            assert np.isnan(rec[b, 11])
    assert rec[3, 5] <= 1e-12 and rec[3, 6] <= 1e-4 and rec[3, 8] <= 1e-5                  # identical poses


def test_no_hand_rows_and_another_label():
    """det_hand NULL: the hand slot is NaN and nothing else moves; label 1 evaluates the rows the default drops."""
    det, gt, pts = S.synthetic(0, num_points=37)
    full = _launch(det, gt, pts, 10)[0].cpu().numpy()
    bare = _launch(det, gt, pts, 10, hand=False)[0].cpu().numpy()
    assert np.array_equal(full[:, :11], bare[:, :11], equal_nan=True) and np.isnan(bare[:, 11]).all() and not np.isnan(full[:, 11]).all()
    want, want_s, want_tp = S.score_batch(det, gt, pts, label=1)
    rec, out_s, out_tp = (t.cpu().numpy() for t in _launch(det, gt, pts, 10, label=1)[:3])
    assert np.array_equal(rec[:, :3], want[:, :3]) and np.array_equal(out_tp, want_tp) and np.array_equal(out_s, want_s) and want[1, 1] == 1


class _Rows:
    """Stands where TrainModelWithLoss stands: ``detect`` hands out the prepared rows batch by batch."""

    def __init__(self, det, sizes):
        self.batches, o = [], 0
        for n in sizes:
            self.batches.append({k: torch.from_numpy(np.ascontiguousarray(v[o:o + n])).cuda() for k, v in det.items()})
            o += n

    def detect(self, x, camera):
        return self.batches.pop(0)


@pytest.mark.parametrize("symmetric", [False, True])
def test_device_evaluator_accumulates(symmetric):
    """11 synthetic images in batches of 4, 4 and 3 give the dictionary of one oracle pass: counts, fractions and AP equal, means and
    standard deviations within the record tolerances.  A 12th image at capacity 11 is refused, as is a wrong dtype, before any launch."""
    from hmd_ego_pose_amd.evaluate import DeviceEvaluator
    det, gt, pts = S.synthetic(3, extra=5, num_points=37)
    rec, out_s, out_tp = S.score_batch(det, gt, pts)
    assert S.margins_ok(rec) and rec[:, 1].sum() >= 5
    want = S.oracle_result(rec, out_s, out_tp, symmetric=symmetric)
    ev = DeviceEvaluator(_Rows(det, (4, 4, 3)), pts, S.DIAMETER, 8, capacity=11, symmetric=symmetric)
    img = lambda n: torch.zeros((n, 3, 8, 8), device="cuda")
    cam = lambda n: torch.zeros((n, 6), device="cuda")
    g = torch.from_numpy(gt).cuda()
    for o, n in ((0, 4), (4, 4), (8, 3)):
        ev.add(img(n), cam(n), g[o:o + n])
    got = ev.result()
    S.assert_results_close(got, want, symmetric)
    assert got["mixed_distance_mean"] == got["ADD-S_distance_mean" if symmetric else "ADD_distance_mean"]
    with pytest.raises(ValueError, match="capacity"):
        ev.add(img(1), cam(1), g[:1])
    assert ev.count == 11 and ev.result() == got                                          # the refused call changed nothing
    ev.reset()
    with pytest.raises(ValueError):
        ev.add(img(2), cam(2), g[:2].float())
    with pytest.raises(ValueError):
        ev.add(img(2), cam(2).cpu(), g[:2])
    with pytest.raises(ValueError):
        ev.add(img(2), cam(3), g[:2])
    assert ev.count == 0 and ev.result()["num_annotations"] == 0.0
    ev.model = _Rows(det, (4, 4, 3))                                                        # after reset the same images give the same dictionary
    for o, n in ((0, 4), (4, 4), (8, 3)):
        ev.add(img(n), cam(n), g[o:o + n])
    assert ev.result() == got


def test_evaluate_device_equals_evaluate(tmp_path):
    """The synthetic Linemod folder of the existing evaluator test (5 frames, phi 0, size 256, seeded weights, IoU threshold 0.05):
    counts, AP, the accuracy fractions and the ADD / ADD-S distances equal, every other shared key within the record tolerances.
    With the seeded weights ``evaluate`` matches 1 of the 5 frames at that threshold (2 at 0.01, 5 at 0), so 0.05 is kept."""
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from tests._util import make_linemod_folder
    make_linemod_folder(str(tmp_path / "ds"), n=5)
    ds = E.LinemodFolder(str(tmp_path / "ds"))
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0, onnx_export=True, input_sizes=[256] * 9)
    m.load_state_dict(seeded_state_dict(0, 0), strict=True)
    model = TrainModelWithLoss(m.to("cuda").eval()).eval()
    kw = dict(score_threshold=0.5, max_detections=10, iou_threshold=IOU_THRESHOLD, batch_size=3)
    want = E.evaluate(ds, model, 256, **kw)
    assert want["num_matched"] >= 1, want                                                   # else the comparison below says nothing
    got = E.evaluate_device(ds, model, 256, **kw)
    print("evaluate       ", want)
    print("evaluate_device", got)
    assert set(want) <= set(got) and {"ADD(-S)", "translation_tip_std", "mixed_distance_mean", "mixed_distance_std"} <= set(got)
    for k in ("num_annotations", "num_matched", "AP", "ADD", "ADD-S", "5cm_5deg", "2D_projection",
              "ADD_distance_mean", "ADD_distance_std", "ADD-S_distance_mean", "ADD-S_distance_std"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in set(want) - set(S.EXACT_KEYS):
        assert abs(got[k] - want[k]) <= S.tolerance(S.KEY_SLOT[k], want[k]), (k, got[k], want[k])
    assert got["mixed_distance_mean"] == want["ADD_distance_mean"] and got["ADD(-S)"] == want["ADD"]


IOU_THRESHOLD = 0.05      # as the existing evaluator test; it leaves one matched frame (see the test's docstring)
