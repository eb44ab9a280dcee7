"""hep_draw_poses_device (annotations and kept detections of a batch drawn into the frames in one launch), draw_poses, the streaming
records and the evaluators' ``draw_into`` / ``save_path`` against the numpy definition of tests/_draw.py: every comparison byte for byte.
Each bit-exact case first asserts the input condition on the oracle alone (tests/_draw.py ``assert_input_condition``): the device's
double-precision sin / cos may differ from libm's in the last bits, so no projected coordinate may lie within 1e-7 of an integer or of
a saturation bound, no depth within 1e-3 of zero and no non-zero angle within 1e-9 of the identity switch.  (An angle of exactly 0 is
exact on both sides.  Where the poses come from the seeded model, whose hand joints lie around depth 0, the depth bound is asserted for the
rotated cuboid corners only: a centre's or a joint's depth is an input that both sides use bit for bit.)"""
import numpy as np
import pytest
import torch

from tests import _draw as D

pytestmark = pytest.mark.gpu
ALL = D.BOX2D | D.CUBOID | D.HAND


@pytest.fixture(scope="module")
def env():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd import draw as DR
    assert torch.cuda.is_available()
    return DR, _capi


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def oracle(c, given_depths=True, **kw):
    """(drawn copy, per-image shapes) of a case dict with the input condition asserted."""
    sh = []
    args = dict(gt=c.get("gt"), camera=c.get("camera"), det=c.get("det"), score_threshold=c["score_threshold"], max_detections=c["max_detections"])
    args.update(kw)
    out = D.draw_poses(c["frames"], c["cuboids"], c["colours"], shapes_out=sh, **args)
    D.assert_input_condition(sh, given_depths)
    return out, sh


def device(DR, c, **kw):
    args = dict(gt=dev(c.get("gt")), camera=dev(c.get("camera")), score_threshold=c["score_threshold"], max_detections=c["max_detections"])
    det = kw.pop("det", c.get("det"))
    args["detections"] = None if det is None else {k: dev(v) for k, v in det.items()}
    args.update(kw)
    frames = dev(c["frames"])
    got = DR.draw_poses(frames, cuboids=dev(c["cuboids"]), colours=c["colours"], **args)
    assert got is frames
    return frames.cpu().numpy()


@pytest.fixture(scope="module")
def main_case():
    return D.case_main()


@pytest.mark.parametrize("t", [1, 2, 3])
def test_main_case_all_layers(env, main_case, t):
    """48 x 64, batch 3: image 0 two annotations (one with joints) and rows at the threshold, padded, out of range and beyond the cap;
    image 1 nothing valid, byte-unchanged; image 2 off-frame shapes, a corner behind the camera, a saturated projection, zero rotations
    and degenerate segments (tests/test_draw_cpu.py asserts that the case holds all of this)."""
    DR, _ = env
    want, _sh = oracle(main_case, ann_layers=ALL, det_layers=ALL, thickness=t)
    got = device(DR, main_case, ann_layers=ALL, det_layers=ALL, thickness=t)
    assert np.array_equal(got[1], main_case["frames"][1])
    assert (want != main_case["frames"]).any(axis=3).sum() > 1000
    bad = np.argwhere((got != want).any(axis=3))
    assert bad.size == 0, (len(bad), bad[:5].tolist())


def test_layers_apart_and_default_arguments(env, main_case):
    DR, _ = env
    for ann, det in ((D.BOX2D, D.HAND), (D.HAND, D.BOX2D), (0, D.CUBOID), (D.CUBOID | D.HAND, 0)):
        want, _ = oracle(main_case, ann_layers=ann, det_layers=det, thickness=4)
        assert np.array_equal(device(DR, main_case, ann_layers=ann, det_layers=det, thickness=4), want), (ann, det)
    want, _ = oracle(main_case)                                     # cuboid layer, thickness 2
    assert np.array_equal(device(DR, main_case), want)
    want, _ = oracle(main_case, ann_layers=ALL, det_layers=ALL, thickness=8)
    assert np.array_equal(device(DR, main_case, ann_layers=ALL, det_layers=ALL, thickness=8), want)


def test_at_the_caps(env):
    """37 x 50 (no multiple of the 64 x 16 tile), batch 1: 16 annotations, 256 rows, more than 64 candidates, max_detections 64."""
    DR, _ = env
    c = D.case_caps()
    for t in (1, 2):
        want, sh = oracle(c, ann_layers=ALL, det_layers=ALL, thickness=t)
        assert len(sh[0]) > 60
        got = device(DR, c, ann_layers=ALL, det_layers=ALL, thickness=t)
        bad = np.argwhere((got != want).any(axis=3))
        assert bad.size == 0, (t, len(bad), bad[:5].tolist())


def test_source_variants(env, main_case):
    DR, _ = env
    c = dict(main_case)
    # gt NULL with camera given (a camera of its own: not the table's)
    cam = np.tile(np.array([280.5, 301.25, 30.2, 25.9, 0.625]), (3, 1))
    v = dict(c, gt=None, camera=cam)
    want, sh = oracle(v, det_layers=ALL)
    assert all(not s.annotation for im in sh for s in im) and (want != c["frames"]).any()
    assert np.array_equal(device(DR, v, det_layers=ALL), want)
    # both given: the camera array wins
    v = dict(c, camera=cam)
    want, _ = oracle(v, ann_layers=ALL, det_layers=ALL)
    assert np.array_equal(device(DR, v, ann_layers=ALL, det_layers=ALL), want)
    assert not np.array_equal(want, oracle(c, ann_layers=ALL, det_layers=ALL)[0])
    # detections NULL with gt given
    v = dict(c, det=None)
    want, sh = oracle(v, ann_layers=ALL)
    assert all(s.annotation for im in sh for s in im) and (want != c["frames"]).any()
    assert np.array_equal(device(DR, v, ann_layers=ALL), want)
    # det_hand NULL with the hand layer on: the annotations' hands only
    nohand = dict(c["det"], hand=None)
    want, _ = oracle(dict(c, det=nohand), ann_layers=ALL, det_layers=ALL)
    assert not np.array_equal(want, oracle(c, ann_layers=ALL, det_layers=ALL)[0])
    assert np.array_equal(device(DR, c, det=nohand, ann_layers=ALL, det_layers=ALL), want)
    # a [B,88] table (gt_table's) is one slot per image
    v = dict(c, gt=c["gt"][:, 0])
    want, _ = oracle(dict(c, gt=c["gt"][:, :1]), ann_layers=ALL, det_layers=ALL)
    assert np.array_equal(device(DR, v, ann_layers=ALL, det_layers=ALL), want)


def test_guard_bands_repeatability_and_streams(env, main_case):
    DR, _capi = env
    from tests._util import GuardedWorkspace
    c = main_case
    want, _ = oracle(c, ann_layers=ALL, det_layers=ALL, thickness=3)
    B, H, W = c["frames"].shape[:3]
    ws = GuardedWorkspace(B * H * W * 3, torch.device("cuda", torch.cuda.current_device()))
    ws.window.copy_(dev(c["frames"]).reshape(-1))
    gt, det, cub = dev(c["gt"]), {k: dev(v) for k, v in c["det"].items()}, dev(c["cuboids"])
    _capi.check(_capi.lib().hep_draw_poses_device(
        ws.ptr, B, H, W, gt.data_ptr(), int(gt.shape[1]), None, *[det[k].data_ptr() for k in DR.DETECTION_KEYS], int(det["scores"].shape[1]),
        c["score_threshold"], c["max_detections"], cub.data_ptr(), c["colours"].ctypes.data, len(c["colours"]), ALL, ALL, 3,
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert ws.changed() == []
    assert np.array_equal(ws.window.cpu().numpy().reshape(B, H, W, 3), want)
    again = device(DR, c, ann_layers=ALL, det_layers=ALL, thickness=3)
    assert np.array_equal(again, want)                               # a second run, byte-identical
    side = torch.cuda.Stream()
    frames = dev(c["frames"])
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        DR.draw_poses(frames, cuboids=cub, colours=c["colours"], gt=gt, detections=det, score_threshold=c["score_threshold"],
                      max_detections=c["max_detections"], ann_layers=ALL, det_layers=ALL, thickness=3)
    side.synchronize()
    assert np.array_equal(frames.cpu().numpy(), want)


def test_draw_poses_refuses_wrong_arguments(env, main_case):
    DR, _ = env
    c = main_case
    f, cub, gt = dev(c["frames"]), dev(c["cuboids"]), dev(c["gt"])
    det = {k: dev(v) for k, v in c["det"].items()}
    ok = dict(cuboids=cub, colours=c["colours"], gt=gt, detections=det, max_detections=3)
    bad = [dict(frames=f.float()), dict(frames=f[0]), dict(frames=f.cpu()), dict(frames=f[:, :, ::2]), dict(frames=f[:, :8]), dict(frames=f[..., :2]),
           dict(cuboids=cub.double()), dict(cuboids=cub[:, :7]), dict(cuboids=cub.cpu()), dict(cuboids=c["cuboids"].astype(np.float64)),
           dict(cuboids=torch.zeros(64, 8, 3, device="cuda")), dict(colours=c["colours"][:2]), dict(colours=c["colours"].astype(np.int32)),
           dict(gt=gt.float()), dict(gt=gt[:2]), dict(gt=gt[:, :, :80]), dict(gt=gt.cpu()), dict(gt=torch.zeros(3, 17, 88, dtype=torch.float64, device="cuda")),
           dict(camera=torch.zeros(3, 5, device="cuda")), dict(camera=torch.zeros(3, 6, dtype=torch.float64, device="cuda")),
           dict(camera=torch.zeros(3, 5, dtype=torch.float64)), dict(gt=None, camera=None),
           dict(detections={k: v for k, v in det.items() if k != "labels"}), dict(detections=dict(det, labels=det["labels"].long())),
           dict(detections=dict(det, boxes=det["boxes"][:, :, :3])), dict(detections=dict(det, hand=det["hand"][:, :5])),
           dict(detections=dict(det, scores=det["scores"].cpu())), dict(max_detections=0), dict(max_detections=7),
           dict(ann_layers=8), dict(det_layers=-1), dict(thickness=0), dict(thickness=9)]
    for change in bad:
        args = dict(ok, **change)
        frames = args.pop("frames", f)
        with pytest.raises(ValueError):
            DR.draw_poses(frames, **args)
    torch.cuda.synchronize()
    assert np.array_equal(f.cpu().numpy(), c["frames"])              # nothing was drawn by a refused call


def test_streaming_records_are_drawn(env):
    """Records of Session.top1 (seeded phi 0 model, size 128, batch 2) through detections_from_records: the drawn frames equal the
    oracle on the same values."""
    DR, _ = env
    from hmd_ego_pose_amd.model import Session
    from hmd_ego_pose_amd.weights import seeded_state_dict
    s = Session(seeded_state_dict(0, 0), 0, 128, 2, "fp32")
    try:
        rng = np.random.Generator(np.random.PCG64(77))
        x = torch.from_numpy(rng.standard_normal((2, 3, 128, 128)).astype(np.float32)).cuda()
        heads = s.forward(x, want_features=False)[1:]
        cam6 = torch.tensor([[480.0, 470.0, 61.0, 66.0, 1000.0, 0.5], [481.0, 470.0, 61.0, 65.0, 1000.0, 0.5]]).cuda()
        top = s.top1(cam6, 0.0, heads=heads)
        det = DR.detections_from_records(top["record"])
        host = {k: v.cpu().numpy() for k, v in det.items()}
        assert top["found"].cpu().numpy().tolist() == [1, 1] and host["boxes"].shape == (2, 1, 4)
        frames = rng.integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)
        cam = np.array([[480.0, 470.0, 61.0, 66.0, 0.5], [481.0, 470.0, 61.0, 65.0, 0.5]])
        c = dict(frames=frames, camera=cam, det=host, cuboids=D.case_cuboids(1), colours=DR.label_colours(1), score_threshold=0.0, max_detections=1)
        want, sh = oracle(c, given_depths=False, det_layers=ALL)              # the model's poses: tests/_draw.py assert_input_condition
        assert [len(im) for im in sh] == [1, 1] and (want != frames).any()
        got = DR.draw_poses(dev(frames), cuboids=c["cuboids"], camera=dev(cam), detections=det, score_threshold=0.0, max_detections=1, det_layers=ALL)
        assert np.array_equal(got.cpu().numpy(), want)
    finally:
        s.close()


def test_evaluate_device_saves_the_oracles_frames_and_keeps_the_metrics(env, tmp_path):
    """Three frames of a synthetic Linemod folder through evaluate_device(save_path=, draw_hand=True) at phi 0, size 128: the PNGs equal
    the oracle on the folder's frames and annotations and on the rows model.detect returns for the same batch; the metric dictionary is
    the one of a run without save_path, key for key and bit for bit."""
    DR, _ = env
    from PIL import Image
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from tests._util import make_linemod_folder
    make_linemod_folder(str(tmp_path / "ds"), n=3, size=128)
    ds = E.LinemodFolder(str(tmp_path / "ds"))
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0, onnx_export=True, input_sizes=[128] * 9)
    m.load_state_dict(seeded_state_dict(0, 0), strict=True)
    model = TrainModelWithLoss(m.to("cuda").eval()).eval()
    kw = dict(score_threshold=0.05, max_detections=10, iou_threshold=0.05, batch_size=3)
    plain = E.evaluate_device(ds, model, 128, **kw)
    out = tmp_path / "png"
    drawn = E.evaluate_device(ds, model, 128, save_path=str(out), draw_hand=True, **kw)
    assert list(plain) == list(drawn)
    for k in plain:
        assert np.array([plain[k]]).tobytes() == np.array([drawn[k]]).tobytes(), (k, plain[k], drawn[k])
    # the oracle on the same batch
    frames = np.stack([ds.load_image(i) for i in range(3)])
    gt = E.gt_table(ds.annotations, ds.camera, 1.0)
    u8 = torch.from_numpy(frames).cuda()
    cam = torch.from_numpy(np.stack([ds.camera_input(i, 1.0) for i in range(3)])).cuda()
    det = model.detect(model.model.session(128, 3, u8.device).preprocess(u8), cam)
    host = {k: det[k].cpu().numpy() for k in DR.DETECTION_KEYS}
    c = dict(frames=frames, gt=gt[:, None, :], det=host, cuboids=ds.cuboid[None], colours=DR.label_colours(1), score_threshold=0.05, max_detections=10)
    want, sh = oracle(c, given_depths=False, ann_layers=D.CUBOID | D.HAND, det_layers=D.CUBOID | D.HAND)
    assert all(im and im[0].annotation for im in sh) and (want != frames).any(axis=3).sum() > 300
    assert sorted(p.name for p in out.iterdir()) == ["0.png", "1.png", "2.png"]
    for i in range(3):
        got = np.asarray(Image.open(out / f"{i}.png"))
        assert got.shape == (128, 128, 3) and np.array_equal(got, want[i]), i


def test_scene_evaluator_draws_into_a_separate_buffer(env, tmp_path):
    """SceneEvaluator.add(draw_into=): a buffer of its own is drawn, the frames stay, and the result equals the oracle on the scene
    table and the batch's rows."""
    DR, _ = env
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from tests._util import make_linemod_folder
    make_linemod_folder(str(tmp_path / "ds"), n=2, size=128)
    ds = E.SceneFolder(str(tmp_path / "ds"), [1])
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0, onnx_export=True, input_sizes=[128] * 9)
    m.load_state_dict(seeded_state_dict(0, 0), strict=True)
    model = TrainModelWithLoss(m.to("cuda").eval()).eval()
    ev = E.SceneEvaluator(model, ds.models, 128, 2, ds.amax, score_threshold=0.05, iou_threshold=0.05, cuboids=ds.cuboids, draw_layers=ALL, draw_thickness=1)
    frames = np.stack([ds.load_image(i) for i in range(2)])
    gt = E.gt_scene_table(ds.annotations, ds.camera, 1.0, ds.amax)
    u8, canvas = torch.from_numpy(frames).cuda(), torch.from_numpy(frames).cuda()
    cam = torch.from_numpy(np.stack([ds.camera_input(i, 1.0) for i in range(2)])).cuda()
    with pytest.raises(ValueError):
        ev.add(u8, cam, torch.from_numpy(gt).cuda(), draw_into=canvas[:, :, ::2])
    with pytest.raises(ValueError):
        E.SceneEvaluator(model, ds.models, 128, 2, ds.amax).add(u8, cam, torch.from_numpy(gt).cuda(), draw_into=canvas)
    ev.add(u8, cam, torch.from_numpy(gt).cuda(), draw_into=canvas)
    det = model.detect(model.model.session(128, 2, u8.device).preprocess(u8), cam)
    host = {k: det[k].cpu().numpy() for k in DR.DETECTION_KEYS}
    c = dict(frames=frames, gt=gt, det=host, cuboids=ds.cuboids, colours=DR.label_colours(1), score_threshold=0.05, max_detections=10)
    want, _ = oracle(c, given_depths=False, ann_layers=ALL, det_layers=ALL, thickness=1)
    assert np.array_equal(u8.cpu().numpy(), frames) and (want != frames).any()
    assert np.array_equal(canvas.cpu().numpy(), want)
    assert ev.result()["mean"]["num_annotations"] == 2.0
