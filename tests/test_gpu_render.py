"""hep_render_models_device (object models under poses: mask, depth, filled overlay) against the numpy definition of tests/_render.py on
the SAME pose, camera and mesh tables: the mask byte for byte, the depth bit for bit as float32, the blended frames byte for byte.  The
rotation matrices are inputs of both sides (the kernel has no sin / cos), so no input condition is needed: every operation of the
definition is an IEEE + - * /, a floor, a comparison or an integer operation."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _render as R

pytestmark = pytest.mark.gpu
OUTPUTS = ("mask", "depth", "frames")


@pytest.fixture(scope="module")
def env():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd import render as RN
    assert torch.cuda.is_available()
    return RN, _capi


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def oracle(c, alpha=128):
    return R.render_models(c["poses"], c["camera"], c["vertices"], c["faces"], c["face_start"], c["H"], c["W"], frames=c.get("frames"),
                           colours=c.get("colours"), alpha=alpha)


def call(_capi, c, bufs, ws, ws_bytes=None, alpha=128, **over):
    """The C ABI on device tensors; ``bufs``: dict of output pointers (absent: NULL).  Returns the status."""
    t = dict(poses=dev(c["poses"]), camera=dev(c["camera"]), vertices=dev(c["vertices"]), faces=dev(c["faces"]))
    fs = np.ascontiguousarray(c["face_start"], np.int32)
    col = None if c.get("colours") is None else np.ascontiguousarray(c["colours"], np.uint8)
    a = dict(poses=t["poses"].data_ptr(), batch=c["poses"].shape[0], pmax=c["poses"].shape[1], camera=t["camera"].data_ptr(),
             vertices=t["vertices"].data_ptr(), num_vertices=len(c["vertices"]), faces=t["faces"].data_ptr(), num_faces=len(c["faces"]),
             face_start=fs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), num_labels=len(fs) - 1, height=c["H"], width=c["W"],
             mask=bufs.get("mask"), depth=bufs.get("depth"), frames=bufs.get("frames"), colours=None if col is None else col.ctypes.data, alpha=alpha,
             workspace=ws.data_ptr() if isinstance(ws, torch.Tensor) else ws, workspace_bytes=ws.numel() if ws_bytes is None else ws_bytes,
             stream=torch.cuda.current_stream().cuda_stream)
    a.update(over)
    rc = _capi.lib().hep_render_models_device(*a.values())
    torch.cuda.synchronize()
    return rc


def device(RN, c, outputs=OUTPUTS, alpha=128):
    """Through render_models; returns host arrays of the outputs asked for (the frames are a blended copy)."""
    frames = dev(c["frames"]) if "frames" in outputs else None
    out = RN.render_models(dev(c["poses"]), dev(c["camera"]), mesh_set(RN, c), c["H"], c["W"], mask="mask" in outputs, depth="depth" in outputs,
                           blend_into=frames, colours=c.get("colours"), alpha=alpha)
    assert set(out) == set(outputs) and (frames is None or out["frames"] is frames)
    return {k: v.cpu().numpy() for k, v in out.items()}


def mesh_set(RN, c):
    """A MeshSet holding the case's concatenated arrays as they are (cases with deliberately bad indices bypass the host check)."""
    m = RN.MeshSet.__new__(RN.MeshSet)
    m.device = torch.device("cuda", torch.cuda.current_device())
    m.vertices, m.faces, m.face_start = dev(c["vertices"]), dev(c["faces"]), np.ascontiguousarray(c["face_start"], np.int32)
    m.num_labels, m.num_vertices, m.num_faces = len(m.face_start) - 1, len(c["vertices"]), len(c["faces"])
    return m


def same(got, want, outputs=OUTPUTS):
    for k in outputs:
        g, w = got[k], want[k]
        if k == "depth":
            g, w = g.view(np.uint32), w.view(np.uint32)                  # bit for bit
        bad = np.argwhere(g != w)
        assert bad.size == 0, (k, len(bad), bad[:5].tolist())


@pytest.fixture(scope="module")
def scene():
    c = R.case_scene()
    return c, oracle(c)


def test_scene_of_three_images(env, scene):
    """48 x 80 (80 is no multiple of the 32 x 8 tile's width, 18 tiles; 33 x 47 below: neither side is), batch 3, pmax 4: a cube and a tetrahedron under three poses at different
    depths in image 0, no valid row in image 1, skipped faces, a mesh cut by the frame and one off screen in image 2."""
    RN, _ = env
    c, want = scene
    assert set(np.unique(want["mask"][0])) == {0, 7, 200, 255} and not want["mask"][1].any() and set(np.unique(want["mask"][2])) == {0, 3, 4, 5}
    got = device(RN, c)
    same(got, want)
    assert np.array_equal(got["frames"][1], c["frames"][1])


def test_one_partial_tile_and_every_subset_of_the_outputs(env):
    RN, _capi = env
    v, f, start = R.concat([R.cube(), R.tetrahedron()])
    poses = np.stack([R.pose_row(0, 11, R.rotation((1, 2, 0), 0.9), (0.0, 0.01, 0.3)), R.pose_row(1, 12, R.rotation((0, 1, 1), 2.0), (0.02, 0.0, 0.25))])[None]
    rng = np.random.Generator(np.random.PCG64(1))
    c = dict(poses=poses, camera=np.array([[30.0, 31.0, 8.2, 7.7, 1.0]]), vertices=v, faces=f, face_start=start, H=16, W=16,
             frames=rng.integers(0, 256, (1, 16, 16, 3), dtype=np.uint8), colours=np.array([[10, 250, 30], [200, 0, 99]], np.uint8))
    want = oracle(c, alpha=77)
    assert set(np.unique(want["mask"])) == {0, 11, 12}
    for outputs in (("mask",), ("depth",), ("frames",), ("mask", "depth"), ("mask", "frames"), ("depth", "frames"), OUTPUTS):
        same(device(RN, c, outputs, alpha=77), want, outputs)
    for alpha in (0, 1, 255, 256):
        same(device(RN, c, ("frames",), alpha=alpha), oracle(c, alpha=alpha), ("frames",))


def case_edges():
    """40 x 72, three single-triangle labels: 0 a face spanning the four tiles around (32, 32) - more than four, 1 a face entirely off screen, 2 a face with a
    vertex far outside whose SATURATED coordinates reach back over the frame."""
    tris = [np.array([[-0.1, -0.09, 0], [0.12, -0.02, 0.05], [-0.02, 0.1, -0.03]], np.float32), np.array([[-9, -1, 0], [-8, -1, 0], [-8.5, 1, 0]], np.float32),
            np.array([[-0.1, -0.1, 0], [3000.0, 0.0, 0], [-0.1, 0.2, 0]], np.float32)]
    v, f, start = R.concat([(t, np.array([[0, 1, 2]], np.int32)) for t in tris])
    poses = np.stack([R.pose_row(0, 1, None, (0.0, 0.02, 0.4)), R.pose_row(1, 2, None, (0, 0, 0.5)), R.pose_row(2, 3, None, (0.1, 0, 0.5))])[None]
    return dict(poses=poses, camera=np.array([[100.0, 100.0, 30.0, 28.0, 1.0]]), vertices=v, faces=f, face_start=start, H=40, W=72)


def test_faces_across_tiles_off_screen_and_saturated(env):
    RN, _ = env
    c = case_edges()
    want = oracle(c)
    m = want["mask"][0]
    assert all((m[y:y + 8, x:x + 32] == 1).any() for y in (24, 32) for x in (0, 32))                                                # four tiles
    assert not (m == 2).any() and (m == 3).sum() > 100
    assert R.project(c["poses"][0, 2], c["camera"][0], c["vertices"])[0][7] == 131056                                                # saturated
    same(device(RN, c, ("mask", "depth")), want, ("mask", "depth"))


def test_depth_ties_and_face_index_ties(env):
    """Two slots with the same mesh and pose (the lower slot's mask value wins everywhere) and a mesh listed twice in ``faces`` (same
    result as listed once); then both orders of two different mask values."""
    RN, _ = env
    v, f = R.cube()
    row = R.pose_row(0, 50, R.rotation((1, 1, 1), 0.8), (0.01, 0.0, 0.3))
    second = row.copy()
    second[2] = 60
    base = dict(camera=np.array([[60.0, 60.0, 24.0, 20.0, 1.0]]), vertices=v, H=40, W=48)
    once = oracle(dict(base, poses=row[None, None], faces=f, face_start=[0, 12]))
    for poses, value in ((np.stack([row, second])[None], 50), (np.stack([second, row])[None], 60)):
        c = dict(base, poses=poses, faces=np.concatenate([f, f]), face_start=[0, 24])
        want = oracle(c)
        assert set(np.unique(want["mask"])) == {0, value} and np.array_equal(want["depth"], once["depth"]) and (want["key"][want["mask"] > 0] < 12).all()
        same(device(RN, c, ("mask", "depth")), want, ("mask", "depth"))


def test_pmax_sixteen_with_rows_0_7_and_15(env):
    RN, _ = env
    v, f, start = R.concat([R.cube(), R.tetrahedron()])
    poses = np.zeros((1, 16, 16))
    poses[0, :, 4:13] = np.eye(3).reshape(9)                       # rows that are not valid still hold finite numbers ...
    poses[0, 3] = R.pose_row(0, 99, None, (0, 0, 0.2), valid=0.0)  # ... and one a pose that would cover the frame
    poses[0, 0] = R.pose_row(0, 1, R.rotation((1, 0, 1), 0.5), (-0.04, 0.0, 0.3))
    poses[0, 7] = R.pose_row(1, 8, R.rotation((0, 1, 0), 1.5), (0.03, 0.01, 0.28))
    poses[0, 15] = R.pose_row(0, 16, R.rotation((0, 0, 1), 0.7), (0.0, -0.03, 0.34))
    c = dict(poses=poses, camera=np.array([[70.0, 70.0, 23.5, 16.5, 1.0]]), vertices=v, faces=f, face_start=start, H=33, W=47)
    want = oracle(c)
    assert set(np.unique(want["mask"])) == {0, 1, 8, 16}
    same(device(RN, c, ("mask", "depth")), want, ("mask", "depth"))


def test_more_faces_than_any_list_holds(env):
    """A fan of 2 * 4096 + 1 faces over the same screen triangle of one tile, each nearer than the one before: the list (at most 4096
    faces by the ABI's contract, 512 in this build) is flushed many times and the nearest face is the LAST."""
    RN, _ = env
    n = 2 * 4096 + 1
    z = np.linspace(0.9, 0.3, n)
    tri = np.array([[-0.08, -0.07, 1.0], [0.09, -0.05, 1.0], [0.0, 0.1, 1.0]])
    v = (tri[None, :, :] * z[:, None, None]).reshape(-1, 3).astype(np.float32)
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    c = dict(poses=R.pose_row(0, 5, None, (0, 0, 0))[None, None], camera=np.array([[40.0, 40.0, 8.0, 8.0, 1.0]]), vertices=v, faces=f, face_start=[0, n], H=16, W=16)
    want = oracle(c)
    assert (want["key"][want["mask"] > 0] == n - 1).sum() > 10 and want["depth"][0, 8, 8] == np.float32(z[-1].astype(np.float32))
    same(device(RN, c, ("mask", "depth")), want, ("mask", "depth"))


def test_out_of_range_face_indices_are_skipped_not_read(env):
    RN, _ = env
    v, f = R.cube()
    bad = np.concatenate([[[0, 1, 8], [-1, 2, 3], [2 ** 31 - 1, 0, 1]], f]).astype(np.int32)
    c = dict(poses=R.pose_row(0, 9, R.rotation((1, 0, 0), 0.4), (0, 0, 0.3))[None, None], camera=np.array([[50.0, 50.0, 16.0, 16.0, 1.0]]), vertices=v, faces=bad,
             face_start=[0, 15], H=32, W=32)
    want = oracle(c)
    assert (want["mask"] == 9).sum() > 100 and (want["key"][want["mask"] > 0] >= 3).all()
    same(device(RN, c, ("mask", "depth")), want, ("mask", "depth"))


def test_guard_words_poisoned_buffers_and_repeatability(env, scene):
    """The ABI on exact-size windows between guard words: all three outputs and the workspace; mask and depth start as NaN bytes (image 1,
    which has no valid row, must come back zero), and a second run gives the same bits."""
    RN, _capi = env
    from tests._util import GuardedWorkspace
    c, want = scene
    B, H, W = c["frames"].shape[:3]
    d = torch.device("cuda", torch.cuda.current_device())
    need = _capi.check(_capi.lib().hep_render_workspace_bytes(B, H, W, c["poses"].shape[1], len(c["vertices"])))
    assert need == B * c["poses"].shape[1] * (len(c["vertices"]) + 1) * 16
    runs = []
    for _ in range(2):
        g = dict(mask=GuardedWorkspace(B * H * W, d), depth=GuardedWorkspace(B * H * W * 4, d), frames=GuardedWorkspace(B * H * W * 3, d), ws=GuardedWorkspace(need, d))
        g["frames"].window.copy_(dev(c["frames"]).reshape(-1))
        assert call(_capi, c, {k: g[k].ptr for k in OUTPUTS}, g["ws"].ptr, ws_bytes=need) == 0
        assert [g[k].changed() for k in g] == [[]] * 4
        got = dict(mask=g["mask"].window.cpu().numpy().reshape(B, H, W), depth=g["depth"].window.cpu().numpy().view(np.float32).reshape(B, H, W),
                   frames=g["frames"].window.cpu().numpy().reshape(B, H, W, 3))
        same(got, want)
        runs.append(got)
    assert not runs[0]["mask"][1].any() and not runs[0]["depth"][1].view(np.uint32).any()
    assert all(runs[0][k].tobytes() == runs[1][k].tobytes() for k in OUTPUTS)


def test_refused_arguments_launch_nothing(env, scene):
    RN, _capi = env
    c, _want = scene
    B, H, W = c["frames"].shape[:3]
    need = _capi.check(_capi.lib().hep_render_workspace_bytes(B, H, W, c["poses"].shape[1], len(c["vertices"])))
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    out = dict(mask=torch.full((B, H, W), 77, dtype=torch.uint8, device="cuda"), depth=torch.full((B, H, W), -3.0, device="cuda"), frames=dev(c["frames"]))
    bufs = {k: v.data_ptr() for k, v in out.items()}
    INVALID, UNSUPPORTED = -1, -4
    down = np.ascontiguousarray([0, 16, 12], np.int32)
    beyond = np.ascontiguousarray([0, 12, 17], np.int32)
    below = np.ascontiguousarray([-1, 12, 16], np.int32)
    as_ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    cases = [(dict(poses=None), INVALID), (dict(camera=None), INVALID), (dict(vertices=None), INVALID), (dict(faces=None), INVALID), (dict(face_start=None), INVALID),
             (dict(workspace=None), INVALID), (dict(mask=None, depth=None, frames=None), INVALID), (dict(batch=0), INVALID), (dict(pmax=0), INVALID),
             (dict(pmax=17), INVALID), (dict(num_vertices=0), INVALID), (dict(num_vertices=(1 << 24) + 1), INVALID), (dict(num_faces=0), INVALID),
             (dict(num_faces=(1 << 24) + 1), INVALID), (dict(num_labels=0), INVALID), (dict(num_labels=64), INVALID), (dict(face_start=as_ptr(down)), INVALID),
             (dict(face_start=as_ptr(beyond)), INVALID), (dict(face_start=as_ptr(below)), INVALID), (dict(colours=None), INVALID), (dict(alpha=-1), INVALID),
             (dict(alpha=257), INVALID), (dict(workspace_bytes=need - 1), INVALID), (dict(workspace=ws.data_ptr() + 8), INVALID),
             (dict(height=15), UNSUPPORTED), (dict(width=4097), UNSUPPORTED), (dict(height=4097), UNSUPPORTED), (dict(width=15), UNSUPPORTED)]
    assert _capi.lib().hep_render_workspace_bytes(B, 15, W, 4, 20) == UNSUPPORTED and _capi.lib().hep_render_workspace_bytes(B, H, W, 17, 20) == INVALID
    for over, code in cases:
        rc = call(_capi, c, bufs, ws, ws_bytes=need, **over)
        assert rc == code, (list(over), rc)
        assert _capi.lib().hep_last_error().decode().startswith("hep_render_models_device: "), list(over)
    assert (out["mask"] == 77).all() and (out["depth"] == -3.0).all() and np.array_equal(out["frames"].cpu().numpy(), c["frames"]) and not ws.any()
    # without frames neither colours nor alpha is read
    assert call(_capi, c, dict(mask=bufs["mask"]), ws, ws_bytes=need, colours=None, alpha=999) == 0
    with pytest.raises(ValueError):
        RN.render_models(dev(c["poses"]).float(), dev(c["camera"]), mesh_set(RN, c), H, W)
    with pytest.raises(ValueError):
        RN.render_models(dev(c["poses"]).cpu(), dev(c["camera"]), mesh_set(RN, c), H, W)


def test_rendered_masks_feed_augment_6dof(env):
    """Masks from poses into the training input: image 0 with apply = 0 - its boxes, made from the rendered mask with torch on the device,
    pass through; image 1 with apply = 1 at angle 0 and scale 1 - the augmentation reads the boxes off the rendered mask itself (the
    identity warp keeps the mask: asserted on its oracle).  Both equal the extents of the ORACLE's mask, times the image scale."""
    RN, _ = env
    from hmd_ego_pose_amd import augment as A
    from tests import _augment as AO
    H = W = 64
    v, f, start = R.concat([R.cube(), R.tetrahedron()])
    rows = [[R.pose_row(0, 40, R.rotation((1, 2, 3), 0.6), (-0.04, 0.02, 0.4)), R.pose_row(1, 90, R.rotation((2, 0, 1), 1.1), (0.05, -0.03, 0.35))],
            [R.pose_row(1, 90, R.rotation((0, 1, 0), 0.3), (-0.03, -0.04, 0.3)), R.pose_row(0, 40, R.rotation((1, 0, 0), 2.2), (0.04, 0.04, 0.45))]]
    c = dict(poses=np.array(rows), camera=np.tile(np.array([120.0, 120.0, 32.0, 32.0, 1.0]), (2, 1)), vertices=v, faces=f, face_start=start, H=H, W=W)
    want = oracle(c)["mask"]
    mesh = RN.MeshSet([R.cube(), R.tetrahedron()])
    mask = RN.render_models(dev(c["poses"]), dev(c["camera"]), mesh, H, W)["mask"]
    values = c["poses"][:, :, 2].astype(np.int32)
    boxes = np.array([AO._boxes_of(want[b], values[b]) for b in range(2)])
    assert (boxes[:, :, 2] > boxes[:, :, 0]).all()
    M = AO.forward_matrix(0.0, 1.0, 32.0, 32.0)
    assert np.array_equal(AO.warp_nearest(want[1], M), want[1])
    given = torch.zeros(2, 2, 4, dtype=torch.float64, device="cuda")
    for k in range(2):                                               # image 0: extents of the DEVICE mask, with torch
        ys, xs = torch.nonzero(mask[0] == int(values[0, k]), as_tuple=True)
        given[0, k] = torch.stack([xs.min(), ys.min(), xs.max(), ys.max()]).double()
    given[1] = -5.0                                                  # image 1: the call replaces them
    ann = dict(boxes=given, labels=dev(c["poses"][:, :, 1].astype(np.int32)), mask_values=dev(values), rvec=torch.zeros(2, 2, 3, device="cuda"),
               tvec=dev(c["poses"][:, :, 13:16].astype(np.float32)), extra=torch.zeros(2, 2, 2, device="cuda"), num_gt=torch.tensor([2, 2], dtype=torch.int32, device="cuda"))
    frames = torch.zeros(2, H, W, 3, dtype=torch.uint8, device="cuda")
    out = A.augment_6dof(frames, mask, ann, np.tile(np.array([120.0, 120.0, 32.0, 32.0], np.float32), (2, 1)), [0.0, 0.0], [1.0, 1.0], [0, 1], 128)
    assert out["applied"].cpu().tolist() == [0, 1] and out["gt_num"].cpu().tolist() == [2, 2]
    assert np.array_equal(out["mask"].cpu().numpy(), want)
    assert np.array_equal(out["gt_boxes"].cpu().numpy(), boxes * (128 / 64))


def test_device_evaluator_blends_the_models_beneath_the_lines(env, tmp_path):
    """DeviceEvaluator.add(draw_into=, meshes=): the oracle's blend on the evaluator's own pose table, then tests/_draw.py's lines; a second
    evaluator without meshes gives the same metrics; evaluate_device(draw_model=) refuses a folder whose PLY file has no faces."""
    RN, _ = env
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import draw as DR
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from tests import _draw as D
    from tests._util import make_linemod_folder
    make_linemod_folder(str(tmp_path / "ds"), n=2, size=128)
    ds = E.LinemodFolder(str(tmp_path / "ds"))
    m = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=0, onnx_export=True, input_sizes=[128] * 9)
    m.load_state_dict(seeded_state_dict(0, 0), strict=True)
    model = TrainModelWithLoss(m.to("cuda").eval()).eval()
    kw = dict(score_threshold=0.05, max_detections=10, iou_threshold=0.05)
    frames = np.stack([ds.load_image(i) for i in range(2)])
    gt = E.gt_table(ds.annotations, ds.camera, 1.0)
    cam = torch.from_numpy(np.stack([ds.camera_input(i, 1.0) for i in range(2)])).cuda()
    mesh = RN.MeshSet([R.cube(60.0)])
    ev = E.DeviceEvaluator(model, ds.points, ds.diameter, 128, 2, cuboid=ds.cuboid, **kw)
    u8, canvas = torch.from_numpy(frames).cuda(), torch.from_numpy(frames).cuda()
    with pytest.raises(ValueError):
        ev.add(u8, cam, torch.from_numpy(gt).cuda(), meshes=mesh)                               # nothing to blend into
    with pytest.raises(ValueError):
        ev.add(u8, cam, torch.from_numpy(gt).cuda(), draw_into=canvas, meshes=R.cube(60.0))
    with pytest.raises(ValueError):
        E.DeviceEvaluator(model, ds.points, ds.diameter, 128, 2, cuboid=ds.cuboid, score_threshold=0.05, max_detections=17).add(
            u8, cam, torch.from_numpy(gt).cuda(), draw_into=canvas, meshes=mesh)
    assert ev.count == 0 and np.array_equal(canvas.cpu().numpy(), frames)
    ev.add(u8, cam, torch.from_numpy(gt).cuda(), draw_into=canvas, meshes=mesh)
    plain = E.DeviceEvaluator(model, ds.points, ds.diameter, 128, 2, **kw)
    plain.add(u8, cam, torch.from_numpy(gt).cuda())
    a, b = ev.result(), plain.result()
    assert list(a) == list(b) and all(np.array([a[k]]).tobytes() == np.array([b[k]]).tobytes() for k in a)
    # the oracle on the same rows: the pose table the evaluator made (device Rodrigues) is the input of both renderers
    det = model.detect(model.model.session(128, 2, u8.device).preprocess(u8), cam)
    poses = RN.poses_from_detections(det, 0.05, 10).cpu().numpy()
    v, f = R.cube(60.0)
    filled = R.render_models(poses, gt[:, 14:19], v, f, [0, 12], 128, 128, frames=frames, colours=DR.label_colours(1), alpha=128)
    assert (filled["mask"] > 0).sum() > 200
    host = {k: det[k].cpu().numpy() for k in DR.DETECTION_KEYS}
    want = D.draw_poses(filled["frames"], ds.cuboid[None], DR.label_colours(1), gt=gt[:, None, :], det=host, score_threshold=0.05, max_detections=10)
    assert (want != filled["frames"]).any()
    assert np.array_equal(canvas.cpu().numpy(), want)
    with pytest.raises(ValueError, match="draw_model needs triangle faces"):
        E.evaluate_device(ds, model, 128, save_path=str(tmp_path / "png"), draw_model=True, batch_size=2, **kw)
    with pytest.raises(ValueError, match="save_path"):
        E.evaluate_device(ds, model, 128, draw_model=True, batch_size=2, **kw)
