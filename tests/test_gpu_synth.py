"""hep_synth_frames_device (shaded models composited over backgrounds, visible boxes, padded annotations) against the numpy definition of
tests/_synth.py on the SAME tables: frames and mask byte for byte, depth bit for bit as float32, visible and the annotation tensors value
for value (float64 boxes and float32 gathers by their bits).  No tolerance and no input condition: every operation of the definition is an
IEEE + - * /, a floor, a comparison or an integer operation; rotation matrices, normals and lights are inputs of both sides."""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests import _render as R
from tests import _synth as S

pytestmark = pytest.mark.gpu
ANN = ("boxes", "labels", "mask_values", "rvec", "tvec", "extra", "num_gt", "slot_of")
ANN_TYPES = dict(boxes=(np.float64, (4,)), labels=(np.int32, ()), mask_values=(np.int32, ()), rvec=(np.float32, (3,)), tvec=(np.float32, (3,)), extra=(np.float32, (2,)),
                 slot_of=(np.int32, ()))
INVALID, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def env():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd import synth as SY
    assert torch.cuda.is_available()
    return SY, _capi


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def same(got, want, keys):
    for k in keys:
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (k, len(bad), bad[:5].tolist())


def mesh_set(SY, c):
    """A ShadedMeshSet holding the case's arrays as they are: its normals are the CASE's (a zeroed one included), not recomputed."""
    m = SY.ShadedMeshSet.__new__(SY.ShadedMeshSet)
    m.device = torch.device("cuda", torch.cuda.current_device())
    m.vertices, m.faces, m.face_start = dev(c["vertices"]), dev(c["faces"]), np.ascontiguousarray(c["face_start"], np.int32)
    m.vertex_colours, m.face_normals = dev(c["vertex_colours"]), dev(c["face_normals"])
    m.num_labels, m.num_vertices, m.num_faces = len(m.face_start) - 1, len(c["vertices"]), len(c["faces"])
    return m


def sizes(c):
    B, K = c["poses"].shape[:2]
    H, W = c["H"], c["W"]
    out = dict(frames=B * H * W * 3, mask=B * H * W, depth=B * H * W * 4, visible=B * K * 5 * 4, num_gt=B * 4)
    for k, (t, tail) in ANN_TYPES.items():
        out[k] = B * K * int(np.prod(tail, dtype=np.int64)) * np.dtype(t).itemsize
    return out


def call(_capi, c, ptrs, ws, ws_bytes, alpha=256, min_pixels=16, **over):
    """The C ABI on device tensors; ``ptrs``: dict of output pointers (absent: NULL) - frames, mask, depth, visible and the eight of ANN;
    the three annotation inputs go in when any annotation output does.  Returns the status."""
    t = {k: dev(c[k]) for k in ("poses", "camera", "vertices", "vertex_colours", "faces", "face_normals", "lights", "rvec", "tvec", "extra")}
    fs = np.ascontiguousarray(c["face_start"], np.int32)
    group = any(k in ptrs for k in ANN)
    a = dict(poses=t["poses"].data_ptr(), batch=c["poses"].shape[0], pmax=c["poses"].shape[1], camera=t["camera"].data_ptr(), vertices=t["vertices"].data_ptr(),
             vertex_colours=t["vertex_colours"].data_ptr(), num_vertices=len(c["vertices"]), faces=t["faces"].data_ptr(), face_normals=t["face_normals"].data_ptr(),
             num_faces=len(c["faces"]), face_start=fs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), num_labels=len(fs) - 1, lights=t["lights"].data_ptr(),
             height=c["H"], width=c["W"], frames=ptrs.get("frames"), alpha=alpha, mask=ptrs.get("mask"), depth=ptrs.get("depth"), visible=ptrs.get("visible"),
             rvec=t["rvec"].data_ptr() if group else None, tvec=t["tvec"].data_ptr() if group else None, extra=t["extra"].data_ptr() if group else None,
             min_pixels=min_pixels, boxes=ptrs.get("boxes"), labels=ptrs.get("labels"), mask_values=ptrs.get("mask_values"), out_rvec=ptrs.get("rvec"),
             out_tvec=ptrs.get("tvec"), out_extra=ptrs.get("extra"), num_gt=ptrs.get("num_gt"), slot_of=ptrs.get("slot_of"), workspace=ws, workspace_bytes=ws_bytes,
             stream=torch.cuda.current_stream().cuda_stream)
    a.update(over)
    rc = _capi.lib().hep_synth_frames_device(*a.values())
    torch.cuda.synchronize()
    return rc


def abi(_capi, c, outputs, alpha=256, min_pixels=16):
    """The ABI into fresh poisoned tensors; returns host arrays of ``outputs`` (names of sizes(c))."""
    B, K = c["poses"].shape[:2]
    H, W = c["H"], c["W"]
    need = _capi.check(_capi.lib().hep_synth_workspace_bytes(B, H, W, K, len(c["vertices"])))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    bufs = {k: torch.full((sizes(c)[k],), 0xA5, dtype=torch.uint8, device="cuda") for k in outputs}
    bufs["frames"] = dev(c["frames"]).reshape(-1)
    assert call(_capi, c, {k: v.data_ptr() for k, v in bufs.items()}, ws.data_ptr(), need, alpha=alpha, min_pixels=min_pixels) == 0, _capi.lib().hep_last_error()
    return unpack(c, {k: v.cpu().numpy() for k, v in bufs.items()})


def unpack(c, raw):
    B, K = c["poses"].shape[:2]
    H, W = c["H"], c["W"]
    shapes = dict(frames=(np.uint8, (B, H, W, 3)), mask=(np.uint8, (B, H, W)), depth=(np.float32, (B, H, W)), visible=(np.int32, (B, K, 5)), num_gt=(np.int32, (B,)))
    shapes.update({k: (t, (B, K) + tail) for k, (t, tail) in ANN_TYPES.items()})
    return {k: v.view(shapes[k][0])[:int(np.prod(shapes[k][1]))].reshape(shapes[k][1]) for k, v in raw.items()}


def flat(want):
    """The oracle's dict with the annotation tensors at the top level, as the ABI names them."""
    out = {k: want[k] for k in ("frames", "mask", "depth", "visible")}
    if want["annotations"] is not None:
        out.update(want["annotations"])
    return out


@pytest.fixture(scope="module")
def overlap():
    c = S.case_overlap()
    return c, flat(S.run(c))


# ---- 1. the scene of three images ------------------------------------------------------------------------------------------------
def test_overlapping_models_every_output_and_every_subset(env, overlap):
    SY, _capi = env
    c, want = overlap
    assert tuple(want["visible"][0, 2]) == S.EMPTY and want["num_gt"].tolist() == [2, 2, 3] and want["visible"][2, 0, 2] == c["W"] - 1
    alone = R.render_models(c["poses"][:1, 1:2], c["camera"][:1], c["vertices"], c["faces"], c["face_start"], c["H"], c["W"])["mask"][0]
    assert (alone > 0).sum() != want["visible"][0, 1, 4]                      # the visible box is not the projected one
    every = ("frames", "mask", "depth", "visible") + ANN
    same(abi(_capi, c, every), want, every)
    for subset in (("visible",), ("mask", "visible"), ("depth", "visible"), ("mask", "depth", "visible"), ("visible",) + ANN, ("depth", "visible") + ANN):
        keys = ("frames",) + subset
        same(abi(_capi, c, subset), want, keys)


def table_case(SY, poses_ann, c):
    """``c`` with its pose table replaced by what ``synth_frames`` builds on the device from the padded annotations (so both sides shade the
    same doubles), and the padded inputs of the gather."""
    from hmd_ego_pose_amd.render import poses_from_annotations
    table = poses_from_annotations(poses_ann).cpu().numpy()
    return dict(c, poses=table, rvec=poses_ann["rvec"].cpu().numpy(), tvec=poses_ann["tvec"].cpu().numpy(), extra=poses_ann["extra"].cpu().numpy())


def drawn_case(SY, B=3, K=3, H=44, W=72, seed=9):
    from hmd_ego_pose_amd.augment import pad_annotations
    cam4 = np.array([88.0, 90.0, W / 2 - 0.4, H / 2 + 0.3])
    dicts = SY.draw_poses(random.Random(seed), B, K, cam4, H, W, (0.25, 0.45), labels=[0, 1, 0], mask_values=[5, 6, 7], symmetric=[0, 1, 0])
    ann = pad_annotations(dicts, "cuda")
    meshes = [R.cube() + (S.colours_for(8, 1),), R.tetrahedron() + (S.colours_for(4, 2),)]
    mesh = SY.ShadedMeshSet(meshes)
    lights = SY.draw_lights(random.Random(seed + 1), B)
    rng = np.random.Generator(np.random.PCG64(seed))
    c = dict(camera=np.tile(np.append(cam4, 1.0), (B, 1)), vertices=mesh.host_vertices, vertex_colours=mesh.host_vertex_colours, faces=mesh.host_faces,
             face_normals=mesh.host_face_normals, face_start=mesh.face_start, lights=lights, H=H, W=W, frames=rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8))
    return table_case(SY, ann, c), ann, mesh, cam4


def test_synth_frames_on_drawn_poses(env):
    """Through the Python entry: draw_poses -> pad_annotations -> synth_frames, every output and the optional ones off."""
    SY, _ = env
    c, ann, mesh, _ = drawn_case(SY)
    want = flat(S.run(c, alpha=200, min_pixels=8))
    assert want["num_gt"].sum() >= 5
    frames = dev(c["frames"])
    out = SY.synth_frames(frames, ann, dev(c["camera"]), mesh, c["lights"], alpha=200, min_pixels=8, mask=True, depth=True)
    assert out["frames"] is frames and set(out) == {"frames", "mask", "depth", "visible", "annotations"} and set(out["annotations"]) == set(ANN)
    got = {k: out[k].cpu().numpy() for k in ("frames", "mask", "depth", "visible")}
    got.update({k: v.cpu().numpy() for k, v in out["annotations"].items()})
    same(got, want, ("frames", "mask", "depth", "visible") + ANN)
    bare = SY.synth_frames(dev(c["frames"]), ann, dev(c["camera"]), mesh, dev(c["lights"]), alpha=200, min_pixels=8, mask=False)
    assert set(bare) == {"frames", "visible", "annotations"} and np.array_equal(bare["frames"].cpu().numpy(), want["frames"])
    assert np.array_equal(bare["annotations"]["boxes"].cpu().numpy(), want["boxes"])


# ---- 2. sixteen slots ----------------------------------------------------------------------------------------------------------------
def test_pmax_sixteen_rows_0_7_15_off_frame_bad_label_and_min_pixels(env):
    _, _capi = env
    v, f, start = R.concat([R.cube(), R.tetrahedron()])
    poses = np.zeros((1, 16, 16))
    poses[0, :, 4:13] = np.eye(3).reshape(9)
    poses[0, 3] = R.pose_row(0, 99, None, (0, 0, 0.2), valid=0.0)            # would cover the frame
    poses[0, 0] = R.pose_row(0, 1, R.rotation((1, 0, 1), 0.5), (-0.04, 0.0, 0.3))
    poses[0, 5] = R.pose_row(0, 6, R.rotation((1, 0, 0), 0.3), (-9.0, 0.0, 0.4))      # wholly off frame
    poses[0, 7] = R.pose_row(1, 8, R.rotation((0, 1, 0), 1.5), (0.03, 0.01, 0.28))
    poses[0, 11] = R.pose_row(2, 12, None, (0.0, 0.0, 0.25))                # label out of range
    poses[0, 15] = R.pose_row(0, 16, R.rotation((0, 0, 1), 0.7), (0.0, -0.03, 0.34))
    rvec, tvec, extra = S.padded_inputs(1, 16)
    rng = np.random.Generator(np.random.PCG64(3))
    c = dict(poses=poses, camera=np.array([[70.0, 70.0, 23.5, 16.5, 1.0]]), vertices=v, vertex_colours=S.colours_for(len(v), 6), faces=f, face_normals=S.face_normals(v, f),
             face_start=start, lights=S.light_row((0.5, 0.5, -1.0))[None], H=33, W=47, frames=rng.integers(0, 256, (1, 33, 47, 3), dtype=np.uint8), rvec=rvec, tvec=tvec, extra=extra)
    every = ("frames", "mask", "visible") + ANN
    counts = S.run(c)["visible"][0, :, 4]
    n15 = int(counts[15])
    assert 16 < n15 < min(counts[0], counts[7])                              # slot 15 wins the fewest pixels: min_pixels at the two sides of ITS count
    for min_pixels, slots in ((n15, [0, 7, 15]), (n15 + 1, [0, 7])):
        want = flat(S.run(c, min_pixels=min_pixels))
        assert want["slot_of"][0].tolist() == slots + [-1] * (16 - len(slots)) and want["visible"][0, [3, 5, 11], 4].tolist() == [0, 0, 0]
        same(abi(_capi, c, every, min_pixels=min_pixels), want, every)


# ---- 3. a list flushed mid-slot, windings, a zero normal, saturation, NaN, alpha ---------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_case():
    v, f = S.sphere(0.05, 24, 40)                                             # 1840 faces, most of them over the one tile of a 16 x 16 frame
    f = f.copy()
    f[::3] = f[::3][:, [0, 2, 1]]                                            # mixed windings
    n = S.face_normals(v, f)
    n[5::7] = 0.0                                                            # zero normals among them
    rng = np.random.Generator(np.random.PCG64(12))
    lights = np.stack([S.light_row((0.3, -0.2, -1.0), 0.3, 0.7), S.light_row((0.0, 1.0, -1.0), 0.4, 0.6, (1.0, 40.0, 0.01)), S.light_row((1.0, 0.0, 0.0), 0.5, 0.5)])
    lights[2, 1] = np.nan
    poses = np.stack([R.pose_row(0, 3, R.rotation((1, 2, 0), 0.9 + b), (0.001 * b, 0.0, 0.11)) for b in range(3)])[:, None]
    rvec, tvec, extra = S.padded_inputs(3, 1)
    return dict(poses=poses, camera=np.tile(np.array([16.0, 16.0, 8.0, 8.0, 1.0]), (3, 1)), vertices=v, vertex_colours=S.colours_for(len(v), 8), faces=f, face_normals=n,
                face_start=np.array([0, len(f)], np.int32), lights=lights, H=16, W=16, frames=rng.integers(0, 256, (3, 16, 16, 3), dtype=np.uint8), rvec=rvec, tvec=tvec, extra=extra)


@pytest.mark.parametrize("alpha", [256, 128, 0])
def test_sphere_flushes_the_list_mixed_windings_zero_normals_saturation_nan(env, sphere_case, alpha):
    _, _capi = env
    c = sphere_case
    sx, sy, _w, ok = R.project(c["poses"][0, 0], c["camera"][0], c["vertices"])
    tri = c["faces"]
    meets = (sx[tri].max(1) >= 8) & (sx[tri].min(1) <= 16 * 15 + 8) & (sy[tri].max(1) >= 8) & (sy[tri].min(1) <= 16 * 15 + 8) & ok[tri].all(1)
    assert meets.sum() > 512                                                 # more than one list of the rasteriser: flushed inside the slot
    full = S.run(c, alpha=alpha)
    want = flat(full)
    if alpha == 256:
        hit = want["mask"] > 0
        assert (want["frames"][1][hit[1]][:, 1] == 255).mean() > 0.9 and not want["frames"][2][hit[2]].any() and hit.sum() > 300      # saturated; NaN light
        won = c["face_normals"][full["key"][0][hit[0]] & 0xFFFFFF]
        assert (won == 0).all(1).any() and (won != 0).any(1).any()                       # faces with a zero normal won pixels, and others did
    every = ("frames", "mask", "depth", "visible") + ANN
    same(abi(_capi, c, every, alpha=alpha), want, every)


# ---- 4. mask and depth against the renderer on the device ------------------------------------------------------------------------------
def test_mask_and_depth_equal_render_models_on_the_device(env, overlap):
    SY, _capi = env
    from hmd_ego_pose_amd import render as RN
    c, _want = overlap
    mesh = mesh_set(SY, c)
    ren = RN.render_models(dev(c["poses"]), dev(c["camera"]), mesh, c["H"], c["W"], mask=True, depth=True)
    got = abi(_capi, c, ("mask", "depth", "visible"))
    assert np.array_equal(ren["mask"].cpu().numpy(), got["mask"]) and np.array_equal(ren["depth"].cpu().numpy().view(np.uint32), got["depth"].view(np.uint32))


# ---- 5. guard words, poison, repeatability, no annotation group -----------------------------------------------------------------------------
def guarded(c, names, d):
    from tests._util import GuardedWorkspace
    return {k: GuardedWorkspace((sizes(c)[k] + 15) // 16 * 16, d) for k in names}


def tails_intact(g, c):
    """The bytes between an output's exact size and its 16-byte window still hold the window's NaN poison."""
    for k, w in g.items():
        n = sizes(c).get(k)
        if n is not None and n < w.nbytes:
            tail = w.window[n:].cpu().numpy()
            fresh = np.full(w.nbytes // 4, np.nan, np.float32).view(np.uint8)[n:]
            if k != "frames" and not np.array_equal(tail, fresh):
                return k
    return None


def test_guard_words_poisoned_outputs_two_runs_and_no_annotation_group(env, overlap):
    SY, _capi = env
    c, want = overlap
    B, K = c["poses"].shape[:2]
    d = torch.device("cuda", torch.cuda.current_device())
    need = _capi.check(_capi.lib().hep_synth_workspace_bytes(B, c["H"], c["W"], K, len(c["vertices"])))
    assert need == B * K * (len(c["vertices"]) + 1) * 16
    every = ("frames", "mask", "depth", "visible") + ANN
    runs = []
    for names in (every, every, ("frames", "mask", "depth", "visible")):
        from tests._util import GuardedWorkspace
        g = guarded(c, names, d)
        ws = GuardedWorkspace(need, d)
        g["frames"].window[:sizes(c)["frames"]].copy_(dev(c["frames"]).reshape(-1))
        assert call(_capi, c, {k: g[k].ptr for k in names}, ws.ptr, need) == 0
        assert [g[k].changed() for k in g] == [[]] * len(g) and ws.changed() == [] and tails_intact(g, c) is None
        got = unpack(c, {k: g[k].window.cpu().numpy() for k in names})
        same(got, want, names)
        runs.append(got)
    assert all(runs[0][k].tobytes() == runs[1][k].tobytes() for k in every)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_launch_nothing(env, overlap):
    SY, _capi = env
    c, _want = overlap
    B, K = c["poses"].shape[:2]
    H, W = c["H"], c["W"]
    need = _capi.check(_capi.lib().hep_synth_workspace_bytes(B, H, W, K, len(c["vertices"])))
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    every = ("frames", "mask", "depth", "visible") + ANN
    out = {k: torch.full((sizes(c)[k] + 16,), 0x5A, dtype=torch.uint8, device="cuda") for k in every}
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    as_ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    down, beyond, below = (np.ascontiguousarray(a, np.int32) for a in ([0, 16, 12], [0, 12, 17], [-1, 12, 16]))
    cases = [(dict(**{k: None}), INVALID) for k in ("poses", "camera", "vertices", "vertex_colours", "faces", "face_normals", "face_start", "lights", "frames", "visible", "workspace")]
    cases += [(dict(**{k: None}), INVALID) for k in ("rvec", "tvec", "extra", "boxes", "labels", "mask_values", "out_rvec", "out_tvec", "out_extra", "num_gt", "slot_of")]      # half given
    cases += [(dict(batch=0), INVALID), (dict(pmax=0), INVALID), (dict(pmax=17), INVALID), (dict(num_vertices=0), INVALID), (dict(num_vertices=(1 << 24) + 1), INVALID),
              (dict(num_faces=0), INVALID), (dict(num_faces=(1 << 24) + 1), INVALID), (dict(num_labels=0), INVALID), (dict(num_labels=64), INVALID),
              (dict(face_start=as_ptr(down)), INVALID), (dict(face_start=as_ptr(beyond)), INVALID), (dict(face_start=as_ptr(below)), INVALID),
              (dict(alpha=-1), INVALID), (dict(alpha=257), INVALID), (dict(min_pixels=0), INVALID), (dict(min_pixels=-5), INVALID),
              (dict(workspace_bytes=need - 1), INVALID), (dict(workspace=ws.data_ptr() + 8), INVALID),
              (dict(height=15), UNSUPPORTED), (dict(width=4097), UNSUPPORTED), (dict(height=4097), UNSUPPORTED), (dict(width=15), UNSUPPORTED)]
    cases += [(dict(**{k: ptrs[k] + 2}), INVALID) for k in ("depth", "visible", "boxes", "labels", "mask_values", "num_gt", "slot_of")]       # misaligned
    cases += [(dict(boxes=ptrs["boxes"] + 4), INVALID), (dict(out_rvec=ptrs["rvec"] + 1), INVALID), (dict(out_tvec=ptrs["tvec"] + 2), INVALID), (dict(out_extra=ptrs["extra"] + 3), INVALID)]
    lib = _capi.lib()
    assert lib.hep_synth_workspace_bytes(B, 15, W, 4, 20) == UNSUPPORTED and lib.hep_synth_workspace_bytes(B, H, W, 17, 20) == INVALID
    assert lib.hep_synth_workspace_bytes(B, H, W, K, 20) == lib.hep_render_workspace_bytes(B, H, W, K, 20)
    for over, code in cases:
        rc = call(_capi, c, ptrs, ws.data_ptr(), need, **over)
        assert rc == code, (list(over), rc)
        assert lib.hep_last_error().decode().startswith("hep_synth_frames_device: "), list(over)
    assert all(bool((v == 0x5A).all()) for v in out.values()) and not ws.any()
    with pytest.raises(ValueError):
        SY.synth_frames(dev(c["frames"]).float(), [], dev(c["camera"]), mesh_set(SY, c), c["lights"])


# ---- 7. into augment_6dof and anchor_targets_device ------------------------------------------------------------------------------------------
def test_annotations_frames_and_mask_feed_augment_6dof_and_anchor_targets(env):
    SY, _capi = env
    from hmd_ego_pose_amd import augment as A
    from hmd_ego_pose_amd import training
    c, ann, mesh, cam4 = drawn_case(SY, B=2, K=3, H=64, W=64, seed=21)
    want = flat(S.run(c, min_pixels=8))
    assert want["num_gt"].min() >= 1
    out = SY.synth_frames(dev(c["frames"]), ann, dev(c["camera"]), mesh, c["lights"], min_pixels=8)
    inp = A.augment_6dof(out["frames"], out["mask"], out["annotations"], np.tile(cam4.astype(np.float32), (2, 1)), [0.0, 0.0], [1.0, 1.0], [0, 0], 128)
    assert inp["applied"].cpu().tolist() == [0, 0]
    assert np.array_equal(inp["gt_num"].cpu().numpy(), want["num_gt"])
    assert np.array_equal(inp["gt_boxes"].cpu().numpy(), want["boxes"] * (128 / 64))
    assert np.array_equal(inp["gt_labels"].cpu().numpy(), want["labels"]) and np.array_equal(inp["mask"].cpu().numpy(), want["mask"])
    n = _capi.lib().hep_anchors(128, None, None)
    anchors = np.empty((n, 4), np.float32)
    assert _capi.lib().hep_anchors(128, anchors.ctypes.data, None) == n
    gt_cls, gt_reg, gt_tr, gt_hand = training.anchor_targets_device(torch.from_numpy(anchors).cuda(), inp["gt_boxes"], inp["gt_labels"], inp["gt_transform"], None, inp["gt_num"], (128, 128), num_classes=2)
    assert gt_hand is None and tuple(gt_cls.shape[:2]) == (2, n) and bool(torch.isfinite(gt_reg).all()) and bool(torch.isfinite(gt_tr).all())


# ---- 8. one training step on synthetic frames, nothing waits for the host ---------------------------------------------------------------------
def test_one_trainer_step_on_synthetic_frames_without_a_host_round_trip(env):
    SY, _capi = env
    from hmd_ego_pose_amd import Trainer
    from hmd_ego_pose_amd import augment as A
    from hmd_ego_pose_amd import training
    from hmd_ego_pose_amd.augment import pad_annotations
    from hmd_ego_pose_amd.weights import seeded_state_dict
    B, S_, H, W = 2, 128, 128, 128
    cam4 = np.array([170.0, 170.0, 64.0, 64.0])
    v, f = R.cube(0.05)
    mesh = SY.ShadedMeshSet([(v, f, S.colours_for(8, 1))])
    tr = Trainer(seeded_state_dict(0, 0), 0, 1, "cuda", optimizer="sgd", lr=1e-5, batch_norm="batch")
    n = _capi.lib().hep_anchors(S_, None, None)
    anchors = np.empty((n, 4), np.float32)
    assert _capi.lib().hep_anchors(S_, anchors.ctypes.data, None) == n
    anchors = torch.from_numpy(anchors).cuda()
    points = torch.from_numpy(v[None].astype(np.float32) * 1000).cuda()
    rng = random.Random(4)
    # the uploads: poses, lights, backgrounds, camera
    ann = pad_annotations(SY.draw_poses(rng, B, 2, cam4, H, W, (0.3, 0.45), labels=[0, 0], margin=0.25), "cuda")
    lights = torch.from_numpy(SY.draw_lights(rng, B)).cuda()
    frames = torch.from_numpy(np.random.Generator(np.random.PCG64(1)).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    cam5 = torch.from_numpy(np.tile(np.append(cam4, 1.0), (B, 1))).cuda()
    angles, scales, apply = A.draw_6dof(rng, B)
    ops, args = A.draw_colour(rng, B, apply=apply, height=H, width=W)

    def loop():
        out = SY.synth_frames(frames.clone(), ann, cam5, mesh, lights)
        coloured = A.colour_augment(out["frames"], ops, args)
        inp = A.augment_6dof(coloured, out["mask"], out["annotations"], np.tile(cam4.astype(np.float32), (B, 1)), angles, scales, apply, S_)
        gt_cls, gt_reg, gt_tr, gt_hand = training.anchor_targets_device(anchors, inp["gt_boxes"], inp["gt_labels"], inp["gt_transform"], None, inp["gt_num"], (S_, S_), num_classes=1)
        return out, tr.step(inp["image"], inp["camera"], gt_cls, gt_reg, gt_tr, gt_hand, points)

    loop()                                                                   # warm: workspaces and the trainer's buffers exist
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")                                  # a device-to-host copy or any other wait for the device raises
    try:
        out, losses = loop()
        kept = losses.clone()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    del out, losses
    assert torch.cuda.memory_allocated() - before <= 512                     # nothing but the kept losses (one allocator block) stays
    assert tr.steps_taken == 2 and bool(torch.isfinite(kept).all()), kept
