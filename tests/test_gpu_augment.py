"""GPU (MI355X): the training input path hep_augment_6dof_device (csrc/k_augment.hip) behind hmd_ego_pose_amd.augment, and
training.anchor_targets_device, against the numpy oracle tests/_augment.py (the definition; tests/test_augment_cpu.py pins its
known answers and what the fixed cases below contain).

Cases (tests/_augment.py:make_case): A fused path, B=4, 128 x 128 -> 128, kmax 3, angles {0, 37.3, 90, 211.7}, scales
{1, 0.7, 1.3, 1}: one image with apply = 0, one whose warped mask is empty (fallback), one that loses one of three objects
(compaction); B padding, 96 x 128 -> 128; C the resize launch, 64 x 64 -> 128; D one object touching the border, taps clamped
at the edge of the last tile; and, beyond the issue's table, E: kmax 16 (every reduction slot), 50 x 70 -> 128 (a width that is no
multiple of a lane's four pixels, in front of the resize launch).

Bit-identical: image, mask, applied, gt_num, gt_labels, gt_boxes, camera, the flag columns of gt_transform (the pixel path is
integer, the normalisation numpy-exact).  gt_transform's pose is compared as matrices (axis_angle_to_matrix(pi row), and the
translation) against the float64 oracle; bound: four times the error of the same oracle evaluated in float32 numpy on the same
inputs (NOTEBOOK section 12's convention).  Measured pairs (rotation, translation; GPU error / float32 error): NOTEBOOK section 20.
"""
import numpy as np
import pytest
import torch

from tests import _augment as A

pytestmark = pytest.mark.gpu

CASES = ("A", "B", "C", "D", "E")
_RUNS = {}


def _inputs(c):
    d = {k: torch.from_numpy(v).cuda() for k, v in c.items() if k not in ("size", "angles_deg")}
    ann = {k: d[k] for k in ("boxes", "labels", "mask_values", "rvec", "tvec", "extra")}
    return d, ann


def _prefilled(B, H, W, S, kmax):
    nan = float("nan")
    return {"image": torch.full((B, 3, S, S), nan, dtype=torch.float32, device="cuda"), "mask": torch.full((B, H, W), 0xFF, dtype=torch.uint8, device="cuda"),
            "camera": torch.full((B, 6), nan, dtype=torch.float32, device="cuda"), "gt_boxes": torch.full((B, kmax, 4), nan, dtype=torch.float64, device="cuda"),
            "gt_labels": torch.full((B, kmax), -1, dtype=torch.int32, device="cuda"), "gt_transform": torch.full((B, kmax, 8), nan, dtype=torch.float32, device="cuda"),
            "gt_num": torch.full((B,), -1, dtype=torch.int32, device="cuda"), "applied": torch.full((B,), -1, dtype=torch.int32, device="cuda")}


def _run(name):
    """Two runs of a case through the ABI into buffers pre-filled with NaN / 0xFF (the workspace too); host copies, computed once."""
    if name not in _RUNS:
        from hmd_ego_pose_amd import _capi, augment
        c = A.make_case(name)
        B, H, W = c["masks"].shape
        S, kmax = c["size"], c["boxes"].shape[1]
        d, ann = _inputs(c)
        l = _capi.lib()
        need = _capi.check(l.hep_augment_workspace_bytes(B, H, W, S, kmax))
        runs = []
        for _ in range(2):
            out = _prefilled(B, H, W, S, kmax)
            ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
            augment._run(l, d["frames"], d["masks"], d["xform"], d["camera_k"], ann, d["num_gt"], B, H, W, S, kmax, 1000.0, out, ws, d["frames"].device)
            torch.cuda.synchronize()
            runs.append({k: v.cpu().numpy() for k, v in out.items()})
        _RUNS[name] = runs
    return _RUNS[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("name", CASES)
def test_matches_the_oracle(name):
    got, again = _run(name)
    ref, ref32 = A.oracle_case(name), A.oracle_case(name, np.float32)
    for k in ("applied", "gt_num", "gt_labels", "mask", "gt_boxes", "camera", "image"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        bad = _bits(got[k]) != _bits(ref[k])
        assert not bad.any(), (name, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert np.array_equal(_bits(got["gt_transform"][..., 6:]), _bits(ref["gt_transform"][..., 6:]))
    assert np.isfinite(got["gt_transform"]).all()                        # every element of the documented extent was written
    er, et = A.rotation_error(got["gt_transform"], ref["gt_transform"])
    br, bt = A.rotation_error(ref32["gt_transform"], ref["gt_transform"])
    print(f"case {name}: gt_transform as matrices, GPU vs float64 oracle: rotation {er:.3e} translation {et:.3e}; float32 oracle: {br:.3e} {bt:.3e}")
    assert er <= 4 * br and et <= 4 * bt, (name, er, br, et, bt)
    n = ref["gt_num"]
    for b in range(len(n)):                                             # rows at and beyond gt_num[b] are zero
        assert not got["gt_transform"][b, n[b]:].any()
    for k in got:                                                       # two runs, bit for bit
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (name, k)


def test_public_call_equals_the_abi_path():
    """augment.augment_6dof (matrices from angles on the host, annotation dicts padded and uploaded) gives the ABI path's case A."""
    from hmd_ego_pose_amd.augment import augment_6dof
    c = A.make_case("A")
    got = _run("A")[0]
    annotations = []
    for b in range(4):
        n = int(c["num_gt"][b])
        annotations.append({"bboxes": c["boxes"][b, :n], "labels": c["labels"][b, :n], "mask_values": c["mask_values"][b, :n],
                            "rotations": np.concatenate([c["rvec"][b, :n], c["extra"][b, :n]], axis=1), "translations": c["tvec"][b, :n]})
    out = augment_6dof(torch.from_numpy(c["frames"]).cuda(), torch.from_numpy(c["masks"]).cuda(), annotations, c["camera_k"],
                       c["angles_deg"], c["xform"][:, 7], c["xform"][:, 8], 128)
    torch.cuda.synchronize()
    assert set(out) == {"image", "camera", "gt_boxes", "gt_labels", "gt_transform", "gt_num", "applied", "mask"}
    for k in sorted(out):
        assert np.array_equal(_bits(out[k].cpu().numpy()), _bits(got[k])), k
    with pytest.raises(ValueError):
        augment_6dof(torch.from_numpy(c["frames"]).cuda(), torch.from_numpy(c["masks"][:, :64]).cuda(), annotations, c["camera_k"],
                     c["angles_deg"], c["xform"][:, 7], c["xform"][:, 8], 128)
    with pytest.raises(ValueError, match="scale"):
        augment_6dof(torch.from_numpy(c["frames"]).cuda(), torch.from_numpy(c["masks"]).cuda(), annotations, c["camera_k"],
                     c["angles_deg"], [1.0, 5.0, 1.0, 1.0], c["xform"][:, 8], 128)


def test_unaugmented_resize_equals_session_preprocess():
    """Case C, the images that were not augmented: the resize launch is Session.preprocess (hep_preprocess_u8_device) bit for bit."""
    from hmd_ego_pose_amd.model import Session
    from hmd_ego_pose_amd.weights import seeded_state_dict
    c, got = A.make_case("C"), _run("C")[0]
    s = Session(seeded_state_dict(0, 0), 0, 128, 2, "fp32")
    try:
        ref = s.preprocess(torch.from_numpy(c["frames"]).cuda()).contiguous().cpu().numpy()
    finally:
        s.close()
    plain = [b for b in range(2) if got["applied"][b] == 0]
    assert plain == [0]
    for b in plain:
        assert np.array_equal(_bits(got["image"][b]), _bits(ref[b]))


def test_anchor_targets_device_equals_the_host_staged_path():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd.training import anchor_targets, anchor_targets_device
    got = _run("A")[0]
    l = _capi.lib()
    n = _capi.check(l.hep_anchors(128, None, None))
    an = np.empty((n, 4), np.float32); ta = np.empty((n, 3), np.float32)
    _capi.check(l.hep_anchors(128, an.ctypes.data, ta.ctypes.data))
    anchors = torch.from_numpy(an).cuda()
    rng = np.random.Generator(np.random.PCG64(5))
    coords = rng.standard_normal((4, 3, 63)).astype(np.float32)
    dev = {k: torch.from_numpy(got[k]).cuda() for k in ("gt_boxes", "gt_labels", "gt_transform", "gt_num")}
    for gc in (None, coords):
        a = anchor_targets_device(anchors, dev["gt_boxes"], dev["gt_labels"], dev["gt_transform"], None if gc is None else torch.from_numpy(gc).cuda(),
                                  dev["gt_num"], (128, 128), num_classes=8)
        num = got["gt_num"]
        b = anchor_targets(anchors, [got["gt_boxes"][i, :num[i]] for i in range(4)], [got["gt_labels"][i, :num[i]] for i in range(4)],
                           [got["gt_transform"][i, :num[i]] for i in range(4)], None if gc is None else [gc[i, :num[i]] for i in range(4)],
                           [(128, 128)] * 4, num_classes=8)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert (x is None) == (y is None)
            if x is not None:
                assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
        assert (a[0][..., -1] == 1).any()                                # some anchors are objects
    hw = torch.tensor([[128, 128]] * 4, dtype=torch.int32, device="cuda")
    c2 = anchor_targets_device(anchors, dev["gt_boxes"], dev["gt_labels"], dev["gt_transform"], None, dev["gt_num"], hw, num_classes=8)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(c2[0].cpu().numpy()), _bits(a[0].cpu().numpy())) and c2[3] is None
