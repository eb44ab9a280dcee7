"""The two upload strategies of the hep_pose(s)_from_* calls (csrc/hep_api_pose.cpp pose_run_locked) move the same bytes: a session whose first
pose call ran under HEP_POSE_UPLOAD=pinned (the sections copied into the handle's pinned buffer, ONE copy up) returns, for every call form, what
a session with the default direct upload (one copy per section) returns, bit for bit.  Geometry, scene and thresholds of tests/test_gpu_windows.py:
2 frames of 48 x 64, crop 32, resized 48, the 3 x 2 grid; phi 0 at size 128, fp32, max_batch 12, seeded 3-class weights.  Two frames put more than
one payload behind the padding; twelve windows of two frames with all four sections make the rectified calls use every offset; six windows of
frame 0 alone are a used size below the reservation.  No tolerance: every output array is compared as int32."""
import numpy as np
import pytest
import torch

from tests.test_gpu_windows import CROP, H48, RS, W64, bits, make_scene

pytestmark = pytest.mark.gpu


def all_calls(s, sc, x):
    """every call form -> {name: {output: array}}"""
    fr, cam, grid, wcam = sc["frames"], sc["cam"], sc["grid"], sc["wcam"]
    out = {}
    for tn in ("zero", "two"):
        t = sc["thr"][tn]
        out["pose_from_input", tn] = s.pose_from_input(x, cam, t)
        out["poses_from_input", tn] = s.poses_from_input(x, cam, t)
        out["pose_from_i420", tn] = s.pose_from_i420(fr, H48, W64, cam, CROP, RS, t)
        out["poses_from_i420", tn] = s.poses_from_i420(fr, H48, W64, cam, CROP, RS, t)
        for pl in (False, True):
            for rect in (False, True):
                out["windows", pl, rect, 12, tn] = s.pose_from_i420_windows(fr, H48, W64, grid, cam if rect else wcam, CROP, RS, t, per_label=pl, rectified=rect)
                out["windows", pl, rect, 6, tn] = s.pose_from_i420_windows(fr[:1], H48, W64, grid[:6], cam[:1] if rect else wcam[:6], CROP, RS, t,
                                                                           per_label=pl, rectified=rect)
                out["tiled", pl, rect, tn] = (s.poses_from_i420_tiled if pl else s.pose_from_i420_tiled)(fr, H48, W64, cam, CROP, RS, 3, 2, t, rectified=rect)
                assert "window" in out["tiled", pl, rect, tn]
    return out


def test_the_pinned_upload_equals_the_direct_one(monkeypatch):
    import hmd_ego_pose_amd as H
    from hmd_ego_pose_amd.model import Session
    from hmd_ego_pose_amd.weights import seeded_state_dict
    assert torch.cuda.is_available()
    sd = seeded_state_dict(0, 0, num_classes=3)
    x = np.random.Generator(np.random.PCG64(128)).standard_normal((2, 3, 128, 128)).astype(np.float32)
    monkeypatch.delenv("HEP_POSE_UPLOAD", raising=False)       # (read by getenv at a handle's first pose call)
    direct = Session(sd, 0, 128, 12, "fp32")
    try:
        sc = make_scene(H, direct, True)                       # the direct session's first pose call is made here
        want = all_calls(direct, sc, x)
        monkeypatch.setenv("HEP_POSE_UPLOAD", "pinned")
        pinned = Session(sd, 0, 128, 12, "fp32")
        try:
            got = all_calls(pinned, sc, x)                     # ... and the pinned session's first one here, the variable set
        finally:
            pinned.close()
    finally:
        direct.close()
    assert got.keys() == want.keys() and len(want) == 2 * (4 + 12)
    assert (want["pose_from_i420", "zero"]["found"] == 1).all() and (want["tiled", True, True, "zero"]["window"] >= 0).all()      # real answers, not empty records
    for call, w in want.items():
        g = got[call]
        assert g.keys() == w.keys(), call
        for k in w:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and np.array_equal(bits(g[k]), bits(w[k])), (call, k)
