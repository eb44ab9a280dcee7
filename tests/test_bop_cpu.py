"""CPU (no GPU): the numpy definition of MSSD, MSPD and VSD (tests/_bop.py) against hand-written cases, the host code of
hmd_ego_pose_amd/bop.py (symmetry sets, the pair table, every refusal, the average recalls) and the two entry points' existence and
refusals before any HIP call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi
from hmd_ego_pose_amd import bop as BP
from tests import _bop as B
from tests import _render as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(3)
IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
CAM = (60.0, 61.0, 32.0, 16.0)


def sym_row(Rm, t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.asarray(Rm, np.float64).reshape(9), np.asarray(t, np.float64)])


def composed_pair(R_gt, t_gt, sym, cam=CAM, label=0):
    """A pair whose estimate is the ground truth composed with ``sym``, by the definition's own arithmetic: bit-equal."""
    row = B.pair_row(label, R_gt, t_gt, EYE, (0, 0, 0), cam)
    Rp, tp = B.compose(row, sym)
    return B.pair_row(label, R_gt, t_gt, Rp, tp, cam)


# ---- MSSD / MSPD -----------------------------------------------------------------------------------------------------------------
def test_mssd_is_zero_under_a_listed_symmetry_and_not_without_it():
    v, _ = R.cube()
    half_turn = sym_row(R.rotation((0, 0, 1), math.pi), (0.0, 0.0, 0.0))
    pair = composed_pair(R.rotation((1, 2, 3), 0.7), (0.01, -0.02, 0.4), half_turn)
    with_it = B.point_errors(pair[None], v, [0, 8], np.stack([IDENTITY, half_turn]), [0, 2])
    without = B.point_errors(pair[None], v, [0, 8], IDENTITY[None], [0, 1])
    assert with_it[0, 0] == 0.0 and with_it[0, 1] == 0.0
    assert without[0, 0] > 0.1 and without[0, 1] > 10.0              # opposite corners of a 0.1 cube, 0.4 away at 60 pixels focal length


def test_single_vertex_model_gives_the_hand_computed_distance():
    v = np.array([[0.5, 0.25, 0.0]], np.float32)
    pair = B.pair_row(0, EYE, (0.0, 0.0, 10.0), EYE, (3.0, 4.0, 10.0), (20.0, 20.0, 5.0, 5.0))
    e = B.point_errors(pair[None], v, [0, 1], IDENTITY[None], [0, 1])
    assert e[0, 0] == 5.0                                           # |(3, 4, 0)|
    assert e[0, 1] == 10.0                                          # u moves by 20 * 3 / 10 = 6, v by 20 * 4 / 10 = 8


def test_min_over_the_symmetries_is_the_brute_force_min():
    rng = np.random.Generator(np.random.PCG64(5))
    v = rng.uniform(-0.05, 0.05, (37, 3)).astype(np.float32)
    syms = np.stack([IDENTITY] + [sym_row(R.rotation(rng.standard_normal(3), rng.uniform(0.2, 3.0)), rng.uniform(-0.01, 0.01, 3)) for _ in range(6)])
    pair = composed_pair(R.rotation((2, 1, 0), 1.1), (0.0, 0.01, 0.5), syms[4])
    pair[16:28] += rng.standard_normal(12) * 1e-3                    # near symmetry 4, not on it
    both = B.point_errors(pair[None], v, [0, 37], syms, [0, 7])[0]
    single = np.array([B.point_errors(pair[None], v, [0, 37], np.stack([IDENTITY, s]), [0, 2])[0] if k else B.point_errors(pair[None], v, [0, 37], IDENTITY[None], [0, 1])[0]
                       for k, s in enumerate(syms)])
    alone = np.array([math.sqrt(B.squared_errors_loop(pair, s, v)[0]) for s in syms])
    assert both[0] == alone.min() and int(np.argmin(alone)) == 4 and both[0] < 0.01 < np.delete(alone, 4).min()
    assert both[1] == min(math.sqrt(B.squared_errors(pair, s, v)[1]) for s in syms)
    assert (single[:, 0] <= alone[0]).all()


def test_mspd_is_nan_exactly_when_a_vertex_is_not_in_front():
    v = np.array([[0.0, 0.0, -0.25], [0.0, 0.0, 0.25]], np.float32)
    for z, nan in ((0.25, True), (0.2500001, False), (0.2, True), (1.0, False)):
        est = B.pair_row(0, EYE, (0, 0, 1.0), EYE, (0.01, 0, z), CAM)            # the estimate's first vertex at Z = z - 0.25
        gt = B.pair_row(0, EYE, (0, 0, z), EYE, (0.01, 0, 1.0), CAM)             # ... and the ground truth's
        for pair in (est, gt):
            e = B.point_errors(pair[None], v, [0, 2], IDENTITY[None], [0, 1])[0]
            assert np.isnan(e[1]) == nan and e[0] > 0.0              # MSSD is unaffected
    # behind the camera only under a symmetry that is not the best one
    flip = sym_row(R.rotation((1, 0, 0), math.pi), (0, 0, -2.0))
    pair = B.pair_row(0, EYE, (0, 0, 1.0), EYE, (0, 0, 1.0), CAM)
    e = B.point_errors(pair[None], v, [0, 2], np.stack([IDENTITY, flip]), [0, 2])[0]
    assert e[0] == 0.0 and np.isnan(e[1])


def test_the_elementwise_statements_equal_the_loops():
    rng = np.random.Generator(np.random.PCG64(3))
    v = rng.uniform(-0.3, 0.3, (37, 3)).astype(np.float32)
    v[5] = (np.nan, 0.0, 0.0)
    for z in (1.0, 0.25):                                           # all in front; some behind
        pair = B.pair_row(0, R.rotation((1, 2, 3), 0.7), (0.01, -0.02, z), R.rotation((1, 2, 2.5), 0.8), (0.0, 0.01, z + 0.05), CAM)
        s = sym_row(R.rotation((0, 1, 0), 2.0), (0.01, 0.0, -0.02))
        assert B.squared_errors(pair, s, v) == B.squared_errors_loop(pair, s, v) and B.squared_errors(pair, s, v)[2] == (1 | 2)
        assert B.squared_errors(pair, s, v[6:]) == B.squared_errors_loop(pair, s, v[6:]) and B.squared_errors(pair, s, v[6:])[2] == (0 if z == 1.0 else 2)
    row = B.pair_row(0, EYE, (0, 0, 1), EYE, (0, 0, 1), (17.3, 15.1, 6.6, 9.2))
    zg = np.where(rng.random((16, 24)) < 0.7, rng.uniform(90, 110, (16, 24)), 0).astype(np.float32)
    ze = np.where(rng.random((16, 24)) < 0.7, zg + rng.choice([0.5, 4.0, 12.0, 30.0], (16, 24)) * rng.choice([-1, 1], (16, 24)), 0).astype(np.float32)
    zt = np.where(rng.random((16, 24)) < 0.6, rng.uniform(70, 130, (16, 24)), 0).astype(np.float32)
    for test in (None, zt):
        counts = B.vsd_pixels(row, zg, ze, test, 15.0, (1.0, 5.0, 20.0))
        assert counts == B.vsd_pixels_loop(row, zg, ze, test, 15.0, (1.0, 5.0, 20.0)) and counts[0] > counts[1] > counts[2] > counts[3] > counts[4] > 0


def test_skipped_rows_are_nan():
    v, _ = R.cube()
    ok = B.pair_row(0, EYE, (0, 0, 1.0), EYE, (0, 0.01, 1.0), CAM)
    rows = [ok, B.pair_row(0, EYE, (0, 0, 1.0), EYE, (0, 0, 1.0), CAM, valid=0.0), B.pair_row(1, EYE, (0, 0, 1.0), EYE, (0, 0, 1.0), CAM),
            B.pair_row(float("nan"), EYE, (0, 0, 1.0), EYE, (0, 0, 1.0), CAM), B.pair_row(0, EYE, (0, 0, float("nan")), EYE, (0, 0, 1.0), CAM), ok]
    e = B.point_errors(np.stack(rows), v, [0, 8], IDENTITY[None], [0, 1])
    assert np.isnan(e[1:5]).all() and np.array_equal(e[0], e[5]) and abs(e[0, 0] - 0.01) < 1e-15


# ---- VSD ---------------------------------------------------------------------------------------------------------------------------
H, W = 32, 64
TAUS = (0.005, 0.02, 0.05)
DELTA = 0.015


def cube_pairs(rows):
    v, f = R.cube()
    pairs = np.stack(rows)
    zg, ze = B.render_depths(pairs, v, f, [0, 12], H, W)
    return pairs, zg, ze


def test_vsd_identical_poses_give_zero_and_disjoint_silhouettes_one():
    Rm = R.rotation((1, 2, 0), 0.6)
    same = B.pair_row(0, Rm, (0.0, 0.0, 0.3), Rm, (0.0, 0.0, 0.3), CAM)
    apart = B.pair_row(0, Rm, (-0.1, 0.0, 0.3), Rm, (0.1, 0.0, 0.3), CAM)
    gone = B.pair_row(0, Rm, (-9.0, 0.0, 0.3), Rm, (9.0, 0.0, 0.3), CAM)         # both off screen: nothing is visible
    pairs, zg, ze = cube_pairs([same, apart, gone])
    out, counts = B.vsd(pairs, zg, ze, None, DELTA, TAUS, 1)
    assert counts[0, 0] == counts[0, 1] > 200 and not counts[0, 2:].any() and out[0].tolist() == [0.0] * 3
    assert counts[1, 0] > 400 and counts[1, 1] == 0 and out[1].tolist() == [1.0] * 3
    assert counts[2].tolist() == [0] * 5 and out[2].tolist() == [1.0] * 3


def test_vsd_an_occluder_removes_its_pixels_from_both_masks():
    Rm = R.rotation((0, 1, 0), 0.3)
    pair = B.pair_row(0, Rm, (0.0, 0.0, 0.3), Rm, (0.004, 0.0, 0.3), CAM)
    pairs, zg, ze = cube_pairs([pair])
    free, c_free = B.vsd(pairs, zg, ze, None, DELTA, TAUS, 1)
    zt = np.zeros((1, H, W), np.float32)
    zt[0, :, 32:] = 0.1                                             # a wall 0.15 in front of the cube over the right half: far nearer than delta
    zt[0, :, :8] = 5.0                                              # background measured behind everything: hides nothing
    out, c = B.vsd(pairs, zg, ze, zt, DELTA, TAUS, 1)
    left_g, left_e = zg[0, :, :32] > 0, ze[0, :, :32] > 0
    assert (zg[0, :, 32:] > 0).sum() > 50 and c[0, 0] == (left_g | left_e).sum() < c_free[0, 0] and c[0, 1] == (left_g & left_e).sum()
    # an occluder nearer than delta to the surface (by distance from the camera) hides nothing
    near = np.where(zg[0] > 0, zg[0] - np.float32(0.004), 0).astype(np.float32)[None]
    assert np.array_equal(B.vsd(pairs, zg, ze, near, DELTA, TAUS, 1)[1], c_free)
    # an image index outside the depth_test: the row is skipped; without a depth_test the index is not read
    pairs[0, 2] = 1.0
    skipped = B.vsd(pairs, zg, ze, zt, DELTA, TAUS, 1)
    assert np.isnan(skipped[0]).all() and (skipped[1] == -1).all() and np.array_equal(B.vsd(pairs, zg, ze, None, DELTA, TAUS, 1)[1], c_free)


def hand_built_triple():
    """16 x 16, fx = fy = 16, cx = cy = 0 (k2 = 1 + (x x + y y) / 256 <= 2.76), delta 15, taus 5 and 20.  Ground truth: rows 2-9, columns 2-9
    at 100.  Estimate: rows 2-9, columns 4-5 at 103, 6-7 at 110, 8-11 at 130.  Test image: rows 2-3 at 50 (an occluder 50 in front: nothing
    of those rows is visible), row 4 at 110 (the ground truth and the estimate up to 110 are in front of it; 130 lies 20 behind: visible
    only where the ground truth is, columns 8-9), no measurement elsewhere."""
    zg, ze, zt = np.zeros((16, 16), np.float32), np.zeros((16, 16), np.float32), np.zeros((16, 16), np.float32)
    zg[2:10, 2:10] = 100.0
    ze[2:10, 4:6], ze[2:10, 6:8], ze[2:10, 8:12] = 103.0, 110.0, 130.0
    zt[2:4, :], zt[4, :] = 50.0, 110.0
    return B.pair_row(0, EYE, (0, 0, 1), EYE, (0, 0, 1), (16.0, 16.0, 0.0, 0.0)), zg, ze, zt


def test_vsd_counts_of_a_hand_built_depth_triple():
    row, zg, ze, zt = hand_built_triple()
    counts = B.vsd_pixels_loop(row, zg, ze, zt, 15.0, (5.0, 20.0))
    assert counts == B.vsd_pixels(row, zg, ze, zt, 15.0, (5.0, 20.0))
    # row 4: union columns 2-9 (8), rows 5-9: columns 2-11 (10 each); intersection columns 4-9 in the six rows 4-9;
    # cost at tau 5: columns 6-9 (differences 10 and 30; 3 costs nothing: 9 k2 < 25), at tau 20: columns 8-9 (100 k2 <= 276 < 400)
    assert counts == [8 + 5 * 10, 6 * 6, 6 * 4, 6 * 2]
    assert B.vsd_from_counts(counts) == [(24 + 22) / 58, (12 + 22) / 58]
    # without the test image: all eight rows, columns 2-11
    assert B.vsd_pixels(row, zg, ze, None, 15.0, (5.0, 20.0)) == [80, 48, 32, 16]
    assert B.vsd_from_counts([0, 0, 0, 0]) == [1.0, 1.0]


def test_sqrt_free_thresholds_agree_with_the_sqrt_form():
    rng = np.random.Generator(np.random.PCG64(9))
    n = 1000
    x, y = rng.integers(0, 4096, n).astype(np.float64), rng.integers(0, 4096, n).astype(np.float64)
    fx, fy, cx, cy = rng.uniform(300, 3000, n), rng.uniform(300, 3000, n), rng.uniform(0, 4096, n), rng.uniform(0, 4096, n)
    a, b = (x - cx) / fx, (y - cy) / fy
    k2 = (a * a + b * b) + 1.0
    d = rng.uniform(1.0, 50.0, n)
    zr = rng.uniform(200.0, 2000.0, n)
    margin = rng.uniform(1e-6, 0.5, n) * rng.choice([-1.0, 1.0], n)
    zm = zr + d / np.sqrt(k2) * (1.0 + margin)                       # the distance difference is d (1 + margin)
    dist = np.sqrt(k2) * (zm - zr)
    assert (np.abs(dist - d) / d > 1e-9).all()                       # none is rejected: every draw keeps its margin
    for i in range(n):
        assert B.far(k2[i], zm[i], zr[i], d[i]) == bool(dist[i] > d[i])
        assert bool(k2[i] * ((zm[i] - zr[i]) * (zm[i] - zr[i])) >= d[i] * d[i]) == bool(abs(dist[i]) >= d[i])
        assert not B.far(k2[i], zr[i], zm[i], d[i]) or zr[i] > zm[i]
    assert not B.far(2.0, 1.0, 1.0, 1e-3) and not B.far(2.0, 1.0, 3.0, 1e-3) and B.far(2.0, 3.0, 1.0, 1e-3)
    assert (margin > 0).sum() > 400 and (margin < 0).sum() > 400


# ---- symmetry sets -----------------------------------------------------------------------------------------------------------------
HALF_TURN_Z = [-1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]


def test_symmetry_transforms():
    none = BP.symmetry_transforms({"diameter": 100.0})
    assert none.shape == (1, 12) and np.array_equal(none[0], IDENTITY) and none.dtype == np.float64
    two = BP.symmetry_transforms({"diameter": 100.0, "symmetries_discrete": [HALF_TURN_Z]})
    assert two.shape == (2, 12) and np.array_equal(two[0], IDENTITY) and two[1, :9].tolist() == [-1, 0, 0, 0, -1, 0, 0, 0, 1]
    shifted = BP.symmetry_transforms({"symmetries_discrete": [HALF_TURN_Z[:3] + [7.0] + HALF_TURN_Z[4:]]})
    assert shifted[1, 9:].tolist() == [7.0, 0.0, 0.0]
    axis = {"symmetries_continuous": [{"axis": [0, 0, 2.0], "offset": [1.0, 0, 0]}]}
    seven = BP.symmetry_transforms(axis, 0.5)
    assert seven.shape == (7, 12) and np.array_equal(seven[0], IDENTITY)
    for k in range(7):                                               # turn k of a full turn in seven steps about the axis through (1, 0, 0)
        Rk = R.rotation((0, 0, 1), k * 2 * math.pi / 7)
        assert np.allclose(seven[k, :9].reshape(3, 3), Rk, atol=1e-15) and np.allclose(seven[k, 9:], np.array([1.0, 0, 0]) - Rk @ [1.0, 0, 0], atol=1e-15)
    with pytest.raises(ValueError, match="coarsen max_sym_disc_step"):
        BP.symmetry_transforms(axis)                                 # 315 steps at the default 0.01
    both = BP.symmetry_transforms(dict(axis, symmetries_discrete=[HALF_TURN_Z]), 0.5)
    assert both.shape == (14, 12) and np.array_equal(both[0], IDENTITY) and len({tuple(np.round(r, 9)) for r in both}) == 14
    assert BP.symmetry_transforms(axis, math.pi / 64).shape == (64, 12)
    with pytest.raises(ValueError):
        BP.symmetry_transforms(dict(axis, symmetries_discrete=[HALF_TURN_Z]), math.pi / 64)
    for bad in ({"symmetries_discrete": [[1.0] * 15]}, {"symmetries_continuous": [{"axis": [0, 0, 0], "offset": [0, 0, 0]}]}, None):
        with pytest.raises(ValueError):
            BP.symmetry_transforms(bad, 0.5)
    with pytest.raises(ValueError):
        BP.symmetry_transforms(axis, 0.0)


def test_symmetry_set():
    cpu = torch.device("cpu")
    two = BP.symmetry_transforms({"symmetries_discrete": [HALF_TURN_Z]})
    s = BP.SymmetrySet([None, two, None], device=cpu)
    assert s.start.tolist() == [0, 1, 3, 4] and s.start.dtype == np.int32 and (s.num_labels, s.num_symmetries) == (3, 4)
    assert s.table.dtype == torch.float64 and np.array_equal(s.table.numpy(), np.stack([IDENTITY, two[0], two[1], IDENTITY]))
    for bad in ([], [two[1:]], [two[:, :11]], [np.full((1, 12), np.nan)], [np.tile(IDENTITY, (65, 1))], [None] * 64):
        with pytest.raises(ValueError):
            BP.SymmetrySet(bad, device=cpu)
    import hmd_ego_pose_amd
    assert hmd_ego_pose_amd.SymmetrySet is BP.SymmetrySet and hmd_ego_pose_amd.bop_errors is BP.bop_errors and hmd_ego_pose_amd.pairs_from_scene is BP.pairs_from_scene


# ---- the pair table and the refusals ---------------------------------------------------------------------------------------------
def scene_tables():
    from tests import _score_scene as SS
    det, gt, _cl, (rec, _s, _t, _l, _c), _M = SS.case("special")
    return det, gt, rec


def host_pairs(det, gt, rec):
    """pairs_from_scene restated on the host with tests/_draw.py's Rodrigues."""
    from tests import _draw as D
    Bn, A = gt.shape[:2]
    out = np.zeros((Bn, A, 32))
    for b in range(Bn):
        for a in range(A):
            m = rec[b, a, 0] == 1.0 and rec[b, a, 1] == 1.0
            r = int(rec[b, a, 2]) if m else 0
            rv = np.asarray(det["rotation"][b, r], np.float32) * np.float32(math.pi)
            out[b, a, 0], out[b, a, 1], out[b, a, 2] = float(m), rec[b, a, 12], b
            out[b, a, 4:13], out[b, a, 13:16] = D.rodrigues(gt[b, a, 5:8])[0], gt[b, a, 8:11]
            out[b, a, 16:25], out[b, a, 25:28] = D.rodrigues(rv)[0], np.asarray(det["translation"][b, r], np.float32).astype(np.float64)
            out[b, a, 28:32] = gt[b, a, 14:18]
    return out.reshape(Bn * A, 32)


def test_pairs_from_scene_against_a_host_restatement():
    det, gt, rec = scene_tables()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in det.items()}
    got = BP.pairs_from_scene(torch.from_numpy(gt), t, torch.from_numpy(rec)).numpy()
    want = host_pairs(det, gt, rec)
    assert got.shape == want.shape == (gt.shape[0] * gt.shape[1], 32) and want[:, 0].sum() >= 6
    for k in (0, 1, 2, 3):
        assert np.array_equal(got[:, k], want[:, k], equal_nan=True)
    on = want[:, 0] == 1.0
    assert np.array_equal(got[on][:, 13:16], want[on][:, 13:16]) and np.array_equal(got[on][:, 25:32], want[on][:, 25:32])
    assert np.allclose(got[on][:, 4:13], want[on][:, 4:13], rtol=0, atol=4e-16) and np.allclose(got[on][:, 16:25], want[on][:, 16:25], rtol=0, atol=4e-16)
    cam = torch.arange(gt.shape[0] * 5, dtype=torch.float64).reshape(-1, 5)
    assert np.array_equal(BP.pairs_from_scene(torch.from_numpy(gt), t, torch.from_numpy(rec), cam).numpy().reshape(gt.shape[0], -1, 32)[:, 1, 28:32], cam[:, :4].numpy())


def test_pairs_from_scene_refuses_wrong_arguments():
    det, gt, rec = scene_tables()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in det.items()}
    g, r = torch.from_numpy(gt), torch.from_numpy(rec)
    ok = dict(gt=g, detections=t, records=r, camera=None)
    for change in (dict(gt=g.float()), dict(gt=g[0]), dict(gt=g[..., :87]), dict(gt=g[:0]), dict(records=r.float()), dict(records=r[:1]), dict(records=r[..., :15]),
                   dict(detections={k: v for k, v in t.items() if k != "rotation"}), dict(detections=dict(t, rotation=t["rotation"].double())),
                   dict(detections=dict(t, translation=t["translation"][:, :5])), dict(detections=dict(t, rotation=t["rotation"][:1])), dict(detections=None),
                   dict(camera=torch.zeros(gt.shape[0], 5)), dict(camera=torch.zeros(gt.shape[0], 3, dtype=torch.float64)), dict(camera=torch.zeros(1, 5, dtype=torch.float64))):
        with pytest.raises(ValueError, match="pairs_from_scene"):
            BP.pairs_from_scene(**dict(ok, **change))


def test_bop_errors_refuses_wrong_arguments_before_the_library():
    from hmd_ego_pose_amd.render import MeshSet
    cpu = torch.device("cpu")
    m = MeshSet([R.cube(), R.tetrahedron()], device=cpu)
    assert m.vertex_start.tolist() == [0, 8, 12] and m.vertex_start.dtype == np.int32
    s = BP.SymmetrySet([None, None], device=cpu)
    pairs = torch.zeros(3, 32, dtype=torch.float64)
    depth = torch.zeros(2, 32, 48)
    ok = dict(pairs=pairs, meshes=m, symmetries=s, height=32, width=48)
    for change in (dict(pairs=pairs.float()), dict(pairs=pairs[0]), dict(pairs=pairs[:, :31]), dict(pairs=pairs[:0]), dict(meshes=R.cube()), dict(symmetries=[None, None]),
                   dict(symmetries=BP.SymmetrySet([None], device=cpu)), dict(height=15), dict(width=4097), dict(depth_test=depth.double()), dict(depth_test=depth[0]),
                   dict(depth_test=depth[:, :, :47]), dict(depth_test=depth[:0]), dict(depth_test=torch.zeros(2, 32, 96)[:, :, ::2]), dict(delta=0.0), dict(delta=float("inf")),
                   dict(delta=float("nan")), dict(taus=()), dict(taus=[1.0] * 17), dict(taus=[1.0, -2.0]), dict(taus=[float("nan")]), dict(taus=np.ones((3, 2))),
                   dict(taus=np.ones((2, 2, 2))), dict(chunk=0)):
        args = dict(ok, **change)
        with pytest.raises(ValueError, match="bop_errors"):
            BP.bop_errors(args.pop("pairs"), args.pop("meshes"), args.pop("symmetries"), args.pop("height"), args.pop("width"), **args)
    with pytest.raises(ValueError):
        BP.BopSettings(m, BP.SymmetrySet([None], device=cpu))
    with pytest.raises(ValueError):
        BP.BopSettings(m, s, tau_fractions=[0.1] * 17)
    with pytest.raises(ValueError):
        BP.BopSettings(m, s, height=64)
    settings = BP.BopSettings(m, s)
    assert np.allclose(settings.tau_fractions, np.arange(1, 11) * 0.05, rtol=0, atol=1e-15) and settings.delta == 15.0
    frames = torch.zeros(2, 32, 48, 3, dtype=torch.uint8)
    assert BP.check_settings("x", settings, None, frames, cpu, 2) == (32, 48) and BP.check_settings("x", None, None, frames, cpu, 2) is None
    assert BP.check_settings("x", BP.BopSettings(m, s, height=64, width=80), None, torch.zeros(2, 3, 128, 128), cpu, 2) == (64, 80)
    for bop, depth_test, fr, labels in ((None, depth, frames, 2), (settings, None, frames, 3), (m, None, frames, 2), (settings, None, torch.zeros(2, 3, 128, 128), 2),
                                        (settings, depth[:1], frames, 2), (settings, depth.double(), frames, 2), (settings, torch.zeros(2, 32, 40), frames, 2)):
        with pytest.raises(ValueError):
            BP.check_settings("x", bop, depth_test, fr, cpu, labels)


# ---- the entry points: symbols, ABI version, refusals ------------------------------------------------------------------------------
POINT_NAMES = ("pairs", "n", "vertices", "num_vertices", "vertex_start", "symmetries", "num_symmetries", "symmetry_start", "num_labels", "errors", "stream")
VSD_NAMES = ("pairs", "n", "num_labels", "depth_gt", "depth_est", "depth_test", "num_images", "height", "width", "delta", "taus", "num_taus", "vsd", "counts",
             "workspace", "workspace_bytes", "stream")


def test_symbols_in_header_binding_and_library():
    l = _capi.lib()
    header = open(os.path.join(ROOT, "include", "hep.h")).read()
    for name, names in (("hep_bop_point_errors_device", POINT_NAMES), ("hep_bop_vsd_device", VSD_NAMES), ("hep_bop_workspace_bytes", ("n", "num_taus"))):
        assert name in _capi.SYMBOLS and len(_capi.SYMBOLS[name][1]) == len(names) and hasattr(l, name)
        decl = re.search(rf"\b{name}\(([^;]*)\);", header)
        assert decl and len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(names)
    for name, value in (("HEP_BOP_PAIR_DOUBLES", 32), ("HEP_BOP_MAX_SYMMETRIES", 64), ("HEP_BOP_MAX_TAUS", 16)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert (_capi.BOP_PAIR_DOUBLES, _capi.BOP_MAX_SYMMETRIES, _capi.BOP_MAX_TAUS) == (32, 64, 16)
    assert re.search(r"#define HEP_ABI_VERSION 1\b", header) and l.hep_abi_version() == 1
    assert "unpinned" in header.lower()


def test_entry_points_refuse_invalid_arguments_before_any_hip_call():
    l = _capi.lib()
    buf = np.zeros(512, np.float64)
    a = buf.ctypes.data
    assert a % 16 == 0 or (a + 8) % 16 == 0
    a += a % 16
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    as_ptr = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    tables = dict(good_v=i32([0, 8, 12]), good_s=i32([0, 1, 3]), below=i32([-1, 1, 3]), flat=i32([0, 0, 3]), down=i32([0, 2, 1]), past=i32([0, 8, 13]), many=i32([0, 65, 66]))
    good = dict(zip(POINT_NAMES, (a, 3, a, 12, as_ptr(tables["good_v"]), a, 3, as_ptr(tables["good_s"]), 2, a, None)))
    cases = [({k: None}, k.encode() + b" is NULL", -1) for k in ("pairs", "vertices", "vertex_start", "symmetries", "symmetry_start", "errors")]
    cases += [({"n": 0}, b"n must be >= 1", -1), ({"num_labels": 0}, b"num_labels outside 1..63", -1), ({"num_labels": 64}, b"num_labels outside 1..63", -1),
              ({"num_vertices": 0}, b"must be >= 1", -1), ({"num_symmetries": 0}, b"must be >= 1", -1),
              ({"vertex_start": as_ptr(tables["below"])}, b"vertex_start starts below 0", -1), ({"vertex_start": as_ptr(tables["flat"])}, b"vertex_start must increase", -1),
              ({"vertex_start": as_ptr(tables["down"])}, b"vertex_start must increase", -1), ({"vertex_start": as_ptr(tables["past"])}, b"vertex_start ends past the array", -1),
              ({"symmetry_start": as_ptr(tables["below"])}, b"symmetry_start starts below 0", -1), ({"symmetry_start": as_ptr(tables["flat"])}, b"symmetry_start must increase", -1),
              ({"symmetry_start": as_ptr(tables["good_v"])}, b"symmetry_start ends past the array", -1),
              ({"symmetry_start": as_ptr(tables["many"]), "num_symmetries": 66}, b"more than 64", -1)]
    for change, reason, code in cases:
        assert l.hep_anchors(100, None, None) < 0                   # another message in between: the text below is never a stale one
        args = dict(good, **change)
        assert l.hep_bop_point_errors_device(*[args[n] for n in POINT_NAMES]) == code, change
        msg = l.hep_last_error()
        assert msg.startswith(b"hep_bop_point_errors_device: ") and reason in msg, (change, msg)

    taus = np.ascontiguousarray([5.0, 20.0])
    tp = lambda v: np.ascontiguousarray(v, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    keep = [np.ascontiguousarray(v, np.float64) for v in ([5.0, 0.0], [5.0, -1.0], [float("nan"), 1.0], [1.0, float("inf")])]
    need = l.hep_bop_workspace_bytes(3, 2)
    assert need == 48 and l.hep_bop_workspace_bytes(1, 1) == 16 and l.hep_bop_workspace_bytes(17, 16) == 1232      # 17 x 18 x 4 = 1224, rounded up to 16
    assert l.hep_bop_workspace_bytes(0, 2) == -1 and l.hep_bop_workspace_bytes(3, 0) == -1 and l.hep_bop_workspace_bytes(3, 17) == -1
    good = dict(zip(VSD_NAMES, (a, 3, 2, a, a, None, 0, 48, 64, 15.0, taus.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 2, a, a, a, need, None)))
    cases = [({k: None}, k.encode() + b" is NULL", -1) for k in ("pairs", "depth_gt", "depth_est", "taus", "vsd", "counts", "workspace")]
    cases += [({"n": 0}, b"n must be >= 1", -1), ({"num_labels": 0}, b"num_labels outside 1..63", -1), ({"num_labels": 64}, b"num_labels outside 1..63", -1),
              ({"num_taus": 0}, b"num_taus outside 1..16", -1), ({"num_taus": 17}, b"num_taus outside 1..16", -1),
              ({"delta": 0.0}, b"delta must be finite and positive", -1), ({"delta": -1.0}, b"delta must be finite and positive", -1),
              ({"delta": float("nan")}, b"delta must be finite and positive", -1), ({"delta": float("inf")}, b"delta must be finite and positive", -1)]
    cases += [({"taus": k.ctypes.data_as(ctypes.POINTER(ctypes.c_double))}, b"must be finite and positive", -1) for k in keep]
    cases += [({"depth_test": a, "num_images": 0}, b"num_images must be >= 1", -1), ({"workspace": a + 8}, b"workspace must be 16-byte aligned", -1),
              ({"workspace_bytes": need - 1}, b"workspace too small", -1),
              ({"height": 15}, b"height and width must be in 16..4096", -4), ({"height": 4097}, b"height and width must be in 16..4096", -4),
              ({"width": 15}, b"height and width must be in 16..4096", -4), ({"width": 4097}, b"height and width must be in 16..4096", -4)]
    for change, reason, code in cases:
        assert l.hep_anchors(100, None, None) < 0
        args = dict(good, **change)
        assert l.hep_bop_vsd_device(*[args[n] for n in VSD_NAMES]) == code, change
        msg = l.hep_last_error()
        assert msg.startswith(b"hep_bop_vsd_device: ") and reason in msg, (change, msg)
    assert not buf.any() and l.hep_abi_version() == 1               # nothing was written, and the ABI version stays


# ---- average recall ----------------------------------------------------------------------------------------------------------------
def test_average_recall_on_a_written_out_table():
    """Label 0, diameter 100, width 640, two taus: four annotations, three matched.  MSSD 4 / 26 / NaN pass 10 / 5 / 0 of the thresholds
    5..50; MSPD 7 / 100 / 12 pass 9 / 0 / 8 of 5..50 pixels; VSD at the first tau 0 / 0.32 / 1 pass 10 / 4 / 0 of 0.05..0.5, at the second
    0 / 0.12 / NaN pass 10 / 8 / 0.  Label 1 (diameter 10): one annotation, unmatched.  Label 2: none."""
    rec = np.zeros((3, 2, 16))
    rec[..., 2], rec[..., 12] = -1.0, -1.0
    for (b, a), (matched, label) in {(0, 0): (1, 0), (0, 1): (1, 0), (1, 0): (1, 0), (1, 1): (0, 0), (2, 1): (0, 1)}.items():
        rec[b, a, 0], rec[b, a, 1], rec[b, a, 12] = 1.0, matched, label
    err = np.full((3, 2, 4), np.nan)
    err[0, 0], err[0, 1], err[1, 0] = (4.0, 7.0, 0.0, 0.0), (26.0, 100.0, 0.32, 0.12), (np.nan, 12.0, 1.0, np.nan)
    err[2, 0] = (0.0, 0.0, 0.0, 0.0)                                 # an invalid slot's numbers are never read
    got = BP.summarise_bop(rec, err, [100.0, 10.0, 50.0], 640)
    d = got["labels"][0]
    assert d["num_annotations"] == 4.0
    assert math.isclose(d["AR_MSSD"], 15 / 40, abs_tol=1e-15) and math.isclose(d["AR_MSPD"], 17 / 40, abs_tol=1e-15)
    assert math.isclose(d["AR_VSD"], (14 / 40 + 18 / 40) / 2, abs_tol=1e-15) and math.isclose(d["AR"], 0.4, abs_tol=1e-15)
    assert got["labels"][1] == dict(AR_VSD=0.0, AR_MSSD=0.0, AR_MSPD=0.0, AR=0.0, num_annotations=1.0)
    assert all(np.isnan(got["labels"][2][k]) for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")) and got["labels"][2]["num_annotations"] == 0.0
    assert math.isclose(got["mean"]["AR"], 0.2, abs_tol=1e-15) and got["mean"]["num_annotations"] == 5.0
    # the oracle's arithmetic on the same label
    o = B.average_recall([4.0, 26.0, np.nan], [7.0, 100.0, 12.0], [[0.0, 0.0], [0.32, 0.12], [1.0, np.nan]], 4, 100.0, 640)
    assert all(math.isclose(o[k], d[k], abs_tol=1e-15) for k in o)
    # r = width / 640 scales the pixel thresholds: at width 320 they are 2.5..25, MSPD 7 / 100 / 12 pass 8 / 0 / 6
    assert math.isclose(BP.summarise_bop(rec, err, [100.0, 10.0, 50.0], 320)["labels"][0]["AR_MSPD"], 14 / 40, abs_tol=1e-15)


def test_folder_settings_and_the_scene_folders_models_info(tmp_path):
    """What ``evaluate_scene_device(bop=True)`` builds from a folder's ``models/``: the PLY mesh with its faces and the symmetry set of
    models_info.yml; a PLY file without faces is refused with the reason."""
    from hmd_ego_pose_amd import evaluate as E
    from tests._util import make_linemod_folder
    make_linemod_folder(str(tmp_path / "ds"), n=2, size=64)
    sc = E.SceneFolder(str(tmp_path / "ds"), [1])
    assert len(sc.models_info) == 1 and float(sc.models_info[0]["diameter"]) == sc.models[0][1]
    with pytest.raises(ValueError, match="bop needs triangle faces"):
        BP.folder_settings("evaluate_scene_device", sc.model_path, sc.object_ids, sc.models_info, torch.device("cpu"))
    v, f = R.cube(60.0)
    os.makedirs(tmp_path / "models")
    with open(tmp_path / "models" / "obj_01.ply", "w") as out:
        out.write("ply\nformat ascii 1.0\nelement vertex 8\nproperty float x\nproperty float y\nproperty float z\nelement face 12\nproperty list uchar int vertex_indices\nend_header\n")
        out.write("".join(f"{a} {b} {c}\n" for a, b, c in v.tolist()) + "".join(f"3 {a} {b} {c}\n" for a, b, c in f.tolist()))
    info = [dict(sc.models_info[0], symmetries_discrete=[HALF_TURN_Z], symmetries_continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}])]
    s = BP.folder_settings("evaluate_scene_device", str(tmp_path / "models"), [1], info, torch.device("cpu"), max_sym_disc_step=0.5)
    assert s.meshes.num_faces == 12 and s.meshes.vertex_start.tolist() == [0, 8] and s.symmetries.start.tolist() == [0, 14] and s.delta == 15.0
    with pytest.raises(ValueError, match="coarsen max_sym_disc_step"):
        BP.folder_settings("evaluate_scene_device", str(tmp_path / "models"), [1], info, torch.device("cpu"))
