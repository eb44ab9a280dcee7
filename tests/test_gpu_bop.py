"""hep_bop_point_errors_device and hep_bop_vsd_device (MSSD / MSPD and VSD of matched pairs), bop.pairs_from_scene, bop.bop_errors and the
evaluators' ``bop=`` against the numpy definition of tests/_bop.py on the SAME tables: MSSD and MSPD within the float64 bound of
tests/_score.py (1e-9 relative - only the final sqrt is not an IEEE + - * /), the VSD counts exactly and the VSD errors bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import _bop as B
from tests import _render as R
from tests import _score as S
from tests import _score_scene as SS

pytestmark = pytest.mark.gpu
GUARD = 64
IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
EYE = np.eye(3)


@pytest.fixture(scope="module")
def env():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd import bop as BP
    from hmd_ego_pose_amd import render as RN
    assert torch.cuda.is_available()
    return BP, RN, _capi


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """An exact-size output window between two guards of GUARD bytes; the window starts as 0xFF bytes - NaN as float32 or float64, -1 as int32."""

    def __init__(self, nbytes):
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.window = self.buf[GUARD:GUARD + nbytes]
        self.window.fill_(0xFF)
        self.ptr = self.window.data_ptr()
        assert self.ptr % 16 == 0

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.window.numel():] == 0xA5).all())

    def host(self, dtype):
        return self.window.cpu().numpy().view(dtype)


def i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def sym_row(Rm, t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.asarray(Rm, np.float64).reshape(9), np.asarray(t, np.float64)])


# ---- MSSD / MSPD -----------------------------------------------------------------------------------------------------------------
def point_case(n, sizes, syms, seed):
    """``n`` pairs over len(sizes) labels with sizes[l] vertices and syms[l] symmetries (random rigid transforms behind the identity).  Row
    i has label i mod labels and an estimate near the ground truth; with n >= 3 row 1 is invalid in one of four ways (by n), with n >= 5
    row 3 sits exactly on its label's last symmetry and row 4 has vertices behind the camera."""
    rng = np.random.Generator(np.random.PCG64([seed, n]))
    L = len(sizes)
    verts = [rng.uniform(-60, 60, (v, 3)).astype(np.float32) for v in sizes]
    tables = [np.stack([IDENTITY] + [sym_row(R.rotation(rng.standard_normal(3), rng.uniform(0.2, 3.0)), rng.uniform(-5, 5, 3)) for _ in range(s - 1)]) for s in syms]
    rows = []
    for i in range(n):
        lab = i % L
        Rg = R.rotation(rng.standard_normal(3), rng.uniform(0.1, 3.0))
        tg = np.array([rng.normal(0, 40), rng.normal(0, 40), 600 + rng.normal(0, 50)])
        Re = R.rotation(rng.standard_normal(3), rng.uniform(0.0, 0.2)) @ Rg
        row = B.pair_row(lab, Rg, tg, Re, tg + rng.standard_normal(3) * 6, (480.0 + i, 470.0, 128.0, 120.0 - i), image=i)
        if i == 3 and n >= 5:
            Rp, tp = B.compose(row, tables[lab][-1])
            row = B.pair_row(lab, Rg, tg, Rp, tp, row[28:32])
        if i == 4 and n >= 5:
            row[27] = 20.0                                          # the estimate's model straddles Z = 0
        if i == 1 and n >= 3:
            bad = n % 4
            if bad == 0:
                row[0] = 0.0
            elif bad == 1:
                row[1] = float(L)
            elif bad == 2:
                row[1] = float("nan")
            else:
                row[20] = float("nan")
        rows.append(row)
    start = np.concatenate([[0], np.cumsum(sizes)])
    sstart = np.concatenate([[0], np.cumsum(syms)])
    return np.stack(rows), np.concatenate(verts), start, np.concatenate(tables), sstart


POINT_CASES = {"n1_v1_s1": (1, (1,), (1,)), "n3_v37_s2": (3, (37, 1), (2, 1)), "n17_v1025_s64": (17, (1025, 37), (64, 2)), "n7_two_labels": (7, (5, 300), (1, 3))}


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_point_errors(env, name):
    BP, RN, _capi = env
    n, sizes, syms = POINT_CASES[name]
    pairs, verts, vstart, table, sstart = point_case(n, sizes, syms, 11)
    want = B.point_errors(pairs, verts, vstart, table, sstart)
    if n >= 3:
        assert np.isnan(want[1]).all() and not np.isnan(want[0]).any() and not np.isnan(want[2]).any()      # an invalid row between valid ones
    if n >= 5:
        assert want[3, 0] == 0.0 and np.isnan(want[4, 1]) and want[4, 0] > 100.0                          # on a symmetry; behind the camera: MSPD only
    assert (want[0] > 0).all()
    p, v, t = dev(pairs), dev(verts), dev(table)
    (vs, vs_p), (ss, ss_p) = i32(vstart), i32(sstart)
    runs = []
    for _ in range(2):
        g = Guarded(n * 16)
        rc = _capi.lib().hep_bop_point_errors_device(p.data_ptr(), n, v.data_ptr(), len(verts), vs_p, t.data_ptr(), len(table), ss_p, len(sizes), g.ptr,
                                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and g.intact()
        runs.append(g.host(np.float64).reshape(n, 2))
    got = runs[0]
    assert runs[0].tobytes() == runs[1].tobytes()                   # two runs are bit-identical
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for i in range(n):
        for k in range(2):
            if not np.isnan(want[i, k]):
                assert abs(got[i, k] - want[i, k]) <= S.tolerance(7, want[i, k]), (i, k, got[i, k], want[i, k])
    assert got[3, 0] == 0.0 if n >= 5 else True


# ---- VSD ---------------------------------------------------------------------------------------------------------------------------
def vsd_case(n, H, W, T, images, seed):
    """``n`` depth triples of H x W in millimetres: a ground-truth blob at about 600, an estimate that is the blob shifted by a pixel or
    two with depth differences from 0.5 to 60 (so that the T taus between 3 and 48 all separate pixels), and - with ``images`` > 0 -
    test images shared by the pairs (image index i mod images) with holes, background, surfaces near delta and an occluder block.  With
    n >= 3 the last pair renders nothing (union 0) and pair 1 is switched off; with n >= 5 pair 2 points at an image that is not there."""
    rng = np.random.Generator(np.random.PCG64([seed, n, H, W, T]))
    ys, xs = np.mgrid[0:H, 0:W]
    zg, ze = np.zeros((n, H, W), np.float32), np.zeros((n, H, W), np.float32)
    rows = []
    for i in range(n):
        cy, cx, r = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, rng.uniform(0.25, 0.45) * min(H, W)
        blob = (ys - cy) ** 2 + (xs - cx) ** 2 < r * r
        zg[i] = np.where(blob, 600 + 0.8 * (xs - cx) + rng.normal(0, 2, (H, W)), 0)
        moved = np.roll(blob, (int(rng.integers(-2, 3)), int(rng.integers(-2, 3))), axis=(0, 1))
        ze[i] = np.where(moved, 600 + 0.8 * (xs - cx) + rng.choice([0.5, 2, 4, 9, 14, 22, 35, 60], (H, W)) * rng.choice([-1, 1], (H, W)), 0)
        rows.append(B.pair_row(0, EYE, (0, 0, 600.0), EYE, (0, 0, 600.0), (300.0 + 7 * i, 310.0, W / 2 + 0.3, H / 2 - 0.4), image=i % max(images, 1)))
    if n >= 3:
        zg[n - 1], ze[n - 1] = 0, 0
        rows[1][0] = 0.0
    if n >= 5 and images:
        rows[2][2] = float(images)
    zt = None
    if images:
        zt = np.zeros((images, H, W), np.float32)
        for m in range(images):
            kind = rng.random((H, W))
            zt[m] = np.where(kind < 0.25, 0, np.where(kind < 0.5, 2000, 600 + rng.choice([-40, -16, -14, -3, 0, 3, 14, 16, 40], (H, W))))      # holes, background, near delta = 15
            zt[m, H // 4:H // 2, W // 4:W // 2] = 350.0                                                                                         # an occluder
    taus = np.linspace(3.0, 48.0, T) if T > 1 else np.array([20.0])
    return np.stack(rows), zg, ze, zt, 15.0, taus


VSD_CASES = {"16x16_n1_T1": (1, 16, 16, 1, 0), "16x16_n1_T1_test": (1, 16, 16, 1, 1), "48x80_n3_T10": (3, 48, 80, 10, 2), "48x80_n3_T10_null": (3, 48, 80, 10, 0),
             "40x72_n17_T16": (17, 40, 72, 16, 3)}


@pytest.mark.parametrize("name", list(VSD_CASES))
def test_vsd(env, name):
    BP, RN, _capi = env
    n, H, W, T, images = VSD_CASES[name]
    pairs, zg, ze, zt, delta, taus = vsd_case(n, H, W, T, images, 23)
    want, want_c = B.vsd(pairs, zg, ze, zt, delta, taus, 1)
    live = want_c[want_c[:, 0] > 0]
    assert len(live) and (live[:, 0] > live[:, 1]).all() and (live[:, 1] > live[:, 2]).all()
    if T > 1:
        assert (live[:, 2] > live[:, 1 + T]).all() and (live[:, 1 + T] > 0).all()          # the taus separate pixels
    if n >= 3:
        assert want_c[n - 1].tolist() == [0] * (2 + T) and want[n - 1].tolist() == [1.0] * T and (want_c[1] == -1).all() and np.isnan(want[1]).all()
    if n >= 5 and images:
        assert (want_c[2] == -1).all() and want_c[3, 0] > 0
    if images:
        free = B.vsd(pairs[:1], zg[:1], ze[:1], None, delta, taus, 1)[1]
        assert 0 < want_c[0, 0] < free[0, 0]                        # the test image hides pixels
    p, g_, e_, t_ = dev(pairs), dev(zg), dev(ze), dev(zt)
    need = _capi.check(_capi.lib().hep_bop_workspace_bytes(n, T))
    assert need == (n * (2 + T) * 4 + 15) // 16 * 16
    th = np.ascontiguousarray(taus, np.float64)
    runs = []
    for _ in range(2):
        out, cnt, ws = Guarded(n * T * 8), Guarded(n * (2 + T) * 4), Guarded(need)
        rc = _capi.lib().hep_bop_vsd_device(p.data_ptr(), n, 1, g_.data_ptr(), e_.data_ptr(), None if t_ is None else t_.data_ptr(), images, H, W, delta,
                                            th.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), T, out.ptr, cnt.ptr, ws.ptr, need, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and out.intact() and cnt.intact() and ws.intact()
        runs.append((out.host(np.float64).reshape(n, T), cnt.host(np.int32).reshape(n, 2 + T)))
    got, got_c = runs[0]
    assert np.array_equal(got_c, want_c), np.argwhere(got_c != want_c)[:5].tolist()        # EXACTLY
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))                      # bit for bit (a skipped row: the default quiet NaN on both sides)
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


# ---- the pair table --------------------------------------------------------------------------------------------------------------
def test_pairs_from_scene_on_device_records(env):
    """Records produced by hep_score_scene_device from the synthetic rows of tests/_score_scene.py, the table against a host restatement."""
    BP, RN, _capi = env
    from tests.test_bop_cpu import host_pairs
    from tests.test_gpu_score_scene import _launch
    det, gt, cl, o, M = SS.case("special")
    (rec, *_), intact, (d, g, _p) = _launch(det, gt, cl, M)
    assert intact and np.array_equal(rec[..., :3], o[0][..., :3]) and (rec[..., 1] == 1.0).sum() >= 6
    got = BP.pairs_from_scene(g, d, dev(rec)).cpu().numpy()
    want = host_pairs(det, gt, rec)
    assert got.shape == want.shape and np.array_equal(got[:, :4], want[:, :4])
    on = want[:, 0] == 1.0
    assert np.array_equal(got[on][:, 13:16], want[on][:, 13:16]) and np.array_equal(got[on][:, 25:32], want[on][:, 25:32])
    assert np.allclose(got[on][:, 4:13], want[on][:, 4:13], rtol=0, atol=4e-16) and np.allclose(got[on][:, 16:25], want[on][:, 16:25], rtol=0, atol=4e-16)
    with pytest.raises(ValueError):
        BP.pairs_from_scene(g, d, dev(rec).cpu())


# ---- bop_errors: renders, both entry points, chunks, taus per label ---------------------------------------------------------------
MODELS = (R.cube(60.0), R.tetrahedron(70.0))
DIAMETERS = (2 * 60.0 * math.sqrt(3.0), 2 * 70.0 * math.sqrt(3.0))


def model_pairs(H, W):
    """Five pairs over the cube (label 0, a half turn about z listed) and the tetrahedron: near misses, one on the symmetry, one invalid."""
    cam = (480.0, 480.0, W / 2, H / 2)
    half = sym_row(R.rotation((0, 0, 1), math.pi))
    rows = []
    for i, (lab, axis, ang, t, dt) in enumerate(((0, (1, 2, 3), 0.7, (-20.0, 10.0, 1000.0), (4.0, -3.0, 12.0)), (1, (3, -1, 2), 1.9, (30.0, 0.0, 900.0), (-2.0, 5.0, -25.0)),
                                                 (0, (0, 1, 0), 0.4, (0.0, -15.0, 1100.0), (0.0, 0.0, 0.0)), (1, (1, 0, 1), 2.5, (10.0, 20.0, 950.0), (40.0, 0.0, 3.0)),
                                                 (0, (1, 1, 0), 1.2, (5.0, 5.0, 1000.0), (1.0, 1.0, 1.0)))):
        Rg = R.rotation(axis, ang)
        rows.append(B.pair_row(lab, Rg, t, R.rotation((0, 0, 1), 0.03) @ Rg, np.add(t, dt), cam, image=i % 2))
    Rp, tp = B.compose(rows[2], half)
    rows[2] = B.pair_row(0, rows[2][4:13], rows[2][13:16], Rp, tp, cam, image=0)
    rows[3][0] = 0.0
    return np.stack(rows), np.stack([IDENTITY, half]), IDENTITY[None]


def test_bop_errors_against_the_definition(env):
    BP, RN, _capi = env
    H, W = 48, 80
    pairs, sym0, sym1 = model_pairs(H, W)
    verts, faces, fstart = R.concat(MODELS)
    zg, ze = B.render_depths(pairs, verts, faces, fstart, H, W)
    assert all((zg[i] > 0).sum() > 15 for i in (0, 1, 2, 4)) and not zg[3].any()
    rng = np.random.Generator(np.random.PCG64(2))
    zt = np.where(rng.random((2, H, W)) < 0.5, 0, 1000 + rng.choice([-200.0, -10.0, 10.0, 300.0], (2, H, W))).astype(np.float32)
    tau = np.array(DIAMETERS)[:, None] * np.array(BP.TAU_FRACTIONS)[None, :]
    mesh, syms = RN.MeshSet(list(MODELS)), BP.SymmetrySet([sym0, None])
    want_p = B.point_errors(pairs, verts, mesh.vertex_start, np.concatenate([sym0, sym1]), [0, 2, 3])
    assert want_p[2, 0] == 0.0 and np.isnan(want_p[3]).all()
    for test in (None, zt):
        want_v, want_c = np.full((5, 10), np.nan), np.full((5, 12), -1, np.int32)
        for l in range(2):                                          # the label's own taus
            own = pairs[:, 1] == l
            v_l, c_l = B.vsd(pairs[own], zg[own], ze[own], test, 15.0, tau[l], 2)
            want_v[own], want_c[own] = v_l, c_l
        for chunk in (2, 64):
            got = BP.bop_errors(dev(pairs), mesh, syms, H, W, depth_test=dev(test), delta=15.0, taus=tau, chunk=chunk)
            assert np.array_equal(got["counts"].cpu().numpy(), want_c) and np.array_equal(got["vsd"].cpu().numpy().view(np.uint64), want_v.view(np.uint64))
            for k, key in enumerate(("mssd", "mspd")):
                g = got[key].cpu().numpy()
                assert np.array_equal(np.isnan(g), np.isnan(want_p[:, k])) and all(abs(a - b) <= S.tolerance(7, b) for a, b in zip(g, want_p[:, k]) if b == b)
        assert want_c[2, 2:].sum() == 0 and want_c[0, 2] > want_c[0, 11]
    one = BP.bop_errors(dev(pairs), mesh, syms, H, W, taus=(20.0, 40.0))                  # the same taus for every label: one launch
    both = [B.vsd(pairs, zg, ze, None, 15.0, (20.0, 40.0), 2)]
    assert np.array_equal(one["counts"].cpu().numpy(), both[0][1]) and one["vsd"].shape == (5, 2)
    with pytest.raises(ValueError):
        BP.bop_errors(dev(pairs).cpu(), mesh, syms, H, W)


# ---- the evaluators ----------------------------------------------------------------------------------------------------------------
class _Planted:
    """The seeded model with rows planted in front of its own: ``detect`` runs the real forward and filter, then overwrites the first rows
    of every image with the prepared detections, so that the matches of the test do not depend on what the seeded weights detect."""

    def __init__(self, inner, planted):
        self.inner, self.model, self.planted = inner, inner.model, planted

    def detect(self, x, camera):
        det = {k: v.clone() for k, v in self.inner.detect(x, camera).items()}
        for b, rows in enumerate(self.planted):
            for j, row in enumerate(rows):
                for k, value in row.items():
                    det[k][b, j] = torch.as_tensor(value, dtype=det[k].dtype, device=det[k].device)
        return det


def _box(pose_R, t, verts, cam):
    p = verts.astype(np.float64) @ np.asarray(pose_R).T + t
    u, v = cam[0] * p[:, 0] / p[:, 2] + cam[2], cam[1] * p[:, 1] / p[:, 2] + cam[3]
    return np.array([u.min(), v.min(), u.max(), v.max()])


def test_scene_evaluator_with_bop(env):
    """phi 0, size 128, batch 2, seeded 2-class weights, a cube and a tetrahedron as models.  Image 0: both annotated, each with a planted
    detection near its pose; image 1: the cube with a planted detection, the tetrahedron without one.  result()["bop"] equals the
    definition evaluated on the detections copied to the host, and every pre-existing key is byte-identical with and without bop=."""
    BP, RN, _capi = env
    from hmd_ego_pose_amd import HMDEgoPose, TrainModelWithLoss
    from hmd_ego_pose_amd import evaluate as E
    from hmd_ego_pose_amd.weights import seeded_state_dict
    size, kw = 128, dict(score_threshold=0.05, max_detections=10, iou_threshold=0.5)
    m = HMDEgoPose({"iter": 0}, num_classes=2, compound_coef=0, onnx_export=True, input_sizes=[size] * 9)
    m.load_state_dict(seeded_state_dict(0, 0, num_classes=2), strict=True)
    inner = TrainModelWithLoss(m.to("cuda").eval()).eval()
    cam4 = (480.0, 480.0, 64.0, 64.0)
    K = np.array([[480.0, 0, 64.0], [0, 480.0, 64.0], [0, 0, 1.0]])
    rng = np.random.Generator(np.random.PCG64(31))
    frames = rng.integers(0, 256, (2, size, size, 3), dtype=np.uint8)
    anns, planted = [], []
    for image, entries in enumerate((((0, (1, 2, 3), 0.7, (-25.0, 10.0, 1000.0), (6.0, -4.0, 20.0)), (1, (3, -1, 2), 1.9, (40.0, -20.0, 1100.0), (-3.0, 2.0, -35.0))),
                                     ((0, (0, 1, 1), 0.4, (10.0, 15.0, 900.0), (1.0, 0.5, 4.0)), (1, (1, 0, 1), 2.5, (-40.0, -30.0, 1200.0), None)))):
        anns.append([]); planted.append([])
        for j, (lab, axis, ang, t, dt) in enumerate(entries):
            rv = np.asarray(axis, np.float64) / np.linalg.norm(axis) * ang
            box = _box(R.rotation(axis, ang), np.asarray(t), MODELS[lab][0], cam4)
            anns[-1].append({"label": lab, "bbox": box.astype(np.float32), "rotation": rv, "translation": np.asarray(t, np.float64), "drill_tip": np.zeros(3)})
            if dt is not None:
                planted[-1].append(dict(scores=0.99 - 0.01 * j, labels=lab, boxes=box + [1.0, -1.0, 1.0, 0.0], rotation=(rv + 0.02) / math.pi,
                                        translation=np.add(t, dt), hand=np.zeros(63)))
    model = _Planted(inner, planted)
    gt = E.gt_scene_table(anns, [K, K], 1.0, 2)
    g, u8 = torch.from_numpy(gt).cuda(), torch.from_numpy(frames).cuda()
    cam = torch.tensor([[480.0, 480.0, 64.0, 64.0, 1000.0, 1.0]] * 2).cuda()
    models = [(MODELS[l][0], DIAMETERS[l], False) for l in range(2)]
    half = sym_row(R.rotation((0, 0, 1), math.pi))
    mesh, syms = RN.MeshSet(list(MODELS)), BP.SymmetrySet([np.stack([IDENTITY, half]), None])
    settings = BP.BopSettings(mesh, syms)
    zt = np.zeros((2, size, size), np.float32)
    zt[:, :, 70:] = 400.0                                           # a wall in front of everything right of column 70
    plain, with_bop, with_depth = (E.SceneEvaluator(model, models, size, capacity=2, amax=2, **kw) for _ in range(3))
    for bad in (dict(bop=mesh), dict(depth_test=dev(zt)), dict(bop=settings, depth_test=dev(zt).double()), dict(bop=settings, depth_test=dev(zt)[:1]),
                dict(bop=BP.BopSettings(RN.MeshSet([MODELS[0]]), BP.SymmetrySet([None])))):
        with pytest.raises(ValueError):
            with_bop.add(u8, cam, g, **bad)
    assert with_bop.count == 0
    plain.add(u8, cam, g)
    with_bop.add(u8, cam, g, bop=settings)
    with_depth.add(u8, cam, g, bop=settings, depth_test=dev(zt))
    a, b, c = plain.result(), with_bop.result(), with_depth.result()
    assert "bop" not in a and list(b) == list(a) + ["bop"] and list(c) == list(b)
    assert plain._buf.cpu().numpy().tobytes() == with_bop._buf.cpu().numpy().tobytes() == with_depth._buf.cpu().numpy().tobytes()
    assert repr({k: b[k] for k in a}) == repr(a) and repr({k: c[k] for k in a}) == repr(a)      # NaN-proof equality of the nested dictionaries
    # the definition on the detections copied to the host
    det = model.detect(inner.model.session(size, 2, u8.device).preprocess(u8), cam)
    rows = {k: det[k].cpu().numpy() for k in ("boxes", "scores", "labels", "rotation", "translation", "hand")}
    rec = SS.score_scene_batch(rows, gt, [MODELS[0][0], MODELS[1][0]], **kw)[0]
    assert rec[..., 1].tolist() == [[1.0, 1.0], [1.0, 0.0]]          # the planted rows are the matches; the last annotation has none
    pairs = BP.pairs_from_scene(g, det, dev(rec)).cpu().numpy()      # the table the evaluator made (device Rodrigues) is the input of both sides
    verts, faces, fstart = R.concat(MODELS)
    zg, ze = B.render_depths(pairs, verts, faces, fstart, size, size)
    errs = B.point_errors(pairs, verts, mesh.vertex_start, syms.host, syms.start)
    for got, test in ((b, None), (c, zt)):
        labels = {}
        for l in range(2):
            own = (pairs[:, 0] == 1.0) & (pairs[:, 1] == l)
            vsd_l = B.vsd(pairs[own], zg[own], ze[own], test, 15.0, np.array(BP.TAU_FRACTIONS) * DIAMETERS[l], 2)[0]
            labels[l] = B.average_recall(errs[own, 0], errs[own, 1], vsd_l, int(((rec[..., 0] == 1.0) & (rec[..., 12] == l)).sum()), DIAMETERS[l], size)
        print("definition", labels, "device", got["bop"]["labels"])
        for l in range(2):
            assert got["bop"]["labels"][l]["num_annotations"] == 2.0
            for k, w in labels[l].items():
                assert math.isclose(got["bop"]["labels"][l][k], w, rel_tol=0, abs_tol=1e-12), (l, k)
        for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
            assert math.isclose(got["bop"]["mean"][k], (labels[0][k] + labels[1][k]) / 2, rel_tol=0, abs_tol=1e-12)
    assert 0.0 < b["bop"]["labels"][0]["AR_MSSD"] <= 1.0 and 0.0 < b["bop"]["labels"][1]["AR"] <= 0.5      # the tetrahedron misses one of two
    assert b["bop"]["mean"]["AR_VSD"] != c["bop"]["mean"]["AR_VSD"] or b["bop"]["mean"]["AR_VSD"] in (0.0, 1.0)
    # bop= for some batches only is refused at the end; reset clears it
    mixed = E.SceneEvaluator(model, models, size, capacity=4, amax=2, **kw)
    mixed.add(u8, cam, g, bop=settings)
    mixed.add(u8, cam, g)
    with pytest.raises(ValueError, match="every add"):
        mixed.result()
    mixed.reset()
    mixed.add(u8, cam, g)
    assert repr(mixed.result()) == repr(a)
    # the single-object evaluator: label 0's annotations alone give label 0's numbers
    single, single_plain = (E.DeviceEvaluator(model, MODELS[0][0], DIAMETERS[0], size, 2, **kw) for _ in range(2))
    one = BP.BopSettings(RN.MeshSet([MODELS[0]]), BP.SymmetrySet([np.stack([IDENTITY, half])]))
    single.add(u8, cam, g[:, 0].contiguous(), bop=one)
    single_plain.add(u8, cam, g[:, 0].contiguous())
    s, sp = single.result(), single_plain.result()
    assert repr({k: s[k] for k in sp}) == repr(sp) and list(s) == list(sp) + ["bop"]
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert math.isclose(s["bop"]["labels"][0][k], b["bop"]["labels"][0][k], rel_tol=0, abs_tol=1e-12), k
