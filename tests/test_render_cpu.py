"""The model renderer's definition (tests/_render.py) pinned against independent formulations, and the host side of
hmd_ego_pose_amd.render: PLY reader, MeshSet, pose tables, argument checks.  No GPU."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _draw as D
from tests import _render as R

U = 2.0 ** -53                                   # unit roundoff of float64


# ---- coverage ------------------------------------------------------------------------------------------------------------------
GRID = 24                                        # pixels per side of the coverage frame
COVER_SEED, COVER_DRAWN, COVER_CAP = 11, 400, 0.05


def general_position_triangles():
    """(kept triangles, number rejected) of COVER_DRAWN random sub-pixel triangles around a GRID x GRID frame: a triangle is rejected
    when its area is zero or a pixel centre of the frame lies exactly on one of its edge lines inside the frame."""
    rng = np.random.Generator(np.random.PCG64(COVER_SEED))
    ys, xs = np.mgrid[0:GRID, 0:GRID]
    kept, rejected = [], 0
    for _ in range(COVER_DRAWN):
        tri = [tuple(int(v) for v in rng.integers(-40, 16 * GRID + 40, 2)) for _ in range(3)]
        cov = R.coverage(tri, xs, ys)
        if cov is None or any((e == 0).any() for e in cov[1]):
            rejected += 1
            continue
        kept.append(tri)
    return kept, rejected


def test_generator_rejects_few_triangles():
    """The seed's rejection count, stated: 14 of 400 drawn (3.5 %), below the cap of 5 %."""
    kept, rejected = general_position_triangles()
    assert rejected == 14 and rejected <= COVER_CAP * COVER_DRAWN and len(kept) + rejected == COVER_DRAWN


def test_coverage_equals_float64_barycentric_test():
    kept, _ = general_position_triangles()
    ys, xs = np.mgrid[0:GRID, 0:GRID]
    px, py = 16.0 * xs + 8.0, 16.0 * ys + 8.0
    covered = 0
    for tri in kept:
        (x0, y0), (x1, y1), (x2, y2) = [(float(a), float(b)) for a, b in tri]
        det = (y1 - y2) * (x0 - x2) + (x2 - x1) * (y0 - y2)
        l0 = ((y1 - y2) * (px - x2) + (x2 - x1) * (py - y2)) / det
        l1 = ((y2 - y0) * (px - x2) + (x0 - x2) * (py - y2)) / det
        l2 = 1.0 - l0 - l1
        want = (l0 > 0) & (l1 > 0) & (l2 > 0)
        got, _E = R.coverage(tri, xs, ys)
        assert np.array_equal(got, want), tri
        assert np.array_equal(got, R.coverage([tri[0], tri[2], tri[1]], xs, ys)[0])          # the other winding covers the same
        covered += int(got.sum())
    assert covered > 5000


# ---- depth ---------------------------------------------------------------------------------------------------------------------
def test_depth_is_the_ray_plane_intersection_of_the_snapped_triangle():
    """z of a fragment against the exact (rational) intersection of the ray through the pixel centre with the plane of the SNAPPED
    triangle: vertices at their sub-pixel positions s_i with their depths Z_i, i.e. the points (s_ix Z_i, s_iy Z_i, Z_i) in the space where
    a pixel's ray is (cx z, cy z, z) - an affine image of camera space, so planes and intersections are the same.
    Bound: 1 / Z_i rounds once, each product E_i w_i once, the two sums once each (all terms positive: no cancellation), the division by
    the exact A once, the reciprocal once - a term carries at most six roundings: |z - exact| <= ((1 + u)^6 - 1) exact < 6.001 u exact."""
    rng = np.random.Generator(np.random.PCG64(5))
    ys, xs = np.mgrid[0:GRID, 0:GRID]
    checked, worst = 0, 0.0
    for _ in range(40):
        tri = [tuple(int(v) for v in rng.integers(-40, 16 * GRID + 40, 2)) for _ in range(3)]
        Z = [float(v) for v in rng.uniform(0.2, 3.0, 3)]
        cov = R.coverage(tri, xs, ys)
        if cov is None or not cov[0].any():
            continue
        inside, E = cov
        z = R.face_depth(E, [1.0 / np.float64(v) for v in Z])
        P = [(Fraction(t[0]) * Fraction(v), Fraction(t[1]) * Fraction(v), Fraction(v)) for t, v in zip(tri, Z)]
        a, b = [P[1][k] - P[0][k] for k in range(3)], [P[2][k] - P[0][k] for k in range(3)]
        n = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
        nP = sum(n[k] * P[0][k] for k in range(3))
        for y, x in np.argwhere(inside)[:12]:
            exact = nP / (n[0] * (16 * int(x) + 8) + n[1] * (16 * int(y) + 8) + n[2])
            err = abs(Fraction(float(z[y, x])) - exact) / exact
            worst = max(worst, float(err) / U)
            assert err <= Fraction(6.001) * Fraction(U), (tri, Z, int(x), int(y), float(err) / U)
            checked += 1
    assert checked > 200
    print(f"depth: {checked} fragments, worst error {worst:.2f} u")


# ---- shared edges --------------------------------------------------------------------------------------------------------------
S = 16
QUADS = {"axis-aligned": [(8, 8), (8 + 6 * S, 8), (8 + 6 * S, 8 + 6 * S), (8, 8 + 6 * S)],
         "rotated": [(8 + 4 * S, 8), (8 + 8 * S, 8 + 4 * S), (8 + 4 * S, 8 + 8 * S), (8, 8 + 4 * S)]}


@pytest.mark.parametrize("name", list(QUADS))
def test_faces_sharing_an_edge_tile_the_quad(name):
    """Corners ON pixel centres, so centres fall on both diagonals and on the outline: the two faces of a split are disjoint, and both
    splits - in either winding - cover the same set."""
    q = QUADS[name]
    ys, xs = np.mgrid[0:12, 0:12]
    unions = []
    for split in (((0, 1, 2), (0, 2, 3)), ((0, 1, 3), (1, 2, 3))):
        for flip in (False, True):
            cov = []
            for tri in split:
                idx = tri[::-1] if flip else tri
                inside, E = R.coverage([q[i] for i in idx], xs, ys)
                cov.append(inside)
            on_diagonal = [(e == 0) for e in E]                       # the last face's edges: centres do lie on them
            assert any(m.any() for m in on_diagonal)
            assert not (cov[0] & cov[1]).any()
            unions.append(cov[0] | cov[1])
    for u in unions[1:]:
        assert np.array_equal(u, unions[0])
    n = int(unions[0].sum())
    assert n == (36 if name == "axis-aligned" else 32), n              # 6 x 6 pixels; the diamond of half-diagonal 4: 2 * 4 * 4


def test_top_left_rule_owns_top_and_left():
    ys, xs = np.mgrid[0:12, 0:12]
    got = R.coverage(QUADS["axis-aligned"][:3], xs, ys)[0] | R.coverage([QUADS["axis-aligned"][i] for i in (0, 2, 3)], xs, ys)[0]
    assert got[0:6, 0:6].all() and not got[6].any() and not got[:, 6].any()


# ---- the other rules of the oracle --------------------------------------------------------------------------------------------
def flat_triangle(z=0.5):
    """A large triangle facing the camera at depth z, one label."""
    v = np.array([[-1, -1, 0], [1, -1, 0], [0, 1.5, 0]], np.float32)
    return v, np.array([[0, 1, 2]], np.int32)


CAM = np.array([[20.0, 20.0, 8.0, 8.0, 1.0]])


def test_ties_go_to_the_lower_slot_then_the_lower_face():
    v, f = flat_triangle()
    poses = np.stack([R.pose_row(0, 10, None, (0, 0, 0.5)), R.pose_row(0, 20, None, (0, 0, 0.5))])[None]
    out = R.render_models(poses, CAM, v, f, [0, 1], 16, 16)
    assert out["mask"].max() == 10 and set(np.unique(out["mask"])) <= {0, 10} and (out["key"][out["mask"] > 0] >> 24 == 0).all()
    out = R.render_models(poses[:, ::-1], CAM, v, f, [0, 1], 16, 16)
    assert out["mask"].max() == 20 and set(np.unique(out["mask"])) <= {0, 20}
    twice = np.concatenate([f, f[:, [1, 2, 0]], f])
    out = R.render_models(poses[:, :1], CAM, v, twice, [0, 3], 16, 16)
    assert (out["key"][out["mask"] > 0] == 0).all() and (out["mask"] > 0).sum() > 50
    near = np.stack([R.pose_row(0, 10, None, (0, 0, 0.5)), R.pose_row(0, 20, None, (0, 0, 0.25))])[None]
    out = R.render_models(near, CAM, v, f, [0, 1], 16, 16)
    assert out["mask"][0, 8, 8] == 20 and out["depth"][0, 8, 8] == np.float32(0.25)


def test_skipped_rows_and_faces():
    v, f = flat_triangle()
    ok = R.render_models(R.pose_row(0, 9, None, (0, 0, 0.5))[None, None], CAM, v, f, [0, 1], 16, 16)
    assert (ok["mask"] == 9).sum() > 100 and ok["depth"][ok["mask"] == 9].min() == np.float32(0.5)
    for row in (R.pose_row(0, 9, None, (0, 0, 0.5), valid=0.0), R.pose_row(1, 9, None, (0, 0, 0.5)), R.pose_row(-1, 9, None, (0, 0, 0.5)),
                R.pose_row(float("nan"), 9, None, (0, 0, 0.5)), R.pose_row(0, 0, None, (0, 0, 0.5)), R.pose_row(0, 256, None, (0, 0, 0.5)),
                R.pose_row(0, 9, None, (0, 0, 0.0)), R.pose_row(0, 9, None, (0, 0, -0.5)), R.pose_row(0, 9, None, (float("nan"), 0, 0.5))):
        out = R.render_models(row[None, None], CAM, v, f, [0, 1], 16, 16)
        assert not out["mask"].any() and not out["depth"].any(), row
    assert R.render_models(R.pose_row(0, 255.5, None, (0, 0, 0.5))[None, None], CAM, v, f, [0, 1], 16, 16)["mask"].max() == 255
    # vertices behind the camera: the face is skipped whole (no clipping); zero area; an index out of range
    tilted = R.pose_row(0, 9, R.rotation((1, 0, 0), 1.2), (0, 0, 0.5))
    assert R.project(tilted, CAM[0], v)[3].tolist() == [False, False, True]
    assert not R.render_models(tilted[None, None], CAM, v, f, [0, 1], 16, 16)["mask"].any()
    row = R.pose_row(0, 9, None, (0, 0, 0.5))[None, None]
    assert not R.render_models(row, CAM, v, np.array([[0, 1, 1]], np.int32), [0, 1], 16, 16)["mask"].any()
    for bad in (3, -1):
        out = R.render_models(row, CAM, v, np.array([[0, 1, bad], [0, 1, 2]], np.int32), [0, 2], 16, 16)
        assert np.array_equal(out["mask"], ok["mask"]) and (out["key"][out["mask"] > 0] == 1).all()
    # a label's faces are its own
    two = R.render_models(R.pose_row(1, 9, None, (0, 0, 0.5))[None, None], CAM, v, np.array([[0, 1, 1], [0, 1, 2]], np.int32), [0, 1, 2], 16, 16)
    assert np.array_equal(two["mask"], ok["mask"])


def test_saturation_and_rounding_of_the_snap():
    assert R.snap(np.array([0.0, 0.03125, 0.03124, -0.03125, -0.04, 1e9, -1e9, np.inf, -np.inf, 8191.0, 8190.99, -8192.0])).tolist() == \
        [0, 1, 0, 0, -1, 131056, -131072, 131056, -131072, 131056, 131056, -131072]
    # a face far outside whose saturated corner reaches back over the frame is drawn from the saturated coordinates
    v = np.array([[-0.1, -0.1, 0], [3000.0, 0.0, 0], [-0.1, 0.2, 0]], np.float32)
    row = R.pose_row(0, 5, None, (0, 0, 0.5))
    sx, _sy, _w, valid = R.project(row, CAM[0], v)
    assert valid.all() and sx[1] == 131056
    out = R.render_models(row[None, None], CAM, v, np.array([[0, 1, 2]], np.int32), [0, 1], 16, 16)
    assert (out["mask"] == 5).sum() > 40


@pytest.mark.parametrize("alpha", [0, 1, 128, 255, 256])
def test_blend_formula(alpha):
    old, col = np.arange(256, dtype=np.uint8)[:, None].repeat(256, 1), np.arange(256, dtype=np.uint8)[None, :].repeat(256, 0)
    got = R.blend(old, col, alpha)
    want = np.array([[math.floor(Fraction(alpha * c + (256 - alpha) * o, 256) + Fraction(1, 2)) for c in range(256)] for o in range(0, 256, 17)])
    assert np.array_equal(got[::17], want)
    if alpha == 0:
        assert np.array_equal(got, old)
    if alpha == 256:
        assert np.array_equal(got, col)


def test_blend_touches_covered_pixels_only():
    c = R.case_scene()
    out = R.render_models(c["poses"], c["camera"], c["vertices"], c["faces"], c["face_start"], c["H"], c["W"], frames=c["frames"], colours=c["colours"], alpha=100)
    hit = out["mask"] > 0
    assert np.array_equal(out["frames"][~hit], c["frames"][~hit]) and np.array_equal(out["frames"][1], c["frames"][1]) and not out["mask"][1].any()
    assert set(np.unique(out["mask"][0])) == {0, 7, 200, 255} and set(np.unique(out["mask"][2])) >= {0, 3, 4, 5}
    assert (out["frames"][hit] != c["frames"][hit]).any()
    assert ((out["depth"] > 0) == hit).all()


# ---- reader and wrappers -------------------------------------------------------------------------------------------------------
def write_ply(path, v, faces, binary):
    head = ["ply", "format " + ("binary_little_endian" if binary else "ascii") + " 1.0", f"element vertex {len(v)}", "property float x", "property float y",
            "property float z", "property uchar red", f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if binary:
            for p in v:
                f.write(struct.pack("<fffB", *[float(c) for c in p], 7))
            for face in faces:
                f.write(struct.pack("<B" + "i" * len(face), len(face), *[int(i) for i in face]))
        else:
            for p in v:
                f.write((" ".join(repr(float(c)) for c in p) + " 7\n").encode())
            for face in faces:
                f.write((" ".join(str(int(i)) for i in (len(face), *face)) + "\n").encode())


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply_mesh(tmp_path, binary):
    from hmd_ego_pose_amd.evaluate import load_ply_vertices
    from hmd_ego_pose_amd.render import load_ply_mesh
    v, f = R.cube()
    p = str(tmp_path / "cube.ply")
    write_ply(p, v, f.tolist(), binary)
    gv, gf = load_ply_mesh(p)
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and np.array_equal(gv, v) and np.array_equal(gf, f)
    assert np.array_equal(load_ply_vertices(p), gv)
    for name, faces in (("quad", f.tolist()[:3] + [[0, 1, 3, 2]] + f.tolist()[3:]), ("quad_first", [[0, 1, 3, 2]]), ("index", [[0, 1, 8]])):
        q = str(tmp_path / f"{name}.ply")
        write_ply(q, v, faces, binary)
        with pytest.raises(ValueError, match=name + ".ply"):
            load_ply_mesh(q)


def test_mesh_set_offsets_and_checks():
    from hmd_ego_pose_amd.render import MeshSet
    cpu = torch.device("cpu")
    m = MeshSet([R.cube(), R.tetrahedron(), R.cube(0.1)], device=cpu)
    v, f, start = R.concat([R.cube(), R.tetrahedron(), R.cube(0.1)])
    assert np.array_equal(m.vertices.numpy(), v) and np.array_equal(m.faces.numpy(), f) and m.face_start.tolist() == start.tolist() == [0, 12, 16, 28]
    assert (m.num_labels, m.num_vertices, m.num_faces) == (3, 20, 28) and m.faces.dtype == torch.int32 and m.face_start.dtype == np.int32
    assert f[12:16].min() == 8 and f[16:].min() == 12
    cv, cf = R.cube()
    for bad in ([], [(cv, cf + 1)], [(cv, cf - 1)], [(cv[:, :2], cf)], [(cv, cf[:, :2])], [(cv, cf.astype(np.float32))], [(cv, cf[:0])], [R.cube()] * 64):
        with pytest.raises(ValueError):
            MeshSet(bad, device=cpu)


def test_poses_from_detections_follows_the_draw_calls_candidate_rule():
    from hmd_ego_pose_amd.render import poses_from_detections
    c = D.case_main()
    det, thr, M = c["det"], c["score_threshold"], c["max_detections"]
    table = poses_from_detections({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in det.items()}, thr, M).numpy()
    B, L = det["scores"].shape[0], len(c["cuboids"])
    assert table.shape == (B, M, 16)
    drawn = 0
    for b in range(B):
        kept = np.nonzero(np.asarray(det["scores"][b], np.float32) > np.float32(thr))[0][:M]      # tests/_draw.py image_shapes
        assert table[b, :, 0].tolist() == [1.0] * len(kept) + [0.0] * (M - len(kept))
        rendered = []
        for k, r in enumerate(kept):
            lab = int(det["labels"][b, r])
            rv = np.asarray(det["rotation"][b, r], np.float32) * np.float32(math.pi)
            assert rv.dtype == np.float32 and table[b, k, 1] == lab and table[b, k, 2] == lab + 1
            assert np.allclose(table[b, k, 4:13], D.rodrigues(rv)[0], rtol=0, atol=4e-16)
            assert table[b, k, 13:16].tolist() == [float(x) for x in det["translation"][b, r]]
            if R.row_label(table[b, k], L) is not None:
                rendered.append(table[b, k, 15])
        # ... and the oracle's own shapes of the image: as many detections, in the same order (a shape's first given depth is its centre's)
        shapes = [s for s in D.image_shapes(c["gt"][b, 0, 14:19], None, {k: v[b] for k, v in det.items()}, c["cuboids"], c["colours"], thr, M) if not s.annotation]
        assert [s.given_depths[0] for s in shapes] == rendered
        drawn += len(shapes)
    assert drawn >= 3
    with pytest.raises(ValueError):
        poses_from_detections({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in det.items()}, thr, 17)


def test_poses_from_annotations_both_sources():
    from hmd_ego_pose_amd.render import poses_from_annotations
    c = D.case_main()
    gt = torch.from_numpy(c["gt"])
    table = poses_from_annotations(gt).numpy()
    for b in range(gt.shape[0]):
        for k in range(gt.shape[1]):
            g = c["gt"][b, k]
            assert table[b, k, 0] == float(g[0] != 0) and np.array_equal(table[b, k, 13:16], g[8:11])
            if g[0] != 0 and g[83] == g[83]:
                assert table[b, k, 1] == g[83] and table[b, k, 2] == g[83] + 1
                assert np.allclose(table[b, k, 4:13], D.rodrigues(g[5:8])[0], rtol=0, atol=4e-16)
    assert poses_from_annotations(gt[:, 0]).shape == (gt.shape[0], 1, 16)
    assert np.array_equal(poses_from_annotations(gt, mask_values=[40, 50, 60, 70]).numpy()[..., 2][table[..., 1] == 1], np.full(int((table[..., 1] == 1).sum()), 50.0))
    padded = dict(labels=torch.tensor([[1, 0], [0, 0]], dtype=torch.int32), mask_values=torch.tensor([[9, 8], [7, 0]], dtype=torch.int32),
                  rvec=torch.tensor([[[0.1, 0.2, 0.3], [0, 0, 0]], [[1, 0, 0], [0, 0, 0]]], dtype=torch.float32), tvec=torch.ones(2, 2, 3),
                  num_gt=torch.tensor([2, 1], dtype=torch.int32))
    t = poses_from_annotations(padded).numpy()
    assert t[..., 0].tolist() == [[1, 1], [1, 0]] and t[..., 2].tolist() == [[9, 8], [7, 0]] and t[0, 1, 4:13].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert np.allclose(t[0, 0, 4:13], D.rodrigues(np.array([0.1, 0.2, 0.3], np.float32))[0], rtol=0, atol=4e-16)
    with pytest.raises(ValueError):
        poses_from_annotations(gt.float())
    with pytest.raises(ValueError):
        poses_from_annotations({k: v for k, v in padded.items() if k != "num_gt"})


def test_render_models_refuses_wrong_arguments_before_the_library():
    from hmd_ego_pose_amd.render import MeshSet, render_models
    m = MeshSet([R.cube()], device=torch.device("cpu"))
    poses, cam = torch.zeros(2, 3, 16, dtype=torch.float64), torch.zeros(2, 5, dtype=torch.float64)
    frames = torch.zeros(2, 32, 32, 3, dtype=torch.uint8)
    ok = dict(poses=poses, camera=cam, meshes=m, height=32, width=32)
    for change in (dict(poses=poses.float()), dict(poses=poses[0]), dict(poses=poses[..., :15]), dict(poses=torch.zeros(2, 17, 16, dtype=torch.float64)),
                   dict(poses=poses[:0]), dict(camera=cam.float()), dict(camera=cam[:1]), dict(camera=torch.zeros(2, 6, dtype=torch.float64)),
                   dict(meshes=(R.cube(),)), dict(height=15), dict(width=4097), dict(mask=False), dict(blend_into=frames.float()),
                   dict(blend_into=frames[:, :16]), dict(blend_into=frames[:, :, ::1, :2]), dict(blend_into=frames, colours=np.zeros((2, 3), np.uint8)),
                   dict(blend_into=frames, colours=np.zeros((1, 3), np.float32)), dict(blend_into=frames, alpha=257), dict(blend_into=frames, alpha=-1)):
        args = dict(ok, **change)
        with pytest.raises(ValueError):
            render_models(args.pop("poses"), args.pop("camera"), args.pop("meshes"), args.pop("height"), args.pop("width"), **args)
    import hmd_ego_pose_amd
    assert hmd_ego_pose_amd.render_models is render_models and hmd_ego_pose_amd.MeshSet is MeshSet
