"""The synthetic-frame definition (tests/_synth.py) against independent statements of its parts, and the host side of
hmd_ego_pose_amd.synth: coloured PLY reader, ShadedMeshSet, draw_poses, draw_lights, argument checks.  No GPU."""
import random
import struct

import numpy as np
import pytest
import torch

from tests import _render as R
from tests import _synth as S


@pytest.fixture(scope="module")
def overlap():
    c = S.case_overlap()
    return c, S.run(c)


def test_mask_and_depth_are_the_renderers(overlap):
    c, got = overlap
    want = R.render_models(c["poses"], c["camera"], c["vertices"], c["faces"], c["face_start"], c["H"], c["W"])
    assert np.array_equal(got["mask"], want["mask"]) and np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(got["key"], want["key"]) and (got["mask"] > 0).sum() > 500


def test_visible_is_the_extent_of_the_pixels_a_slot_won_and_boxes_those_of_the_mask_values(overlap):
    c, got = overlap
    B, K = c["poses"].shape[:2]
    slot = np.where(got["key"] != R.NO_KEY, got["key"] >> 24, -1)
    for b in range(B):
        for k in range(K):
            ys, xs = np.where(slot[b] == k)
            want = S.EMPTY if not len(ys) else (xs.min(), ys.min(), xs.max(), ys.max(), len(ys))
            assert tuple(got["visible"][b, k]) == tuple(want), (b, k)
    assert tuple(got["visible"][0, 2]) == S.EMPTY and tuple(got["visible"][1, 2]) == S.EMPTY      # wholly hidden; a skipped row
    ann = got["annotations"]
    assert ann["num_gt"].tolist() == [2, 2, 3]
    for b in range(B):                                               # distinct mask values: the box of a kept row is the extent of its mask value
        for n in range(ann["num_gt"][b]):
            ys, xs = np.where(got["mask"][b] == ann["mask_values"][b, n])
            assert ann["boxes"][b, n].tolist() == [xs.min(), ys.min(), xs.max(), ys.max()]
    # the overlap shows: a visible box is smaller than the projected one of the same pose alone
    alone = R.render_models(c["poses"][:1, :1], c["camera"][:1], c["vertices"], c["faces"], c["face_start"], c["H"], c["W"])["mask"][0]
    assert (alone > 0).sum() > got["visible"][0, 0, 4] > 0


# ---- shading -------------------------------------------------------------------------------------------------------------------
def one_face(colours=((200, 10, 30), (20, 220, 40), (60, 70, 250)), light=None, normal=(0.0, 0.0, -1.0), winding=(0, 1, 2), alpha=256, frame_value=77, Rm=None):
    """A triangle facing the camera at Z = 0.5 in a 24 x 24 frame."""
    v = np.array([[-0.05, -0.04, 0.0], [0.06, -0.03, 0.0], [0.0, 0.05, 0.0]], np.float32)
    f = np.array([list(winding)], np.int32)
    c = dict(poses=R.pose_row(0, 9, Rm, (0.0, 0.0, 0.5))[None, None], camera=np.array([[100.0, 100.0, 12.0, 12.0, 1.0]]), vertices=v,
             vertex_colours=np.asarray(colours, np.uint8), faces=f, face_normals=np.asarray([normal], np.float64), face_start=np.array([0, 1], np.int32),
             lights=(S.light_row((0, 0, -1), 0.0, 1.0) if light is None else np.asarray(light, np.float64))[None], H=24, W=24,
             frames=np.full((1, 24, 24, 3), frame_value, np.uint8), rvec=np.zeros((1, 1, 3), np.float32), tvec=np.zeros((1, 1, 3), np.float32), extra=np.zeros((1, 1, 2), np.float32))
    return c, S.run(c, alpha=alpha, min_pixels=1)


def test_head_on_light_reproduces_the_interpolated_colours():
    """Ambient 0, diffuse 1, gains 1, the normal against the light: s = 1 exactly, so the byte is floor(c + 0.5) of the perspective-correct
    interpolation - here affine, all Z equal - computed independently from float64 barycentric coordinates of the snapped triangle."""
    c, got = one_face()
    hit = got["mask"][0] > 0
    assert hit.sum() > 40
    sx, sy, _w, _ = R.project(c["poses"][0, 0], c["camera"][0], c["vertices"])
    ys, xs = np.nonzero(hit)
    px, py = 16.0 * xs + 8, 16.0 * ys + 8
    (x0, x1, x2), (y0, y1, y2) = sx.astype(float), sy.astype(float)
    det = (y1 - y2) * (x0 - x2) + (x2 - x1) * (y0 - y2)
    l0 = ((y1 - y2) * (px - x2) + (x2 - x1) * (py - y2)) / det
    l1 = ((y2 - y0) * (px - x2) + (x0 - x2) * (py - y2)) / det
    col = c["vertex_colours"].astype(np.float64)
    want = l0[:, None] * col[0] + l1[:, None] * col[1] + (1 - l0 - l1)[:, None] * col[2]
    g = got["frames"][0][hit].astype(np.float64)
    assert np.abs(g - want).max() <= 0.5 + 1e-9
    assert np.array_equal(got["frames"][0][~hit], c["frames"][0][~hit])


def test_zero_normal_gives_ambient_only_and_winding_does_not_matter():
    flat = ((100, 100, 100),) * 3
    _, got = one_face(colours=flat, normal=(0, 0, 0), light=S.light_row((0, 0, -1), 0.5, 0.9))
    assert set(np.unique(got["frames"][0][got["mask"][0] > 0])) == {50}
    light = S.light_row((0.3, 0.2, -1), 0.2, 0.7, (1.0, 0.9, 1.1))
    _, a = one_face(light=light, normal=(0.1, 0.2, -0.9))
    cols = ((200, 10, 30), (60, 70, 250), (20, 220, 40))                                       # vertices 1 and 2 swapped with their colours ...
    c2, b = one_face(light=light, normal=(-0.1, -0.2, 0.9), colours=cols)                      # ... and the normal the flipped winding gives
    c2["vertices"] = c2["vertices"][[0, 2, 1]]
    b = S.run(c2, min_pixels=1)
    assert np.array_equal(a["frames"], b["frames"]) and np.array_equal(a["mask"], b["mask"])
    # the index order alone: the same face listed as (0, 2, 1) with the same normal
    _, d = one_face(light=light, normal=(0.1, 0.2, -0.9), winding=(0, 2, 1))
    assert np.array_equal(a["frames"], d["frames"]) and np.array_equal(a["visible"], d["visible"])


def test_saturation_nan_and_alpha():
    _, sat = one_face(light=S.light_row((0, 0, -1), 0.5, 0.5, (1.0, 300.0, 1.0)))
    hit = sat["mask"][0] > 0
    assert (sat["frames"][0][hit][:, 1] == 255).all() and (sat["frames"][0][hit][:, 0] < 255).any()
    nan_light = S.light_row((0, 0, -1), 0.5, 0.5)
    nan_light[1] = np.nan
    _, nan = one_face(light=nan_light)
    assert not nan["frames"][0][hit].any()
    neg = S.light_row((0, 0, -1), 0.5, 0.5, (-1.0, 1.0, 1.0))
    _, n = one_face(light=neg)
    assert not n["frames"][0][hit][:, 0].any() and n["frames"][0][hit][:, 1].any()
    _, full = one_face(alpha=256)
    _, none = one_face(alpha=0)
    _, half = one_face(alpha=128)
    assert (none["frames"] == 77).all()
    assert np.array_equal(half["frames"][0][hit].astype(int), (128 * full["frames"][0][hit].astype(int) + 128 * 77 + 128) >> 8)


# ---- compaction ---------------------------------------------------------------------------------------------------------------
def test_compaction_drops_hidden_off_frame_invalid_and_small_slots():
    vertices, faces, face_start = R.concat([R.cube(), R.tetrahedron()])
    poses = np.zeros((1, 6, 16))
    poses[0, 0] = R.pose_row(0, 10, R.rotation((1, 2, 3), 0.7), (0.0, 0.0, 0.30))
    poses[0, 1] = R.pose_row(1, 20, None, (0.0, 0.0, 0.9))                                      # hidden behind slot 0
    poses[0, 2] = R.pose_row(0, 30, None, (-9.0, 0.0, 0.4))                                     # off frame
    poses[0, 3] = R.pose_row(5, 40, None, (0.05, 0.0, 0.3))                                     # label out of range: the row is skipped
    poses[0, 4] = R.pose_row(1, 50, R.rotation((0, 1, 0), 0.4), (-0.12, 0.05, 0.6))
    poses[0, 5] = R.pose_row(1, 60, None, (0, 0, 0.3), valid=0.0)
    rvec, tvec, extra = S.padded_inputs(1, 6)
    c = dict(poses=poses, camera=np.array([[90.0, 90.0, 36.0, 22.0, 1.0]]), vertices=vertices, vertex_colours=S.colours_for(len(vertices), 2), faces=faces,
             face_normals=S.face_normals(vertices, faces), face_start=face_start, lights=S.light_row()[None], H=44, W=72,
             frames=np.zeros((1, 44, 72, 3), np.uint8), rvec=rvec, tvec=tvec, extra=extra)
    got = S.run(c, min_pixels=1)
    counts = got["visible"][0, :, 4].tolist()
    assert counts[1] == counts[2] == counts[3] == counts[5] == 0 and counts[0] > 100 and counts[4] > 10
    ann = got["annotations"]
    assert ann["num_gt"].tolist() == [2] and ann["slot_of"][0].tolist() == [0, 4, -1, -1, -1, -1]
    assert ann["labels"][0].tolist() == [0, 1, 0, 0, 0, 0] and ann["mask_values"][0].tolist() == [10, 50, 0, 0, 0, 0]
    for k in ("rvec", "tvec", "extra"):
        assert np.array_equal(ann[k][0, :2], c[k][0, [0, 4]]) and not ann[k][0, 2:].any()
    assert ann["boxes"][0, 1].tolist() == got["visible"][0, 4, :4].tolist() and not ann["boxes"][0, 2:].any()
    # count == min_pixels keeps the slot, count == min_pixels - 1 drops it
    assert S.run(c, min_pixels=counts[4])["annotations"]["slot_of"][0].tolist()[:2] == [0, 4]
    low = S.run(c, min_pixels=counts[4] + 1)["annotations"]
    assert low["slot_of"][0].tolist() == [0, -1, -1, -1, -1, -1] and low["num_gt"].tolist() == [1] and not low["boxes"][0, 1:].any()
    assert S.run(c, annotations=False)["annotations"] is None


# ---- the host side -------------------------------------------------------------------------------------------------------------
def write_ply(path, v, f, colours, binary, colour_names=("red", "green", "blue")):
    head = ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if colours is not None:
        head += [f"property uchar {n}" for n in colour_names]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        for i, p in enumerate(v):
            c = [] if colours is None else [int(x) for x in colours[i]]
            fh.write(struct.pack("<3f", *p) + bytes(c) if binary else (" ".join([repr(float(x)) for x in p] + [str(x) for x in c]) + "\n").encode())
        for t in f:
            fh.write(struct.pack("<B3i", 3, *t) if binary else ("3 " + " ".join(str(int(x)) for x in t) + "\n").encode())


@pytest.mark.parametrize("binary", [False, True])
def test_coloured_ply_loader(tmp_path, binary):
    from hmd_ego_pose_amd import load_ply_coloured_mesh, load_ply_mesh
    v, f = R.cube()
    col = S.colours_for(len(v), 4)
    p = str(tmp_path / "c.ply")
    write_ply(p, v, f, col, binary)
    gv, gf, gc = load_ply_coloured_mesh(p)
    assert gc.dtype == np.uint8 and np.array_equal(gc, col) and np.array_equal(gv, v) and np.array_equal(gf, f)
    pv, pf = load_ply_mesh(p)                                        # the plain loader on the same file: the same mesh, as before
    assert np.array_equal(pv, v) and np.array_equal(pf, f) and pf.dtype == np.int32
    q = str(tmp_path / "plain.ply")
    write_ply(q, v, f, None, binary)
    assert np.array_equal(load_ply_mesh(q)[0], v)
    with pytest.raises(ValueError, match="plain.ply"):
        load_ply_coloured_mesh(q)
    r = str(tmp_path / "nogreen.ply")
    write_ply(r, v, f, col, binary, colour_names=("red", "diffuse_green", "blue"))
    with pytest.raises(ValueError, match="nogreen.ply.*green"):
        load_ply_coloured_mesh(r)


def test_shaded_mesh_set_normals_and_refusals():
    from hmd_ego_pose_amd.synth import ShadedMeshSet
    v, f = R.cube()
    tv = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [2, 0, 0]], np.float32)
    tf = np.array([[0, 1, 2], [0, 2, 1], [0, 1, 3]], np.int32)      # the third is degenerate: collinear
    m = ShadedMeshSet([(v, f, S.colours_for(8, 1)), (tv, tf, S.colours_for(4, 2))], device=torch.device("cpu"))
    n = m.host_face_normals
    assert n.dtype == np.float64 and n.shape == (15, 3) and m.face_normals.dtype == torch.float64 and m.vertex_colours.dtype == torch.uint8
    assert np.abs(np.sqrt((n[:14] ** 2).sum(1)) - 1).max() < 1e-15 and n[12].tolist() == [0, 0, 1] and n[13].tolist() == [0, 0, -1] and not n[14].any()
    assert np.array_equal(n, S.face_normals(m.host_vertices, m.host_faces))
    # the cube's normals are its axes, pointing out of or into it as the winding says
    assert all(sorted(np.abs(r).tolist()) == [0, 0, 1] for r in n[:12])
    assert np.array_equal(m.host_vertex_colours[8:], S.colours_for(4, 2)) and m.num_faces == 15
    with pytest.raises(ValueError):
        ShadedMeshSet([(v, f)], device=torch.device("cpu"))
    with pytest.raises(ValueError):
        ShadedMeshSet([(v, f, S.colours_for(7, 1))], device=torch.device("cpu"))
    with pytest.raises(ValueError):
        ShadedMeshSet([(v, f, S.colours_for(8, 1).astype(np.int32))], device=torch.device("cpu"))


class Counting:
    def __init__(self, seed):
        self.r, self.calls = random.Random(seed), 0

    def random(self):
        self.calls += 1
        return self.r.random()


def test_draw_poses_and_draw_lights():
    from hmd_ego_pose_amd import synth
    from hmd_ego_pose_amd.augment import pad_annotations
    B, K, H, W, margin = 5, 3, 120, 200, 0.1
    cam = np.array([300.0, 310.0, 101.5, 58.0])
    rng = Counting(17)
    ann = synth.draw_poses(rng, B, K, cam, H, W, (0.3, 0.9), labels=[0, 1, 0], margin=margin, symmetric=[0, 1, 0])
    assert rng.calls == 6 * B * K and len(ann) == B
    again = synth.draw_poses(random.Random(17), B, K, cam, H, W, (0.3, 0.9), labels=[0, 1, 0], margin=margin, symmetric=[0, 1, 0])
    for a, b in zip(ann, again):
        assert all(np.array_equal(a[k], b[k]) for k in a)
    for a in ann:
        assert not a["bboxes"].any() and a["bboxes"].shape == (K, 4) and a["labels"].tolist() == [0, 1, 0] and a["mask_values"].tolist() == [1, 2, 3]
        assert a["rotations"][:, 3].tolist() == [0, 1, 0] and a["rotations"][:, 4].tolist() == [0, 1, 0]
        for k in range(K):
            rv = a["rotations"][k, :3]
            th = np.linalg.norm(rv)
            Rm = R.rotation(rv, th)
            assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12 and 0 < th <= 2 * np.pi              # 2 atan2(|xyz|, w), w of either sign
            X, Y, Z = a["translations"][k]
            u, v = cam[0] * X / Z + cam[2], cam[1] * Y / Z + cam[3]
            assert margin * W - 1e-9 <= u <= (1 - margin) * W + 1e-9 and margin * H - 1e-9 <= v <= (1 - margin) * H + 1e-9 and 0.3 <= Z <= 0.9
    padded = pad_annotations(ann, "cpu")                             # the dicts are what pad_annotations takes
    assert padded["num_gt"].tolist() == [K] * B and tuple(padded["rvec"].shape) == (B, K, 3)
    # the first object's draws, restated: Shoemake's quaternion, the centre, the distance
    r = random.Random(17)
    u1, u2, u3, a, c, d = (r.random() for _ in range(6))
    q = np.array([np.sqrt(1 - u1) * np.sin(2 * np.pi * u2), np.sqrt(1 - u1) * np.cos(2 * np.pi * u2), np.sqrt(u1) * np.sin(2 * np.pi * u3), np.sqrt(u1) * np.cos(2 * np.pi * u3)])
    x, y, z, w = q
    Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    rv = ann[0]["rotations"][0, :3]
    assert np.abs(R.rotation(rv, np.linalg.norm(rv)) - Rq).max() < 1e-12
    Z = 0.3 + d * 0.6
    assert np.allclose(ann[0]["translations"][0], [(W * (0.1 + a * 0.8) - cam[2]) * Z / cam[0], (H * (0.1 + c * 0.8) - cam[3]) * Z / cam[1], Z], rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        synth.draw_poses(random.Random(1), 1, 17, cam, H, W, (0.3, 0.9), labels=[0] * 17)
    with pytest.raises(ValueError):
        synth.draw_poses(random.Random(1), 1, 2, cam, H, W, (0.3, 0.9), labels=[0])
    rng = Counting(3)
    L = synth.draw_lights(rng, 40)
    assert rng.calls == 7 * 40 and L.dtype == np.float64 and L.shape == (40, 8)
    assert np.abs(np.sqrt((L[:, :3] ** 2).sum(1)) - 1).max() <= 2 ** -52
    assert (L[:, 3] >= 0.3).all() and (L[:, 3] <= 0.6).all() and (L[:, 4] >= 0.4).all() and (L[:, 4] <= 0.8).all() and (L[:, 5:] >= 0.9).all() and (L[:, 5:] <= 1.1).all()
    assert np.array_equal(L, synth.draw_lights(random.Random(3), 40))


def test_synth_frames_refuses_wrong_arguments_before_the_library_is_touched(monkeypatch):
    from hmd_ego_pose_amd import _capi, synth
    from hmd_ego_pose_amd.augment import pad_annotations
    from hmd_ego_pose_amd.render import MeshSet

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_capi, "lib", touched)
    cpu = torch.device("cpu")
    v, f = R.cube()
    mesh = synth.ShadedMeshSet([(v, f, S.colours_for(8, 1))], device=cpu)
    B, H, W = 2, 32, 48
    ann = pad_annotations(synth.draw_poses(random.Random(2), B, 2, [60.0, 60.0, 24.0, 16.0], H, W, (0.3, 0.5), labels=[0, 0]), cpu)
    good = dict(backgrounds_u8=torch.zeros((B, H, W, 3), dtype=torch.uint8), annotations=ann, camera=torch.tensor([[60.0, 60.0, 24.0, 16.0, 1.0]] * B, dtype=torch.float64),
                meshes=mesh, lights=synth.draw_lights(random.Random(1), B))
    bad = [dict(backgrounds_u8=good["backgrounds_u8"].float()), dict(backgrounds_u8=good["backgrounds_u8"][:, :, :, :2]), dict(backgrounds_u8=good["backgrounds_u8"][:, :, ::2]),
           dict(backgrounds_u8=torch.zeros((B, 8, W, 3), dtype=torch.uint8)), dict(backgrounds_u8=good["backgrounds_u8"].numpy()),
           dict(camera=good["camera"].float()), dict(camera=good["camera"][:, :4]), dict(camera=good["camera"].numpy()),
           dict(meshes=MeshSet([(v, f)], device=cpu)), dict(lights=good["lights"].astype(np.float32)), dict(lights=good["lights"][:1]),
           dict(lights=torch.from_numpy(good["lights"]).float()), dict(alpha=257), dict(alpha=-1), dict(min_pixels=0),
           dict(annotations={k: t for k, t in ann.items() if k != "extra"}), dict(annotations=dict(ann, labels=ann["labels"].long())),
           dict(annotations=dict(ann, tvec=ann["tvec"][:, :1])), dict(annotations=dict(ann, num_gt=ann["num_gt"][:1])), dict(annotations=[{}])]
    for over in bad:
        with pytest.raises(ValueError):
            synth.synth_frames(**dict(good, **over))
    with pytest.raises(AssertionError, match="touched"):              # ... and the good arguments get as far as the library
        synth.synth_frames(**good)
