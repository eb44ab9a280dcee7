"""GPU (MI355X): the colour augmentation hep_colour_augment_device (csrc/k_colour.hip) behind hmd_ego_pose_amd.augment.colour_augment,
against the numpy oracle tests/_colour.py (the definition; tests/test_colour_cpu.py pins it against PIL and by hand).

Every case runs twice through the ABI into an output and a workspace pre-filled with 0xFF; the two runs must match bit for bit, and
every operation but the noise must equal the oracle byte for byte.  The noise (id 13) is evaluated in float32 on the device and in
float64 by the oracle: an element whose sigma * z lies within 1e-3 of a half-integer may differ by one, every other element must be
identical (|sigma z| <= 35.7 * 6 = 215, where float32 is spaced 1.5e-5; the argument 2 pi u carries about 4e-7 of absolute error, about
1e-4 after scaling: the band is some five times that).  Measured shares of differing elements: NOTEBOOK section 22."""
import numpy as np
import pytest
import torch

from tests import _augment as A
from tests import _colour as C

pytestmark = pytest.mark.gpu


def _run(frames, ops, args):
    """Two runs through the ABI; output and workspace start as 0xFF."""
    from hmd_ego_pose_amd import _capi, augment
    B, H, W = frames.shape[:3]
    l = _capi.lib()
    d_frames, d_ops, d_args = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (frames, ops, args))
    need = _capi.check(l.hep_colour_workspace_bytes(B, H, W))
    runs = []
    for _ in range(2):
        out = torch.full((B, H, W, 3), 0xFF, dtype=torch.uint8, device="cuda")
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        augment._run_colour(l, d_frames, d_ops, d_args, B, H, W, out, ws, d_frames.device)
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
    assert np.array_equal(d_frames.cpu().numpy(), frames)                  # the input is not written
    return runs


def _exact(frames, rows, what):
    ops, args = C.table(rows, frames.shape[0])
    got, again = _run(frames, ops, args)
    ref = C.colour_augment(frames, ops, args)
    bad = got != ref
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), ref[bad][:4].tolist())
    assert np.array_equal(got, again), (what, "two runs differ")
    return got


def _slot(op, m, H, W, sign=1, centre=(0.5, 0.5), seed=0):
    from hmd_ego_pose_amd.augment import colour_parameters
    i0, i1, i2, i3, seed, f = colour_parameters(op, m, H, W, sign, centre, seed)
    return (op, dict(i=(i0, i1, i2, i3), seed=seed, f=f))


@pytest.mark.parametrize("op", range(13))
def test_every_operation_alone(op):
    """B = 2, 37 x 50: a row is 150 bytes (no multiple of 4) and the width no multiple of a lane's four pixels."""
    frames = C.random_frames((2, 37, 50), 10 + op)
    frames[1] = frames[1] // 2 + 30                                         # a lower range: the tables of ids 1 and 2 are not the identity
    for m in (1, 14):
        for sign in ((1, -1) if 6 <= op <= 9 else (1,)):
            rows = [[_slot(op, m, 37, 50, sign, (0.3, 0.6))], [_slot(op, 15 - m, 37, 50, -sign, (0.8, 0.1))]]
            got = _exact(frames, rows, (C.NAMES[op], m, sign))
            assert op == 0 or not np.array_equal(got, frames)


CHAINS = {
    "equalize-contrast-autocontrast": [(2, {}), (7, dict(f=0.58)), (1, {})],
    "blur-sharpness-smooth": [(11, {}), (9, dict(f=1.9)), (12, {})],
    "autocontrast-solarize-equalize": [(1, {}), (5, dict(i=(137, 0, 0, 0))), (2, {})],
    "contrast-contrast-equalize": [(7, dict(f=0.58)), (7, dict(f=1.03)), (2, {})],
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_chains_through_the_fused_statistics(name):
    """B = 1, 130 x 70: 2340 quads, three workgroups per image - the counters are summed across workgroups."""
    frames = (C.random_frames((1, 130, 70), 30) // 2 + 40).astype(np.uint8)
    got = _exact(frames, [CHAINS[name]], name)
    step = frames[0]
    for k, (op, kw) in enumerate(CHAINS[name]):                             # every link changes the image: none of the tables is the identity
        ops, args = C.table([[(op, kw)]])
        nxt = C.apply_slot(step, ops[0, 0], args[0, 0], 0, k)
        assert not np.array_equal(nxt, step), (name, k)
        step = nxt
    assert np.array_equal(step, got[0])


MIXED = [[(2, {})],
         [(7, dict(f=0.58)), (1, {})],
         [(10, dict(i=(40, 0, 48, 9))), (2, {}), (6, dict(f=1.9))],
         [],
         [],                                                               # what draw_colour leaves for an apply = 0 image
         ]


def _mixed_frames():
    return (C.random_frames((5, 32, 48), 40) // 3 + 20).astype(np.uint8)


def test_mixed_batch():
    """B = 5, 32 x 48: 1, 2, 3 and 0 operations, an apply = 0 row, another id per image in the same slot."""
    from hmd_ego_pose_amd.augment import draw_colour
    import random
    assert (draw_colour(random.Random(1), 5, apply=[1, 1, 1, 1, 0], height=32, width=48)[0][4, :, 0] == -1).all()
    frames = _mixed_frames()
    got = _exact(frames, MIXED, "mixed")
    assert np.array_equal(got[3], frames[3]) and np.array_equal(got[4], frames[4])
    assert all(not np.array_equal(got[b], frames[b]) for b in range(3))


def test_edges():
    s0, s1 = C.step0_image(), C.step1_image()
    assert np.array_equal(C.equalize(s0), s0) and not np.array_equal(C.equalize(s1), s1)
    small = np.stack([s0, s1, s0, s1])
    # 16 x 16, the minimum: equalize with step 0 and step 1, a constant channel under autocontrast; the 5 x 5 filter's interior is 12 x 12
    _exact(small, [[(2, {})], [(2, {})], [(1, {}), (11, {})], [(11, {}), (2, {}), (1, {})]], "16 x 16")
    frames = C.random_frames((2, 37, 50), 50)
    frames[0, :, :, 2] = 9                                                  # a constant channel
    _exact(frames, [[(1, {}), (2, {})], [(2, {}), (1, {})]], "constant channel")
    corner = _slot(10, 14, 37, 50, centre=(0.0, 0.0))
    far = _slot(10, 14, 37, 50, centre=(0.999, 0.999))
    assert corner[1]["i"][:2] == (0, 0) and far[1]["i"][2:] == (50, 37)
    _exact(frames, [[corner], [far]], "Cutout clipped at two borders")
    _exact(frames, [[(10, dict(i=(7, 5, 7, 5)))], [(10, dict(i=(50, 37, 50, 37)))]], "Cutout of side 0")
    got = _exact(frames, [[(5, dict(i=(256, 0, 0, 0)))], [(5, dict(i=(0, 0, 0, 0)))]], "Solarize at 256 and 0")
    assert np.array_equal(got[0], frames[0]) and np.array_equal(got[1], 255 - frames[1])
    got = _exact(frames, [[(4, dict(i=(8, 0, 0, 0)))], [(4, dict(i=(2, 0, 0, 0)))]], "Posterize at 8 and 2 bits")
    assert np.array_equal(got[0], frames[0])
    # what the device cannot refuse runs as Identity, as the oracle says
    got = _exact(frames, [[(14, {}), (3, {})], [(6, dict(f=2.5)), (4, dict(i=(1, 0, 0, 0))), (10, dict(i=(0, 0, 51, 37)))]], "slots the device does not accept")
    assert np.array_equal(got[0], 255 - frames[0]) and np.array_equal(got[1], frames[1])


@pytest.mark.parametrize("sigma", [2.55, 35.7])
def test_noise(sigma):
    """Image 0: the noise in slot 0; image 1: in slot 1, behind Invert - the counter carries the image index and the slot."""
    frames = C.random_frames((2, 37, 50), 60)
    seeds = (0x5EED0000 + int(sigma * 100), 0xFEDCBA9876543210)
    rows = [[(13, dict(f=sigma, seed=seeds[0]))], [(3, {}), (13, dict(f=sigma, seed=seeds[1]))]]
    ops, args = C.table(rows)
    got, again = _run(frames, ops, args)
    assert np.array_equal(got, again)
    ref = C.colour_augment(frames, ops, args)
    near = np.stack([C.near_boundary(frames[0].shape, 0, 0, seeds[0], sigma), C.near_boundary(frames[1].shape, 1, 1, seeds[1], sigma)])
    diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    print(f"sigma {sigma}: {(diff != 0).mean():.4%} of the elements differ from the float64 oracle, {near.mean():.4%} lie within 1e-3 of a rounding boundary, "
          f"largest difference {diff.max()}")
    assert near.mean() <= 0.01
    assert not diff[~near].any(), (int((diff[~near] != 0).sum()), np.argwhere((diff != 0) & ~near)[:4].tolist())
    assert diff[near].max(initial=0) <= 1
    assert not np.array_equal(got[0], frames[0]) and (got != ref).mean() < 0.01


def test_public_call_equals_the_abi_path():
    from hmd_ego_pose_amd.augment import colour_augment
    frames = _mixed_frames()
    ops, args = C.table(MIXED)
    ref = _run(frames, ops, args)[0]
    d = torch.from_numpy(frames).cuda()
    out = colour_augment(d, ops, args)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == frames.shape and np.array_equal(out.cpu().numpy(), ref)
    mine = torch.full_like(d, 0xFF)
    assert colour_augment(d, torch.from_numpy(ops), torch.from_numpy(args), out=mine) is mine
    torch.cuda.synchronize()
    assert np.array_equal(mine.cpu().numpy(), ref)
    bad_id, gap, bad_f = (ops.copy(), args.copy()), (ops.copy(), args.copy()), (ops.copy(), args.copy())
    bad_id[0][0, 0, 0] = 14
    gap[0][3, 1, 0] = 3
    bad_f[1][1, 0, 0] = 2.0
    for o, a in (bad_id, gap, bad_f):
        with pytest.raises(ValueError):
            colour_augment(d, o, a)
    with pytest.raises(ValueError):
        colour_augment(d.to(torch.float32), ops, args)                      # a wrong dtype
    with pytest.raises(ValueError):
        colour_augment(torch.from_numpy(frames), ops, args)                 # a CPU tensor
    with pytest.raises(ValueError):
        colour_augment(d, ops, args, out=d)


def test_composes_with_augment_6dof():
    """colour_augment -> augment_6dof on case A of tests/_augment.py equals the numpy chain of the two oracles bit for bit on image."""
    from hmd_ego_pose_amd.augment import augment_6dof, colour_augment
    c = A.make_case("A")
    size = c.pop("size")
    angles = c.pop("angles_deg")
    H, W = c["frames"].shape[1:3]
    rows = [[(2, {}), (9, dict(f=1.42))], [(5, dict(i=(171, 0, 0, 0)))], [(11, {}), (7, dict(f=0.58)), (4, dict(i=(6, 0, 0, 0)))], [_slot(10, 14, H, W)]]
    ops, args = C.table(rows)
    coloured = C.colour_augment(c["frames"], ops, args)
    assert all(not np.array_equal(coloured[b], c["frames"][b]) for b in range(4))
    ref = A.augment_6dof(size=size, **dict(c, frames=coloured))
    annotations = []
    for b in range(4):
        n = int(c["num_gt"][b])
        annotations.append({"bboxes": c["boxes"][b, :n], "labels": c["labels"][b, :n], "mask_values": c["mask_values"][b, :n],
                            "rotations": np.concatenate([c["rvec"][b, :n], c["extra"][b, :n]], axis=1), "translations": c["tvec"][b, :n]})
    d_frames = colour_augment(torch.from_numpy(c["frames"]).cuda(), ops, args)
    out = augment_6dof(d_frames, torch.from_numpy(c["masks"]).cuda(), annotations, c["camera_k"], angles, c["xform"][:, 7], c["xform"][:, 8], size)
    torch.cuda.synchronize()
    assert np.array_equal(d_frames.cpu().numpy(), coloured)
    got = out["image"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref["image"].view(np.uint32))
    assert np.array_equal(out["applied"].cpu().numpy(), ref["applied"])
