"""The shape-specialised BiFPN kernels (csrc/k_sep_impl.h SEP_SHAPES: sep_shape_kernel<true, D>, the single nodes; csrc/k_chain_impl.h
chain_shape(): chain_shape_kernel<true, D>, the LDS-resident chains; the node's / the chain's dimensions as compile-time constants)
against the generic kernels (sep_kernel, chain_kernel: every shape from the arguments; HEP_NECK_GENERIC=1 forces them).

Only where the index arithmetic gets its numbers from differs between the two, so the results must be IDENTICAL, not close: every
BiFPN stage tensor and every head output, bit for bit.  A row is selected only when every folded field of a launch equals it; the
rows describe phi 0 @ 256 in bf16 and do not depend on the batch, so batch 1 and batch 3 (a frame at a non-zero batch position)
run all six rows, as the benchmarked batch 16 does.  fp32 sessions, other widths and other map sizes keep the generic kernels
(tests/test_gpu_parity.py pins chain_kernel<false, ...> by name).

The fallback is pinned by phi 1 @ 256 (BiFPN width 88: no row) and by phi 0 @ 128.  At 128 x 128 the pyramid is 16 .. 1 pixels: the
chains and their external maps have other sizes and run chain_kernel, and the one single node per cell, conv3_up, is a 16x16 node
fused from a 16x16 and an 8x8 map - field for field the shape of row 1 (conv4_up at 256 x 256), so it runs that row; it is held to
the generic kernel bit for bit like the others, and the session to the gate test_gpu_parity.py test_other_input_sizes has."""
import ctypes
import re

import pytest
import torch

from hmd_ego_pose_amd import pack_bytes
from hmd_ego_pose_amd.planning import plan_launch_list
from tests._util import seeded_input, seeded_state_dict_once

gpu = pytest.mark.gpu          # (the launch-list cases plan on the host and run without a GPU)

HEADS = ("regression", "classification", "rotation", "translation_raw", "hand")
NODE = "sep_shape_kernel<true, %d>"
CHAIN = "chain_shape_kernel<true, %d>"
GENERIC = {"sep_kernel<true, 0, false, true>", "chain_kernel<true, 0>"}
# the thirteen neck launches of phi 0 @ 256 (nine single nodes, four chains) and the row that runs each
ROWS = {f"c{r}.{conv}": NODE % d for r in range(3) for conv, d in (("conv4_up", 1), ("conv3_up", 2), ("conv4_down", 3))}
ROWS.update({
    "c0.conv6_up+conv5_up": CHAIN % 1,
    "c0.conv5_down+conv6_down+conv7_down+conv6_up+conv5_up": CHAIN % 2,
    "c1.conv5_down+conv6_down+conv7_down+conv6_up+conv5_up": CHAIN % 2,
    "c2.conv5_down+conv6_down+conv7_down": CHAIN % 3,
})
# every map the neck writes: the five outputs and the three top-down maps of every cell, and cell 0's two pooled inputs
STAGES = [f"c{r}.p{l}_out" for r in range(3) for l in range(3, 8)] + [f"c{r}.p{l}_up" for r in range(3) for l in (4, 5, 6)] + ["c0.p6_in", "c0.p7_in"]


@pytest.fixture(scope="module")
def api():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd.model import Session
    from oracle import efficientpose_ref
    assert torch.cuda.is_available(), "these tests need the MI355X box"
    return dict(capi=_capi, Session=Session, R=efficientpose_ref)


def _same_bits(a, b):
    """bit for bit, NaNs included"""
    assert a.dtype == b.dtype and a.shape == b.shape and a.element_size() in (2, 4)
    as_int = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def _neck(launches):
    """{launch name: device function} of the BiFPN node and chain launches in a list of (name, device function)"""
    return {n: y for n, y in launches if re.match(r"c\d+\.conv", n)}


def _planned(phi, size, batch, precision, env=None, seed=0):
    return _neck([(n, y) for y, n in plan_launch_list(pack_bytes(seeded_state_dict_once(phi, seed)), phi, size, batch, precision, env=env)])


def _stage_names(capi, s):
    l, names = capi.lib(), []
    for i in range(l.hep_debug_tensor_count(s.handle)):
        nm = ctypes.c_char_p(); dims = (ctypes.c_int64 * 4)()
        l.hep_debug_tensor_info(s.handle, i, ctypes.byref(nm), dims)
        names.append(nm.value.decode())
    return names


def _run(api, sd, phi, size, batch, x, stages):
    """(neck launches of the session, head outputs, {stage name: tensor}) of one bf16 forward"""
    capi = api["capi"]
    s = api["Session"](sd, phi, size, batch, "bf16", flags=capi.FLAG_KEEP_INTERMEDIATES)
    neck = _neck([(n, y) for n, _b, _f, y in s.kernels(batch)])
    heads = [t.clone() for t in s.forward(x)[1:]]
    torch.cuda.synchronize()
    have = _stage_names(capi, s)
    assert all(n in have for n in stages), sorted(set(stages) - set(have))
    kept = {n: s.stage(n, batch) for n in stages}
    s.close()
    return neck, heads, kept


def _assert_identical(tag, hs, hg, ss, sg):
    for name, a, b in zip(HEADS, hs, hg):
        assert _same_bits(a, b), f"{tag} {name}: max |diff| {(a.float() - b.float()).abs().max().item():.3e}"
    assert sorted(ss) == sorted(sg)
    for n in ss:
        assert _same_bits(ss[n], sg[n]), f"{tag} stage {n}: max |diff| {(ss[n].float() - sg[n].float()).abs().max().item():.3e}"


@gpu
@pytest.mark.parametrize("batch", [1, 3])
def test_specialised_neck_equals_the_generic_kernels_bit_for_bit(api, batch, monkeypatch):
    """phi 0 @ 256 in bf16 as planned and with HEP_NECK_GENERIC=1 (read when the session is created): the first names only rows for
    the nine node and four chain launches, the second only sep_kernel<true, 0, false, true> and chain_kernel<true, 0>; all five heads
    and every BiFPN stage tensor are bit-equal."""
    phi, size = 0, 256
    sd = seeded_state_dict_once(phi, 0)
    x = torch.from_numpy(seeded_input((batch, 3, size, size), 41)).cuda()
    ns, hs, ss = _run(api, sd, phi, size, batch, x, STAGES)
    monkeypatch.setenv("HEP_NECK_GENERIC", "1")
    ng, hg, sg = _run(api, sd, phi, size, batch, x, STAGES)
    assert ns == ROWS, ns
    assert sorted(ng) == sorted(ROWS) and set(ng.values()) == GENERIC, ng
    assert sum(y.startswith("sep_kernel<") for y in ng.values()) == 9 and sum(y.startswith("chain_kernel<") for y in ng.values()) == 4, ng
    assert len(ss) == 26
    _assert_identical(f"b{batch}", hs, hg, ss, sg)


@pytest.mark.parametrize("batch", [1, 3, 16])
def test_every_neck_launch_runs_its_row_at_every_batch_and_no_row_is_dead(batch):
    """The launch list of phi 0 @ 256 bf16 (planned on the host): each of the thirteen neck launches names the row listed for it, every
    row is reached, HEP_NECK_GENERIC=1 reaches none, and an fp32 session names no shape kernel."""
    neck = _planned(0, 256, batch, "bf16")
    assert neck == ROWS, neck
    assert set(neck.values()) == {NODE % d for d in (1, 2, 3)} | {CHAIN % d for d in (1, 2, 3)}
    generic = _planned(0, 256, batch, "bf16", env={"HEP_NECK_GENERIC": "1"})
    assert sorted(generic) == sorted(ROWS) and set(generic.values()) == GENERIC, generic
    f32 = _planned(0, 256, batch, "fp32")
    assert sorted(f32) == sorted(ROWS) and not any("_shape_kernel" in y for y in f32.values()), f32
    assert all(y.startswith(("sep_kernel<false, ", "chain_kernel<false, ")) for y in f32.values()), f32


@gpu
def test_other_map_sizes_fall_back_phi0_at_128(api, monkeypatch):
    """phi 0 @ 128 (bf16, batch 1): no chain and no three-source node matches a row - they run the generic kernels; conv3_up has row 1's
    shape field for field and runs it (module docstring).  Finite and within the gate of test_gpu_parity.py test_other_input_sizes
    (0.15 of the oracle's range end to end), and bit-equal to the all-generic plan."""
    R = api["R"]
    phi, size, batch = 0, 128, 1
    sd = seeded_state_dict_once(phi, 2)
    neck = _planned(phi, size, batch, "bf16", seed=2)
    assert len(neck) == 7, neck
    rows = {n: y for n, y in neck.items() if "_shape_kernel" in y}
    assert rows == {f"c{r}.conv3_up": NODE % 1 for r in range(3)}, neck
    assert all(y == "chain_kernel<true, 0>" for n, y in neck.items() if n not in rows), neck
    x = torch.from_numpy(seeded_input((batch, 3, size, size), 9))
    ref = R.forward(sd, x, phi)
    stages = [f"c{r}.p{l}_out" for r in range(3) for l in range(3, 8)]
    ns, hs, ss = _run(api, sd, phi, size, batch, x.cuda(), stages)
    assert ns == neck
    for name, a, b in zip(HEADS, hs, ref[1:]):
        assert torch.isfinite(a).all(), name
        err = (a.float().cpu() - b).abs().max().item()
        print(f"phi 0 @ 128 b1 bf16 {name}: max |hip - oracle| = {err:.3e} (bound {0.15 * max(1.0, b.abs().max().item()):.3e})")
        assert err <= 0.15 * max(1.0, b.abs().max().item()), (name, err)
    monkeypatch.setenv("HEP_NECK_GENERIC", "1")
    ng, hg, sg = _run(api, sd, phi, size, batch, x.cuda(), stages)
    assert not any("_shape_kernel" in y for y in ng.values()), ng
    _assert_identical("phi 0 @ 128", hs, hg, ss, sg)


def test_other_widths_name_no_shape_kernel_phi1_at_256():
    """phi 1 @ 256 in bf16 (planned on the host): BiFPN width 88 - no neck launch names a shape kernel."""
    neck = _planned(1, 256, 1, "bf16", seed=2)
    assert len(neck) >= 13 and not any("_shape_kernel" in y for y in neck.values()), neck
