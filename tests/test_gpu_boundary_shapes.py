"""The shape-specialised block boundaries (csrc/k_xbf_impl.h XBF_SHAPES: xbf_kernel_shape<true, D>, the whole layer shape - map
and output size, pads, tile counts, channel chunking, LDS offsets, squeeze-excite widths, residual - as compile-time constants)
against xbf_kernel, which takes all of that from XbfArgs: HEP_XBF_GENERIC=2 runs the width-specialised instantiation the rows
replaced (K1 and NT2 folded, nothing else), HEP_XBF_GENERIC=1 the generic one (no width folded either).

The three kernels share one text (csrc/k_xbf_body.h) and differ only in where the index arithmetic gets its numbers from, so the
results must be IDENTICAL, not close: every stage tensor and every head output, bit for bit.  A row is selected only when every
folded field of a launch equals it (xbf_shape_id); the sessions are phi 0 @ 256 in bf16 - the only sessions whose boundaries the
table describes (phi 1 @ 256 repeats them).  What depends on the batch stays an argument of the rows, so the batches are chosen
by the paths they take: 1 (a single image), 3 (an odd count, images at non-zero batch positions), 9 (the smallest batch at which
the planner gives b0.project+b1.front two tiles per workgroup: 64 tiles x 9 > 512 workgroups) and 2 under HEP_XBF_TPW=2 (all
three boundaries run a second tile in the same workgroup).  fp32 boundaries and the other map sizes have no rows."""
import pytest
import torch

from hmd_ego_pose_amd import _capi, pack_bytes
from hmd_ego_pose_amd.planning import plan_launch_list
from tests._util import seeded_input, seeded_state_dict_once
from tests.test_gpu_front_shapes import HEADS, _same_bits, _stage_names

gpu = pytest.mark.gpu          # (the launch-list cases plan on the host and run without a GPU)

# the rows of XBF_SHAPES as hep_plan_launch_list / hep_kernel_symbol name them, by the launch of phi 0 @ 256 that runs them, and the
# device functions those launches ran before the table existed (HEP_XBF_GENERIC=2) / run without any folded width (=1)
ROWS = {
    "b0.project+b1.front": "xbf_kernel_shape<true, 1>",
    "b1.project+b2.front": "xbf_kernel_shape<true, 2>",
    "b2.project+b3.front": "xbf_kernel_shape<true, 3>",
}
WIDTHS = {
    "b0.project+b1.front": "xbf_kernel<true, 3, 2, 8, 8, 1, 32, 6>",
    "b1.project+b2.front": "xbf_kernel<true, 3, 1, 8, 16, 2, 96, 9>",
    "b2.project+b3.front": "xbf_kernel<true, 5, 2, 8, 8, 2, 144, 9>",
}
GENERIC = {
    "b0.project+b1.front": "xbf_kernel<true, 3, 2, 8, 8, 1, 0, 0>",
    "b1.project+b2.front": "xbf_kernel<true, 3, 1, 8, 16, 2, 0, 0>",
    "b2.project+b3.front": "xbf_kernel<true, 5, 2, 8, 8, 2, 0, 0>",
}


def _boundaries(launches):
    """{launch name: device function} of the boundary launches in a list of (name, device function)"""
    return {n: y for n, y in launches if "xbf_kernel" in y}


def _planned(phi, size, batch, precision, env=None, flags=0):
    return _boundaries([(n, y) for y, n in plan_launch_list(pack_bytes(seeded_state_dict_once(phi, 0)), phi, size, batch, precision, flags, env=env)])


@pytest.mark.parametrize("batch", [1, 3, 16])
def test_every_boundary_of_phi0_at_256_runs_its_row_and_no_row_is_dead(batch):
    """phi 0 @ 256 bf16, planned on the host: each of the three boundary launches names its row and every row is reached, at every
    batch (nothing a row folds depends on the batch); HEP_XBF_GENERIC=1 names the generic instantiations, =2 the three device
    functions the launches had before the table; FLAG_KEEP_INTERMEDIATES (mid is stored: an argument) changes nothing."""
    assert _planned(0, 256, batch, "bf16") == ROWS
    assert set(_planned(0, 256, batch, "bf16").values()) == set(ROWS.values())
    generic = _planned(0, 256, batch, "bf16", env={"HEP_XBF_GENERIC": "1"})
    assert generic == GENERIC and all(y.endswith(", 0, 0>") for y in generic.values()), generic
    assert _planned(0, 256, batch, "bf16", env={"HEP_XBF_GENERIC": "2"}) == WIDTHS
    pack = pack_bytes(seeded_state_dict_once(0, 0))
    assert plan_launch_list(pack, 0, 256, batch, "bf16", _capi.FLAG_KEEP_INTERMEDIATES) == plan_launch_list(pack, 0, 256, batch, "bf16")
    assert _planned(0, 256, batch, "bf16", flags=_capi.FLAG_KEEP_INTERMEDIATES) == ROWS
    # tiles per workgroup is an argument of the rows too
    assert _planned(0, 256, batch, "bf16", env={"HEP_XBF_TPW": "2"}) == ROWS


def test_sessions_the_table_does_not_describe_name_no_row():
    """fp32 at the rows' shapes, phi 0 on other map sizes (@ 128, @ 384) and phi 3 @ 256 (other widths) name no row - xbf_shape_id
    compares every folded field; phi 1 @ 256 (B0's widths and map sizes, more blocks per stage) names only rows or xbf_kernel."""
    f32 = _planned(0, 256, 16, "fp32")
    assert f32 and all(y.startswith("xbf_kernel<false, ") for y in f32.values()), f32
    for phi, size in ((0, 128), (0, 384), (3, 256)):
        for batch in (1, 16):
            got = _planned(phi, size, batch, "bf16")
            assert got and all(y.startswith("xbf_kernel<true, ") for y in got.values()), (phi, size, batch, got)
    # (phi 0 @ 384 runs the rows' widths on 192 x 192 / 96 x 96 maps: the device functions the rows replaced at 256)
    assert _planned(0, 384, 16, "bf16") == WIDTHS
    phi1 = _planned(1, 256, 3, "bf16")
    assert phi1 and all(y in ROWS.values() or y.startswith("xbf_kernel<true, ") for y in phi1.values()), phi1


@pytest.fixture(scope="module")
def api():
    from hmd_ego_pose_amd.model import Session
    assert torch.cuda.is_available(), "these tests need the MI355X box"
    return dict(capi=_capi, Session=Session)


def _run(api, sd, batch, x):
    """(boundary launches, head outputs, {stage name: tensor}) of one forward of phi 0 @ 256 bf16 under the knobs of the environment"""
    capi = api["capi"]
    s = api["Session"](sd, 0, 256, batch, "bf16", flags=capi.FLAG_KEEP_INTERMEDIATES)
    bounds = _boundaries([(n, y) for n, _b, _f, y in s.kernels(batch)])
    heads = [t.clone() for t in s.forward(x)[1:]]
    torch.cuda.synchronize()
    kept = {n: s.stage(n, batch) for n in _stage_names(capi, s)}
    s.close()
    return bounds, heads, kept


@gpu
@pytest.mark.parametrize("batch,tpw", [(1, None), (3, None), (9, None), (2, "2")])
def test_shape_rows_equal_the_kernels_they_replace_bit_for_bit(api, batch, tpw, monkeypatch):
    """phi 0 @ 256 bf16 as planned (the rows), with HEP_XBF_GENERIC=2 (the width-specialised xbf_kernel of each boundary) and with
    HEP_XBF_GENERIC=1 (the generic xbf_kernel): the launch lists say so, and all five heads and every stage tensor - block outputs,
    depthwise outputs, squeeze-excite partial rows - are bit-equal, NaNs included."""
    sd = seeded_state_dict_once(0, 0)
    x = torch.from_numpy(seeded_input((batch, 3, 256, 256), 43)).cuda()
    if tpw is not None:
        monkeypatch.setenv("HEP_XBF_TPW", tpw)
    br, hr, sr = _run(api, sd, batch, x)
    assert br == ROWS, br
    assert len(sr) >= 28, sorted(sr)
    for knob, names in (("2", WIDTHS), ("1", GENERIC)):
        monkeypatch.setenv("HEP_XBF_GENERIC", knob)
        bg, hg, sg = _run(api, sd, batch, x)
        assert bg == names, (knob, bg)
        assert sorted(sg) == sorted(sr)
        for name, a, b in zip(HEADS, hr, hg):
            assert _same_bits(a, b), f"b{batch} HEP_XBF_GENERIC={knob} {name}: max |diff| {(a.float() - b.float()).abs().max().item():.3e}"
        for n in sr:
            assert _same_bits(sr[n], sg[n]), f"b{batch} HEP_XBF_GENERIC={knob} stage {n}: max |diff| {(sr[n].float() - sg[n].float()).abs().max().item():.3e}"
