"""The shape-specialised fused fronts (csrc/k_mbf_impl.h MBF_SHAPES: mbf_shape_kernel<..., D>, the layer's dimensions and flags as
compile-time constants) against the generic kernel (mbf_kernel, every shape from MbfArgs; HEP_MBF_GENERIC=1 forces it).

Only where the index arithmetic gets its numbers from differs between the two, so the results must be IDENTICAL, not close:
every stage tensor and every head output, bit for bit.  A row of the table is selected only when every folded field of a
launch equals it; the sessions below are phi 0 @ 256 in bf16 - the only sessions whose fronts the table describes - at batch 1
and 3 (a frame at a non-zero batch position; out_frag of blocks 4 and 11-15 depends on the batch, so batch 1 reaches 6 of the
8 rows, batch 3 all but row 1) and at the benchmarked batch 16 (all 8 rows, row 1 only there).  fp32 fronts are not specialised
(tests/test_gpu_parity.py test_default_fp32_plan_uses_multi_pass_fronts pins their device functions by name).

The fallback is pinned by the sessions whose shapes are NOT in the table: phi 0 @ 128 (other map sizes: no row matches) and
phi 1 @ 256.  EfficientNet-B1 has B0's widths and only more blocks per stage, so at 256 x 256 its fronts repeat phi 0's shapes
and run the same rows; the one width phi 0 does not have - block 22, 320 -> 1920 channels - runs the generic kernel.  Both are
held to the parity gates those configurations already have in tests/test_gpu_parity.py."""
import ctypes

import pytest
import torch

from hmd_ego_pose_amd import pack_bytes
from hmd_ego_pose_amd.planning import plan_launch_list
from tests._util import seeded_input, seeded_state_dict_once

gpu = pytest.mark.gpu          # (the launch-list case plans on the host and runs without a GPU)

HEADS = ("regression", "classification", "rotation", "translation_raw", "hand")
# the rows of MBF_SHAPES as hep_plan_launch_list / hep_kernel_symbol name them, by the blocks of phi 0 @ 256 (batch 16) that run them
ROWS = {
    "mbf_shape_kernel<true, 5, 1, 16, 0, 1>": (4,),
    "mbf_shape_kernel<true, 3, 2, 8, 0, 2>": (5,),
    "mbf_shape_kernel<true, 3, 1, 16, 0, 3>": (6, 7),
    "mbf_shape_kernel<true, 5, 1, 16, 0, 4>": (8,),
    "mbf_shape_kernel<true, 5, 1, 16, 0, 5>": (9, 10),
    "mbf_shape_kernel<true, 5, 2, 8, 0, 6>": (11,),
    "mbf_shape_kernel<true, 5, 1, 8, 0, 7>": (12, 13, 14),
    "mbf_shape_kernel<true, 3, 1, 8, 0, 8>": (15,),
}


@pytest.fixture(scope="module")
def api():
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd.model import Session
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from oracle import decode_ref, efficientpose_ref
    assert torch.cuda.is_available(), "these tests need the MI355X box"
    return dict(capi=_capi, Session=Session, sd=seeded_state_dict, R=efficientpose_ref, D=decode_ref)      # (the keys tests/test_gpu_parity.py's helpers take)


def _same_bits(a, b):
    """bit for bit, NaNs included (the pad columns of a squeeze-excite partial row are written by nobody: NaN in both runs under the
    LDS- and workspace-poisoning builds)"""
    assert a.dtype == b.dtype and a.shape == b.shape and a.element_size() in (2, 4)
    as_int = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def _fronts(launches):
    """{launch name: device function} of the fused fronts in a list of (name, device function)"""
    return {n: y for n, y in launches if n.endswith(".front") and "mbf_" in y}      # (not the boundary launches: "b1.project+b2.front")


def _stage_names(capi, s):
    l, names = capi.lib(), []
    for i in range(l.hep_debug_tensor_count(s.handle)):
        nm = ctypes.c_char_p(); dims = (ctypes.c_int64 * 4)()
        l.hep_debug_tensor_info(s.handle, i, ctypes.byref(nm), dims)
        names.append(nm.value.decode())
    return names


def _run(api, sd, phi, size, batch, precision, x, stages):
    """(fronts of the session's launch list, head outputs, {stage name: tensor}) of one forward; ``stages``: None = every stage tensor"""
    capi = api["capi"]
    s = api["Session"](sd, phi, size, batch, precision, flags=capi.FLAG_KEEP_INTERMEDIATES)
    fronts = _fronts([(n, y) for n, _b, _f, y in s.kernels(batch)])
    heads = [t.clone() for t in s.forward(x)[1:]]
    torch.cuda.synchronize()
    names = [n for n in _stage_names(capi, s) if stages is None or n in stages]
    kept = {n: s.stage(n, batch) for n in names}
    s.close()
    return fronts, heads, kept


@gpu
@pytest.mark.parametrize("batch", [1, 3, 16])
def test_specialised_fronts_equal_the_generic_kernel_bit_for_bit(api, batch, monkeypatch):
    """phi 0 @ 256 in bf16 as planned and with HEP_MBF_GENERIC=1 (read when the session is created): the first runs the rows of the
    table, the second mbf_kernel on every front; every stage tensor (batch 16: every block output and every front's own
    output) and all five heads are bit-equal."""
    phi, size = 0, 256
    sd = seeded_state_dict_once(phi, 0)
    x = torch.from_numpy(seeded_input((batch, 3, size, size), 41)).cuda()
    stages = None if batch < 16 else [f"block{i}" for i in range(16)] + [f"b{i}.dw" for i in range(4, 16)]
    fs, hs, ss = _run(api, sd, phi, size, batch, "bf16", x, stages)
    monkeypatch.setenv("HEP_MBF_GENERIC", "1")
    fg, hg, sg = _run(api, sd, phi, size, batch, "bf16", x, stages)
    assert sorted(fs) == sorted(fg) == sorted(f"b{i}.front" for i in range(4, 16)), (fs, fg)
    assert all(y.startswith("mbf_kernel<") for y in fg.values()), f"HEP_MBF_GENERIC=1 left a specialised front: {fg}"
    want = {"1": 6, "3": 11, "16": 12}[str(batch)]          # fronts whose out_frag equals their row's at this batch (module docstring)
    spec = {n: y for n, y in fs.items() if y.startswith("mbf_shape_kernel<")}
    assert len(spec) == want and set(spec.values()) <= set(ROWS), fs
    assert all(int(n[1:n.index(".")]) in ROWS[y] for n, y in spec.items()), spec
    assert sorted(ss) == sorted(sg) and len(ss) >= 28, sorted(ss)
    for name, a, b in zip(HEADS, hs, hg):
        assert _same_bits(a, b), f"b{batch} {name}: max |diff| {(a.float() - b.float()).abs().max().item():.3e}"
    for n in ss:
        assert _same_bits(ss[n], sg[n]), f"b{batch} stage {n}: max |diff| {(ss[n] - sg[n]).abs().max().item():.3e}"


def test_every_front_of_the_benchmarked_session_runs_its_row_and_no_row_is_dead():
    """The launch list of phi 0 @ 256 batch 16 bf16 (planned on the host): all twelve fronts report a specialised instance, the one
    listed for their block, and every row of the table is reached by at least one launch."""
    launches = plan_launch_list(pack_bytes(seeded_state_dict_once(0, 0)), 0, 256, 16, "bf16")
    fronts = _fronts([(n, y) for y, n in launches])
    assert sorted(fronts) == sorted(f"b{i}.front" for i in range(4, 16)), fronts
    assert {n: y for n, y in fronts.items()} == {f"b{i}.front": y for y, blocks in ROWS.items() for i in blocks}, fronts
    assert set(fronts.values()) == set(ROWS)
    # ... and the knob reaches the planner the same way hep_create does
    generic = _fronts([(n, y) for y, n in plan_launch_list(pack_bytes(seeded_state_dict_once(0, 0)), 0, 256, 16, "bf16", env={"HEP_MBF_GENERIC": "1"})])
    assert all(y.startswith("mbf_kernel<true, ") and y.endswith(", false, 0>") for y in generic.values()), generic
    # fp32 fronts have no rows
    f32 = _fronts([(n, y) for y, n in plan_launch_list(pack_bytes(seeded_state_dict_once(0, 0)), 0, 256, 16, "fp32")])
    assert len(f32) == 12 and all(y.startswith("mbf_kernel<false, ") for y in f32.values()), f32


@gpu
def test_other_map_sizes_run_the_generic_kernel_phi0_at_128(api):
    """phi 0 @ 128 (bf16, batch 1): the widths of the table on other map sizes - no row matches, every front runs mbf_kernel - within
    the gate of test_gpu_parity.py test_other_input_sizes (finite, 0.15 of the oracle's range end to end)."""
    R = api["R"]
    phi, size, batch = 0, 128, 1
    sd = seeded_state_dict_once(phi, 2)
    launches = plan_launch_list(pack_bytes(sd), phi, size, batch, "bf16")
    fronts = _fronts([(n, y) for y, n in launches])
    assert len(fronts) == 14 and all(y.startswith("mbf_kernel<true, ") for y in fronts.values()), fronts
    x = torch.from_numpy(seeded_input((batch, 3, size, size), 9))
    ref = R.forward(sd, x, phi)
    s = api["Session"](sd, phi, size, batch, "bf16")
    assert _fronts([(n, y) for n, _b, _f, y in s.kernels(batch)]) == fronts
    out = s.forward(x.cuda())
    torch.cuda.synchronize()
    s.close()
    for name, a, b in zip(HEADS, out[1:], ref[1:]):
        assert torch.isfinite(a).all(), name
        err = (a.float().cpu() - b).abs().max().item()
        print(f"phi 0 @ 128 b1 bf16 {name}: max |hip - oracle| = {err:.3e} (bound {0.15 * max(1.0, b.abs().max().item()):.3e})")
        assert err <= 0.15 * max(1.0, b.abs().max().item()), (name, err)


@gpu
def test_other_widths_run_the_generic_kernel_phi1_at_256(api, monkeypatch):
    """phi 1 @ 256 (bf16, batch 1): the front of block 22 (320 -> 1920 channels, a width phi 0 does not have) runs mbf_kernel; the
    fronts that repeat phi 0's layer shapes run their rows (module docstring) and nothing else is named.  The session passes the
    stage-wise gate test_other_widths_match_oracle holds phi 1 @ 256 to (_teacher_forced_bf16, not strict) and equals the
    all-generic plan bit for bit."""
    from tests.test_gpu_parity import _teacher_forced_bf16
    R = api["R"]
    phi, size, batch = 1, 256, 1
    sd = seeded_state_dict_once(phi, 2)
    fronts = _fronts([(n, y) for y, n in plan_launch_list(pack_bytes(sd), phi, size, batch, "bf16")])
    assert fronts["b22.front"] == "mbf_kernel<true, 3, 1, 8, false, 0>", fronts
    assert all(y in ROWS or y.startswith("mbf_kernel<true, ") for y in fronts.values()), fronts
    x = torch.from_numpy(seeded_input((batch, 3, size, size), 2))
    _teacher_forced_bf16(api, sd, phi, size, batch, x, R.forward(sd, x, phi), strict=False)
    blocks = [f"block{i}" for i in range(23)]
    _, hs, ss = _run(api, sd, phi, size, batch, "bf16", x.cuda(), blocks)
    monkeypatch.setenv("HEP_MBF_GENERIC", "1")
    fg, hg, sg = _run(api, sd, phi, size, batch, "bf16", x.cuda(), blocks)
    assert all(y.startswith("mbf_kernel<") for y in fg.values()), fg
    for name, a, b in zip(HEADS, hs, hg):
        assert _same_bits(a, b), name
    assert sorted(ss) == sorted(blocks)
    for n in blocks:
        assert _same_bits(ss[n], sg[n]), n
