"""CPU (no GPU): the GPU parity suite against the planner.  ``plan_session`` picks template instantiations - GEMM tile shapes,
squeeze-excite variants, single- and multi-pass fronts, depthwise tile widths, chained or segmented separable kernels - from
phi, the input size, max_batch and the dtype; a variant that no parity test selects has never been compared with anything.
hep_plan_launch_list plans on the host, so the whole support matrix is planned here and held against tests/_util.py
PARITY_CONFIGS, the table the parity tests of tests/test_gpu_parity.py take their parameters from."""
import pytest

from hmd_ego_pose_amd import _capi, pack_bytes
from hmd_ego_pose_amd.planning import by_variant, plan_launch_list, plan_matrix, table_variants
from tests._util import PARITY_CONFIGS, PARITY_GROUPS, VARIANT_COVER, seeded_state_dict_once

# The support matrix.  Rule: every phi the library accepts; input sizes 128 .. 1024 in steps of 128 (the sizes the reference's
# up- and down-sampling allows, up to 4x the benchmarked 256); the batch sizes the notebook quotes figures for plus the odd one
# (3), at most 8 from size 768 up (beyond that a batch no longer fits a caller's latency budget on one device); both shipped
# dtypes; default knobs.  880 configurations.  It may grow and never shrink, and no variant it yields may be exempted below.
PHIS = tuple(range(8))
SIZES = tuple(range(128, 1025, 128))
BATCHES = (1, 2, 3, 4, 8, 16, 32, 64)
BIG_SIZE, BIG_BATCH = 768, 8
DTYPES = ("fp32", "bf16")
MATRIX = [(phi, size, batch, dtype) for phi in PHIS for size in SIZES for batch in BATCHES if size < BIG_SIZE or batch <= BIG_BATCH
          for dtype in DTYPES]


def _fmt(cfg):
    return f"phi {cfg[0]} @ {cfg[1]} b{cfg[2]} {cfg[3]}"


@pytest.fixture(scope="module")
def packs():
    """phi -> seed-0 weight pack, built once (the weights decide nothing about a plan but the class count)"""
    return {phi: pack_bytes(seeded_state_dict_once(phi, 0)) for phi in PHIS}


@pytest.fixture(scope="module")
def planned(packs):
    assert len(MATRIX) == 880
    return plan_matrix(MATRIX, packs)


def test_every_variant_of_the_support_matrix_is_compared_with_a_reference(packs, planned):
    """Every device function the planner selects somewhere in the support matrix is selected by at least one entry of
    PARITY_CONFIGS, i.e. by a session that a GPU test compares with the oracle."""
    inv = by_variant(planned)
    assert len(inv) >= 206, len(inv)                       # (the inventory when this test was written: a planner that lost variants also lost code)
    reached = table_variants(PARITY_CONFIGS, packs)
    missing = sorted(set(inv) - reached)
    assert not missing, f"{len(missing)} of {len(inv)} variants are compared with no reference:\n" + "\n".join(
        f"  {v}: {len(inv[v])} configurations, cheapest {_fmt(inv[v][0])}" for v in missing)


def test_variant_cover_entries_select_the_variants_they_are_listed_for(packs):
    """tests/_util.py VARIANT_COVER names, per case, the variants it is there for: each is in that case's launch list (the GPU test
    checks the stages of exactly those launches), and none of them is reached by the other groups (then the case would be spare)."""
    others = table_variants([e for g, es in PARITY_GROUPS.items() if g != "variant_cover" for e in es], packs)
    for phi, size, batch, dtype, wanted in VARIANT_COVER:
        syms = {sym for sym, _ in plan_launch_list(packs[phi], phi, size, batch, dtype, _capi.FLAG_KEEP_INTERMEDIATES)}
        assert set(wanted) <= syms, (_fmt((phi, size, batch, dtype)), sorted(set(wanted) - syms))
        assert not set(wanted) & others, (_fmt((phi, size, batch, dtype)), sorted(set(wanted) & others))


def test_every_launch_of_the_support_matrix_names_an_instantiation(planned):
    """No configuration of the matrix fails to plan (plan_matrix raises on a refusal, and plan_session refuses a launch whose pick
    has no instantiation), and every line of every launch list names a device function of the form name<...>."""
    import re
    assert set(planned) == set(MATRIX)
    form = re.compile(r"^[A-Za-z_][A-Za-z0-9_]*<[^<>]+>$")
    bad = [(_fmt(c), sym, name) for c, launches in planned.items() for sym, name in launches if not form.match(sym) or not name]
    assert all(planned.values()) and not bad, bad[:10]


@pytest.mark.parametrize("size,batch", [(128, 1), (256, 16), (640, 3)])
def test_phi7_plans_the_launch_list_of_phi6(packs, size, batch):
    """phi 6 and 7 share the backbone (EfficientNet-B6), the BiFPN width and depth and the heads: the inference planner selects
    the same device function for the same launch, in both dtypes - phi 7 adds no variant beyond phi 6."""
    for dtype in DTYPES:
        assert plan_launch_list(packs[7], 7, size, batch, dtype) == plan_launch_list(packs[6], 6, size, batch, dtype), (size, batch, dtype)


def test_keep_intermediates_flag_changes_no_launch(packs, planned):
    """FLAG_KEEP_INTERMEDIATES only stops the arena from reusing memory: the launch list is identical with and without it at every
    configuration of the matrix.  The stage-wise parity tests rely on that - they run with the flag and vouch for sessions without."""
    kept = plan_matrix(MATRIX, packs, flags=_capi.FLAG_KEEP_INTERMEDIATES)
    differ = [_fmt(c) for c in MATRIX if kept[c] != planned[c]]
    assert not differ, differ[:10]


def test_launch_list_reads_the_knobs_and_refuses_what_create_refuses(packs):
    """hep_plan_launch_list mirrors hep_create_from_memory: knobs come from the environment at the call, bad arguments are refused
    with the same codes, and a buffer that is too small is reported with the size that is needed."""
    import ctypes
    base = plan_launch_list(packs[0], 0, 256, 3, "fp32")
    assert base[0] == ("stem_valu_kernel<false>", "stem") and len(base) > 40 and all(sym and name for sym, name in base)
    forced = plan_launch_list(packs[0], 0, 256, 3, "fp32", env={"HEP_SE_MAXMB": "1000"})
    assert forced != base and not any("se_finish_kernel" in sym for sym, _ in forced)
    assert plan_launch_list(packs[0], 0, 256, 3, "fp32") == base                       # the environment was restored
    l = _capi.lib()
    need = ctypes.c_size_t()
    assert l.hep_plan_launch_list(packs[0], len(packs[0]), 0, 256, 3, _capi.HEP_F32, 0, None, 0, ctypes.byref(need)) == 0
    assert need.value == sum(len(sym) + len(name) + 4 for sym, name in base) + 1
    small = ctypes.create_string_buffer(16)
    assert l.hep_plan_launch_list(packs[0], len(packs[0]), 0, 256, 3, _capi.HEP_F32, 0, small, 16, ctypes.byref(need)) == -1
    assert l.hep_plan_launch_list(packs[0], len(packs[0]), 8, 256, 3, _capi.HEP_F32, 0, None, 0, ctypes.byref(need)) == -4   # phi 8
    assert l.hep_plan_launch_list(packs[0], len(packs[0]), 0, 200, 3, _capi.HEP_F32, 0, None, 0, ctypes.byref(need)) == -4   # size
    assert l.hep_plan_launch_list(packs[0], len(packs[0]), 3, 256, 3, _capi.HEP_F32, 0, None, 0, ctypes.byref(need)) == -2   # phi 0's pack
    assert b"weight pack" in l.hep_last_error()
    assert l.hep_plan_launch_list(packs[0][:1000], 1000, 0, 256, 3, _capi.HEP_F32, 0, None, 0, ctypes.byref(need)) == -2
