#!/usr/bin/env python3
"""Inventory of the kernel variants the inference planner can select, planned on the host (no GPU needed).

A variant is the device function of a launch (hep_kernel_symbol's string).  For a matrix of (phi, size, batch, dtype) with the
knobs of the environment, print every variant with the number of configurations that select it and the cheapest of them:

    python tools/plan_variants.py                          # the support matrix of tests/test_plan_coverage_cpu.py
    python tools/plan_variants.py --phi 0 3 --sizes 256 512 --batches 1 16
    python tools/plan_variants.py --uncovered              # the variants no entry of tests/_util.py PARITY_CONFIGS reaches, each with
                                                           # the cheapest configuration that selects it, and a greedy cover of them
    python tools/plan_variants.py --uncovered --without variant_cover     # ... as if that group of PARITY_GROUPS were empty
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmd_ego_pose_amd import pack_bytes, seeded_state_dict  # noqa: E402
from hmd_ego_pose_amd.planning import by_variant, config_cost, plan_matrix, table_variants, variants  # noqa: E402


def fmt(cfg):
    return f"phi {cfg[0]} @ {cfg[1]} b{cfg[2]} {cfg[3]}" + "".join(f" {k}={v}" for k, v in (cfg[4] if len(cfg) > 4 else {}).items())


def greedy_cover(missing, planned):
    """[(configuration, the variants of ``missing`` it is the cheapest pick for)]: together they select every variant of ``missing``.
    Most new variants per unit of cost first, then redundant picks dropped."""
    left, cover = set(missing), []
    while left:
        best = max(planned, key=lambda c: (len(planned[c] & left) / config_cost(c), c))
        gain = planned[best] & left
        if not gain:
            break
        cover.append(best)
        left -= gain
    need = set(missing) - left
    for cfg in sorted(cover, key=config_cost, reverse=True):          # drop what later picks made redundant, dearest first
        rest = [c for c in cover if c != cfg]
        if rest and need <= set().union(*(planned[c] for c in rest)):
            cover = rest
    seen, out = set(), []
    for cfg in sorted(cover, key=lambda c: (config_cost(c), c)):
        out.append((cfg, sorted((planned[cfg] & set(missing)) - seen)))
        seen |= planned[cfg]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--phi", type=int, nargs="+", default=list(range(8)))
    ap.add_argument("--sizes", type=int, nargs="+", default=list(range(128, 1025, 128)))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 3, 4, 8, 16, 32, 64])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--big-size", type=int, default=768, help="from this size up only batches <= --big-batch")
    ap.add_argument("--big-batch", type=int, default=8)
    ap.add_argument("--uncovered", action="store_true", help="only the variants that tests/_util.py PARITY_CONFIGS does not reach")
    ap.add_argument("--without", nargs="*", default=[], help="groups of PARITY_GROUPS to leave out of the table")
    args = ap.parse_args()
    configs = [(phi, size, batch, dt) for phi in args.phi for size in args.sizes for batch in args.batches
               if size < args.big_size or batch <= args.big_batch for dt in args.dtypes]
    packs = {phi: pack_bytes(seeded_state_dict(phi, 0)) for phi in args.phi}
    planned = {c: variants(l) for c, l in plan_matrix(configs, packs).items()}
    inv = by_variant({c: [(v, "") for v in vs] for c, vs in planned.items()})
    print(f"{len(configs)} configurations, {len(inv)} variants")
    if not args.uncovered:
        for v in sorted(inv):
            print(f"{v:60s} {len(inv[v]):5d} configurations, cheapest {fmt(inv[v][0])}")
        return 0
    from tests._util import PARITY_GROUPS
    entries = [e for g, es in PARITY_GROUPS.items() if g not in args.without for e in es]
    for phi in {e[0] for e in entries} - set(packs):
        packs[phi] = pack_bytes(seeded_state_dict(phi, 0))
    reached = table_variants(entries, packs)
    missing = sorted(set(inv) - reached)
    print(f"{len(entries)} table entries reach {len(set(inv) & reached)} of them; {len(missing)} are compared with no reference:")
    for v in missing:
        print(f"  {v:60s} {len(inv[v]):5d} configurations, cheapest {fmt(inv[v][0])}")
    if missing:
        print("greedy cover:")
        for cfg, gain in greedy_cover(missing, planned):
            print(f"  {cfg!r}: " + "; ".join(gain))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
