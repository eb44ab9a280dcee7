"""Host-only view of the inference planner: the launch list a session WOULD run, without creating one.

``hep_plan_launch_list`` (include/hep.h) fills a Session as ``hep_create_from_memory`` does and stops after ``plan_session``; it makes
no HIP call, so everything here works on a machine without a GPU.  A *variant* is the device function of a launch (the template
instantiation ``hep_kernel_symbol`` names): what the planner picks from phi, the input size, ``max_batch``, the dtype and the knobs
of the environment.  tools/plan_variants.py prints the inventory of a matrix of configurations, tests/test_plan_coverage_cpu.py
holds the GPU parity suite to it.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Dict, Iterable, List, Mapping, Optional, Tuple

from . import _capi

_DTYPES = {"fp32": _capi.HEP_F32, "f32": _capi.HEP_F32, "bf16": _capi.HEP_BF16, "fp8": _capi.HEP_FP8}


@contextlib.contextmanager
def knob_environment(env: Optional[Mapping[str, str]]):
    """The plan knobs are read from the environment when a session is planned: set ``env`` for the duration of the block."""
    env = dict(env or {})
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def plan_launch_list(pack: bytes, phi: int, size: int, max_batch: int, precision: str = "fp32", flags: int = 0,
                     env: Optional[Mapping[str, str]] = None) -> List[Tuple[str, str]]:
    """[(device function, launch name)] of the session ``Session(sd, phi, size, max_batch, precision, flags=flags)`` would build,
    in launch order.  ``pack`` is ``pack_bytes(state_dict)`` (built once per phi by the caller: the weights decide nothing but
    the class count); ``env`` are plan knobs (HEP_*) set while the plan is made."""
    l = _capi.lib()
    need = ctypes.c_size_t()
    args = (pack, len(pack), phi, size, max_batch, _DTYPES[precision], flags)
    buf = ctypes.create_string_buffer(1 << 16)
    with knob_environment(env):
        rc = l.hep_plan_launch_list(*args, buf, len(buf), ctypes.byref(need))
        if rc != 0 and need.value > len(buf):
            buf = ctypes.create_string_buffer(need.value)
            rc = l.hep_plan_launch_list(*args, buf, len(buf), ctypes.byref(need))
    _capi.check(rc)
    out = []
    for line in buf.value.decode().splitlines():
        sym, _, name = line.partition(" | ")
        out.append((sym, name))
    return out


def variants(launch_list: Iterable[Tuple[str, str]]) -> frozenset:
    """The set of variants (launch-list line minus the launch name) of one launch list."""
    return frozenset(sym for sym, _ in launch_list)


def config_cost(cfg) -> float:
    """What a stage-wise parity case of this configuration costs, roughly.  The oracle side evaluates single stages on a few
    images, so the batch weighs little (the device run and the read-back of its stage tensors); pixels and the depth and width
    of the phi weigh fully.  Orders the configurations that select a variant: the first is "the cheapest"."""
    phi, size, batch, _prec = cfg[:4]
    return size * size * (1.0 + 0.6 * phi) ** 2 * (1.0 + batch / 32.0)


def plan_matrix(configs, packs: Dict[int, bytes], flags: int = 0, threads: Optional[int] = None) -> Dict[tuple, List[Tuple[str, str]]]:
    """{(phi, size, batch, precision): launch list} under the knobs of the environment as it stands.  ``packs`` maps a phi to its
    weight pack, built once.  Planned on a few threads: the library call holds no interpreter lock and the environment is only read."""
    from concurrent.futures import ThreadPoolExecutor
    configs = list(configs)
    with ThreadPoolExecutor(threads or min(8, os.cpu_count() or 1)) as ex:
        got = list(ex.map(lambda c: plan_launch_list(packs[c[0]], c[0], c[1], c[2], c[3], flags), configs))
    return dict(zip(configs, got))


def by_variant(planned: Mapping[tuple, Iterable[Tuple[str, str]]]) -> Dict[str, List[tuple]]:
    """variant -> the configurations of ``planned`` that select it, cheapest first."""
    inv: Dict[str, List[tuple]] = {}
    for cfg, launches in planned.items():
        for v in variants(launches):
            inv.setdefault(v, []).append(cfg)
    for v in inv:
        inv[v].sort(key=lambda c: (config_cost(c), c))
    return inv


def table_variants(entries, packs: Dict[int, bytes]) -> set:
    """The variants that the entries (phi, size, batch, precision, knob environment, ...) of a table reach, each planned under
    its own knobs, one at a time (the environment belongs to the whole process)."""
    reached = set()
    for phi, size, batch, prec, env, *_ in entries:
        reached |= variants(plan_launch_list(packs[phi], phi, size, batch, prec, 0, env))
    return reached
