"""The sum hook of synchronised BatchNorm: a ``torch.distributed`` process group (or none) as the ``hep_sum_fn`` callback of
the hep_{heads,neck,backbone}_*_device_sync calls (include/hep.h).

The library hands the hook one block of doubles inside the workspace of the call; when the work the hook enqueued on the
stream has run, every element has to be the sum over all replicas.  ``SumHook`` finds the workspace tensor the caller
registered, views the block and runs ``dist.all_reduce`` on the view.  With no group, or a group of one, it does nothing: the
identity, and ``torch.distributed`` is never imported.  Under the gloo backend (two ranks on one device, the tests) device
tensors are staged through the host, as ``dist._wire`` does for point-to-point messages; under nccl / RCCL the collective is
enqueued behind the current stream and nothing waits for the host.

The callback never lets a Python exception through (ctypes would print it and return 0, i.e. success): it returns 1, the
entry point then launches nothing further, and ``SumHook.error`` keeps the exception for the caller's message.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

LOCAL = "local"      # ``Trainer(batch_norm="sync", process_group=LOCAL)``: this process alone - no group, the identity hook

SUM_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p)


class HepSync(ctypes.Structure):
    """``hep_sync`` of include/hep.h."""
    _fields_ = [("sum", SUM_FN), ("ctx", ctypes.c_void_p)]


def group_world(process_group) -> int:
    """Ranks of ``process_group``; 1 for None (``torch.distributed`` is not imported then)."""
    if process_group is None:
        return 1
    import torch.distributed as dist
    return dist.get_world_size(process_group)


def group_rank(process_group) -> int:
    if process_group is None:
        return 0
    import torch.distributed as dist
    return dist.get_rank(process_group)


def stages_on_host(process_group) -> bool:
    """gloo has no collectives for device tensors here: they go through the host."""
    if process_group is None:
        return False
    import torch.distributed as dist
    return dist.get_backend(process_group) == "gloo"


def all_reduce_sum(t: torch.Tensor, process_group, force: bool = False) -> None:
    """``t`` (device or host, contiguous) summed over the group in place; nothing for no group or - unless ``force`` - a group of one."""
    if process_group is None or (group_world(process_group) == 1 and not force):
        return
    import torch.distributed as dist
    if t.is_cuda and stages_on_host(process_group):
        h = t.cpu()
        dist.all_reduce(h, group=process_group)
        t.copy_(h)
    else:
        dist.all_reduce(t, group=process_group)


def broadcast(t: torch.Tensor, process_group, src: int = 0) -> None:
    """``t`` of rank ``src`` of the group into every rank's ``t``, in place."""
    if group_world(process_group) == 1:
        return
    import torch.distributed as dist
    gsrc = dist.get_global_rank(process_group, src)
    if t.is_cuda and stages_on_host(process_group):
        h = t.cpu()
        dist.broadcast(h, gsrc, group=process_group)
        t.copy_(h)
    else:
        dist.broadcast(t, gsrc, group=process_group)


class SumHook:
    """One hook object per caller.  ``register(ws)`` names a workspace tensor (uint8, device) a following call may hand blocks
    of; ``ref()`` is the ``const hep_sync*`` argument.  ``calls`` counts the hook calls (identity ones included).  ``force``
    (False): run the collective in a group of one too - what tools/sync_step_time.py times on a one-GPU box.  The object keeps
    the ctypes callback alive: keep the object as long as the library may call it."""

    def __init__(self, process_group=None):
        self.group = process_group
        self.world = group_world(process_group)
        self.calls, self.force = 0, False
        self.error: Optional[BaseException] = None
        self._ws = []
        self._cb = SUM_FN(self._sum)
        self._struct = HepSync(self._cb, None)

    def __deepcopy__(self, memo):       # (a module that carries a hook can be copied: the copy gets a callback of its own)
        return SumHook(self.group)

    def register(self, *workspaces: torch.Tensor) -> None:
        self._ws = [w for w in workspaces if w is not None]

    def ref(self):
        return ctypes.byref(self._struct)

    def _view(self, data: int, count: int, is_double: bool) -> torch.Tensor:
        size, dtype = (8, torch.float64) if is_double else (4, torch.float32)
        for w in self._ws:
            off = data - w.data_ptr()
            if 0 <= off and off + count * size <= w.numel() * w.element_size():
                return w.view(torch.uint8)[off:off + count * size].view(dtype)
        raise RuntimeError("the sum hook got a block outside every registered workspace")

    def _sum(self, ctx, data, count, is_double, stream) -> int:
        try:
            self.calls += 1
            if self.world > 1 or (self.force and self.group is not None):
                all_reduce_sum(self._view(int(data), int(count), bool(is_double)), self.group, self.force)
            return 0
        except BaseException as e:      # nothing may leave a ctypes callback
            self.error = e
            return 1

    def check(self, rc: int) -> int:
        """``_capi.check`` with the hook's own exception, if it had one, as the cause."""
        from . import _capi
        if rc < 0 and self.error is not None:
            e, self.error = self.error, None
            raise _capi.HepError(f"libhep error {rc}: {_capi.lib().hep_last_error().decode(errors='replace')} ({type(e).__name__}: {e})") from e
        return _capi.check(rc)
