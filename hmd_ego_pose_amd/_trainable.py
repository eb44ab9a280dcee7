"""What ``TrainableHeads``, ``TrainableNeck`` and ``TrainableBackbone`` share: a part of the model as an ``nn.Module`` that
carries the reference's keys, its flat fp32 parameter buffer for the hep_{part}_*_device calls, and the small helpers around
those calls.  A part says which tensors it is (``spec``) and what to call them in an error (``NOUN``); the module-level helpers
take the part's name in the library's symbols ("heads", "neck", "backbone")."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Tuple

import torch
from torch import nn

from . import _capi


def without_counters(spec) -> List[Tuple[str, tuple]]:
    """A spec without the int64 ``num_batches_tracked`` counters: the tensors of the flat fp32 buffer, in buffer order."""
    return [(k, s) for k, s in spec if not k.endswith("num_batches_tracked")]


def ptrs(tensors):
    return None if tensors is None else _capi.ptr_array(list(tensors))


def cotangents(grads, shapes, device):
    """The cotangents autograd hands to a ``backward`` as contiguous float32 tensors, zeros where it hands None."""
    return [torch.zeros(tuple(s), dtype=torch.float32, device=device) if g is None else g.to(torch.float32).contiguous()
            for g, s in zip(grads, shapes)]


def param_layout(part: str, *cfg):
    """(total floats, [offset of every flat tensor]) as hep_{part}_param_count / hep_{part}_param_layout report them."""
    l = _capi.lib()
    count, layout = getattr(l, f"hep_{part}_param_count"), getattr(l, f"hep_{part}_param_layout")
    total = _capi.check(count(*cfg))
    n = _capi.check(layout(*cfg, None, 0))
    arr = (ctypes.c_int64 * n)()
    _capi.check(layout(*cfg, arr, n))
    return int(total), [int(v) for v in arr]


def stage_views(part: str, ws: torch.Tensor, compound_coef: int, size: int, batch: int) -> Dict[str, torch.Tensor]:
    """name -> float32 view (NHWC) of every tensor hep_{part}_stage_info names in the workspace of a forward."""
    l = _capi.lib()
    count, info = getattr(l, f"hep_{part}_stage_count"), getattr(l, f"hep_{part}_stage_info")
    out = {}
    for i in range(_capi.check(count(compound_coef))):
        nm = ctypes.c_char_p(); dims = (ctypes.c_int64 * 4)(); off = ctypes.c_int64()
        _capi.check(info(compound_coef, size, batch, i, ctypes.byref(nm), dims, ctypes.byref(off)))
        shape = tuple(int(d) for d in dims)
        n = shape[0] * shape[1] * shape[2] * shape[3]
        out[nm.value.decode()] = ws[off.value:off.value + 4 * n].view(torch.float32).view(shape)
    return out


BN_RUNNING, BN_BATCH = 0, 1        # HEP_BN_RUNNING, HEP_BN_BATCH of include/hep.h
BN_MODES = {"running": BN_RUNNING, "batch": BN_BATCH}
BN_SYNC = "sync"                   # batch statistics over the rows of all replicas: its own entry points (hep_*_device_sync), no bn_mode value
BN_NAMES = (*BN_MODES, BN_SYNC)
BN_MOMENTUM = 0.01                 # every nn.BatchNorm2d of the reference (efficientnet/model.py, efficientdet/model.py, hmdegopose/model.py)


class TrainablePart(nn.Module):
    """Base of the three trainable parts.  A subclass sets ``spec`` and ``NOUN``, calls ``_attach_spec`` in its ``__init__``
    and adds its own ``forward``.  ``batch_norm``: "running" (every mode evaluates BatchNorm with the running statistics) or
    "batch" (``train()`` mode normalises with the statistics of the batch and moves the running statistics, as
    ``nn.BatchNorm2d`` does; ``eval()`` is the running-statistics function) or "sync" ("batch" with every BatchNorm seeing the
    rows of ALL replicas of ``process_group``, a ``torch.distributed`` group - the reference's ``utils/sync_batchnorm``; with no
    group it is "batch" bit for bit).  Under "sync" this replica's parameter gradients are its own contribution: their plain SUM
    over the replicas is the gradient of the global-batch function."""
    NOUN = ""     # "head" | "BiFPN" | "backbone": what from_model's error calls the part's tensors
    spec = None   # staticmethod(*cfg) -> [(key, shape)]: the part's subset of ``param_spec``, in state_dict order

    def _set_batch_norm(self, batch_norm, process_group=None):
        if batch_norm not in BN_NAMES:
            raise ValueError(f"batch_norm must be 'running', 'batch' or 'sync', not {batch_norm!r}")
        if process_group is not None and batch_norm != BN_SYNC:
            raise ValueError("process_group goes with batch_norm='sync'")
        self.batch_norm = batch_norm
        self._hook = None                  # (a plain attribute: no tensor, nothing in state_dict)
        if batch_norm == BN_SYNC:
            from .sync import SumHook
            self._hook = SumHook(process_group)

    def _sync_hook(self):
        """The sum hook of this call: only in ``train()`` mode of a ``batch_norm="sync"`` part (None otherwise)."""
        return self._hook if self.batch_norm == BN_SYNC and self.training else None

    def _bn_mode(self) -> int:
        """The BatchNorm mode of this call: batch statistics only in ``train()`` mode of a ``batch_norm="batch"`` part."""
        return BN_BATCH if self.batch_norm in ("batch", BN_SYNC) and self.training else BN_RUNNING

    def _store_statistics(self, stats: torch.Tensor):
        """After a batch-statistics forward: ``stats`` (layout of ``flat_parameters``, its running_mean / running_var elements
        new) into the buffers in place, and every ``num_batches_tracked`` up by one."""
        buffers = dict(self.named_buffers())
        tensors = dict(self.named_parameters())
        tensors.update(buffers)
        dst, src = [], []
        for k, v in zip(self._flat_keys, stats.split([tensors[k].numel() for k in self._flat_keys])):
            if k.endswith(("running_mean", "running_var")):
                dst.append(buffers[k]); src.append(v.view_as(buffers[k]))
        counters = [b for k, b in buffers.items() if k.endswith("num_batches_tracked")]
        with torch.no_grad():
            torch._foreach_copy_(dst, src)
            torch._foreach_add_(counters, 1)

    def _attach_spec(self, *cfg):
        """Register the part's parameters and buffers under the reference's keys; ``cfg``: the arguments of ``spec``."""
        from .model import _attach
        spec = self.spec(*cfg)
        self._spec_keys = [k for k, _ in spec]
        for key, shape in spec:
            _attach(self, key, shape)
        self._flat_keys = [k for k, _ in without_counters(spec)]

    @classmethod
    def _model_cfg(cls, model) -> tuple:
        """The constructor arguments that ``from_model`` takes from ``model``."""
        return (model.compound_coef,)

    @classmethod
    def from_model(cls, model, **kwargs):
        """This part with the tensors of an ``HMDEgoPose`` (or any module with the reference's keys), on the model's device.
        ``kwargs``: further constructor arguments (``batch_norm=...``)."""
        m = cls(*cls._model_cfg(model), **kwargs)
        sd = model.state_dict()
        missing = [k for k in m._spec_keys if k not in sd]
        if missing:
            raise KeyError(f"the model's state_dict lacks {cls.NOUN} tensors, e.g. {missing[0]}")
        m.load_state_dict(sd, strict=False)
        return m.to(next(iter(sd.values())).device)

    def export_to(self, model):
        """Copy every tensor of this part into ``model`` (an ``HMDEgoPose``) and drop its packed device weights."""
        own, dst = self.state_dict(), model.state_dict()
        with torch.no_grad():
            for k, v in own.items():
                dst[k].copy_(v)
        model.invalidate()
        return model

    def flat_parameters(self) -> torch.Tensor:
        """The flat fp32 buffer of hep_*_device calls (autograd-tracked: its gradient splits back onto the parameters)."""
        tensors = dict(self.named_parameters())
        tensors.update(dict(self.named_buffers()))
        return torch.cat([tensors[k].reshape(-1) for k in self._flat_keys])
