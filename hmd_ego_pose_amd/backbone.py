"""Trainable EfficientNet trunk: the stem and every MBConv block of ``backbone_net.model.*`` with a HIP forward AND backward
(csrc/k_backbone_grad.hip: hep_backbone_forward_device / hep_backbone_backward_device) as a function of its parameters and the
image [B, 3, S, S], giving the three taps P3 / P4 / P5 that ``TrainableNeck`` takes.

With the trunk trainable the reference's whole ``train.py`` step stays on the GPU:

    image -> HIP backbone forward (TrainableBackbone) -> HIP neck forward (TrainableNeck) -> HIP heads forward (TrainableHeads)
    -> training.format_translation -> HIP losses (training.losses) -> HIP loss backward -> HIP heads backward -> HIP neck
    backward -> HIP backbone backward -> a stock torch.optim step over the three modules' parameters

and ``export_to(model)`` copies the fitted tensors back into the ``HMDEgoPose`` drop-in.

The rules are those of ``hmd_ego_pose_amd.heads`` and ``hmd_ego_pose_amd.neck``: fp32 only; by default BatchNorm uses its RUNNING
statistics in every mode, forward and backward (``weight`` / ``bias`` get gradients, ``running_mean`` / ``running_var`` get
exactly zero and never change); ``batch_norm="batch"`` makes ``train()`` mode the reference's ``model.train()``: the stem's
BatchNorm and every block's ``_bn0`` / ``_bn1`` / ``_bn2`` normalise with the statistics of their map's ``B * s * s`` pixels and
move their running statistics (momentum 0.01), ``eval()`` stays the running-statistics function bit for bit.  Drop-connect (efficientnet/utils.py:85-94 with the rate of efficientdet/model.py:447-449), the
only stochastic op on the path, enters the kernels as DATA: a per-block, per-image scale of the residual branch,
``y = bn2(project) * scale[i][b] + input``, used only where the block adds its input.  The module draws the scales itself only
when ``drop_connect_rate`` is non-zero AND it is in ``train()``; the default rate 0.0 makes it deterministic.
``batch_norm="sync"`` (with ``process_group=``): batch statistics over the rows of all replicas (``_trainable.TrainablePart``).
Out of scope: bf16 training.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _capi, _trainable
from .arch import get_arch, param_spec

PREFIX = "backbone_net."


def backbone_spec(compound_coef: int) -> List[Tuple[str, tuple]]:
    """The ``backbone_net.*`` subset of ``param_spec`` (key, shape), in the reference's state_dict order."""
    get_arch(compound_coef)
    return [(k, s) for k, s in param_spec(compound_coef) if k.startswith(PREFIX)]


def flat_keys(compound_coef: int) -> List[Tuple[str, tuple]]:
    """The tensors of the flat fp32 parameter buffer of hep_backbone_*_device, in buffer order: ``backbone_spec`` without the
    int64 ``num_batches_tracked`` counters."""
    return _trainable.without_counters(backbone_spec(compound_coef))


def _check_size(size: int):
    if size < 128 or size > 2048 or size % 128 != 0:
        raise ValueError(f"input size {size}: the trainable backbone takes a multiple of 128 in [128, 2048]")


def backbone_forward(flat: torch.Tensor, image: torch.Tensor, compound_coef: int, branch_scale: Optional[torch.Tensor] = None,
                     bn_mode: int = _trainable.BN_RUNNING, momentum: float = _trainable.BN_MOMENTUM, stats: Optional[torch.Tensor] = None, sync=None):
    """hep_backbone_forward_device_bn on the current stream.  ``flat``: the flat parameter buffer (``flat_keys`` order), ``image``:
    contiguous float32 NCHW [B, 3, S, S], ``branch_scale``: float32 [blocks, B] on the same device or None (all ones).
    Returns (taps, workspace): P3, P4, P5 as float32 NCHW and the workspace hep_backbone_backward_device_bn needs (same
    ``bn_mode``).  ``stats`` (batch statistics): a buffer like ``flat`` whose running_mean / running_var elements receive the
    updated statistics.  No host synchronisation.  ``sync``: a ``sync.SumHook`` - hep_backbone_forward_device_sync instead (batch
    statistics over all replicas; ``bn_mode`` is not read)."""
    a = get_arch(compound_coef)
    dev, B, size = flat.device, int(image.shape[0]), int(image.shape[-1])
    _check_size(size)
    l = _capi.lib()
    nbytes = _capi.check(l.hep_backbone_workspace_bytes_bn(compound_coef, size, B, bn_mode) if sync is None else
                         l.hep_backbone_workspace_bytes_sync(compound_coef, size, B))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    taps = tuple(torch.empty((B, c, size // (8 << t), size // (8 << t)), dtype=torch.float32, device=dev) for t, c in enumerate(a.tap_channels))
    stream = torch.cuda.current_stream(dev).cuda_stream
    if sync is not None:
        sync.register(ws)
        sync.check(l.hep_backbone_forward_device_sync(flat.data_ptr(), image.data_ptr(), _capi.ptr(branch_scale), compound_coef, size, B,
                                                      _capi.ptr_array(list(taps)), ws.data_ptr(), nbytes, momentum, _capi.ptr(stats), sync.ref(), stream))
        return taps, ws
    _capi.check(l.hep_backbone_forward_device_bn(flat.data_ptr(), image.data_ptr(), _capi.ptr(branch_scale), compound_coef, size, B,
                                                 _capi.ptr_array(list(taps)), ws.data_ptr(), nbytes, bn_mode, momentum, _capi.ptr(stats), stream))
    return taps, ws


def backbone_backward(flat: torch.Tensor, grad_taps, ws: torch.Tensor, compound_coef: int, size: int,
                      branch_scale: Optional[torch.Tensor] = None, want_image: bool = False, bn_mode: int = _trainable.BN_RUNNING, sync=None):
    """hep_backbone_backward_device_bn on the current stream, after ``backbone_forward`` with the same ``flat``, ``branch_scale``,
    ``ws`` and ``bn_mode``.  Returns (grad_flat, grad_image): the parameter gradients in the layout of ``flat`` (running statistics zero)
    and the image gradient (None unless ``want_image``: the ABI then gets NULL and skips it)."""
    dev, B = flat.device, int(grad_taps[0].shape[0])
    g_flat = torch.empty_like(flat)
    g_img = torch.empty((B, 3, size, size), dtype=torch.float32, device=dev) if want_image else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    if sync is not None:               # (the forward's hook: grad_flat is this replica's contribution, to be SUMMED over the replicas)
        sync.register(ws)
        sync.check(_capi.lib().hep_backbone_backward_device_sync(flat.data_ptr(), _capi.ptr_array(list(grad_taps)), _capi.ptr(branch_scale), compound_coef,
                                                                 size, B, g_flat.data_ptr(), _capi.ptr(g_img), ws.data_ptr(), ws.numel(), sync.ref(), stream))
        return g_flat, g_img
    _capi.check(_capi.lib().hep_backbone_backward_device_bn(flat.data_ptr(), _capi.ptr_array(list(grad_taps)), _capi.ptr(branch_scale), compound_coef,
                                                            size, B, g_flat.data_ptr(), _capi.ptr(g_img), ws.data_ptr(), ws.numel(), bn_mode, stream))
    return g_flat, g_img


def stage_views(ws: torch.Tensor, compound_coef: int, size: int, batch: int) -> Dict[str, torch.Tensor]:
    """name -> float32 view [B, s, s, C] (NHWC) of every tensor hep_backbone_stage_info names in the workspace of a forward:
    ``stem`` and ``block{i}``, the names of ``Session.stage``."""
    return _trainable.stage_views("backbone", ws, compound_coef, size, batch)


def param_layout(compound_coef: int):
    """(total floats, [offset of every ``flat_keys`` tensor]) as the library reports them."""
    return _trainable.param_layout("backbone", compound_coef)


def draw_branch_scale(compound_coef: int, rate: float, batch: int, device) -> Optional[torch.Tensor]:
    """The drop-connect scales [blocks, B] of one training step, drawn as the reference draws them: in block order, one
    ``torch.rand([B, 1, 1, 1])`` on ``device`` per block that adds its input and has a non-zero rate
    ``rate * idx / len(blocks)``; scale = floor(keep + U) / keep with keep = 1 - that rate.  Every other entry is 1.
    None when ``rate`` is zero (nothing is drawn)."""
    if not rate:
        return None
    blocks = get_arch(compound_coef).blocks
    rows = []
    for idx, b in enumerate(blocks):
        r = rate * float(idx) / len(blocks)
        if b.skip and r:
            keep = 1 - r
            u = torch.rand([batch, 1, 1, 1], dtype=torch.float32, device=device)
            rows.append((torch.floor(keep + u) / keep).reshape(batch))
        else:
            rows.append(torch.ones(batch, dtype=torch.float32, device=device))
    return torch.stack(rows).contiguous()


class _Backbone(torch.autograd.Function):
    """The two ABI calls as one differentiable function of (flat parameters, image); the branch scales are data."""

    @staticmethod
    def forward(ctx, flat, image, phi, scale, bn_mode, stats, sync):
        taps, ws = backbone_forward(flat, image, phi, scale, bn_mode, stats=stats, sync=sync)
        ctx.save_for_backward(flat, ws, *(() if scale is None else (scale,)))
        ctx.cfg = (phi, int(image.shape[-1]), [tuple(t.shape) for t in taps], bn_mode, sync)
        return taps

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_taps):
        flat, ws, *rest = ctx.saved_tensors
        phi, size, shapes, bn_mode, sync = ctx.cfg
        gs = _trainable.cotangents(grad_taps, shapes, flat.device)
        g_flat, g_img = backbone_backward(flat, gs, ws, phi, size, rest[0] if rest else None, want_image=ctx.needs_input_grad[1], bn_mode=bn_mode,
                                         sync=sync)
        return (g_flat if ctx.needs_input_grad[0] else None, g_img, None, None, None, None, None)


class TrainableBackbone(_trainable.TrainablePart):
    """The EfficientNet trunk as an ``nn.Module`` whose parameters and buffers carry exactly the reference's ``backbone_net.*``
    keys, so that ``load_state_dict(model.state_dict(), strict=False)`` fills it.  ``forward(x)`` takes a float32 ROCm image
    batch [B, 3, S, S] (S a multiple of 128 in [128, 2048]) and gives the taps (P3, P4, P5) as float32 NCHW with a ``grad_fn``:
    HIP forward and HIP backward, gradients to every parameter and, where it requires grad, to the image.  ``TrainableNeck``
    and ``TrainableHeads`` chain behind it.  Runs on a ROCm device only (no CPU fallback).  ``batch_norm="running"`` (the default):
    BatchNorm uses the running statistics in EVERY mode, ``train()`` included; they receive no gradient and never change.
    ``batch_norm="batch"``: batch statistics in ``train()`` mode, the running statistics move.  ``drop_connect_rate`` (default
    0.0) is the reference's global rate: non-zero and in ``train()``, every forward draws fresh branch scales
    (``draw_branch_scale``); otherwise the module is deterministic."""

    NOUN, spec = "backbone", staticmethod(backbone_spec)

    def __init__(self, compound_coef: int = 0, drop_connect_rate: float = 0.0, batch_norm: str = "running", process_group=None):
        super().__init__()
        self._set_batch_norm(batch_norm, process_group)
        self.compound_coef = int(compound_coef)
        self.arch = get_arch(self.compound_coef)
        self.drop_connect_rate = float(drop_connect_rate)
        self._attach_spec(self.compound_coef)

    def draw_branch_scale(self, batch: int, device) -> Optional[torch.Tensor]:
        """The branch scales ``forward`` would draw now: None unless ``drop_connect_rate`` is non-zero and the module trains."""
        if not (self.training and self.drop_connect_rate):
            return None
        return draw_branch_scale(self.compound_coef, self.drop_connect_rate, batch, device)

    def _check_image(self, x) -> None:
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError("x must be a tensor [B, 3, S, S]")
        if x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError("x must be a float32 ROCm tensor")
        B, C, H, W = (int(v) for v in x.shape)
        if C != 3 or H != W or B < 1:
            raise ValueError(f"x has shape {tuple(x.shape)}, expected [B, 3, S, S]")
        _check_size(H)

    def forward(self, x, branch_scale: Optional[torch.Tensor] = None):
        """``branch_scale``: explicit drop-connect scales [blocks, B] (e.g. a recorded table); None: drawn as described above."""
        self._check_image(x)
        flat = self.flat_parameters()
        if flat.device != x.device:
            raise ValueError("the backbone and the image live on different devices: move the module with .to(device)")
        B = int(x.shape[0])
        if branch_scale is None:
            branch_scale = self.draw_branch_scale(B, x.device)
        else:
            if tuple(branch_scale.shape) != (len(self.arch.blocks), B):
                raise ValueError(f"branch_scale has shape {tuple(branch_scale.shape)}, expected {(len(self.arch.blocks), B)}")
            branch_scale = branch_scale.detach().to(device=x.device, dtype=torch.float32).contiguous()
        bn_mode = self._bn_mode()
        stats = torch.empty_like(flat) if bn_mode == _trainable.BN_BATCH else None
        taps = _Backbone.apply(flat, x.contiguous(), self.compound_coef, branch_scale, bn_mode, stats, self._sync_hook())
        if stats is not None:
            self._store_statistics(stats)
        return taps
