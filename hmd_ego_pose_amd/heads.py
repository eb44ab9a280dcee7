"""Trainable pose heads: the five head nets (regressor, classifier, rotation_net, translation_net, hand_net) with a HIP
forward AND backward (csrc/k_head_grad.hip: hep_heads_forward_device / hep_heads_backward_device).

The heads are what the reference added to EfficientDet and what one re-fits when the tracked instrument changes.  With
them trainable the whole fitting loop stays on the GPU: run the inference path once over a dataset and keep the five
BiFPN maps (``feats``, the first value ``HMDEgoPose.forward`` returns), then per step

    HIP targets (training.anchor_targets) -> HIP heads forward (TrainableHeads) -> training.format_translation ->
    HIP losses (training.losses) -> HIP loss backward -> HIP heads backward -> a stock torch.optim step

and finally ``export_to(model)`` copies the fitted heads back into the ``HMDEgoPose`` drop-in.

BatchNorm, by default (``batch_norm="running"``): RUNNING statistics in every mode (``train()`` and ``eval()`` compute the
same function), in forward and backward - frozen-statistics fine-tuning, the reference's ``freeze_bn`` (backbone.py:99).  That
is the gradient of the function the inference path computes, so "train here, serve here" is consistent: ``gamma`` and
``beta`` get gradients, ``running_mean`` / ``running_var`` never change.
``batch_norm="batch"`` is ``nn.BatchNorm2d(momentum=0.01, eps=1e-3)`` as the reference's train.py:162 (``model.train()``)
runs it: in ``train()`` mode every ``bn_list.{level}.{i}`` normalises with the mean and biased variance of its level's
``B * s * s`` pixels, the backward is that function's, and each forward (under ``torch.no_grad()`` or not) moves
``running_mean`` / ``running_var`` in place and adds one to every ``num_batches_tracked``; in ``eval()`` mode it is the
running-statistics function, bit for bit.  A level with fewer than 2 rows (size 128 with batch 1) raises ``ValueError``, as
torch does.  ``batch_norm="sync"`` (with ``process_group=``) is "batch" over the rows of all replicas of a data-parallel step
(``_trainable.TrainablePart``, ``trainer.Trainer``).  ``export_to`` copies the buffers, so the fitted statistics reach the
inference session.  Out of scope: bf16 training (the BiFPN and the backbone in front of the heads are trainable too:
``hmd_ego_pose_amd.neck.TrainableNeck``, ``hmd_ego_pose_amd.backbone.TrainableBackbone``).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _capi, _trainable
from ._trainable import ptrs as _ptrs
from .arch import HEAD_NAMES, NUM_ANCHORS, get_arch, level_sizes, param_spec


def head_spec(compound_coef: int, num_classes: int = 1) -> List[Tuple[str, tuple]]:
    """The head subset of ``param_spec`` (key, shape), in the reference's state_dict order."""
    return [(k, s) for k, s in param_spec(compound_coef, num_classes) if k.split(".", 1)[0] in HEAD_NAMES]


def flat_keys(compound_coef: int, num_classes: int = 1) -> List[Tuple[str, tuple]]:
    """The tensors of the flat fp32 parameter buffer of hep_heads_*_device, in buffer order: ``head_spec`` without the
    int64 ``num_batches_tracked`` counters."""
    return _trainable.without_counters(head_spec(compound_coef, num_classes))


def heads_forward(flat: torch.Tensor, feats: Sequence[torch.Tensor], compound_coef: int, num_classes: int, size: int,
                  bn_mode: int = _trainable.BN_RUNNING, momentum: float = _trainable.BN_MOMENTUM, stats: torch.Tensor = None, sync=None):
    """hep_heads_forward_device_bn on the current stream.  ``flat``: the flat parameter buffer (``flat_keys`` order),
    ``feats``: five contiguous float32 NCHW maps.  Returns (outs, workspace): the five [B, N, K] outputs and the workspace
    that hep_heads_backward_device_bn needs (same ``bn_mode``).  ``stats`` (batch statistics): a buffer like ``flat`` whose
    running_mean / running_var elements receive the updated statistics.  No host synchronisation.  ``sync``: a
    ``sync.SumHook`` - hep_heads_forward_device_sync instead (batch statistics over all replicas; ``bn_mode`` is not read)."""
    dev, B = flat.device, int(feats[0].shape[0])
    N = NUM_ANCHORS * sum(s * s for s in level_sizes(size))
    l = _capi.lib()
    nbytes = _capi.check(l.hep_heads_workspace_bytes_bn(compound_coef, num_classes, size, B, bn_mode) if sync is None else
                         l.hep_heads_workspace_bytes_sync(compound_coef, num_classes, size, B))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    outs = tuple(torch.empty((B, N, k), dtype=torch.float32, device=dev) for k in (4, num_classes, 3, 3, 63))
    stream = torch.cuda.current_stream(dev).cuda_stream
    if sync is not None:
        sync.register(ws)
        sync.check(l.hep_heads_forward_device_sync(flat.data_ptr(), _ptrs(feats), compound_coef, num_classes, size, B, _ptrs(outs), ws.data_ptr(),
                                                   nbytes, momentum, None if stats is None else stats.data_ptr(), sync.ref(), stream))
        return outs, ws
    _capi.check(l.hep_heads_forward_device_bn(flat.data_ptr(), _ptrs(feats), compound_coef, num_classes, size, B, _ptrs(outs),
                                              ws.data_ptr(), nbytes, bn_mode, momentum, None if stats is None else stats.data_ptr(), stream))
    return outs, ws


def heads_backward(flat: torch.Tensor, grad_outs: Sequence[torch.Tensor], ws: torch.Tensor, compound_coef: int, num_classes: int,
                   size: int, feat_shapes=None, bn_mode: int = _trainable.BN_RUNNING, sync=None):
    """hep_heads_backward_device_bn on the current stream, after ``heads_forward`` with the same ``flat``, ``ws`` and ``bn_mode``.
    Returns (grad_flat, grad_feats): the parameter gradients in the layout of ``flat`` (running statistics zero) and the
    five map gradients (None when ``feat_shapes`` is None: the ABI then gets NULL and skips them)."""
    dev, B = flat.device, int(grad_outs[0].shape[0])
    g_flat = torch.empty_like(flat)
    g_feats = None if feat_shapes is None else tuple(torch.empty(tuple(s), dtype=torch.float32, device=dev) for s in feat_shapes)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if sync is not None:               # (the forward's hook: grad_flat is this replica's contribution, to be SUMMED over the replicas)
        sync.register(ws)
        sync.check(_capi.lib().hep_heads_backward_device_sync(flat.data_ptr(), _ptrs(grad_outs), compound_coef, num_classes, size, B,
                                                              g_flat.data_ptr(), _ptrs(g_feats), ws.data_ptr(), ws.numel(), sync.ref(), stream))
        return g_flat, g_feats
    _capi.check(_capi.lib().hep_heads_backward_device_bn(flat.data_ptr(), _ptrs(grad_outs), compound_coef, num_classes, size, B,
                                                         g_flat.data_ptr(), _ptrs(g_feats), ws.data_ptr(), ws.numel(), bn_mode, stream))
    return g_flat, g_feats


class _Heads(torch.autograd.Function):
    """The two ABI calls as one differentiable function of (flat parameters, five maps)."""

    @staticmethod
    def forward(ctx, flat, phi, num_classes, size, bn_mode, stats, sync, *feats):
        outs, ws = heads_forward(flat, feats, phi, num_classes, size, bn_mode, stats=stats, sync=sync)
        ctx.save_for_backward(flat, ws)
        ctx.cfg = (phi, num_classes, size, [tuple(f.shape) for f in feats], bn_mode, sync)
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outs):
        flat, ws = ctx.saved_tensors
        phi, num_classes, size, shapes, bn_mode, sync = ctx.cfg
        N = NUM_ANCHORS * sum(s * s for s in level_sizes(size))
        B = shapes[0][0]
        gs = _trainable.cotangents(grad_outs, [(B, N, k) for k in (4, num_classes, 3, 3, 63)], flat.device)
        want_feats = any(ctx.needs_input_grad[7:])
        g_flat, g_feats = heads_backward(flat, gs, ws, phi, num_classes, size, shapes if want_feats else None, bn_mode, sync)
        return (g_flat if ctx.needs_input_grad[0] else None, None, None, None, None, None, None, *(g_feats if want_feats else (None,) * 5))


class TrainableHeads(_trainable.TrainablePart):
    """The five head nets as an ``nn.Module`` whose parameters and buffers carry exactly the reference's head keys
    (``regressor.conv_list.0.depthwise_conv.conv.weight`` ... ``hand_net.bn_list.4.2.running_var``), so that
    ``load_state_dict(model.state_dict(), strict=False)`` fills it.  ``forward(feats)`` takes the 5-tuple of BiFPN maps
    that ``HMDEgoPose.forward`` returns first and gives (regression, classification, rotation, translation_raw, hand) with
    a ``grad_fn``: HIP forward and HIP backward, gradients to the parameters and, where they require grad, to the maps.
    Runs on a ROCm device only (no CPU fallback).  ``batch_norm="running"`` (the default): BatchNorm uses the running
    statistics in EVERY mode, ``train()`` included; they receive no gradient and never change.  ``batch_norm="batch"``:
    batch statistics in ``train()`` mode, the running statistics move (see the module docstring)."""

    NOUN, spec = "head", staticmethod(head_spec)

    def __init__(self, compound_coef: int = 0, num_classes: int = 1, batch_norm: str = "running", process_group=None):
        super().__init__()
        self._set_batch_norm(batch_norm, process_group)
        self.compound_coef = int(compound_coef)
        self.num_classes = int(num_classes)
        self.arch = get_arch(self.compound_coef)
        self._attach_spec(self.compound_coef, self.num_classes)

    @classmethod
    def _model_cfg(cls, model):
        return (model.compound_coef, model.num_classes)

    def _check_feats(self, feats):
        if len(feats) != 5:
            raise ValueError("feats must be the five BiFPN maps P3..P7")
        f0 = feats[0]
        if f0.dim() != 4:
            raise ValueError("feats[0] must be [B, W, s, s]")
        B, W, side = int(f0.shape[0]), self.arch.fpn_w, int(f0.shape[2])
        size = side * 8
        if size < 128 or size % 128 != 0:
            raise ValueError(f"feats[0] has side {side}: the input size must be a multiple of 128 (side a multiple of 16)")
        for l, (f, s) in enumerate(zip(feats, level_sizes(size))):
            if tuple(f.shape) != (B, W, s, s):
                raise ValueError(f"feats[{l}] has shape {tuple(f.shape)}, expected {(B, W, s, s)} (phi {self.compound_coef}, size {size})")
            if not f.is_cuda or f.dtype != torch.float32:
                raise ValueError(f"feats[{l}] must be a float32 ROCm tensor")
        return size

    def forward(self, feats):
        feats = tuple(feats)
        size = self._check_feats(feats)
        flat = self.flat_parameters()
        if flat.device != feats[0].device:
            raise ValueError("the heads and the maps live on different devices: move the module with .to(device)")
        bn_mode, stats, sync = self._bn_mode(), None, self._sync_hook()
        if bn_mode == _trainable.BN_BATCH:
            rows = int(feats[4].shape[0]) * int(feats[4].shape[2]) ** 2
            if rows < 2 and (sync is None or sync.world == 1):      # (a replica cannot know the global rows: the caller's to check)
                raise ValueError(f"batch statistics need more than 1 value per channel: the top level has {rows} row (batch "
                                 f"{int(feats[4].shape[0])} at size {size})")
            stats = torch.empty_like(flat, requires_grad=False)
        outs = _Heads.apply(flat, self.compound_coef, self.num_classes, size, bn_mode, stats, sync, *(f.contiguous() for f in feats))
        if stats is not None:
            self._store_statistics(stats)
        return outs


def param_layout(compound_coef: int, num_classes: int = 1):
    """(total floats, [offset of every ``flat_keys`` tensor]) as the library reports them."""
    return _trainable.param_layout("heads", compound_coef, num_classes)
