"""Trainable BiFPN neck: every cell of ``bifpn.{r}`` with a HIP forward AND backward (csrc/k_neck_grad.hip:
hep_neck_forward_device / hep_neck_backward_device) as a function of its parameters and the three backbone taps P3 / P4 / P5.

In the reference the backbone is what is loaded pretrained and frozen (backbone.py:99 ``freeze_bn``, ``init_backbone``); the
BiFPN and the heads are what a new instrument or a new camera re-fits.  With the neck trainable that loop stays on the GPU:
run the backbone once over a dataset and keep the three taps (``backbone_taps``), then per step

    taps -> HIP neck forward (TrainableNeck) -> HIP heads forward (TrainableHeads) -> training.format_translation ->
    HIP losses (training.losses) -> HIP loss backward -> HIP heads backward -> HIP neck backward -> a stock torch.optim step

and ``export_to(model)`` copies the fitted tensors back into the ``HMDEgoPose`` drop-in.

The rules are those of ``hmd_ego_pose_amd.heads``: by default BatchNorm uses its RUNNING statistics in every mode, forward and
backward (``gamma`` / ``beta`` get gradients, ``running_mean`` / ``running_var`` never change); ``batch_norm="batch"`` makes
``train()`` mode the reference's ``model.train()``: every BatchNorm (six laterals, eight nodes per cell) normalises with the
statistics of its map's ``B * s * s`` pixels and moves its running statistics (momentum 0.01), ``eval()`` stays the
running-statistics function bit for bit, and P7 of one 128-pixel image (a single row) raises ``ValueError``; fast-attention fusion
``w = relu(p) / (sum relu(p) + 1e-4)`` with ``relu'(p) = 0`` for ``p <= 0``; a max-pool window sends its gradient to its first
maximal element in row-major order of the zero-padded window.  phi 6 and 7 (plain-sum fusion) are refused.  The taps are
inputs; their gradient is available when they require grad, which is how ``hmd_ego_pose_amd.backbone.TrainableBackbone`` chains
in front of the neck.  ``batch_norm="sync"`` (with ``process_group=``): batch statistics over the rows of all replicas
(``_trainable.TrainablePart``).  Out of scope: bf16 training.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _capi, _trainable
from ._trainable import ptrs as _ptrs
from .arch import get_arch, level_sizes, param_spec


def _check_phi(compound_coef: int):
    if compound_coef in (6, 7):
        raise ValueError(f"compound_coef {compound_coef}: the trainable neck covers the fast-attention BiFPN (phi 0..5); phi 6 and 7 fuse by plain sums")
    if not 0 <= compound_coef <= 5:
        raise ValueError(f"compound_coef {compound_coef} is not supported by the trainable neck (0..5)")


def neck_spec(compound_coef: int) -> List[Tuple[str, tuple]]:
    """The ``bifpn.*`` subset of ``param_spec`` (key, shape), in the reference's state_dict order."""
    _check_phi(compound_coef)
    return [(k, s) for k, s in param_spec(compound_coef) if k.startswith("bifpn.")]


def flat_keys(compound_coef: int) -> List[Tuple[str, tuple]]:
    """The tensors of the flat fp32 parameter buffer of hep_neck_*_device, in buffer order: ``neck_spec`` without the int64
    ``num_batches_tracked`` counters."""
    return _trainable.without_counters(neck_spec(compound_coef))


def neck_forward(flat: torch.Tensor, taps: Sequence[torch.Tensor], compound_coef: int, size: int, bn_mode: int = _trainable.BN_RUNNING,
                 momentum: float = _trainable.BN_MOMENTUM, stats: torch.Tensor = None, sync=None):
    """hep_neck_forward_device_bn on the current stream.  ``flat``: the flat parameter buffer (``flat_keys`` order), ``taps``:
    three contiguous float32 NCHW tensors.  Returns (feats, workspace): the five maps [B, W, s_l, s_l] and the workspace that
    hep_neck_backward_device_bn needs (same ``bn_mode``).  ``stats`` (batch statistics): a buffer like ``flat`` whose
    running_mean / running_var elements receive the updated statistics.  No host synchronisation.  ``sync``: a ``sync.SumHook`` -
    hep_neck_forward_device_sync instead (batch statistics over all replicas; ``bn_mode`` is not read)."""
    _check_phi(compound_coef)
    dev, B, W = flat.device, int(taps[0].shape[0]), get_arch(compound_coef).fpn_w
    l = _capi.lib()
    nbytes = _capi.check(l.hep_neck_workspace_bytes_bn(compound_coef, size, B, bn_mode) if sync is None else
                         l.hep_neck_workspace_bytes_sync(compound_coef, size, B))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    feats = tuple(torch.empty((B, W, s, s), dtype=torch.float32, device=dev) for s in level_sizes(size))
    stream = torch.cuda.current_stream(dev).cuda_stream
    if sync is not None:
        sync.register(ws)
        sync.check(l.hep_neck_forward_device_sync(flat.data_ptr(), _ptrs(taps), compound_coef, size, B, _ptrs(feats), ws.data_ptr(), nbytes,
                                                  momentum, None if stats is None else stats.data_ptr(), sync.ref(), stream))
        return feats, ws
    _capi.check(l.hep_neck_forward_device_bn(flat.data_ptr(), _ptrs(taps), compound_coef, size, B, _ptrs(feats), ws.data_ptr(), nbytes,
                                             bn_mode, momentum, None if stats is None else stats.data_ptr(), stream))
    return feats, ws


def neck_backward(flat: torch.Tensor, grad_feats: Sequence[torch.Tensor], ws: torch.Tensor, compound_coef: int, size: int, tap_shapes=None,
                  bn_mode: int = _trainable.BN_RUNNING, sync=None):
    """hep_neck_backward_device_bn on the current stream, after ``neck_forward`` with the same ``flat``, ``ws`` and ``bn_mode``.  Returns
    (grad_flat, grad_taps): the parameter gradients in the layout of ``flat`` (running statistics zero) and the three tap
    gradients (None when ``tap_shapes`` is None: the ABI then gets NULL and skips them)."""
    dev, B = flat.device, int(grad_feats[0].shape[0])
    g_flat = torch.empty_like(flat)
    g_taps = None if tap_shapes is None else tuple(torch.empty(tuple(s), dtype=torch.float32, device=dev) for s in tap_shapes)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if sync is not None:               # (the forward's hook: grad_flat is this replica's contribution, to be SUMMED over the replicas)
        sync.register(ws)
        sync.check(_capi.lib().hep_neck_backward_device_sync(flat.data_ptr(), _ptrs(grad_feats), compound_coef, size, B, g_flat.data_ptr(),
                                                             _ptrs(g_taps), ws.data_ptr(), ws.numel(), sync.ref(), stream))
        return g_flat, g_taps
    _capi.check(_capi.lib().hep_neck_backward_device_bn(flat.data_ptr(), _ptrs(grad_feats), compound_coef, size, B, g_flat.data_ptr(),
                                                        _ptrs(g_taps), ws.data_ptr(), ws.numel(), bn_mode, stream))
    return g_flat, g_taps


def stage_views(ws: torch.Tensor, compound_coef: int, size: int, batch: int) -> Dict[str, torch.Tensor]:
    """name -> float32 view [B, s, s, W] (NHWC) of every tensor hep_neck_stage_info names in the workspace of a forward."""
    return _trainable.stage_views("neck", ws, compound_coef, size, batch)


class _Neck(torch.autograd.Function):
    """The two ABI calls as one differentiable function of (flat parameters, three taps)."""

    @staticmethod
    def forward(ctx, flat, phi, size, bn_mode, stats, sync, *taps):
        feats, ws = neck_forward(flat, taps, phi, size, bn_mode, stats=stats, sync=sync)
        ctx.save_for_backward(flat, ws)
        ctx.cfg = (phi, size, [tuple(t.shape) for t in taps], [tuple(f.shape) for f in feats], bn_mode, sync)
        return feats

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_feats):
        flat, ws = ctx.saved_tensors
        phi, size, tap_shapes, feat_shapes, bn_mode, sync = ctx.cfg
        gs = _trainable.cotangents(grad_feats, feat_shapes, flat.device)
        want_taps = any(ctx.needs_input_grad[6:])
        g_flat, g_taps = neck_backward(flat, gs, ws, phi, size, tap_shapes if want_taps else None, bn_mode, sync)
        return (g_flat if ctx.needs_input_grad[0] else None, None, None, None, None, None, *(g_taps if want_taps else (None,) * 3))


class TrainableNeck(_trainable.TrainablePart):
    """The BiFPN neck as an ``nn.Module`` whose parameters and buffers carry exactly the reference's ``bifpn.*`` keys, so that
    ``load_state_dict(model.state_dict(), strict=False)`` fills it.  ``forward(taps)`` takes the three backbone taps
    (P3, P4, P5: float32 NCHW, ``backbone_taps``) and gives the 5-tuple of maps ``TrainableHeads`` takes, with a ``grad_fn``:
    HIP forward and HIP backward, gradients to the parameters and, where they require grad, to the taps.  Runs on a ROCm
    device only (no CPU fallback).  ``batch_norm="running"`` (the default): BatchNorm uses the running statistics in EVERY
    mode, ``train()`` included; they receive no gradient and never change.  ``batch_norm="batch"``: batch statistics in
    ``train()`` mode, the running statistics move (see the module docstring)."""

    NOUN, spec = "BiFPN", staticmethod(neck_spec)

    def __init__(self, compound_coef: int = 0, batch_norm: str = "running", process_group=None):
        super().__init__()
        self._set_batch_norm(batch_norm, process_group)
        self.compound_coef = int(compound_coef)
        _check_phi(self.compound_coef)
        self.arch = get_arch(self.compound_coef)
        self._attach_spec(self.compound_coef)

    def _check_taps(self, taps) -> int:
        if len(taps) != 3:
            raise ValueError("taps must be the three backbone taps P3, P4, P5")
        t0 = taps[0]
        if t0.dim() != 4:
            raise ValueError("taps[0] must be [B, C3, s, s]")
        B, side = int(t0.shape[0]), int(t0.shape[2])
        size = side * 8
        if size < 128 or size > 2048 or size % 128 != 0:
            raise ValueError(f"taps[0] has side {side}: the input size must be a multiple of 128 in [128, 2048] (side a multiple of 16)")
        for i, (t, c) in enumerate(zip(taps, self.arch.tap_channels)):
            s = size // (8 << i)
            if tuple(t.shape) != (B, c, s, s):
                raise ValueError(f"taps[{i}] has shape {tuple(t.shape)}, expected {(B, c, s, s)} (phi {self.compound_coef}, size {size})")
            if not t.is_cuda or t.dtype != torch.float32:
                raise ValueError(f"taps[{i}] must be a float32 ROCm tensor")
        return size

    def forward(self, taps):
        taps = tuple(taps)
        size = self._check_taps(taps)
        flat = self.flat_parameters()
        if flat.device != taps[0].device:
            raise ValueError("the neck and the taps live on different devices: move the module with .to(device)")
        bn_mode, stats, sync = self._bn_mode(), None, self._sync_hook()
        if bn_mode == _trainable.BN_BATCH:
            rows = int(taps[0].shape[0]) * (size // 128) ** 2
            if rows < 2 and (sync is None or sync.world == 1):      # (a replica cannot know the global rows: the caller's to check)
                raise ValueError(f"batch statistics need more than 1 value per channel: P7 has {rows} row (batch {int(taps[0].shape[0])} at size {size})")
            stats = torch.empty_like(flat)
        feats = _Neck.apply(flat, self.compound_coef, size, bn_mode, stats, sync, *(t.contiguous() for t in taps))
        if stats is not None:
            self._store_statistics(stats)
        return feats


def param_layout(compound_coef: int):
    """(total floats, [offset of every ``flat_keys`` tensor]) as the library reports them."""
    return _trainable.param_layout("neck", compound_coef)


def backbone_taps(model, x: torch.Tensor):
    """The three backbone taps (P3, P4, P5) of an fp32 ``HMDEgoPose`` forward on ``x`` [B, 3, S, S], as contiguous float32
    NCHW tensors on ``x``'s device: what one saves per dataset image to fit the neck and the heads.  They are read through
    ``Session.stage("block{i}")``, i.e. a host round trip, from a session of the helper's own that keeps its intermediates
    (``FLAG_KEEP_INTERMEDIATES``); that is acceptable because it runs once per dataset, not per training step."""
    from .model import Session
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError("x must be a float32 ROCm tensor [B, 3, S, S]")
    B, size = int(x.shape[0]), int(x.shape[-1])
    s = Session(model.state_dict(), model.compound_coef, size, B, "fp32", x.device, flags=_capi.FLAG_KEEP_INTERMEDIATES)
    try:
        s.forward(x, want_features=False)
        torch.cuda.synchronize(x.device)
        return tuple(s.stage(f"block{i}", B).permute(0, 3, 1, 2).contiguous().to(x.device) for i in get_arch(model.compound_coef).taps)
    finally:
        s.close()
