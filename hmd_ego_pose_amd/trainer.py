"""One-call training step: the reference's ``train.py`` step (train.py:88-342) as plain C-ABI calls on the current stream.

``TrainableBackbone`` / ``TrainableNeck`` / ``TrainableHeads`` put the three parts of the model on the project's kernels, but every
step still builds each part's flat parameter buffer with a ``torch.cat``, lets autograd split the flat gradient back and hands
about a thousand small tensors to ``torch.optim``.  ``Trainer`` owns the flat buffers instead:

    params | grad | stats | m | v     float32 [total]: backbone | neck | heads, each part in its own ABI layout (``param_layout``),
                                      each part starting at a multiple of 4 floats
    kind                              uint8 [total]: 0 trainable, 1 running_mean / running_var, 2 frozen (padding, a frozen backbone)
    state                             the 32-byte block of hep_optim_*_device: norm, clip_coef, bias terms, step, skipped

and ``step`` is: three hep_*_forward_device_bn -> hep_transformation_pack_device -> hep_losses_device ->
hep_losses_backward_device (constant upstream gradient ``weight_k * scale_k / B``) -> hep_transformation_unpack_grad_device ->
heads / neck / backbone backward -> hep_optim_grad_norm_device -> hep_optim_update_device (csrc/k_train.hip).  No autograd, no
``cat``, no ``split``; after the first call of a shape a step allocates nothing and never synchronises with the host (with
``drop_connect_rate`` > 0 the table of the step is drawn with torch, ``backbone.draw_branch_scale``: one small tensor per block from the
caching allocator - the default rate 0.0 draws nothing).  The three
``Trainable*`` modules are not touched by any of this: they stay the yardstick of the new path (tests/test_gpu_trainer.py).

Data-parallel: ``Trainer(..., batch_norm="sync", process_group=pg)`` on every rank of a ``torch.distributed`` group, each rank
stepping on its shard (``dist.shard_range``) of the global batch.  The forwards and backwards are the hep_*_device_sync calls:
every BatchNorm sees the rows of all ranks (``sync.SumHook``), the upstream gradient is ``weight_k * scale_k / global_batch``,
and each rank's ``grad`` is its own contribution, so ONE ``all_reduce`` of the flat buffer gives every rank the gradient of the
global-batch function - the same bits on all ranks, hence the same norm, clipping, skip decision and update.  The step equals
the single-process step on the concatenated batch up to summation order.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _capi, _trainable, backbone as _bb, heads as _hd, neck as _nk, sync as _sync, training
from .arch import NUM_ANCHORS, get_arch, level_sizes

PARTS = ("backbone", "neck", "heads")
OPTIMIZERS = {"adam": _capi.OPT_ADAM, "sgd": _capi.OPT_SGD_NESTEROV}
LOSS_WEIGHTS = (1.0, 1.0, 100.0, 0.1, 1.0)            # train.py:61-65: classification, regression, rotation, translation, hand
STATE_BYTES = 32
HEAD_K = (4, None, 3, 3, 63)                          # regression, classification (num_classes), rotation, translation raw, hand
NUM_ROTATION = 3


def combined_layout(compound_coef: int, num_classes: int = 1, freeze_backbone: bool = False):
    """The flat buffer of the whole model: dict(total, parts {name: (offset, count)}, entries [(key, shape, offset)], kind uint8
    [total]).  Every part keeps its own ABI layout (``param_layout``) and starts at a multiple of 4 floats; ``total`` is the padded
    sum.  kind: 1 for ``running_mean`` / ``running_var``, 2 for padding and - with ``freeze_backbone`` - every backbone element,
    0 for the rest.  Host only (the library's layout calls need no device)."""
    _nk._check_phi(int(compound_coef))
    specs = {"backbone": (_bb.flat_keys(compound_coef), _bb.param_layout(compound_coef)),
             "neck": (_nk.flat_keys(compound_coef), _nk.param_layout(compound_coef)),
             "heads": (_hd.flat_keys(compound_coef, num_classes), _hd.param_layout(compound_coef, num_classes))}
    parts, entries, base = {}, [], 0
    for name in PARTS:
        keys, (count, offsets) = specs[name]
        assert len(keys) == len(offsets)
        parts[name] = (base, count)
        entries += [(k, tuple(s), base + o) for (k, s), o in zip(keys, offsets)]
        base += (count + 3) // 4 * 4
    kind = np.full((base,), _capi.PK_FROZEN, np.uint8)
    for k, s, o in entries:
        n = int(np.prod(s)) if len(s) else 1
        frozen = freeze_backbone and k.startswith(_bb.PREFIX)
        kind[o:o + n] = _capi.PK_FROZEN if frozen else _capi.PK_STAT if k.endswith(("running_mean", "running_var")) else _capi.PK_TRAIN
    return dict(total=base, parts=parts, entries=entries, kind=kind)


class PlateauSchedule:
    """The learning-rate rule of the reference's epoch tail, train.py:107-109 and :276 - ``ReduceLROnPlateau(mode='min', factor=0.5,
    patience=15, threshold=1e-4, threshold_mode='rel', cooldown=0, min_lr=1e-7, eps=1e-8)`` - restated on the host with no optimiser
    behind it (``Trainer`` keeps its rate in ``Trainer.lr``): ``tr.lr = sched.step(res["mixed_distance_mean"])``.

    ``step(metric)``: a metric below ``best * (1 - threshold)`` becomes the best and clears the count of bad epochs; any other (a NaN
    included) adds one.  More than ``patience`` bad epochs in a row: ``lr = max(lr * factor, min_lr)`` - unless that lowers the rate
    by ``eps`` or less, then it stays - and the count starts again.  Exactly torch's arithmetic (tests/test_score_cpu.py)."""

    def __init__(self, lr: float, factor: float = 0.5, patience: int = 15, threshold: float = 1e-4, min_lr: float = 1e-7, eps: float = 1e-8):
        if not factor < 1.0:
            raise ValueError("PlateauSchedule: factor must be < 1.0")
        self.lr, self.factor, self.patience, self.threshold = float(lr), float(factor), int(patience), float(threshold)
        self.min_lr, self.eps = float(min_lr), float(eps)
        self.best, self.num_bad_epochs, self.last_epoch = float("inf"), 0, 0

    def step(self, metric) -> float:
        current = float(metric)
        self.last_epoch += 1
        if current < self.best * (1.0 - self.threshold):
            self.best, self.num_bad_epochs = current, 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            new_lr = max(self.lr * self.factor, self.min_lr)
            if self.lr - new_lr > self.eps:
                self.lr = new_lr
            self.num_bad_epochs = 0
        return self.lr

    def state_dict(self) -> Dict[str, float]:
        return dict(lr=self.lr, best=self.best, num_bad_epochs=self.num_bad_epochs, last_epoch=self.last_epoch)

    def load_state_dict(self, sd) -> None:
        self.lr, self.best = float(sd["lr"]), float(sd["best"])
        self.num_bad_epochs, self.last_epoch = int(sd["num_bad_epochs"]), int(sd["last_epoch"])


class _Shape:
    """Everything one (size, batch, hand) needs, allocated once."""


class Trainer:
    """The whole model's training state in flat device buffers and ``step``, the reference's training step in one call.

    ``Trainer.from_model(model, optimizer="adam" | "sgd", lr=..., batch_norm="batch" | "running", max_grad_norm=None,
    drop_connect_rate=0.0, freeze_backbone=False, loss_weights=(1, 1, 100, 0.1, 1))``.  "adam": ``torch.optim.Adam``'s defaults
    (train.py:100); "sgd": ``SGD(momentum=0.9, nesterov=True)`` (train.py:103).  ``max_grad_norm``: ``clip_grad_norm_`` over every
    trainable element (train.py:210).  A step whose gradient norm is not finite changes nothing and counts in ``steps_skipped``.
    ``batch_norm`` as the three modules define it; ``freeze_backbone`` runs the trunk with its running statistics, skips its
    backward and leaves every one of its elements bit-unchanged.  phi 0..5 (the neck's range).  ROCm device only.

    ``process_group`` (a ``torch.distributed`` group; every rank builds the same trainer): data-parallel steps.  With
    ``batch_norm="sync"`` the step is the single-process step on the concatenated batch; with "running" it is plain gradient
    averaging; "batch" is refused (the running statistics of the ranks would drift apart).  The constructor and
    ``load_state_dict`` broadcast ``params``, ``m``, ``v`` and ``state`` from rank 0.  The drop-connect table stays per-rank local.
    ``batch_norm="sync"`` always names its replicas: ``process_group=sync.LOCAL`` is this process alone - no group, "batch" bit for
    bit, ``torch.distributed`` never imported; ``batch_norm="sync"`` without ``process_group`` raises ``ValueError``."""

    def __init__(self, state_dict, compound_coef: int = 0, num_classes: int = 1, device=None, optimizer: str = "adam", lr: float = 1e-4,
                 batch_norm: str = "batch", max_grad_norm: Optional[float] = None, drop_connect_rate: float = 0.0,
                 freeze_backbone: bool = False, loss_weights=LOSS_WEIGHTS, betas=(0.9, 0.999), eps: float = 1e-8, momentum: float = 0.9,
                 process_group=None):
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be 'adam' or 'sgd', not {optimizer!r}")
        if batch_norm not in _trainable.BN_NAMES:
            raise ValueError(f"batch_norm must be 'running', 'batch' or 'sync', not {batch_norm!r}")
        if batch_norm == _trainable.BN_SYNC and process_group is None:
            raise ValueError("batch_norm='sync' takes process_group=: a torch.distributed group, or sync.LOCAL for this process alone "
                             "(then it is batch_norm='batch' bit for bit)")
        if isinstance(process_group, str):
            if process_group != _sync.LOCAL:
                raise ValueError(f"process_group must be a torch.distributed group, sync.LOCAL or None, not {process_group!r}")
            process_group = None
        if process_group is not None and batch_norm == "batch":
            raise ValueError("process_group with batch_norm='batch': every rank would move its running statistics with its own shard "
                             "and they would drift apart - use batch_norm='sync' (or 'running' for plain gradient averaging)")
        if len(loss_weights) != 5:
            raise ValueError("loss_weights: five values (classification, regression, rotation, translation, hand)")
        self.compound_coef, self.num_classes = int(compound_coef), int(num_classes)
        self.arch = get_arch(self.compound_coef)
        lay = combined_layout(self.compound_coef, self.num_classes, freeze_backbone)
        self.total, self.parts, self.entries = lay["total"], lay["parts"], lay["entries"]
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise ValueError("the trainer runs on a ROCm device only (no CPU fallback)")
        self.device = dev
        self.optimizer, self.lr, self.batch_norm = optimizer, float(lr), batch_norm
        self.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        self.drop_connect_rate, self.freeze_backbone = float(drop_connect_rate), bool(freeze_backbone)
        self.loss_weights = tuple(float(w) for w in loss_weights)
        self.beta1, self.beta2 = (float(betas[0]), float(betas[1])) if optimizer == "adam" else (float(momentum), 0.0)
        self.eps = float(eps)
        missing = [k for k, _, _ in self.entries if k not in state_dict]
        if missing:
            raise KeyError(f"the state_dict lacks {missing[0]}")
        host = np.zeros((self.total,), np.float32)
        for k, s, o in self.entries:
            a = state_dict[k].detach().to("cpu", torch.float32).numpy().reshape(-1)
            if a.size != (int(np.prod(s)) if len(s) else 1):
                raise ValueError(f"{k} has {a.size} elements, expected shape {s}")
            host[o:o + a.size] = a
        z = lambda: torch.zeros((self.total,), dtype=torch.float32, device=dev)
        self.params = torch.from_numpy(host).to(dev)
        self.grad, self.stats, self.m = z(), z(), z()                  # grad zero once: a frozen backbone's slice is never written
        self.v = z() if optimizer == "adam" else None
        self.kind = torch.from_numpy(lay["kind"]).to(dev)
        self.state = torch.zeros((STATE_BYTES,), dtype=torch.uint8, device=dev)
        nws = _capi.check(_capi.lib().hep_optim_workspace_bytes(self.total))
        self._optim_ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
        self._weights = torch.tensor(self.loss_weights, dtype=torch.float32).to(dev)
        self._shapes: Dict[tuple, _Shape] = {}
        self._exported = 0                                             # steps already added to a model's num_batches_tracked
        self.process_group = process_group
        self.world, self.rank = _sync.group_world(process_group), _sync.group_rank(process_group)
        self._hook = _sync.SumHook(process_group) if batch_norm == _trainable.BN_SYNC else None
        self._broadcast()

    def _broadcast(self):
        """Rank 0's ``params``, ``m``, ``v`` and ``state`` into every rank's (nothing without a group)."""
        for t in (self.params, self.m, self.v, self.state):
            if t is not None:
                _sync.broadcast(t, self.process_group, 0)

    @classmethod
    def from_model(cls, model, **kwargs):
        """A trainer with the tensors of an ``HMDEgoPose`` (or any module with the reference's keys), on the model's device."""
        sd = model.state_dict()
        return cls(sd, model.compound_coef, getattr(model, "num_classes", 1), next(iter(sd.values())).device, **kwargs)

    # ---- views -------------------------------------------------------------------------------------------------------
    def _views(self, flat) -> Dict[str, torch.Tensor]:
        return {k: flat[o:o + (int(np.prod(s)) if len(s) else 1)].view(s) for k, s, o in self.entries}

    def named_views(self) -> Dict[str, torch.Tensor]:
        """The reference's keys (without the int64 counters) as views into ``params``."""
        return self._views(self.params)

    def grad_views(self) -> Dict[str, torch.Tensor]:
        """The same keys as views into ``grad`` (the gradient of the last step, before clipping)."""
        return self._views(self.grad)

    def part(self, flat, name) -> torch.Tensor:
        o, n = self.parts[name]
        return flat[o:o + n]

    # ---- the state block (these synchronise) -------------------------------------------------------------------------------
    def _state(self):
        raw = self.state.cpu().numpy()
        return raw[:16].view(np.float32), raw[16:24].view(np.int32)

    @property
    def grad_norm(self) -> float:
        return float(self._state()[0][0])

    @property
    def steps_taken(self) -> int:
        return int(self._state()[1][0])

    @property
    def steps_skipped(self) -> int:
        return int(self._state()[1][1])

    # ---- per-shape buffers ---------------------------------------------------------------------------------------------------
    def _bn_modes(self):
        """The BatchNorm mode of backbone, neck, heads ("sync" is HEP_BN_BATCH through the hep_*_device_sync calls)."""
        mode = _trainable.BN_BATCH if self.batch_norm == _trainable.BN_SYNC else _trainable.BN_MODES[self.batch_norm]
        return (_trainable.BN_RUNNING if self.freeze_backbone else mode), mode, mode

    def _shape(self, size: int, B: int, hand: bool, global_batch: Optional[int] = None) -> _Shape:
        G = B * self.world if global_batch is None else int(global_batch)
        if G < B or (self.world == 1 and G != B):
            raise ValueError(f"global_batch {G} with a local batch of {B} on {self.world} rank(s)")
        key = (size, B, hand, G)
        c = self._shapes.get(key)
        if c is not None:
            return c
        _bb._check_size(size)
        phi, K, dev, l = self.compound_coef, self.num_classes, self.device, _capi.lib()
        modes = self._bn_modes()
        if _trainable.BN_BATCH in modes and G * (size // 128) ** 2 < 2:
            raise ValueError(f"batch statistics need more than 1 value per channel: P7 has {G * (size // 128) ** 2} row (batch {G} at size {size})")
        c = _Shape()
        c.G = G
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        ws = lambda n: torch.empty((_capi.check(n),), dtype=torch.uint8, device=dev)
        W, N = self.arch.fpn_w, NUM_ANCHORS * sum(s * s for s in level_sizes(size))
        c.N = N
        if self._hook is None:
            c.ws = (ws(l.hep_backbone_workspace_bytes_bn(phi, size, B, modes[0])), ws(l.hep_neck_workspace_bytes_bn(phi, size, B, modes[1])),
                    ws(l.hep_heads_workspace_bytes_bn(phi, K, size, B, modes[2])))
        else:                                                          # (a frozen backbone runs its running statistics: the _bn call)
            c.ws = (ws(l.hep_backbone_workspace_bytes_bn(phi, size, B, modes[0]) if self.freeze_backbone else l.hep_backbone_workspace_bytes_sync(phi, size, B)),
                    ws(l.hep_neck_workspace_bytes_sync(phi, size, B)), ws(l.hep_heads_workspace_bytes_sync(phi, K, size, B)))
        tap_shapes = [(B, ch, size // (8 << t), size // (8 << t)) for t, ch in enumerate(self.arch.tap_channels)]
        feat_shapes = [(B, W, s, s) for s in level_sizes(size)]
        out_k = [K if k is None else k for k in HEAD_K]
        c.taps, c.g_taps = [f(*s) for s in tap_shapes], [f(*s) for s in tap_shapes]
        c.feats, c.g_feats = [f(*s) for s in feat_shapes], [f(*s) for s in feat_shapes]
        c.outs = [f(B, N, k) for k in out_k]
        c.g_outs = [f(B, N, k) for k in out_k]                         # regression, classification, rotation, translation raw, hand
        if not hand:
            c.g_outs[4].zero_()                                        # no hand targets: the hand cotangent is this persistent zero
        c.transformation, c.g_transformation = f(B, N, NUM_ROTATION + 3), f(B, N, NUM_ROTATION + 3)
        c.per, c.out5, c.result = f(B, 5), f(5), f(6)
        scale = torch.tensor([w * s / G for w, s in zip(self.loss_weights, training._MEAN_SCALE)], dtype=torch.float32)
        c.upstream = scale[None].repeat(B, 1).contiguous().to(dev)
        c.loss_ws = torch.empty((B * (N + 4),), dtype=torch.int32, device=dev)
        c.anchors = training.translation_anchors(size).to(dev).contiguous()
        P = _capi.ptr_array
        c.p_taps, c.p_g_taps, c.p_feats, c.p_g_feats, c.p_outs, c.p_g_outs = P(c.taps), P(c.g_taps), P(c.feats), P(c.g_feats), P(c.outs), P(c.g_outs)
        self._shapes[key] = c
        return c

    # ---- the step --------------------------------------------------------------------------------------------------------------
    def _check(self, image, camera, gt_classification, gt_regression, gt_transformation, gt_hand, model_3d_points, global_batch=None):
        def chk(t, name, shape):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.params.device:
                raise ValueError(f"{name} must be a float32 tensor on {self.params.device}")
            if shape is not None and tuple(t.shape) != shape:
                raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {shape}")
            return t.contiguous()
        if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[1] != 3 or image.shape[2] != image.shape[3] or image.shape[0] < 1:
            raise ValueError("image must be a tensor [B, 3, S, S]")
        B, size = int(image.shape[0]), int(image.shape[-1])
        image = chk(image, "image", None)
        c = self._shape(size, B, gt_hand is not None, global_batch)
        N, K = c.N, self.num_classes
        t = (image, chk(camera, "camera", (B, 6)), chk(gt_classification, "gt_classification", (B, N, K + 1)),
             chk(gt_regression, "gt_regression", (B, N, 5)), chk(gt_transformation, "gt_transformation", (B, N, NUM_ROTATION + 6)),
             None if gt_hand is None else chk(gt_hand, "gt_hand", (B, N, 64)), chk(model_3d_points, "model_3d_points", None))
        pts = t[6]
        if pts.dim() != 3 or pts.shape[2] != 3 or not 1 <= pts.shape[1] <= 2048:
            raise ValueError("model_3d_points must be [classes, P, 3] with P in 1..2048")
        return c, B, size, t

    def step(self, image, camera, gt_classification, gt_regression, gt_transformation, gt_hand, model_3d_points, global_batch: Optional[int] = None):
        """One training step on the current stream.  ``image`` [B, 3, S, S], ``camera`` [B, 6], the targets as
        ``training.anchor_targets`` returns them (``gt_hand`` [B, N, 64] or None), ``model_3d_points`` [classes, P, 3]: float32
        tensors on the trainer's device.  Raises ``ValueError`` before any pointer reaches the ABI.  Returns a float32 [6] device
        tensor: the five weighted losses and their sum, in the order of train.py:70.  It is the trainer's own buffer of this
        shape: the next step overwrites it (``.clone()`` what has to last).  With a process group: ``image`` and the targets are
        this rank's shard, ``global_batch`` the images of all ranks in this step (default ``B * world``: even shards); the losses
        returned are those of the global batch, the same on every rank."""
        c, B, size, (image, camera, gt_cls, gt_reg, gt_tr, gt_hand, pts) = self._check(image, camera, gt_classification, gt_regression,
                                                                                         gt_transformation, gt_hand, model_3d_points, global_batch)
        l, check, ptr = _capi.lib(), _capi.check, _capi.ptr
        phi, K, N, R = self.compound_coef, self.num_classes, c.N, NUM_ROTATION
        stream = torch.cuda.current_stream(self.device).cuda_stream
        m_bb, m_nk, m_hd = self._bn_modes()
        batch_stats = self.batch_norm in ("batch", _trainable.BN_SYNC)
        mom = _trainable.BN_MOMENTUM
        par = {n: self.part(self.params, n).data_ptr() for n in PARTS}
        grd = {n: self.part(self.grad, n).data_ptr() for n in PARTS}
        sts = {n: (self.part(self.stats, n).data_ptr() if batch_stats and not (n == "backbone" and self.freeze_backbone) else None) for n in PARTS}
        scale = None if self.freeze_backbone else _bb.draw_branch_scale(phi, self.drop_connect_rate, B, self.device)
        hook = self._hook
        # 1. forward
        if hook is None:
            check(l.hep_backbone_forward_device_bn(par["backbone"], image.data_ptr(), ptr(scale), phi, size, B, c.p_taps, c.ws[0].data_ptr(),
                                                   c.ws[0].numel(), m_bb, mom, sts["backbone"], stream))
            check(l.hep_neck_forward_device_bn(par["neck"], c.p_taps, phi, size, B, c.p_feats, c.ws[1].data_ptr(), c.ws[1].numel(), m_nk, mom,
                                               sts["neck"], stream))
            check(l.hep_heads_forward_device_bn(par["heads"], c.p_feats, phi, K, size, B, c.p_outs, c.ws[2].data_ptr(), c.ws[2].numel(), m_hd, mom,
                                                sts["heads"], stream))
        else:
            hook.register(*c.ws)
            check, ref = hook.check, hook.ref()
            if self.freeze_backbone:
                check(l.hep_backbone_forward_device_bn(par["backbone"], image.data_ptr(), ptr(scale), phi, size, B, c.p_taps, c.ws[0].data_ptr(),
                                                       c.ws[0].numel(), m_bb, mom, sts["backbone"], stream))
            else:
                check(l.hep_backbone_forward_device_sync(par["backbone"], image.data_ptr(), ptr(scale), phi, size, B, c.p_taps, c.ws[0].data_ptr(),
                                                         c.ws[0].numel(), mom, sts["backbone"], ref, stream))
            check(l.hep_neck_forward_device_sync(par["neck"], c.p_taps, phi, size, B, c.p_feats, c.ws[1].data_ptr(), c.ws[1].numel(), mom,
                                                 sts["neck"], ref, stream))
            check(l.hep_heads_forward_device_sync(par["heads"], c.p_feats, phi, K, size, B, c.p_outs, c.ws[2].data_ptr(), c.ws[2].numel(), mom,
                                                  sts["heads"], ref, stream))
        reg, cls, rot, raw, hand = c.outs
        # 2. - 5. pack, losses, their backward, unpack
        check(l.hep_transformation_pack_device(rot.data_ptr(), raw.data_ptr(), camera.data_ptr(), c.anchors.data_ptr(), B, N, R,
                                               c.transformation.data_ptr(), stream))
        H = 63 if gt_hand is not None else 0
        p_hand, g_hand = (hand.data_ptr(), c.g_outs[4].data_ptr()) if H else (None, None)
        loss_in = (gt_cls.data_ptr(), cls.data_ptr(), gt_reg.data_ptr(), reg.data_ptr(), gt_tr.data_ptr(), c.transformation.data_ptr(),
                   ptr(gt_hand), p_hand, pts.data_ptr(), B, N, K, R, H, int(pts.shape[0]), int(pts.shape[1]))
        check(l.hep_losses_device(*loss_in, c.per.data_ptr(), c.out5.data_ptr(), stream))
        check(l.hep_losses_backward_device(*loss_in, c.upstream.data_ptr(), c.g_outs[1].data_ptr(), c.g_outs[0].data_ptr(),
                                           c.g_transformation.data_ptr(), g_hand, c.loss_ws.data_ptr(), stream))
        check(l.hep_transformation_unpack_grad_device(c.g_transformation.data_ptr(), raw.data_ptr(), camera.data_ptr(), c.anchors.data_ptr(),
                                                      B, N, R, c.g_outs[2].data_ptr(), c.g_outs[3].data_ptr(), stream))
        # 6. backward of the parts
        if hook is None:
            check(l.hep_heads_backward_device_bn(par["heads"], c.p_g_outs, phi, K, size, B, grd["heads"], c.p_g_feats, c.ws[2].data_ptr(),
                                                 c.ws[2].numel(), m_hd, stream))
            check(l.hep_neck_backward_device_bn(par["neck"], c.p_g_feats, phi, size, B, grd["neck"], None if self.freeze_backbone else c.p_g_taps,
                                                c.ws[1].data_ptr(), c.ws[1].numel(), m_nk, stream))
            if not self.freeze_backbone:
                check(l.hep_backbone_backward_device_bn(par["backbone"], c.p_g_taps, ptr(scale), phi, size, B, grd["backbone"], None,
                                                        c.ws[0].data_ptr(), c.ws[0].numel(), m_bb, stream))
        else:
            check(l.hep_heads_backward_device_sync(par["heads"], c.p_g_outs, phi, K, size, B, grd["heads"], c.p_g_feats, c.ws[2].data_ptr(),
                                                   c.ws[2].numel(), ref, stream))
            check(l.hep_neck_backward_device_sync(par["neck"], c.p_g_feats, phi, size, B, grd["neck"], None if self.freeze_backbone else c.p_g_taps,
                                                  c.ws[1].data_ptr(), c.ws[1].numel(), ref, stream))
            if not self.freeze_backbone:
                check(l.hep_backbone_backward_device_sync(par["backbone"], c.p_g_taps, ptr(scale), phi, size, B, grd["backbone"], None,
                                                          c.ws[0].data_ptr(), c.ws[0].numel(), ref, stream))
            check = _capi.check
        # every rank's grad is its own contribution to the gradient of the global-batch function: one collective over the flat buffer
        _sync.all_reduce_sum(self.grad, self.process_group)
        # 7. - 8. norm and update
        opt = OPTIMIZERS[self.optimizer]
        check(l.hep_optim_grad_norm_device(self.grad.data_ptr(), self.kind.data_ptr(), self.total, opt, self.beta1, self.beta2, self.max_grad_norm,
                                           self.state.data_ptr(), self._optim_ws.data_ptr(), self._optim_ws.numel(), stream))
        check(l.hep_optim_update_device(self.params.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(), ptr(self.v),
                                        self.stats.data_ptr() if batch_stats else None, self.kind.data_ptr(), self.total, opt, self.lr,
                                        self.beta1, self.beta2, self.eps, self.state.data_ptr(), stream))
        torch.mul(c.out5, self._weights, out=c.result[:5])
        if self.world > 1:                                             # this rank's five batch means -> the global batch's, one small collective
            c.result[:5].mul_(B / c.G)
            _sync.all_reduce_sum(c.result[:5], self.process_group)
        torch.sum(c.result[:5], dim=0, keepdim=True, out=c.result[5:])
        return c.result

    @torch.no_grad()
    def forward_eval(self, image):
        """The five head outputs (regression, classification, rotation, translation raw, hand) of the CURRENT parameters with the
        running statistics - the function an exported model serves.  Fresh tensors; changes nothing."""
        if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.dtype != torch.float32 or image.device != self.params.device:
            raise ValueError(f"image must be a float32 tensor [B, 3, S, S] on {self.params.device}")
        phi, K = self.compound_coef, self.num_classes
        taps, _ = _bb.backbone_forward(self.part(self.params, "backbone"), image.contiguous(), phi)
        feats, _ = _nk.neck_forward(self.part(self.params, "neck"), taps, phi, int(image.shape[-1]))
        outs, _ = _hd.heads_forward(self.part(self.params, "heads"), feats, phi, K, int(image.shape[-1]))
        return outs

    # ---- out of the trainer ---------------------------------------------------------------------------------------------------
    def export_to(self, model):
        """Copy every tensor into ``model`` (an ``HMDEgoPose``), add the steps taken since the last export to every
        ``num_batches_tracked`` (a frozen backbone's stay) and drop the model's packed device weights."""
        dst = model.state_dict()
        taken = self.steps_taken
        with torch.no_grad():
            for k, v in self.named_views().items():
                dst[k].copy_(v)
            for k, t in dst.items():
                if k.endswith("num_batches_tracked") and not (self.freeze_backbone and k.startswith(_bb.PREFIX)):
                    t.add_(taken - self._exported)
        self._exported = taken
        model.invalidate()
        return model

    def state_dict(self):
        """What resuming needs: clones of ``params``, ``m``, ``v`` (None under SGD) and the state block."""
        return dict(params=self.params.clone(), m=self.m.clone(), v=None if self.v is None else self.v.clone(), state=self.state.clone(),
                    optimizer=self.optimizer, compound_coef=self.compound_coef, num_classes=self.num_classes)

    def load_state_dict(self, sd):
        """Resume from ``state_dict()`` of a trainer of the same model and optimiser: parameters, moments and the state block (step
        count, skipped count).  The hyper-parameters are not part of the state: ``lr``, ``max_grad_norm``, the betas, ``batch_norm``
        and ``freeze_backbone`` stay those this trainer was built with."""
        if (sd["optimizer"], sd["compound_coef"], sd["num_classes"]) != (self.optimizer, self.compound_coef, self.num_classes):
            raise ValueError("the state is another trainer's (optimizer, compound_coef or num_classes differ)")
        for name, own in (("params", self.params), ("m", self.m), ("v", self.v), ("state", self.state)):
            t = sd.get(name)
            if own is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != own.dtype or tuple(t.shape) != tuple(own.shape):
                raise ValueError(f"state_dict['{name}'] must be a {own.dtype} tensor of shape {tuple(own.shape)}")
        with torch.no_grad():
            self.params.copy_(sd["params"]); self.m.copy_(sd["m"]); self.state.copy_(sd["state"])
            if self.v is not None:
                self.v.copy_(sd["v"])
        self._broadcast()
        self._exported = self.steps_taken                              # the saved steps are taken to be in the model's counters already
