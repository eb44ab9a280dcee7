"""Training-side ops of the reference on the GPU.

``anchor_targets`` is ``anchor_targets_bbox`` (pytorch-sandbox/generators/utils/anchors.py:69-221): the reference builds
the per-batch classification / regression / transformation / hand targets on the host with numpy and a Cython IoU matrix
(generators/utils/compute_overlap.pyx:33-73); here the assignment runs in one kernel (csrc/k_eval.hip,
hep_anchor_targets_device) and its outputs stay on the device for the losses.

``losses`` is ``batch_iterate`` (pytorch-sandbox/hmdegopose/loss.py:54-99): the focal, box, rotation (model-point
distance), translation and hand losses, one workgroup per image (hep_losses_device).  The reference computes them with a
Python loop over the batch and per-image gathers.  When a prediction requires grad the outputs carry a ``grad_fn`` whose
backward is HIP as well (csrc/k_loss_grad.hip, hep_losses_backward_device): the gradients the reference's autograd returns,
computed on the whole GPU without a host synchronisation.  ``batch_iterate`` is the drop-in with the reference's signature
and return shape.  The five head nets under these losses are trainable as well (``heads.TrainableHeads``: HIP forward and
backward, csrc/k_head_grad.hip); ``format_translation`` is the differentiable step between them (the losses take the DECODED
translation, train.py:39,49).  The BiFPN (``neck.TrainableNeck``) and the EfficientNet trunk (``backbone.TrainableBackbone``) in
front of them have a HIP forward and backward of their own as well, so image -> backbone -> neck -> heads -> losses is differentiable
end to end on the project's kernels.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _capi


def anchor_targets(anchors: torch.Tensor, boxes: Sequence[np.ndarray], labels: Sequence[np.ndarray],
                   transformation_targets: Sequence[np.ndarray], coords_3d: Optional[Sequence[np.ndarray]],
                   image_shapes: Sequence[Tuple[int, int]], num_classes: int = 1, negative_overlap: float = 0.4,
                   positive_overlap: float = 0.5):
    """anchors: float32 [N,4] on the device.  Per image: boxes [K,4] (x1,y1,x2,y2, any float dtype: used as float64 like
    the reference), labels [K], transformation targets [K,RT], coords_3d [K,63] (or None), image shape (height, width).
    Returns device tensors (labels [B,N,C+1], regression [B,N,5], transformation [B,N,RT+1], coords [B,N,64] or None);
    the last column of each is the anchor state (-1 ignore, 0 background, 1 object)."""
    if not anchors.is_cuda or anchors.dtype != torch.float32 or anchors.dim() != 2 or anchors.shape[1] != 4:
        raise ValueError("anchors must be a float32 ROCm tensor [N,4]")
    dev, B, N = anchors.device, len(boxes), anchors.shape[0]
    kmax = max(1, max(int(b.shape[0]) for b in boxes))
    rt = int(transformation_targets[0].shape[1]) if len(transformation_targets) else 0
    gb = np.zeros((B, kmax, 4), np.float64); gl = np.zeros((B, kmax), np.int32); gt = np.zeros((B, kmax, rt), np.float32)
    gc = np.zeros((B, kmax, 63), np.float32) if coords_3d is not None else None
    ng = np.zeros((B,), np.int32); hw = np.zeros((B, 2), np.int32)
    for i in range(B):
        k = int(boxes[i].shape[0])
        ng[i] = k; hw[i] = (int(image_shapes[i][0]), int(image_shapes[i][1]))
        if k:
            gb[i, :k] = boxes[i]; gl[i, :k] = np.asarray(labels[i]).astype(np.int32); gt[i, :k] = transformation_targets[i]
            if gc is not None:
                gc[i, :k] = np.asarray(coords_3d[i]).reshape(k, 63)
    t = lambda a: torch.from_numpy(a).to(dev)
    d_gb, d_gl, d_gt, d_ng, d_hw = t(gb), t(gl), t(gt), t(ng), t(hw)
    d_gc = t(gc) if gc is not None else None
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    lab, reg, tra = f(B, N, num_classes + 1), f(B, N, 5), f(B, N, rt + 1)
    crd = f(B, N, 64) if gc is not None else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    a = anchors.contiguous()
    _capi.check(_capi.lib().hep_anchor_targets_device(a.data_ptr(), N, d_gb.data_ptr(), d_gl.data_ptr(), d_gt.data_ptr(), _capi.ptr(d_gc),
                                                      d_ng.data_ptr(), d_hw.data_ptr(), B, kmax, num_classes, rt, float(negative_overlap),
                                                      float(positive_overlap), lab.data_ptr(), reg.data_ptr(), tra.data_ptr(), _capi.ptr(crd), stream))
    torch.cuda.current_stream(dev).synchronize()      # the staging tensors above must outlive the launch
    return lab, reg, tra, crd


def anchor_targets_device(anchors: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_transform: torch.Tensor,
                          gt_coords: Optional[torch.Tensor], gt_num: torch.Tensor, image_hw, num_classes: int = 1,
                          negative_overlap: float = 0.4, positive_overlap: float = 0.5):
    """``anchor_targets`` on annotation tables that are ALREADY on the device, in the layout hep_anchor_targets_device reads (and
    ``augment.augment_6dof`` writes): gt_boxes float64 [B,kmax,4], gt_labels int32 [B,kmax], gt_transform float32 [B,kmax,RT],
    gt_coords float32 [B,kmax,63] or None, gt_num int32 [B] (the first gt_num[b] rows of image b count), ``image_hw`` an int32
    device tensor [B,2] = (height, width) of the unpadded image or one (height, width) pair for the whole batch.  No numpy staging
    and no stream synchronise: the launch is enqueued on the current stream and the outputs of ``anchor_targets`` are returned."""
    if not anchors.is_cuda or anchors.dtype != torch.float32 or anchors.dim() != 2 or anchors.shape[1] != 4:
        raise ValueError("anchors must be a float32 ROCm tensor [N,4]")
    dev, N = anchors.device, anchors.shape[0]

    def chk(t, name, dtype, dims):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or t.dim() != dims:
            raise ValueError(f"{name} must be a {dtype} tensor with {dims} dimensions on {dev}")
        return t.contiguous()

    gb, gl, gt, ng = chk(gt_boxes, "gt_boxes", torch.float64, 3), chk(gt_labels, "gt_labels", torch.int32, 2), chk(gt_transform, "gt_transform", torch.float32, 3), chk(gt_num, "gt_num", torch.int32, 1)
    B, kmax, rt = gl.shape[0], gl.shape[1], gt.shape[2]
    if B < 1 or kmax < 1 or tuple(gb.shape) != (B, kmax, 4) or tuple(gt.shape) != (B, kmax, rt) or tuple(ng.shape) != (B,):
        raise ValueError("gt_boxes [B,kmax,4], gt_labels [B,kmax], gt_transform [B,kmax,RT] and gt_num [B] must agree")
    gc = None
    if gt_coords is not None:
        gc = chk(gt_coords, "gt_coords", torch.float32, 3)
        if tuple(gc.shape) != (B, kmax, 63):
            raise ValueError("gt_coords must be [B,kmax,63]")
    if isinstance(image_hw, torch.Tensor):
        hw = chk(image_hw, "image_hw", torch.int32, 2)
        if tuple(hw.shape) != (B, 2):
            raise ValueError("image_hw must be [B,2]")
    else:
        hw = torch.tensor([[int(image_hw[0]), int(image_hw[1])]] * B, dtype=torch.int32).to(dev, non_blocking=True)
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    lab, reg, tra = f(B, N, num_classes + 1), f(B, N, 5), f(B, N, rt + 1)
    crd = f(B, N, 64) if gc is not None else None
    a = anchors.contiguous()
    _capi.check(_capi.lib().hep_anchor_targets_device(a.data_ptr(), N, gb.data_ptr(), gl.data_ptr(), gt.data_ptr(), _capi.ptr(gc), ng.data_ptr(),
                                                      hw.data_ptr(), B, kmax, num_classes, rt, float(negative_overlap), float(positive_overlap),
                                                      lab.data_ptr(), reg.data_ptr(), tra.data_ptr(), _capi.ptr(crd), torch.cuda.current_stream(dev).cuda_stream))
    return lab, reg, tra, crd


_T_ANCHORS = {}


def translation_anchors(size: int) -> torch.Tensor:
    """The translation anchors [N, 3] = (cx, cy, stride) of a square input (hep_anchors, host code), float32 on the CPU."""
    size = int(size)
    if size not in _T_ANCHORS:
        l = _capi.lib()
        n = _capi.check(l.hep_anchors(size, None, None))
        a = np.empty((n, 4), np.float32); t = np.empty((n, 3), np.float32)
        _capi.check(l.hep_anchors(size, a.ctypes.data, t.ctypes.data))
        _T_ANCHORS[size] = torch.from_numpy(t)
    return _T_ANCHORS[size]


def format_translation(translation_raw: torch.Tensor, camera: torch.Tensor, size: int) -> torch.Tensor:
    """``format_translation`` (hmdegopose/loss.py:30-51: RegressTranslation layers.py:142-166, CalculateTxTy :203-249) as
    plain differentiable torch ops: the translation half of ``torch.ops.hep.decode`` with a ``grad_fn``.
    translation_raw [B, N, 3] (any device and float dtype), camera [B, 6] = fx, fy, px, py, tz_scale, image_scale, ``size``
    the square input side the anchors are built for.  Returns (tx, ty, tz) [B, N, 3].  Elementwise, not a hot path."""
    if translation_raw.dim() != 3 or translation_raw.shape[2] != 3:
        raise ValueError("translation_raw must be [B, N, 3]")
    ta = translation_anchors(size).to(device=translation_raw.device, dtype=translation_raw.dtype)
    if ta.shape[0] != translation_raw.shape[1]:
        raise ValueError(f"translation_raw has {translation_raw.shape[1]} anchors, size {size} has {ta.shape[0]}")
    cam = camera.to(device=translation_raw.device, dtype=translation_raw.dtype)
    if cam.shape != (translation_raw.shape[0], 6):
        raise ValueError("camera must be [B, 6]")
    stride = ta[None, :, 2]
    x = ta[None, :, 0] + translation_raw[..., 0] * stride
    y = ta[None, :, 1] + translation_raw[..., 1] * stride
    fx, fy, px, py, tzs, isc = (cam[:, i:i + 1] for i in range(6))
    x = x / isc - px
    y = y / isc - py
    tz = translation_raw[..., 2] * tzs
    return torch.stack((x * tz / fx, y * tz / fy, tz), dim=-1)


_PRED_NAMES = ("classification", "regression", "transformation", "hand")
_MEAN_SCALE = (1.0, 50.0, 1.0, 1.0, 1.0)      # d losses / d per_image[b] = scale / B (regression x 50)


def _loss_inputs(gt_classification, classification, gt_regression, regression, gt_transformation, transformation, gt_hand, hand,
                 model_3d_points, num_rotation_parameter):
    """Validated, contiguous float32 device tensors and sizes (the contiguous copies are autograd-tracked)."""
    def chk(x, name):
        if x is None:
            return None
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 ROCm tensor")
        return x.contiguous()
    gc, pc, gr, pr = chk(gt_classification, "gt_classification"), chk(classification, "classification"), chk(gt_regression, "gt_regression"), chk(regression, "regression")
    gt, pt, gh, ph = chk(gt_transformation, "gt_transformation"), chk(transformation, "transformation"), chk(gt_hand, "gt_hand"), chk(hand, "hand")
    if pc.dim() != 3:
        raise ValueError("loss inputs do not have the reference's shapes")
    B, N, K = pc.shape
    R = int(num_rotation_parameter)
    if gc.shape != (B, N, K + 1) or gr.shape != (B, N, 5) or pr.shape != (B, N, 4) or gt.shape != (B, N, R + 6) or pt.shape != (B, N, R + 3):
        raise ValueError("loss inputs do not have the reference's shapes")
    H = 0
    if ph is not None:
        H = int(ph.shape[2]) if ph.dim() == 3 else -1
        if gh is None or gh.shape != (B, N, H + 1) or ph.shape != (B, N, H):
            raise ValueError("gt_hand must be [B, N, H + 1] next to hand [B, N, H]")
    pts = torch.as_tensor(np.asarray(model_3d_points, dtype=np.float32) if not torch.is_tensor(model_3d_points) else model_3d_points,
                          dtype=torch.float32).to(pc.device).contiguous()
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise ValueError("model_3d_points must be [classes, P, 3]")
    return (gc, pc, gr, pr, gt, pt, gh, ph, pts), (B, N, K, R, H, int(pts.shape[0]), int(pts.shape[1]))


def _losses_forward(t, sizes):
    gc, pc, gr, pr, gt, pt, gh, ph, pts = t
    B, N, K, R, H, C, P = sizes
    dev = pc.device
    per = torch.empty((B, 5), dtype=torch.float32, device=dev)
    out = torch.empty((5,), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(_capi.lib().hep_losses_device(gc.data_ptr(), pc.data_ptr(), gr.data_ptr(), pr.data_ptr(), gt.data_ptr(), pt.data_ptr(),
                                              _capi.ptr(gh), _capi.ptr(ph), pts.data_ptr(), B, N, K, R, H, C, P,
                                              per.data_ptr(), out.data_ptr(), stream))
    torch.cuda.current_stream(dev).synchronize()      # the contiguous copies above must outlive the launch
    return out, per


def losses_backward(t, sizes, grad_per_image, need=(True, True, True, True)):
    """hep_losses_backward_device on the current stream: the gradients of (classification, regression, transformation,
    hand) for the upstream gradient ``grad_per_image`` [B, 5] of the per-image losses (None where ``need`` is False or
    there is no hand).  ``t`` / ``sizes`` as _loss_inputs returns them.  No host synchronisation: every tensor involved is
    allocated on, and stays alive with respect to, the current stream."""
    gc, pc, gr, pr, gt, pt, gh, ph, pts = t
    B, N, K, R, H, C, P = sizes
    dev = pc.device
    u = grad_per_image.to(device=dev, dtype=torch.float32).contiguous()
    if u.shape != (B, 5):
        raise ValueError("grad_per_image must be [B, 5]")
    f = lambda on, *shape: torch.empty(shape, dtype=torch.float32, device=dev) if on else None
    g_cls, g_reg, g_tr = f(need[0], B, N, K), f(need[1], B, N, 4), f(need[2], B, N, R + 3)
    g_hand = f(need[3] and ph is not None, B, N, H)
    ws = torch.empty((B * (N + 4),), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(_capi.lib().hep_losses_backward_device(gc.data_ptr(), pc.data_ptr(), gr.data_ptr(), pr.data_ptr(), gt.data_ptr(), pt.data_ptr(),
                                                       _capi.ptr(gh), _capi.ptr(ph), pts.data_ptr(), B, N, K, R, H, C, P, u.data_ptr(),
                                                       _capi.ptr(g_cls), _capi.ptr(g_reg), _capi.ptr(g_tr), _capi.ptr(g_hand),
                                                       ws.data_ptr(), stream))
    return g_cls, g_reg, g_tr, g_hand


class _Losses(torch.autograd.Function):
    """losses() with a HIP backward; inputs are _loss_inputs' tensors, gradients flow to the four predictions only."""

    @staticmethod
    def forward(ctx, gc, pc, gr, pr, gt, pt, gh, ph, pts, sizes):
        out, per = _losses_forward((gc, pc, gr, pr, gt, pt, gh, ph, pts), sizes)
        ctx.save_for_backward(gc, pc, gr, pr, gt, pt, gh, ph, pts)
        ctx.sizes = sizes
        return out, per

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_per):
        t = ctx.saved_tensors
        B = ctx.sizes[0]
        dev = t[1].device
        u = torch.zeros((B, 5), dtype=torch.float32, device=dev)
        if g_per is not None:
            u = u + g_per
        if g_out is not None:
            u = u + (g_out * torch.tensor(_MEAN_SCALE, dtype=torch.float32, device=dev) / B)[None]
        nig = ctx.needs_input_grad
        g_cls, g_reg, g_tr, g_hand = losses_backward(t, ctx.sizes, u, (nig[1], nig[3], nig[5], nig[7]))
        return None, g_cls, None, g_reg, None, g_tr, None, g_hand, None, None


def losses(gt_classification: torch.Tensor, classification: torch.Tensor, gt_regression: torch.Tensor, regression: torch.Tensor,
           gt_transformation: torch.Tensor, transformation: torch.Tensor, gt_hand: Optional[torch.Tensor], hand: Optional[torch.Tensor],
           model_3d_points, num_rotation_parameter: int = 3):
    """``batch_iterate`` (hmdegopose/loss.py:54-99) on float32 ROCm tensors laid out as the generator / the network
    produce them (see include/hep.h: hep_losses_device); ``model_3d_points`` [classes, P, 3] (numpy or tensor).  Returns
    (losses [5] = classification, regression x 50, rotation, translation, hand - the batch means, per_image [B, 5]).
    When grad mode is on and a prediction (classification / regression / transformation / hand) requires grad, both
    outputs carry a ``grad_fn`` whose backward is hep_losses_backward_device; the targets and the model points get no
    gradient.  The values are the same either way."""
    t, sizes = _loss_inputs(gt_classification, classification, gt_regression, regression, gt_transformation, transformation, gt_hand,
                            hand, model_3d_points, num_rotation_parameter)
    if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (t[1], t[3], t[5], t[7])):
        return _Losses.apply(*t, sizes)
    return _losses_forward(t, sizes)


def batch_iterate(gt_classification, classification, gt_regression, regression, gt_transformation, transformation, gt_hand, hand,
                  model_3d_points, num_rotation_parameter):
    """Drop-in for the reference's ``hmdegopose.loss.batch_iterate`` (loss.py:54-99), differentiable: returns the five
    losses (classification, regression x 50, rotation, translation, hand) as tensors of shape [1], like the reference.
    The predictions must be float32 ROCm tensors (any strides); targets on the host are moved to their device;
    ``model_3d_points`` may be numpy."""
    dev = classification.device
    mv = lambda x: None if x is None else (x if x.is_cuda else x.to(dev)).to(torch.float32)
    out, _per = losses(mv(gt_classification), classification, mv(gt_regression), regression, mv(gt_transformation), transformation,
                       mv(gt_hand), hand, model_3d_points, num_rotation_parameter)
    return tuple(out[k:k + 1] for k in range(5))
