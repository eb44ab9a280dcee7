"""The training input on the GPU: the reference's 6DoF augmentation and group preprocess in front of the training step.

The reference prepares every batch on the host (pytorch-sandbox/generators/common.py): ``augmentation_6DoF`` (:410-479: one
``cv2.warpAffine`` pair, a ``np.where`` per object, two ``cv2.Rodrigues`` per image) and ``preprocess_group_entry`` (:543-607).
Here one call (``augment_6dof`` -> hep_augment_6dof_device, csrc/k_augment.hip) takes the raw uint8 frames, masks and dataset
annotations on the device and leaves the normalised network input, the camera vectors and the annotation tables that
``training.anchor_targets_device`` reads - three launches (four with a resize), no host synchronisation.

``draw_6dof`` draws the random parameters in the reference's order (:329-371), ``rotation_matrices`` computes the forward
matrices of ``cv2.getRotationMatrix2D`` in float64 on the host; they are uploaded as data, so the kernels and the numpy oracle
(tests/_augment.py, the definition) see the same doubles.  OpenCV's conventions are restated, not pinned against cv2 (DESIGN.md
section 7e).  Not reproduced: the rotation of hand joints (the reference does not rotate ``coords_3d`` either: pass them to
``anchor_targets_device`` untouched), ``translations_x_y_2D`` (never read downstream).

The reference's colour augmentation (``RandAugment(n=(1, 3), m=(1, 14))``, generators/randaug.py, common.py:334-341) comes first, on
the uint8 frames: ``draw_colour`` -> ``colour_augment`` (hep_colour_augment_device, csrc/k_colour.hip) -> ``augment_6dof``.  Its 14
operations reproduce the numpy oracle tests/_colour.py bit for bit (the noise up to float32 rounding); that oracle is pinned against PIL
for the ten operations that are PIL's.  Cutout, Invert, the noise and the random stream are restated, not pinned against imgaug
(DESIGN.md section 7g).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _capi

SCALE_MIN, SCALE_MAX = 0.25, 4.0      # the supported range of the augmentation scale (include/hep.h)
KMAX = 16                             # annotations per image


def draw_6dof(rng, batch: int, scale_range: Tuple[float, float] = (0.7, 1.3), chance_no_augmentation: float = 0.02):
    """Per image, in the reference's order: the chance to skip; then - only when augmenting - the scale, then the angle
    (common.py:330, :370, :371).  ``rng`` needs a ``random()`` in [0, 1): a ``random.Random(seed)`` reproduces the reference's
    sequence.  Returns (angles_deg float64 [B], scales float64 [B], apply int32 [B]); a skipped image has angle 0, scale 1."""
    min_scale, max_scale = (float(v) for v in scale_range)
    if max_scale < min_scale:                                   # get_scale_6DoF_augmentation_parameter :489-493
        scale_span, min_scale = 0.0, 1.0
    else:
        scale_span = max_scale - min_scale
    if not (SCALE_MIN <= min_scale and min_scale + scale_span <= SCALE_MAX):
        raise ValueError(f"scale_range must lie inside [{SCALE_MIN}, {SCALE_MAX}]")
    angles, scales, apply = np.zeros(batch, np.float64), np.ones(batch, np.float64), np.zeros(batch, np.int32)
    for b in range(batch):
        if rng.random() >= chance_no_augmentation:
            scales[b] = rng.random() * scale_span + min_scale
            angles[b] = rng.random() * 360
            apply[b] = 1
    return angles, scales, apply


def rotation_matrices(angles_deg, scales, centres) -> np.ndarray:
    """``cv2.getRotationMatrix2D((cx, cy), -angle, scale)`` per image as float64 [B, 6] (2 x 3, row major): a = scale cos, b = scale
    sin of -angle, M = [[a, b, (1-a)cx - b cy], [-b, a, b cx + (1-a)cy]].  ``centres`` [B, 2] = (cx, cy): the principal point."""
    angles = np.asarray(angles_deg, np.float64).reshape(-1)
    scales = np.asarray(scales, np.float64).reshape(-1)
    centres = np.asarray(centres, np.float64).reshape(-1, 2)
    if not (angles.shape[0] == scales.shape[0] == centres.shape[0]):
        raise ValueError("angles_deg, scales and centres must have one entry per image")
    if not (np.isfinite(angles).all() and np.isfinite(centres).all()):
        raise ValueError("angles_deg and centres must be finite")
    if not ((scales >= SCALE_MIN) & (scales <= SCALE_MAX)).all():
        raise ValueError(f"every scale must be in [{SCALE_MIN}, {SCALE_MAX}]")
    out = np.empty((angles.shape[0], 6), np.float64)
    for i in range(angles.shape[0]):
        rad = -float(angles[i]) * math.pi / 180.0
        a, b = float(scales[i]) * math.cos(rad), float(scales[i]) * math.sin(rad)
        cx, cy = float(centres[i, 0]), float(centres[i, 1])
        out[i] = (a, b, (1.0 - a) * cx - b * cy, -b, a, b * cx + (1.0 - a) * cy)
    return out


_ANNOTATION_KEYS = (("boxes", torch.float64, (4,)), ("labels", torch.int32, ()), ("mask_values", torch.int32, ()), ("rvec", torch.float32, (3,)),
                    ("tvec", torch.float32, (3,)), ("extra", torch.float32, (2,)))


def pad_annotations(annotations: Sequence[dict], device, kmax: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """A list of the reference's annotation dicts (``bboxes`` [K,4], ``labels`` [K], ``rotations`` [K,5] = axis-angle, is_symmetric,
    class, ``translations`` [K,3], and ``mask_values`` [K]: name_to_mask_value of each label, common.py:366) -> the padded tensors
    of the ABI on ``device``, uploaded once: boxes float64 [B,kmax,4], labels / mask_values int32 [B,kmax], rvec / tvec float32
    [B,kmax,3], extra float32 [B,kmax,2], num_gt int32 [B]."""
    B = len(annotations)
    if B < 1:
        raise ValueError("no annotations")
    counts = [int(np.asarray(a["labels"]).shape[0]) for a in annotations]
    kmax = max(1, max(counts)) if kmax is None else int(kmax)
    if kmax > KMAX or max(counts) > kmax:
        raise ValueError(f"at most {KMAX} annotations per image (kmax {kmax}, the largest image has {max(counts)})")
    host = {"boxes": np.zeros((B, kmax, 4), np.float64), "labels": np.zeros((B, kmax), np.int32), "mask_values": np.zeros((B, kmax), np.int32),
            "rvec": np.zeros((B, kmax, 3), np.float32), "tvec": np.zeros((B, kmax, 3), np.float32), "extra": np.zeros((B, kmax, 2), np.float32),
            "num_gt": np.asarray(counts, np.int32)}
    for b, (a, k) in enumerate(zip(annotations, counts)):
        if not k:
            continue
        rot = np.asarray(a["rotations"], np.float64).reshape(k, -1)
        if rot.shape[1] != 5:
            raise ValueError("rotations must be [K, 5]: axis-angle, is_symmetric, class index")
        host["boxes"][b, :k] = np.asarray(a["bboxes"], np.float64).reshape(k, 4)
        host["labels"][b, :k] = np.asarray(a["labels"]).reshape(k)
        host["mask_values"][b, :k] = np.asarray(a["mask_values"]).reshape(k)
        host["rvec"][b, :k] = rot[:, :3]
        host["extra"][b, :k] = rot[:, 3:]
        host["tvec"][b, :k] = np.asarray(a["translations"], np.float64).reshape(k, 3)
    return {k: torch.from_numpy(v).to(device) for k, v in host.items()}


def _check(t, name, dtype, shape, device):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != device or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a {dtype} tensor {list(shape)} on {device}")
    return t.contiguous()


def augment_6dof(frames_u8: torch.Tensor, masks_u8: torch.Tensor, annotations: Union[Dict[str, torch.Tensor], Sequence[dict]], camera_k,
                 angles_deg, scales, apply, size: int, translation_scale_norm: float = 1000.0) -> Dict[str, torch.Tensor]:
    """frames_u8 uint8 [B,H,W,3] and masks_u8 uint8 [B,H,W] on the device; ``annotations``: the padded device tensors of
    ``pad_annotations`` (keys boxes, labels, mask_values, rvec, tvec, extra, num_gt) or a list of the reference's annotation
    dicts, which is padded and uploaded once; camera_k [B,4] = fx, fy, px, py on the HOST (array or CPU tensor: the principal point
    is the centre of the rotation, whose matrix is computed on the host); angles_deg, scales, apply: ``draw_6dof``'s.
    Returns device tensors: image float32 [B,3,size,size] (what ``TrainableBackbone`` takes), camera [B,6], gt_boxes float64
    [B,kmax,4], gt_labels int32 [B,kmax], gt_transform float32 [B,kmax,8], gt_num int32 [B] (the inputs of
    ``training.anchor_targets_device``), applied int32 [B], mask uint8 [B,H,W] (the mask that goes with the image).
    Raises ValueError for a wrong dtype, device or shape before the ABI sees a pointer.  Enqueues on the current stream and does
    not synchronise; the inputs must stay alive until the stream has passed the call (torch's allocator sees to that for tensors
    used on the current stream)."""
    if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError("frames_u8 must be a uint8 ROCm tensor [B,H,W,3]")
    dev = frames_u8.device
    B, H, W = (int(v) for v in frames_u8.shape[:3])
    size = int(size)
    if B < 1 or not (16 <= H <= 4096 and 16 <= W <= 4096):
        raise ValueError("frames must be [B >= 1, H, W, 3] with H and W in [16, 4096]")
    if not (16 <= size <= 4096) or size % 4:
        raise ValueError("size must be a multiple of 4 in [16, 4096]")
    frames = frames_u8.contiguous()
    masks = _check(masks_u8, "masks_u8", torch.uint8, (B, H, W), dev)
    if isinstance(camera_k, torch.Tensor):
        if camera_k.is_cuda:
            raise ValueError("camera_k must be on the host (the rotation's centre is read there)")
        camera_k = camera_k.numpy()
    cam = np.ascontiguousarray(np.asarray(camera_k, np.float32))
    if cam.shape != (B, 4) or not np.isfinite(cam).all():
        raise ValueError("camera_k must be finite [B, 4] = fx, fy, px, py")
    if not (float(translation_scale_norm) > 0.0 and math.isfinite(float(translation_scale_norm))):
        raise ValueError("translation_scale_norm must be positive")
    apply_h = np.asarray(apply).reshape(-1)
    angles_h = np.asarray(angles_deg, np.float64).reshape(-1)
    scales_h = np.asarray(scales, np.float64).reshape(-1)
    if not (apply_h.shape[0] == angles_h.shape[0] == scales_h.shape[0] == B):
        raise ValueError("angles_deg, scales and apply must have one entry per image")
    xform = np.empty((B, 9), np.float64)
    xform[:, :6] = rotation_matrices(angles_h, scales_h, cam[:, 2:4].astype(np.float64))      # (refuses a scale outside [0.25, 4])
    xform[:, 6] = angles_h / 180.0 * math.pi
    xform[:, 7] = scales_h
    xform[:, 8] = (apply_h != 0)
    if not isinstance(annotations, dict):
        annotations = pad_annotations(annotations, dev)
    missing = [k for k, _, _ in _ANNOTATION_KEYS if k not in annotations] + ([] if "num_gt" in annotations else ["num_gt"])
    if missing:
        raise ValueError(f"annotations lack {missing}")
    if not isinstance(annotations["labels"], torch.Tensor) or annotations["labels"].dim() != 2:
        raise ValueError("annotations['labels'] must be an int32 tensor [B, kmax]")
    kmax = int(annotations["labels"].shape[1])
    if not 1 <= kmax <= KMAX:
        raise ValueError(f"kmax must be in 1..{KMAX}")
    ann = {k: _check(annotations[k], f"annotations['{k}']", dt, (B, kmax) + tail, dev) for k, dt, tail in _ANNOTATION_KEYS}
    num_gt = _check(annotations["num_gt"], "annotations['num_gt']", torch.int32, (B,), dev)
    d_xform = torch.from_numpy(xform).to(dev, non_blocking=True)
    d_cam_k = torch.from_numpy(cam).to(dev, non_blocking=True)
    l = _capi.lib()
    need = _capi.check(l.hep_augment_workspace_bytes(B, H, W, size, kmax))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    out = {"image": torch.empty((B, 3, size, size), dtype=torch.float32, device=dev), "mask": torch.empty((B, H, W), dtype=torch.uint8, device=dev),
           "camera": torch.empty((B, 6), dtype=torch.float32, device=dev), "gt_boxes": torch.empty((B, kmax, 4), dtype=torch.float64, device=dev),
           "gt_labels": torch.empty((B, kmax), dtype=torch.int32, device=dev), "gt_transform": torch.empty((B, kmax, 8), dtype=torch.float32, device=dev),
           "gt_num": torch.empty((B,), dtype=torch.int32, device=dev), "applied": torch.empty((B,), dtype=torch.int32, device=dev)}
    _run(l, frames, masks, d_xform, d_cam_k, ann, num_gt, B, H, W, size, kmax, float(translation_scale_norm), out, ws, dev)
    return out


def _run(l, frames, masks, d_xform, d_cam_k, ann, num_gt, B, H, W, size, kmax, tsn, out, ws, dev):
    """The ABI call on tensors that passed the checks (tools/augment_time.py and the tests call it with buffers of their own)."""
    stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(l.hep_augment_6dof_device(
        frames.data_ptr(), masks.data_ptr(), d_xform.data_ptr(), d_cam_k.data_ptr(), ann["boxes"].data_ptr(), ann["labels"].data_ptr(),
        ann["mask_values"].data_ptr(), ann["rvec"].data_ptr(), ann["tvec"].data_ptr(), ann["extra"].data_ptr(), num_gt.data_ptr(),
        B, H, W, size, kmax, tsn, out["image"].data_ptr(), _capi.ptr(out.get("mask")), out["camera"].data_ptr(), out["gt_boxes"].data_ptr(),
        out["gt_labels"].data_ptr(), out["gt_transform"].data_ptr(), out["gt_num"].data_ptr(), out["applied"].data_ptr(),
        ws.data_ptr(), ws.numel(), stream))


# ---- colour augmentation: the reference's RandAugment (generators/randaug.py:244-279) in front of the 6DoF warp ----
COLOUR_OPS = ("Identity", "Autocontrast", "Equalize", "Invert", "Posterize", "Solarize", "EnhanceColor", "EnhanceContrast", "EnhanceBrightness",
              "EnhanceSharpness", "Cutout", "FilterBlur", "FilterSmooth", "AdditiveGaussianNoise")
COLOUR_SLOTS = 3                      # operations per image (include/hep.h)
_M_MAX = 30                           # RandAugment._M_MAX


def _clip(v, lo, hi):
    return min(max(v, lo), hi)


def colour_parameters(op: int, m: int, height: int, width: int, sign: int = 1, centre=(0.5, 0.5), seed: int = 0):
    """One operation at magnitude ``m`` -> (i0, i1, i2, i3, seed, f): the formulas of randaug.py:244-279.  Posterize keeps
    ``8 - min(int(m 6/30), 6)`` bits; Solarize's threshold is ``clip(256 - int(m 256/30), 0, 256)``; the enhance factor is
    ``clip(1 + sign m 0.9/30, 0.1, 1.9)``; Cutout's square has the side ``clip(m (20/32)/30, 0, 0.625) height`` about
    ``centre`` = (cx, cy) in [0, 1)^2, clipped to the frame and truncated; the noise has sigma ``(m / 100) 255``."""
    i, f = [0, 0, 0, 0], 0.0
    if op == 4:
        i[0] = 8 - min(int(m * (6 / _M_MAX)), 6)
    elif op == 5:
        i[0] = _clip(256 - int(m * (256 / _M_MAX)), 0, 256)
    elif op in (6, 7, 8, 9):
        f = _clip(1.0 + sign * m * (0.9 / _M_MAX), 0.1, 1.9)
    elif op == 10:
        side = _clip(m * ((20 / 32) / _M_MAX), 0.0, 20 / 32) * height
        x1 = centre[0] * width - side / 2
        y1 = centre[1] * height - side / 2
        i = [int(_clip(x1, 0, width)), int(_clip(y1, 0, height)), int(_clip(x1 + side, 0, width)), int(_clip(y1 + side, 0, height))]
    elif op == 13:
        f = (m / 100.0) * 255
    return i[0], i[1], i[2], i[3], int(seed), f


def draw_colour(rng, batch: int, n: Tuple[int, int] = (1, 3), m: Tuple[int, int] = (1, 14), apply=None, height: int = 0, width: int = 0):
    """The table of ``colour_augment`` for one batch: (ops int32 [B,3,8], args float32 [B,3,2]) as numpy arrays (layout: include/hep.h).
    ``rng`` needs a ``random()`` in [0, 1); an integer in 0..k-1 is ``int(rng.random() * k)``.  ``apply`` is ``draw_6dof``'s third
    result (the reference's chance_no_augmentation gates both augmentations, common.py:330-331); None augments every image.
    Draw order, per image with apply[b] != 0 and nothing for the others: the number of operations n_b in n[0]..n[1]; n_b distinct ids
    in random order (partial Fisher-Yates over 0..13: for i < n_b, j = i + int(random() (14 - i)), swap); then per operation, in
    that order, only for the ids that have a magnitude (4-10 and 13): the magnitude in m[0]..m[1], and after it the sign for 6-9
    (+ when random() < 0.5), the centre cx then cy for 10, the seed's low then high 32 bits for 13.  Same seed, same table.
    This is the project's stream: imgaug's is not reproduced."""
    n0, n1, m0, m1 = int(n[0]), int(n[1]), int(m[0]), int(m[1])
    if not 0 <= n0 <= n1 <= COLOUR_SLOTS:
        raise ValueError(f"n must satisfy 0 <= n[0] <= n[1] <= {COLOUR_SLOTS}")
    if not 0 <= m0 <= m1 <= _M_MAX:
        raise ValueError(f"m must satisfy 0 <= m[0] <= m[1] <= {_M_MAX}")
    if not (16 <= int(height) <= 4096 and 16 <= int(width) <= 4096):
        raise ValueError("height and width (of the frames, for Cutout's rectangle) must be in [16, 4096]")
    apply_h = np.ones(batch, np.int32) if apply is None else np.asarray(apply).reshape(-1)
    if apply_h.shape[0] != batch:
        raise ValueError("apply must have one entry per image")
    ops = np.zeros((batch, COLOUR_SLOTS, 8), np.int32)
    ops[:, :, 0] = -1
    args = np.zeros((batch, COLOUR_SLOTS, 2), np.float32)
    for b in range(batch):
        if apply_h[b] == 0:
            continue
        n_b = n0 + int(rng.random() * (n1 - n0 + 1))
        ids = list(range(len(COLOUR_OPS)))
        for i in range(n_b):
            j = i + int(rng.random() * (len(ids) - i))
            ids[i], ids[j] = ids[j], ids[i]
        for k in range(n_b):
            op, mag, sign, centre, seed = ids[k], 0, 1, (0.5, 0.5), 0
            if 4 <= op <= 10 or op == 13:
                mag = m0 + int(rng.random() * (m1 - m0 + 1))
                if 6 <= op <= 9:
                    sign = 1 if rng.random() < 0.5 else -1
                elif op == 10:
                    cx = rng.random()
                    centre = (cx, rng.random())
                elif op == 13:
                    lo = int(rng.random() * 4294967296.0)
                    seed = lo | (int(rng.random() * 4294967296.0) << 32)
            i0, i1, i2, i3, seed, f = colour_parameters(op, mag, int(height), int(width), sign, centre, seed)
            ops[b, k, :5] = (op, i0, i1, i2, i3)
            ops[b, k, 5:7] = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32).view(np.int32)
            args[b, k, 0] = f
    return ops, args


def check_colour_table(ops, args, batch: int, height: int, width: int):
    """The host check of ``colour_augment``: (ops int32 [B,3,8], args float32 [B,3,2]) as contiguous numpy arrays, or ValueError."""
    ops = np.asarray(ops)
    args = np.asarray(args)
    if ops.shape != (batch, COLOUR_SLOTS, 8) or not np.issubdtype(ops.dtype, np.integer):
        raise ValueError(f"ops must be an integer array [{batch}, {COLOUR_SLOTS}, 8]")
    if args.shape != (batch, COLOUR_SLOTS, 2) or not np.issubdtype(args.dtype, np.floating):
        raise ValueError(f"args must be a float array [{batch}, {COLOUR_SLOTS}, 2]")
    ops = np.ascontiguousarray(ops, np.int32)
    args = np.ascontiguousarray(args, np.float32)
    f01, f19, f255 = np.float32(0.1), np.float32(1.9), np.float32(255)
    for b in range(batch):
        empty = False
        for k in range(COLOUR_SLOTS):
            op, i, f = int(ops[b, k, 0]), [int(v) for v in ops[b, k, 1:5]], args[b, k, 0]
            where = f"image {b} slot {k}"
            if not -1 <= op < len(COLOUR_OPS):
                raise ValueError(f"{where}: operation id {op} is not in -1..{len(COLOUR_OPS) - 1}")
            if op == -1:
                empty = True
                continue
            if empty:
                raise ValueError(f"{where}: an operation behind an empty slot (slots are filled from the front)")
            if op == 4 and not 2 <= i[0] <= 8:
                raise ValueError(f"{where}: Posterize keeps 2..8 bits, not {i[0]}")
            if op == 5 and not 0 <= i[0] <= 256:
                raise ValueError(f"{where}: Solarize's threshold must be in 0..256, not {i[0]}")
            if 6 <= op <= 9 and not f01 <= f <= f19:
                raise ValueError(f"{where}: the enhance factor must be in [0.1, 1.9], not {f}")
            if op == 10 and not (0 <= i[0] <= i[2] <= width and 0 <= i[1] <= i[3] <= height):
                raise ValueError(f"{where}: Cutout's rectangle x1, y1, x2, y2 = {i} is not inside the {width} x {height} frame")
            if op == 13 and not 0 <= f <= f255:
                raise ValueError(f"{where}: the noise's sigma must be in [0, 255], not {f}")
    return ops, args


def colour_augment(frames_u8: torch.Tensor, ops, args, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames_u8 uint8 [B,H,W,3] on the device; (ops, args): ``draw_colour``'s table (numpy arrays or CPU tensors).  Returns the
    augmented frames, uint8 [B,H,W,3] (``out`` when given: same shape, dtype and device, not ``frames_u8``) - what ``augment_6dof``
    takes.  The table is checked on the host (ids in -1..13, slots filled from the front, 2..8 bits, threshold in 0..256, factor in
    [0.1, 1.9], sigma in [0, 255], rectangles inside the frame): ValueError before the ABI sees a pointer.  Uploads the two small
    tables, enqueues on the current stream (at most four launches and a memset) and does not synchronise."""
    if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError("frames_u8 must be a uint8 ROCm tensor [B,H,W,3]")
    dev = frames_u8.device
    B, H, W = (int(v) for v in frames_u8.shape[:3])
    if B < 1 or not (16 <= H <= 4096 and 16 <= W <= 4096):
        raise ValueError("frames must be [B >= 1, H, W, 3] with H and W in [16, 4096]")
    if isinstance(ops, torch.Tensor) or isinstance(args, torch.Tensor):
        if any(isinstance(t, torch.Tensor) and t.is_cuda for t in (ops, args)):
            raise ValueError("ops and args must be on the host (they are checked there)")
        ops = ops.numpy() if isinstance(ops, torch.Tensor) else ops
        args = args.numpy() if isinstance(args, torch.Tensor) else args
    ops_h, args_h = check_colour_table(ops, args, B, H, W)
    frames = frames_u8.contiguous()
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != (B, H, W, 3) or not out.is_contiguous()
          or out.data_ptr() == frames.data_ptr()):
        raise ValueError(f"out must be a contiguous uint8 tensor {[B, H, W, 3]} on {dev}, and not frames_u8")
    d_ops = torch.from_numpy(ops_h).to(dev, non_blocking=True)
    d_args = torch.from_numpy(args_h).to(dev, non_blocking=True)
    l = _capi.lib()
    ws = torch.empty((_capi.check(l.hep_colour_workspace_bytes(B, H, W)),), dtype=torch.uint8, device=dev)
    _run_colour(l, frames, d_ops, d_args, B, H, W, out, ws, dev)
    return out


def _run_colour(l, frames, d_ops, d_args, B, H, W, out, ws, dev):
    """The ABI call on tensors that passed the checks (tools/colour_time.py and the tests call it with buffers of their own)."""
    _capi.check(l.hep_colour_augment_device(frames.data_ptr(), d_ops.data_ptr(), d_args.data_ptr(), B, H, W, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream(dev).cuda_stream))
