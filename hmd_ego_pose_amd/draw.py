"""Pose overlays on the GPU: the annotations and the kept detections of a batch drawn into uint8 frames in place, one launch
(hep_draw_poses_device, csrc/k_draw.hip) - what the reference's evaluator draws per validation image (eval/common.py:452-479;
generators/utils/visualization.py:85-117, 143-232, 234-290): the projected cuboid with its centre point, optionally the 2D box and the
hand skeleton.

The rasterisation is this project's own definition in integer arithmetic (include/hep.h; tests/_draw.py states it in numpy and the
kernel matches it byte for byte).  cv2's line and circle rasterisers, ``LINE_AA`` and fonts are NOT restated (parity unpinned: cv2 is
absent from the build image); captions are not drawn."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _capi

HEP_DRAW_BOX2D, HEP_DRAW_CUBOID, HEP_DRAW_HAND = _capi.DRAW_BOX2D, _capi.DRAW_CUBOID, _capi.DRAW_HAND
MAX_DETECTIONS = _capi.DRAW_MAX_DETECTIONS
DETECTION_KEYS = ("boxes", "scores", "labels", "rotation", "translation", "hand")


def cuboid_corners(min_xyz, size_xyz) -> np.ndarray:
    """The eight corners, float32 [8,3], of the model cuboid ``min_* / size_*`` of models_info.yml in the corner order of
    generators/colibri.py:121-151: the lower level (z = min) counter-clockwise from the minimum corner - (0,0) (sx,0) (sx,sy) (0,sy) -
    then the upper level (z = min + size) in the same order."""
    m, s = np.asarray(min_xyz, np.float64).reshape(3), np.asarray(size_xyz, np.float64).reshape(3)
    c = np.empty((8, 3), np.float64)
    for k in range(8):
        c[k] = (m[0] + (s[0] if k % 4 in (1, 2) else 0.0), m[1] + (s[1] if k % 4 in (2, 3) else 0.0), m[2] + (s[2] if k >= 4 else 0.0))
    return c.astype(np.float32)


def label_colours(n: int) -> np.ndarray:
    """uint8 [n,3]: the colour of label i is the fully saturated, full-value HSV colour of hue h = (47 + 137 i) mod 360 degrees in
    integer arithmetic: sector = h // 60, f = h % 60, up = (255 f + 30) // 60, down = 255 - up, and (R, G, B) = (255, up, 0),
    (down, 255, 0), (0, 255, up), (0, down, 255), (up, 0, 255), (255, 0, down) for sector 0..5.  137 and 360 are coprime and a step of f
    moves ``up`` by more than 4, so the colours of up to 360 labels are distinct.  The project's own palette (the reference's colour
    table is not used)."""
    out = np.zeros((int(n), 3), np.uint8)
    for i in range(int(n)):
        h = (47 + 137 * i) % 360
        up = (255 * (h % 60) + 30) // 60
        out[i] = ((255, up, 0), (255 - up, 255, 0), (0, 255, up), (0, 255 - up, 255), (up, 0, 255), (255, 0, 255 - up))[h // 60]
    return out


def detections_from_records(records: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The six detection arrays ``draw_poses`` takes from the 80-word records of ``Session.top1`` ([B,80] int32: one row per image) or
    ``Session.top_labels`` ([B,K,80]: K rows per image): boxes [B,rows,4], scores [B,rows], labels [B,rows] int32, rotation, translation
    [B,rows,3], hand [B,rows,63] - contiguous re-packs of words 5-8, 4, 1, 9-11, 12-14 and 15-77 (include/hep.h).  A record without a
    detection holds the filter's padding (score -1) and is no candidate for any threshold >= -1.  No synchronisation."""
    if not isinstance(records, torch.Tensor) or records.dtype != torch.int32 or records.dim() not in (2, 3) or records.shape[-1] != _capi.POSE_RECORD_WORDS:
        raise ValueError(f"detections_from_records: records must be an int32 tensor [B,{_capi.POSE_RECORD_WORDS}] or [B,K,{_capi.POSE_RECORD_WORDS}]")
    rec = records.contiguous()
    if rec.dim() == 2:
        rec = rec[:, None, :]
    f = rec.view(torch.float32)
    return dict(boxes=f[..., 5:9].contiguous(), scores=f[..., 4].contiguous(), labels=rec[..., 1].contiguous(), rotation=f[..., 9:12].contiguous(),
                translation=f[..., 12:15].contiguous(), hand=f[..., 15:78].contiguous())


def draw_poses(frames: torch.Tensor, *, cuboids, colours=None, gt: Optional[torch.Tensor] = None, camera: Optional[torch.Tensor] = None,
               detections: Optional[Dict[str, torch.Tensor]] = None, score_threshold: float = 0.5, max_detections: int = 10,
               ann_layers: int = HEP_DRAW_CUBOID, det_layers: int = HEP_DRAW_CUBOID, thickness: int = 2) -> torch.Tensor:
    """Draw into ``frames`` (uint8 [B,H,W,3], contiguous, on the GPU) in place, asynchronously on the current stream, and return it.

    ``cuboids``: float32 [L,8,3] (``cuboid_corners`` per label; a device tensor, or a host array that is copied up).  ``colours``: host
    uint8 [L,3], default ``label_colours(L)``.  ``gt``: float64 [B,amax,88] (``evaluate.gt_scene_table``) or [B,88] (``gt_table``) on
    the device - its valid rows are drawn in annotation colours.  ``camera``: float64 [B,5] fx, fy, cx, cy, image scale on the device;
    required without ``gt``, else the default is the one in ``gt``.  ``detections``: the rows of ``Session.filter`` / ``model.detect`` /
    ``detections_from_records`` (keys boxes, scores, labels, rotation, translation and optionally hand); rows with score >
    ``score_threshold`` are candidates, the first ``max_detections`` are kept.  ``*_layers``: HEP_DRAW_BOX2D | HEP_DRAW_CUBOID |
    HEP_DRAW_HAND.  Every argument is checked here (ValueError) before a pointer reaches the library."""
    who = "draw_poses"
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError(f"{who}: frames must be a uint8 tensor [B,H,W,3]")
    if not frames.is_cuda or not frames.is_contiguous():
        raise ValueError(f"{who}: frames must be contiguous and on the GPU (they are drawn in place)")
    dev = frames.device
    B, H, W = (int(v) for v in frames.shape[:3])
    if not (16 <= H <= 4096 and 16 <= W <= 4096):
        raise ValueError(f"{who}: frames of {H} x {W}: height and width must be in 16..4096")
    if not isinstance(cuboids, torch.Tensor):
        c = np.asarray(cuboids)
        if c.dtype != np.float32 or c.ndim != 3:
            raise ValueError(f"{who}: cuboids must be float32 [L,8,3]")
        cuboids = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
    if cuboids.dtype != torch.float32 or cuboids.dim() != 3 or tuple(cuboids.shape[1:]) != (8, 3) or cuboids.device != dev:
        raise ValueError(f"{who}: cuboids must be float32 [L,8,3] on {dev}")
    L = int(cuboids.shape[0])
    if not 1 <= L <= _capi.SCORE_MAX_LABELS:
        raise ValueError(f"{who}: {L} labels: must be 1..{_capi.SCORE_MAX_LABELS}")
    col = label_colours(L) if colours is None else np.asarray(colours)
    if col.dtype != np.uint8 or col.shape != (L, 3):
        raise ValueError(f"{who}: colours must be a host uint8 array [{L},3]")
    col = np.ascontiguousarray(col)
    amax = 0
    if gt is not None:
        if not isinstance(gt, torch.Tensor) or gt.dtype != torch.float64 or gt.device != dev:
            raise ValueError(f"{who}: gt must be a float64 tensor on {dev}")
        if gt.dim() == 2:
            gt = gt[:, None, :]
        if gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != _capi.SCORE_GT_DOUBLES or not 1 <= gt.shape[1] <= _capi.SCORE_MAX_ANNOTATIONS:
            raise ValueError(f"{who}: gt must be [{B},amax,{_capi.SCORE_GT_DOUBLES}] with amax in 1..{_capi.SCORE_MAX_ANNOTATIONS} (or [{B},{_capi.SCORE_GT_DOUBLES}])")
        gt = gt.contiguous()
        amax = int(gt.shape[1])
    if camera is not None:
        if not isinstance(camera, torch.Tensor) or camera.dtype != torch.float64 or camera.device != dev or tuple(camera.shape) != (B, 5):
            raise ValueError(f"{who}: camera must be a float64 tensor [{B},5] on {dev}")
        camera = camera.contiguous()
    if gt is None and camera is None:
        raise ValueError(f"{who}: without gt a camera [B,5] is required")
    d = [None] * 6
    rows, M = 0, 0
    if detections is not None:
        missing = [k for k in DETECTION_KEYS[:5] if detections.get(k) is None]
        if missing:
            raise ValueError(f"{who}: detections lack {missing}")
        rows = int(detections["scores"].shape[1]) if detections["scores"].dim() == 2 else 0
        for i, (k, w, dt) in enumerate(zip(DETECTION_KEYS, (4, None, None, 3, 3, 63), (torch.float32, torch.float32, torch.int32) + (torch.float32,) * 3)):
            t = detections.get(k)
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != ((B, rows) if w is None else (B, rows, w)) or t.dtype != dt or t.device != dev:
                raise ValueError(f"{who}: detection rows '{k}' must be {dt} {(B, rows) if w is None else (B, rows, w)} on {dev}")
            d[i] = t.contiguous()
        M = int(max_detections)
        if not 1 <= rows <= 256 or not 1 <= M <= min(rows, MAX_DETECTIONS):
            raise ValueError(f"{who}: {rows} detection rows, max_detections {M}: rows must be 1..256, max_detections 1..min(rows, {MAX_DETECTIONS})")
    all_layers = HEP_DRAW_BOX2D | HEP_DRAW_CUBOID | HEP_DRAW_HAND
    if int(ann_layers) & ~all_layers or int(det_layers) & ~all_layers or int(ann_layers) < 0 or int(det_layers) < 0:
        raise ValueError(f"{who}: layers must be a combination of HEP_DRAW_BOX2D, HEP_DRAW_CUBOID and HEP_DRAW_HAND")
    if not 1 <= int(thickness) <= 8:
        raise ValueError(f"{who}: thickness must be in 1..8")
    _capi.check(_capi.lib().hep_draw_poses_device(
        frames.data_ptr(), B, H, W, _capi.ptr(gt), amax, _capi.ptr(camera), *[_capi.ptr(t) for t in d], rows, float(score_threshold), M,
        cuboids.data_ptr(), col.ctypes.data, L, int(ann_layers), int(det_layers), int(thickness), torch.cuda.current_stream(dev).cuda_stream))
    return frames
