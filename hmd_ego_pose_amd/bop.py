"""The three BOP pose-error functions on the GPU for matched (ground truth, estimate) pairs: MSSD and MSPD over a model's vertices and its
set of symmetry transforms (hep_bop_point_errors_device), VSD over depth maps rendered by ``render.render_models``, optionally against a
measured depth image (hep_bop_vsd_device; csrc/k_bop.hip), and the average recalls BOP reports since 2019 as the evaluators' ``"bop"``
entry.  The errors are BOP's mssd, mspd and vsd (bop19 visibility rule, step cost) RESTATED with this project's own roundings -
include/hep.h states them, tests/_bop.py states them in numpy and is the definition; bop_toolkit is not part of this project's
environment, so parity with it is unpinned.  Deviation from BOP in the recalls: the scored pair of an annotation is the evaluator's IoU
match (hep_score_scene_device), not BOP's error-based matching of estimates to annotations; an annotation without a match, or with a
NaN error, is a miss.  No tlinear cost, no depth PNG reader: ``depth_test`` is a tensor."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _capi
from .render import MeshSet, _rodrigues, render_models

PAIR_DOUBLES, MAX_SYMMETRIES, MAX_TAUS = _capi.BOP_PAIR_DOUBLES, _capi.BOP_MAX_SYMMETRIES, _capi.BOP_MAX_TAUS
TAU_FRACTIONS = tuple(float(v) for v in np.arange(0.05, 0.51, 0.05))      # BOP19: VSD's tau and the correctness thresholds, ten each
_IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])


def _axis_rotation(axis: np.ndarray, angle: float) -> np.ndarray:
    k = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def symmetry_transforms(info: dict, max_sym_disc_step: float = 0.01) -> np.ndarray:
    """The set of symmetry transforms of one ``models_info.yml`` entry, float64 [S,12] (R row-major, then t), the identity first - host
    numpy.  ``symmetries_discrete``: lists of 16 numbers (4 x 4, row-major); ``symmetries_continuous``: dicts with ``axis`` and
    ``offset``, taken in ``ceil(pi / max_sym_disc_step)`` steps of a full turn (step 0 is the identity) and combined with the discrete
    ones: S = (1 + discrete) x steps ^ continuous.  More than 64 transforms raise ValueError: coarsen ``max_sym_disc_step``."""
    who = "symmetry_transforms"
    if not isinstance(info, dict):
        raise ValueError(f"{who}: a models_info entry (dict) is needed")
    if not (isinstance(max_sym_disc_step, (int, float)) and math.isfinite(max_sym_disc_step) and max_sym_disc_step > 0):
        raise ValueError(f"{who}: max_sym_disc_step must be finite and positive")
    disc = [(np.eye(3), np.zeros(3))]
    for m in info.get("symmetries_discrete", None) or []:
        m = np.asarray(m, np.float64)
        if m.size != 16 or not np.isfinite(m).all():
            raise ValueError(f"{who}: a discrete symmetry must be 16 finite numbers")
        m = m.reshape(4, 4)
        disc.append((m[:3, :3].copy(), m[:3, 3].copy()))
    if len(disc) > MAX_SYMMETRIES:
        raise ValueError(f"{who}: {len(disc)} discrete transforms exceed {MAX_SYMMETRIES}")
    steps = int(math.ceil(math.pi / max_sym_disc_step))
    out = disc
    for c in info.get("symmetries_continuous", None) or []:
        axis, offset = np.asarray(c["axis"], np.float64).reshape(-1), np.asarray(c["offset"], np.float64).reshape(-1)
        if axis.size != 3 or offset.size != 3 or not np.isfinite(axis).all() or not np.isfinite(offset).all() or not np.linalg.norm(axis) > 0:
            raise ValueError(f"{who}: a continuous symmetry needs a non-zero axis and an offset of 3 finite numbers each")
        if len(out) * steps > MAX_SYMMETRIES:
            raise ValueError(f"{who}: {len(out)} x {steps} transforms exceed {MAX_SYMMETRIES}: coarsen max_sym_disc_step "
                             f"(>= {math.pi / (MAX_SYMMETRIES // len(out)):.4g} keeps this object within the limit)")
        turned = []
        for Rd, td in out:
            for i in range(steps):
                if i == 0:
                    turned.append((Rd, td))
                    continue
                Rc = _axis_rotation(axis, i * (2.0 * math.pi / steps))
                tc = offset - Rc @ offset
                turned.append((Rc @ Rd, Rc @ td + tc))
        out = turned
    return np.stack([np.concatenate([Rm.reshape(9), t]) for Rm, t in out])


class SymmetrySet:
    """The symmetry transforms of labels 0..L-1 concatenated and uploaded once, like ``MeshSet``: ``table`` float64 [S_total,12] on the
    device, ``start`` host int32 [L+1].  ``per_label``: a sequence of [S,12] arrays (``symmetry_transforms`` results) or None for a label
    without symmetries, which gets the identity.  Every set must be finite, hold 1..64 transforms and begin with the identity."""

    def __init__(self, per_label: Sequence[Optional[np.ndarray]], device: Optional[torch.device] = None):
        if not 1 <= len(per_label) <= _capi.SCORE_MAX_LABELS:
            raise ValueError(f"SymmetrySet: {len(per_label)} labels: must be 1..{_capi.SCORE_MAX_LABELS}")
        sets, start = [], [0]
        for l, s in enumerate(per_label):
            s = _IDENTITY[None] if s is None else np.asarray(s, np.float64)
            if s.ndim != 2 or s.shape[1] != 12 or not 1 <= s.shape[0] <= MAX_SYMMETRIES or not np.isfinite(s).all():
                raise ValueError(f"SymmetrySet: the transforms of label {l} must be finite [S,12] with S in 1..{MAX_SYMMETRIES}")
            if not np.array_equal(s[0], _IDENTITY):
                raise ValueError(f"SymmetrySet: the first transform of label {l} must be the identity")
            sets.append(s)
            start.append(start[-1] + s.shape[0])
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.host = np.ascontiguousarray(np.concatenate(sets))
        self.start = np.ascontiguousarray(np.asarray(start, np.int32))
        self.num_labels, self.num_symmetries = len(sets), int(start[-1])
        self.table = torch.from_numpy(self.host).to(self.device)


def pairs_from_scene(gt: torch.Tensor, detections: Dict[str, torch.Tensor], records: torch.Tensor, camera: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pair table float64 [B*amax,32] (include/hep.h has the layout) of what ``SceneEvaluator.add`` holds, with torch float64
    operations on the device and no synchronisation: ``gt`` float64 [B,amax,88] (``evaluate.gt_scene_table``), ``detections`` the
    detection rows (``rotation`` and ``translation`` float32 [B,rows,3] are read), ``records`` float64 [B,amax,16] as
    hep_score_scene_device just wrote them (slot 0 valid, 1 matched, 2 the matched row, 12 the label).  One row per (image, annotation
    slot) in that order, valid only where the annotation is matched; image index = the image's position in the batch.  Roundings of
    ``render.poses_from_detections``: rotation = float32(r) * float32(pi) in float32, then Rodrigues in float64 (the ground truth's
    axis-angle directly in float64); the translation is widened.  ``camera``: float64 [B,4 or more] fx, fy, cx, cy, default slots
    14-17 of each ground-truth row."""
    who = "pairs_from_scene"
    if not isinstance(gt, torch.Tensor) or gt.dtype != torch.float64 or gt.dim() != 3 or gt.shape[2] != _capi.SCORE_GT_DOUBLES or gt.shape[0] < 1 or gt.shape[1] < 1:
        raise ValueError(f"{who}: gt must be a float64 tensor [B,amax,{_capi.SCORE_GT_DOUBLES}]")
    B, A = int(gt.shape[0]), int(gt.shape[1])
    dev = gt.device
    if not isinstance(records, torch.Tensor) or records.dtype != torch.float64 or tuple(records.shape) != (B, A, _capi.SCORE_RECORD_DOUBLES) or records.device != dev:
        raise ValueError(f"{who}: records must be a float64 tensor [{B},{A},{_capi.SCORE_RECORD_DOUBLES}] on {dev}")
    if not isinstance(detections, dict) or any(not isinstance(detections.get(k), torch.Tensor) for k in ("rotation", "translation")):
        raise ValueError(f"{who}: detections lack 'rotation' or 'translation'")
    rot, trn = detections["rotation"], detections["translation"]
    if rot.dtype != torch.float32 or trn.dtype != torch.float32 or rot.dim() != 3 or rot.shape[0] != B or rot.shape[1] < 1 or rot.shape[2] != 3 \
            or tuple(trn.shape) != tuple(rot.shape) or rot.device != dev or trn.device != dev:
        raise ValueError(f"{who}: rotation and translation must be float32 tensors [{B},rows,3] on {dev}")
    if camera is not None and (not isinstance(camera, torch.Tensor) or camera.dtype != torch.float64 or camera.dim() != 2 or camera.shape[0] != B
                               or camera.shape[1] < 4 or camera.device != dev):
        raise ValueError(f"{who}: camera must be a float64 tensor [{B},4 or more] on {dev}")
    rows = int(rot.shape[1])
    matched = (records[..., 0] == 1.0) & (records[..., 1] == 1.0)
    row = torch.where(matched, records[..., 2], torch.zeros_like(records[..., 2])).clamp(0, rows - 1).long()
    index = row[..., None].expand(B, A, 3)
    rv = torch.gather(rot, 1, index) * torch.tensor(math.pi, dtype=torch.float32, device=dev)      # float32
    tv = torch.gather(trn, 1, index)
    out = torch.zeros((B, A, PAIR_DOUBLES), dtype=torch.float64, device=dev)
    out[..., 0], out[..., 1] = matched.to(torch.float64), records[..., 12]
    out[..., 2] = torch.arange(B, dtype=torch.float64, device=dev)[:, None]
    out[..., 4:13], out[..., 13:16] = _rodrigues(gt[..., 5:8]), gt[..., 8:11]
    out[..., 16:25], out[..., 25:28] = _rodrigues(rv.to(torch.float64)), tv.to(torch.float64)
    out[..., 28:32] = gt[..., 14:18] if camera is None else camera[:, None, :4]
    return out.reshape(B * A, PAIR_DOUBLES)


_workspaces: Dict[tuple, torch.Tensor] = {}


def _workspace(dev, n: int, T: int) -> torch.Tensor:
    """The caller-owned counter workspace of one shape, kept: launches on one stream are ordered, so successive calls may share it."""
    key = (dev, n, T)
    ws = _workspaces.get(key)
    if ws is None:
        if len(_workspaces) >= 8:
            _workspaces.clear()
        ws = _workspaces[key] = torch.empty((_capi.check(_capi.lib().hep_bop_workspace_bytes(n, T)),), dtype=torch.uint8, device=dev)
    return ws


def _taus(who: str, taus, num_labels: int) -> np.ndarray:
    t = np.asarray(taus, np.float64)
    if t.ndim == 1:
        t = np.broadcast_to(t, (num_labels,) + t.shape)
    if t.ndim != 2 or t.shape[0] != num_labels or not 1 <= t.shape[1] <= MAX_TAUS or not np.isfinite(t).all() or not (t > 0).all():
        raise ValueError(f"{who}: taus must be 1..{MAX_TAUS} finite positive numbers, or one such row per label [{num_labels},T]")
    return np.ascontiguousarray(t)


def bop_errors(pairs: torch.Tensor, meshes: MeshSet, symmetries: SymmetrySet, height: int, width: int, depth_test: Optional[torch.Tensor] = None,
               delta: float = 15.0, taus=(20.0,), chunk: int = 64) -> Dict[str, torch.Tensor]:
    """MSSD, MSPD and VSD of the pair table ``pairs`` (float64 [n,32] on the meshes' device: ``pairs_from_scene``).  The depth maps of the
    ground truth and of the estimate are rendered through ``render_models`` with one pose per image, ``chunk`` pairs at a time, so that
    the two float32 [chunk,height,width] buffers stay bounded.  ``depth_test``: float32 [images,height,width] in the model's unit (0: no
    measurement), addressed by each pair's image index, or None: everything rendered is visible.  ``delta`` and ``taus`` are in the
    model's unit; ``taus`` is a sequence of 1..16 numbers, or an array [labels,T] with a row per label (the VSD launch then runs once
    per label).  Returns ``{"mssd": [n], "mspd": [n], "vsd": [n,T]}`` float64 and ``"counts"`` int32 [n,2+T] (union, intersection, cost
    per tau) on the device; a skipped row holds NaN and -1.  Raises ValueError for a wrong dtype, device or shape before the library
    sees a pointer; enqueues on the current stream and does not synchronise."""
    who = "bop_errors"
    if not isinstance(meshes, MeshSet) or getattr(meshes, "vertex_start", None) is None:
        raise ValueError(f"{who}: meshes must be a MeshSet (with its vertex_start table)")
    dev = meshes.device
    if not isinstance(symmetries, SymmetrySet) or symmetries.device != dev or symmetries.num_labels != meshes.num_labels:
        raise ValueError(f"{who}: symmetries must be a SymmetrySet of {meshes.num_labels} labels on {dev}")
    if not isinstance(pairs, torch.Tensor) or pairs.dtype != torch.float64 or pairs.dim() != 2 or pairs.shape[1] != PAIR_DOUBLES or pairs.shape[0] < 1 or pairs.device != dev:
        raise ValueError(f"{who}: pairs must be a float64 tensor [n,{PAIR_DOUBLES}] on {dev} with n >= 1")
    H, W = int(height), int(width)
    if not (16 <= H <= 4096 and 16 <= W <= 4096):
        raise ValueError(f"{who}: {H} x {W}: height and width must be in 16..4096")
    if depth_test is not None and (not isinstance(depth_test, torch.Tensor) or depth_test.dtype != torch.float32 or depth_test.dim() != 3 or depth_test.shape[0] < 1
                                   or tuple(depth_test.shape[1:]) != (H, W) or depth_test.device != dev or not depth_test.is_contiguous()):
        raise ValueError(f"{who}: depth_test must be a contiguous float32 tensor [images,{H},{W}] on {dev}")
    if not (isinstance(delta, (int, float)) and math.isfinite(delta) and delta > 0):
        raise ValueError(f"{who}: delta must be finite and positive")
    L = meshes.num_labels
    tau = _taus(who, taus, L)
    T = int(tau.shape[1])
    per_label = any(not np.array_equal(tau[l], tau[0]) for l in range(1, L))
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"{who}: chunk must be >= 1")
    pairs = pairs.contiguous()
    n = int(pairs.shape[0])
    lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    as_i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    errors = torch.empty((n, 2), dtype=torch.float64, device=dev)
    _capi.check(lib.hep_bop_point_errors_device(pairs.data_ptr(), n, meshes.vertices.data_ptr(), meshes.num_vertices, as_i32(meshes.vertex_start),
                                                symmetries.table.data_ptr(), symmetries.num_symmetries, as_i32(symmetries.start), L, errors.data_ptr(), stream))
    vsd = torch.empty((n, T), dtype=torch.float64, device=dev)
    counts = torch.empty((n, 2 + T), dtype=torch.int32, device=dev)
    for c0 in range(0, n, chunk):
        p = pairs[c0:c0 + chunk]
        m = int(p.shape[0])
        cam = torch.ones((m, 5), dtype=torch.float64, device=dev)
        cam[:, :4] = p[:, 28:32]
        depth = []
        for o in (4, 16):                                             # the ground truth's pose, then the estimate's: one pose per image, mask value 1
            poses = torch.zeros((m, 1, 16), dtype=torch.float64, device=dev)
            poses[:, 0, 0], poses[:, 0, 1], poses[:, 0, 2] = p[:, 0], p[:, 1], 1.0
            poses[:, 0, 4:16] = p[:, o:o + 12]
            depth.append(render_models(poses, cam, meshes, H, W, mask=False, depth=True)["depth"])
        ws = _workspace(dev, m, T)

        def launch(table, row, out_vsd, out_counts):
            t = np.ascontiguousarray(tau[row])
            _capi.check(lib.hep_bop_vsd_device(table.data_ptr(), m, L, depth[0].data_ptr(), depth[1].data_ptr(), _capi.ptr(depth_test),
                                               0 if depth_test is None else int(depth_test.shape[0]), H, W, float(delta),
                                               t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), T, out_vsd.data_ptr(), out_counts.data_ptr(),
                                               ws.data_ptr(), ws.numel(), stream))
        if not per_label:
            launch(p, 0, vsd[c0:c0 + m], counts[c0:c0 + m])
            continue
        vsd[c0:c0 + m], counts[c0:c0 + m] = float("nan"), -1
        for l in range(L):                                            # the taus are the label's: the rows of the other labels are switched off
            own = p[:, 1] == float(l)
            q = p.clone()
            q[:, 0] = torch.where(own, p[:, 0], torch.zeros_like(p[:, 0]))
            v_l, c_l = torch.empty((m, T), dtype=torch.float64, device=dev), torch.empty((m, 2 + T), dtype=torch.int32, device=dev)
            launch(q, l, v_l, c_l)
            vsd[c0:c0 + m] = torch.where(own[:, None], v_l, vsd[c0:c0 + m])
            counts[c0:c0 + m] = torch.where(own[:, None], c_l, counts[c0:c0 + m])
    return {"mssd": errors[:, 0], "mspd": errors[:, 1], "vsd": vsd, "counts": counts}


class BopSettings:
    """What the evaluators' ``add(..., bop=)`` takes: the ``MeshSet`` and the ``SymmetrySet`` of the labels, VSD's ``delta`` (model unit,
    BOP's 15 mm) and the tau fractions of the diameter (BOP19's 0.05..0.5), and the size of the ORIGINAL images the ground truth's camera
    belongs to - ``height`` / ``width`` may be left out when ``add`` gets uint8 frames (their size is taken) or else a ``depth_test`` (its size)."""

    def __init__(self, meshes: MeshSet, symmetries: SymmetrySet, delta: float = 15.0, tau_fractions: Sequence[float] = TAU_FRACTIONS,
                 height: Optional[int] = None, width: Optional[int] = None, chunk: int = 64):
        if not isinstance(meshes, MeshSet) or not isinstance(symmetries, SymmetrySet) or symmetries.num_labels != meshes.num_labels or symmetries.device != meshes.device:
            raise ValueError("BopSettings: a MeshSet and a SymmetrySet of the same labels on the same device")
        f = np.asarray(tau_fractions, np.float64)
        if f.ndim != 1 or not 1 <= f.size <= MAX_TAUS or not np.isfinite(f).all() or not (f > 0).all():
            raise ValueError(f"BopSettings: tau_fractions must be 1..{MAX_TAUS} finite positive numbers")
        if not (isinstance(delta, (int, float)) and math.isfinite(delta) and delta > 0):
            raise ValueError("BopSettings: delta must be finite and positive")
        if (height is None) != (width is None):
            raise ValueError("BopSettings: height and width come together")
        self.meshes, self.symmetries, self.delta, self.tau_fractions = meshes, symmetries, float(delta), f
        self.height, self.width, self.chunk = height, width, int(chunk)


def check_settings(who: str, bop, depth_test, frames, dev, num_labels: int):
    """The ``bop`` and ``depth_test`` arguments of the evaluators' ``add``, checked before anything is launched.  Returns (height, width)."""
    if bop is None:
        if depth_test is not None:
            raise ValueError(f"{who}: depth_test without bop")
        return None
    if not isinstance(bop, BopSettings) or bop.meshes.device != dev or bop.meshes.num_labels != num_labels:
        raise ValueError(f"{who}: bop must be a BopSettings whose sets hold the evaluator's {num_labels} labels on {dev}")
    if bop.height is not None:
        H, W = int(bop.height), int(bop.width)
    elif isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.dim() == 4:
        H, W = int(frames.shape[1]), int(frames.shape[2])
    elif isinstance(depth_test, torch.Tensor) and depth_test.dim() == 3:
        H, W = int(depth_test.shape[1]), int(depth_test.shape[2])
    else:
        raise ValueError(f"{who}: bop needs the original image size: BopSettings(height=, width=), uint8 frames or a depth_test")
    if not (16 <= H <= 4096 and 16 <= W <= 4096):
        raise ValueError(f"{who}: bop: {H} x {W}: height and width must be in 16..4096")
    B = int(frames.shape[0]) if isinstance(frames, torch.Tensor) and frames.dim() == 4 else -1
    if depth_test is not None and (not isinstance(depth_test, torch.Tensor) or depth_test.dtype != torch.float32 or tuple(depth_test.shape) != (B, H, W)
                                   or depth_test.device != dev or not depth_test.is_contiguous()):
        raise ValueError(f"{who}: depth_test must be a contiguous float32 tensor [{B},{H},{W}] on {dev}, one image per frame")
    return H, W


def score_batch(bop: BopSettings, size, gt: torch.Tensor, detections: Dict[str, torch.Tensor], records: torch.Tensor, diameters: Sequence[float],
                depth_test: Optional[torch.Tensor], out: torch.Tensor) -> None:
    """One batch of an evaluator: the pairs of ``records``, their errors, and ``out`` float64 [B,amax,2+T] = MSSD, MSPD, VSD per tau."""
    pairs = pairs_from_scene(gt, detections, records)
    tau = np.asarray(diameters, np.float64)[:, None] * bop.tau_fractions[None, :]
    e = bop_errors(pairs, bop.meshes, bop.symmetries, size[0], size[1], depth_test=depth_test, delta=bop.delta, taus=tau, chunk=bop.chunk)
    B, A = int(gt.shape[0]), int(gt.shape[1])
    out[..., 0], out[..., 1] = e["mssd"].view(B, A), e["mspd"].view(B, A)
    out[..., 2:] = e["vsd"].view(B, A, -1)


def _recall(errors: np.ndarray, num: float, thresholds) -> float:
    return float(np.mean([np.count_nonzero(errors < th) / num for th in thresholds]))


def summarise_bop(rec: np.ndarray, errors: np.ndarray, diameters: Sequence[float], width: int) -> Dict[str, dict]:
    """The host tail of the evaluators' ``"bop"`` entry: ``rec`` [n,amax,16] (slot 0 valid, 1 matched, 12 label) and ``errors``
    [n,amax,2+T].  Per label ``AR_VSD`` (the recall of VSD(tau) < threshold, averaged over every tau and the correctness thresholds
    0.05..0.5), ``AR_MSSD`` (MSSD < 0.05..0.5 of the diameter), ``AR_MSPD`` (MSPD < 5r..50r pixels, r = width / 640) and their mean
    ``AR``; recall counts EVERY valid annotation of the label - one without a match, or with a NaN error, is a miss; NaN for a label
    without annotations.  ``"mean"``: each key averaged over the labels that have annotations."""
    flat, err = rec.reshape(-1, rec.shape[-1]), errors.reshape(-1, errors.shape[-1])
    correct = np.arange(0.05, 0.51, 0.05)
    pixels = np.arange(5, 51, 5) * (width / 640.0)
    nan = float("nan")
    labels = {}
    for l, dia in enumerate(diameters):
        ann = (flat[:, 0] == 1.0) & (flat[:, 12] == l)
        num = float(np.count_nonzero(ann))
        if num == 0:
            labels[l] = dict(AR_VSD=nan, AR_MSSD=nan, AR_MSPD=nan, AR=nan, num_annotations=0.0)
            continue
        e = err[ann & (flat[:, 1] == 1.0)]
        d = dict(AR_VSD=float(np.mean([_recall(e[:, 2 + j], num, correct) for j in range(e.shape[1] - 2)])),
                 AR_MSSD=_recall(e[:, 0], num, correct * dia), AR_MSPD=_recall(e[:, 1], num, pixels))
        d["AR"] = (d["AR_VSD"] + d["AR_MSSD"] + d["AR_MSPD"]) / 3.0
        d["num_annotations"] = num
        labels[l] = d
    have = [d for d in labels.values() if d["num_annotations"] > 0]
    mean = {k: (sum(d[k] for d in have) / len(have) if have else nan) for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")}
    mean["num_annotations"] = float(sum(d["num_annotations"] for d in labels.values()))
    return {"labels": labels, "mean": mean}


def folder_settings(who: str, model_path: str, object_ids, models_info, device, max_sym_disc_step: float = 0.01, **kw) -> BopSettings:
    """``BopSettings`` of a dataset folder's ``models/``: the PLY meshes and the symmetry sets of ``models_info.yml``, one label per object."""
    from .evaluate import _folder_meshes
    try:
        meshes = _folder_meshes(who, model_path, object_ids, device)
    except ValueError as e:
        raise ValueError(str(e).replace("draw_model", "bop")) from None
    return BopSettings(meshes, SymmetrySet([symmetry_transforms(i, max_sym_disc_step) for i in models_info], device), **kw)
