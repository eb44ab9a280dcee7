"""Evaluator for the MI355X inference path: the host side of the reference's ``evaluate.py`` loop.

What the reference does per image (pytorch-sandbox/eval/common.py:357-447, 866-1121; evaluate.py:58-128) and where
it runs here:

  load + preprocess           Linemod-style folder reader below; uint8 -> normalised fp32 on the GPU
                              (``Session.preprocess``, hep_preprocess_u8_device)
  forward / decode / filter   libhep kernels (``TrainModelWithLoss.detect``)
  post-filter (a15)           ``post_filter``: boxes /= scale, rotations *= pi, score > threshold, score order,
                              first max_detections (eval/common.py:419-447)
  matching                    ``compute_overlap`` (IoU with the +1 pixel convention of
                              generators/utils/compute_overlap.pyx:33-73), greedy by score like common.py:942-957
  ADD / ADD-S                 hep_pose_errors on the GPU (csrc/k_eval.hip; eval/common.py:682-746,
                              calc_min_distances.h:24-35)
  5 cm / 5 degree, t / R diff ``calc_rotation_diff`` etc. below (eval/common.py:750-778,829-833), float64 numpy
  2D reprojection             ``reprojection_distance`` (eval/common.py:646-679): cv2.projectPoints with zero rotation, translation
                              and distortion is the pinhole projection u = fx X / Z + cx, v = fy Y / Z + cy (float64)
  hand joints                 mean end-point error over the 21 joints in mm (eval/common.py:970-982), ground truth from the
                              dataset's ``hands/<frame>_coords_3d.npy`` (generators/colibri.py:430-436)
  AP                          ``compute_ap`` (eval/common.py:328-354)

``evaluate_device`` / ``DeviceEvaluator`` run the same loop with matching and EVERY metric above on the GPU - one launch of
hep_score_detections_device per batch (csrc/k_score.hip), one device-to-host copy per evaluation - and add the keys train.py
reports and steers by (``ADD(-S)``, ``mixed_distance_mean`` / ``_std``, ``translation_tip_std``; train.py:255-334).
``evaluate_scene_device`` / ``SceneEvaluator`` / ``SceneFolder`` do it for scenes - several annotations per image over several labels,
every label scored in ONE launch of hep_score_scene_device per batch, each detection assigned to the annotation of its label it
overlaps most (eval/common.py:953-960), per-label dictionaries and evaluate_model's average of them (eval/common.py:92-265);
``--object-ids 1,5,6`` on the command line.

``python -m hmd_ego_pose_amd.evaluate --dataset-path <object folder> --weights ckpt.pth --phi 0`` runs it on a
supplied dataset; nothing ships with the reference (dataset, checkpoint and mesh are absent), so the numbers of the
paper cannot be reproduced here - tests drive this module with a synthetic folder.

  drawing (eval/common.py:452-479)  ``save_path`` of ``evaluate_device`` / ``evaluate_scene_device`` (``--save-images DIR``): ground truth and kept
                              detections drawn into the frames on the GPU by ONE launch of hep_draw_poses_device per batch
                              (``draw_into`` of the evaluators' ``add``; hmd_ego_pose_amd/draw.py), written as ``<i>.png``
  filled models (no counterpart)    ``draw_model`` (``--draw-model``; ``meshes`` of the evaluators' ``add``): the model mesh of every kept detection
                              under its pose blended in beneath the lines by hep_render_models_device (hmd_ego_pose_amd/render.py)

Not reproduced: ``draw_samplevis`` / MANO hand meshes (eval/common.py:481-590), captions and anti-aliased lines; ``cv2.Rodrigues`` and
``cv2.projectPoints`` are restated, and the overlays' line and disc rasterisation is this project's own integer definition, not
``cv2.line`` / ``cv2.circle`` (parity unpinned: cv2 is absent from the build image).
"""
from __future__ import annotations

import argparse
import ctypes
import math
import os
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi


# ----------------------------------------------------------------------------------------------------------------
# small host-side pieces of eval/common.py
# ----------------------------------------------------------------------------------------------------------------
def post_filter(det: Dict[str, torch.Tensor], scale: float, score_threshold: float = 0.05, max_detections: int = 10):
    """``_get_detections`` after the model call, eval/common.py:419-447, for ONE image: ``det`` holds the padded rows of
    the detection filter (boxes [M,4], scores [M], labels [M], rotation [M,3], translation [M,3], hand [M,63]; padding
    rows carry -1).  Returns numpy arrays (boxes, scores, labels, rotations in radians, translations, hands) of the
    rows with score > threshold in descending score order (equal scores: lower row first), at most max_detections."""
    boxes = det["boxes"].detach().cpu().numpy().astype(np.float32) / np.float32(scale)
    scores = det["scores"].detach().cpu().numpy().astype(np.float32)
    rotations = det["rotation"].detach().cpu().numpy().astype(np.float32) * np.float32(math.pi)
    ind = np.nonzero(scores > score_threshold)[0]
    order = np.argsort(-scores[ind], kind="stable")[:max_detections]
    sel = ind[order]
    return (boxes[sel], scores[sel], det["labels"].detach().cpu().numpy()[sel], rotations[sel],
            det["translation"].detach().cpu().numpy()[sel], det["hand"].detach().cpu().numpy()[sel])


def compute_overlap(boxes: np.ndarray, query_boxes: np.ndarray) -> np.ndarray:
    """IoU matrix [N,K] with the "+1" pixel convention of generators/utils/compute_overlap.pyx:33-73 (float64)."""
    b = np.asarray(boxes, dtype=np.float64)[:, None, :]
    q = np.asarray(query_boxes, dtype=np.float64)[None, :, :]
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0]) + 1
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1]) + 1
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
    ua = (b[..., 2] - b[..., 0] + 1) * (b[..., 3] - b[..., 1] + 1) + (q[..., 2] - q[..., 0] + 1) * (q[..., 3] - q[..., 1] + 1) - inter
    return np.where(inter > 0, inter / ua, 0.0)


def compute_ap(recall: np.ndarray, precision: np.ndarray) -> float:
    """py-faster-rcnn average precision as used at eval/common.py:328-354."""
    mrec = np.concatenate(([0.], recall, [1.]))
    mpre = np.concatenate(([0.], precision, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def axis_angle_to_matrix(rvec: Sequence[float]) -> np.ndarray:
    """cv2.Rodrigues (vector -> matrix) restated, float64 (colibri_common.py:803-813)."""
    r = np.asarray(rvec, dtype=np.float64).reshape(3)
    th = float(np.linalg.norm(r))
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) * math.cos(th) + (1 - math.cos(th)) * np.outer(k, k) + math.sin(th) * K


def matrix_to_axis_angle(R: np.ndarray) -> np.ndarray:
    """cv2.Rodrigues (matrix -> vector) restated, float64 (colibri_common.py:791-801)."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(v)) / 2.0, (np.trace(R) - 1.0) / 2.0
    th = math.atan2(s, c)                        # well conditioned at 0 and at pi (acos of the trace is not)
    if s < 1e-10:
        if c > 0:
            return v / 2.0                       # theta -> 0: r = vee(R - R^T) / 2
        A = (R + np.eye(3)) / 2.0                # theta -> pi: the antisymmetric part vanishes, the axis comes from R + I = 2 k k^T
        k = np.sqrt(np.maximum(np.diag(A), 0.0))
        i = int(np.argmax(k))
        k = A[i] / max(k[i], 1e-300)
        if np.dot(k, v) < 0:
            k = -k
        return k / np.linalg.norm(k) * th
    return v / (2.0 * s) * th


def calc_rotation_diff(R_gt: np.ndarray, R_pr: np.ndarray) -> float:
    """Angular distance in degrees, eval/common.py:762-778."""
    tr = (np.trace(np.dot(R_pr, R_gt.T)) - 1.0) / 2.0
    return abs(float(np.rad2deg(np.arccos(min(1.0, max(-1.0, tr))))))


def reprojection_distance(points: np.ndarray, R_gt: np.ndarray, t_gt: np.ndarray, R_pr: np.ndarray, t_pr: np.ndarray, K: np.ndarray) -> float:
    """Mean pixel distance between the model points projected with the two poses (check_6d_pose_2d_reprojection,
    eval/common.py:646-679; correct when <= 5 px).  Pinhole projection, float64."""
    K = np.asarray(K, dtype=np.float64)

    def project(R, t):
        p = np.dot(np.asarray(points, np.float64), np.asarray(R, np.float64).T) + np.asarray(t, np.float64).reshape(1, 3)
        return np.stack([K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]], axis=-1)
    return float(np.linalg.norm(project(R_gt, t_gt) - project(R_pr, t_pr), axis=-1).mean())


def pose_errors(points: np.ndarray, rvec_gt: np.ndarray, t_gt: np.ndarray, rvec_pr: np.ndarray, t_pr: np.ndarray,
                device: int = 0, max_points: int = 1000) -> Tuple[np.ndarray, np.ndarray]:
    """ADD and ADD-S mean distances of D pose pairs on the GPU (hep_pose_errors).  Rotations: axis-angle, radians."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3) for a in (rvec_gt, t_gt, rvec_pr, t_pr)]
    d = arrs[0].shape[0]
    add, add_s = np.zeros(d, np.float64), np.zeros(d, np.float64)
    _capi.check(_capi.lib().hep_pose_errors(device, pts.ctypes.data, pts.shape[0], *[a.ctypes.data for a in arrs], d, max_points,
                                            add.ctypes.data, add_s.ctypes.data))
    return add, add_s


# ----------------------------------------------------------------------------------------------------------------
# Linemod-style object folder (generators/colibri.py:60-120,293-443,460-510)
# ----------------------------------------------------------------------------------------------------------------
def load_ply_vertices(path: str) -> np.ndarray:
    """x, y, z of every vertex of an ASCII or binary-little-endian PLY file (generators/colibri.py:293-307)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, n, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    n = int(tok[2])
            elif tok[0] == "property" and in_vertex and tok[1] != "list":
                props.append((tok[2], tok[1]))
            elif tok[0] == "end_header":
                break
        names = [p[0] for p in props]
        if not all(k in names for k in "xyz"):
            raise ValueError(f"{path}: vertex element has no x/y/z")
        if fmt == "ascii":
            rows = np.loadtxt(f, max_rows=n, ndmin=2)
            return np.stack([rows[:, names.index(k)] for k in "xyz"], axis=-1).astype(np.float32)
        if fmt != "binary_little_endian":
            raise ValueError(f"{path}: unsupported PLY format {fmt}")
        code = {"float": "f4", "float32": "f4", "double": "f8", "float64": "f8", "uchar": "u1", "uint8": "u1", "char": "i1", "int8": "i1",
                "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4"}
        dt = np.dtype([(nm, "<" + code[ty]) for nm, ty in props])
        v = np.frombuffer(f.read(n * dt.itemsize), dtype=dt, count=n)
        return np.stack([v["x"], v["y"], v["z"]], axis=-1).astype(np.float32)


def _model_cuboid(info: dict) -> Optional[np.ndarray]:
    """The model cuboid of one models_info.yml entry (``min_x`` .. ``size_z``) as ``draw.cuboid_corners``, or None when the entry lacks it."""
    keys = [p + a for p in ("min_", "size_") for a in "xyz"]
    if not all(k in info for k in keys):
        return None
    from .draw import cuboid_corners
    v = [float(info[k]) for k in keys]
    return cuboid_corners(v[:3], v[3:])


class _Folder:
    """What ``LinemodFolder`` and ``SceneFolder`` read alike of ``<root>/data/<NN>/`` and ``<root>/models/``: the split, ground-truth, camera
    and model files, the frames of the split (``image_paths``), one camera matrix and one ``_annotation`` per frame.  The readers supply
    ``_read_models`` (what they keep of models_info.yml and the PLY files) and ``_annotation`` (a frame's ground-truth entries -> its annotation)."""

    def __init__(self, dataset_path: str, folder_id: int, fold: int, split: str, image_extension: str):
        import yaml
        loader = getattr(yaml, "CSafeLoader", yaml.SafeLoader)
        self.object_path = os.path.join(dataset_path, "data", f"{folder_id:02}")
        self.model_path = os.path.join(dataset_path, "models")
        with open(os.path.join(self.object_path, f"{split}_{fold}.txt")) as f:
            examples = [e.strip() for e in f if e.strip()]
        with open(os.path.join(self.object_path, f"gt_{fold}.yml")) as f:
            gt = yaml.load(f, Loader=loader)
        with open(os.path.join(self.object_path, f"info_{fold}.yml")) as f:
            info = yaml.load(f, Loader=loader)
        with open(os.path.join(self.model_path, "models_info.yml")) as f:
            self._read_models(yaml.load(f, Loader=loader))
        names = sorted(n for n in os.listdir(os.path.join(self.object_path, "rgb"))
                       if n.endswith(image_extension) and n[:-len(image_extension)] in examples)
        self.image_paths = [os.path.join(self.object_path, "rgb", n) for n in names]
        self.annotations, self.camera = [], []
        for n in names:
            key = int(n.split(".")[0])
            self.annotations.append(self._annotation(n, gt[key], image_extension))
            self.camera.append(np.array(info[key]["cam_K"], dtype=np.float64).reshape(3, 3))

    @staticmethod
    def _pose(a: dict) -> dict:
        """The pose keys of an annotation from one ground-truth entry."""
        R = np.array(a["cam_R_m2c"], dtype=np.float64).reshape(3, 3)
        return {"rotation": matrix_to_axis_angle(R), "translation": np.array(a["cam_t_m2c"], dtype=np.float64),
                "drill_tip": np.array(a.get("drill_tip_transform", [0, 0, 0, 1]), dtype=np.float64)}

    @staticmethod
    def _obj_bb(a: dict) -> np.ndarray:
        """Linemod's own field: x, y, w, h."""
        x, y, w, h = a["obj_bb"]
        return np.array([x, y, x + w, y + h], dtype=np.float32)

    @staticmethod
    def _mask_box(inside: np.ndarray) -> np.ndarray:
        """get_bbox_from_mask, colibri_common.py:540-561: (min_x, min_y, max_x, max_y) of the pixels that are set."""
        ys, xs = np.nonzero(inside)
        if ys.size == 0:
            return np.zeros(4, np.float32)
        return np.array([xs.min(), ys.min(), xs.max(), ys.max()], dtype=np.float32)

    def __len__(self):
        return len(self.image_paths)

    def load_image(self, i: int) -> np.ndarray:
        """uint8 RGB [H,W,3] (the reference reads BGR with cv2 and flips, colibri.py:546-552)."""
        from PIL import Image
        return np.asarray(Image.open(self.image_paths[i]).convert("RGB"))

    def camera_input(self, i: int, image_scale: float, translation_scale_norm: float = 1000.0) -> np.ndarray:
        """get_camera_parameter_input, colibri_common.py:658-678: [fx, fy, px, py, translation_scale_norm, image_scale]."""
        K = self.camera[i]
        return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], translation_scale_norm, image_scale], dtype=np.float32)


class LinemodFolder(_Folder):
    """One object of a Linemod-format dataset as the reference's ColibriGenerator reads it: ``<root>/data/<NN>/`` with
    ``rgb/*.png``, ``mask/*.png``, ``gt_<fold>.yml``, ``info_<fold>.yml``, ``test_<fold>.txt`` and
    ``<root>/models/obj_<NN>.ply`` + ``models_info.yml``."""

    def __init__(self, dataset_path: str, object_id: int = 1, fold: int = 0, split: str = "test", image_extension: str = ".png"):
        self.object_id = object_id
        super().__init__(dataset_path, object_id, fold, split, image_extension)

    def _read_models(self, models: dict) -> None:
        self.diameter = float(models[self.object_id]["diameter"])
        self.cuboid = _model_cuboid(models[self.object_id])            # float32 [8,3], or None without min_* / size_*
        self.points = load_ply_vertices(os.path.join(self.model_path, f"obj_{self.object_id:02}.ply"))

    def _annotation(self, n: str, entries: list, image_extension: str) -> dict:
        """The FIRST entry of the folder's object; its box from the frame's mask where there is one."""
        annos = [a for a in entries if a["obj_id"] == self.object_id]
        if not annos:
            raise ValueError(f"no annotation of object {self.object_id} for frame {n}")
        entry = self._pose(annos[0])
        mask_path = os.path.join(self.object_path, "mask", n)
        entry["bbox"] = self._bbox_from_mask(mask_path) if os.path.exists(mask_path) else self._obj_bb(annos[0])
        hands_path = os.path.join(self.object_path, "hands", n[:-len(image_extension)] + "_coords_3d.npy")      # generators/colibri.py:430-436
        if os.path.exists(hands_path):
            entry["coords_3d"] = np.load(hands_path).astype(np.float64).reshape(21, 3)
        return entry

    @classmethod
    def _bbox_from_mask(cls, path: str) -> np.ndarray:
        """The box of the non-zero pixels of a mask file, whichever channel they are in."""
        from PIL import Image
        m = np.asarray(Image.open(path))
        return cls._mask_box(m.reshape(m.shape[0], m.shape[1], -1).max(axis=2))


# ----------------------------------------------------------------------------------------------------------------
# the evaluation loop
# ----------------------------------------------------------------------------------------------------------------
def evaluate(dataset: LinemodFolder, model, image_size: int, score_threshold: float = 0.05, max_detections: int = 10,
             iou_threshold: float = 0.5, diameter_threshold: float = 0.1, batch_size: int = 16, device: Optional[torch.device] = None,
             detections_out: Optional[list] = None) -> Dict[str, float]:
    """eval/common.py:866-1121 for the single-class datasets of the reference.  ``model`` is a
    ``hmd_ego_pose_amd.TrainModelWithLoss`` (eval mode, on the GPU).  Frames must not need a resize
    (max(H, W) == image_size) unless the session's preprocess supports it.  Returns the metric dictionary."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    n = len(dataset)
    all_det = []
    for i0 in range(0, n, batch_size):
        idx = list(range(i0, min(n, i0 + batch_size)))
        frames = [dataset.load_image(i) for i in idx]
        h, w = frames[0].shape[:2]
        if any(f.shape[:2] != (h, w) for f in frames):
            raise ValueError("frames of one batch must share a size")
        scale = image_size / max(h, w)
        u8 = torch.from_numpy(np.stack(frames)).to(device)
        x = model.model.session(image_size, len(idx), device).preprocess(u8)
        cam = torch.from_numpy(np.stack([dataset.camera_input(i, scale) for i in idx])).to(device)
        det = model.detect(x, cam)
        for j in range(len(idx)):
            all_det.append(post_filter({k: v[j] for k, v in det.items() if k != "count" and k != "index"}, scale, score_threshold, max_detections))
    if detections_out is not None:
        detections_out.extend(all_det)

    tp, scores = [], []
    pairs = []                      # (rvec_gt, t_gt, rvec_pr, t_pr, drill_tip) of every correct 2D detection
    pair_cam, hand_err = [], []     # its camera matrix; mean joint distance in mm where the dataset carries hand joints
    for i, (boxes, sc, labels, rots, trans, hands) in enumerate(all_det):
        # eval/common.py:603-611: detections are split by label and only the generator's labels are evaluated; the object
        # folders of the reference hold ONE object (label 0), so rows a many-class model labels otherwise are dropped
        own = labels == 0
        boxes, sc, rots, trans, hands = boxes[own], sc[own], rots[own], trans[own], hands[own]
        ann = dataset.annotations[i]
        detected = False
        for d in range(boxes.shape[0]):
            scores.append(float(sc[d]))
            ov = compute_overlap(boxes[d:d + 1], ann["bbox"][None])[0, 0]
            if ov >= iou_threshold and not detected:
                detected = True
                tp.append(1)
                pairs.append((ann["rotation"], ann["translation"], rots[d].astype(np.float64), trans[d].astype(np.float64), ann["drill_tip"]))
                pair_cam.append(dataset.camera[i])
                if "coords_3d" in ann:       # eval/common.py:970-982: mean over the 21 joints of |gt - pred|, metres -> mm
                    hand_err.append(float(np.linalg.norm(ann["coords_3d"] - hands[d].astype(np.float64).reshape(21, 3), axis=-1).mean() * 1000.0))
            else:
                tp.append(0)
    m = None
    if pairs:
        rg, tg, rp, tpv, tips = (np.stack([p[k] for p in pairs]) for k in range(5))
        add, add_s = pose_errors(dataset.points, rg, tg, rp, tpv, device.index or 0)
        t_diff = np.linalg.norm(tg - tpv, axis=1)
        r_diff = np.array([calc_rotation_diff(axis_angle_to_matrix(a), axis_angle_to_matrix(b)) for a, b in zip(rg, rp)])
        tip_gt = np.stack([axis_angle_to_matrix(a) @ t[:3] + b for a, b, t in zip(rg, tg, tips)])
        tip_pr = np.stack([axis_angle_to_matrix(a) @ t[:3] + b for a, b, t in zip(rp, tpv, tips)])
        reproj = np.array([reprojection_distance(dataset.points, axis_angle_to_matrix(a), b, axis_angle_to_matrix(c), d_, K)
                           for a, b, c, d_, K in zip(rg, tg, rp, tpv, pair_cam)])
        m = dict(add=add, add_s=add_s, t_diff=t_diff, r_diff=r_diff, tip=np.linalg.norm(tip_gt - tip_pr, axis=1), reproj=reproj, hand=hand_err)
    return metric_summary(float(n), scores, tp, m, dataset.diameter * diameter_threshold)


def metric_summary(num_ann: float, scores, tp, m: Optional[dict], thr: float, symmetric: Optional[bool] = None) -> Dict[str, float]:
    """The tail of eval/common.py:1040-1121 shared by ``evaluate`` and ``DeviceEvaluator.result``: AP from the considered detections'
    scores and flags (stable sort by score), the accuracy fractions over ``num_ann`` and ``np.mean`` / ``np.std`` over the matched
    images in image order.  ``m``: the per-matched-image arrays add, add_s, t_diff, r_diff, tip, reproj and the list hand, or None
    without a match.  ``symmetric`` not None adds the keys train.py reports and steers by: ``translation_tip_std``, ``ADD(-S)`` and
    ``mixed_distance_mean`` / ``mixed_distance_std`` (the ADD-S values of a symmetric object, else ADD: eval/common.py:1105-1119)."""
    out: Dict[str, float] = {"num_annotations": num_ann, "num_matched": float(len(m["add"])) if m else 0.0}
    tp = np.asarray(tp, np.float64)
    order = np.argsort(-np.asarray(scores), kind="stable") if len(scores) else np.zeros(0, np.int64)
    tpc, fpc = np.cumsum(tp[order]), np.cumsum((1.0 - tp)[order])
    out["AP"] = compute_ap(tpc / num_ann, tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)) if num_ann else 0.0
    if m:
        add, add_s, t_diff, r_diff, tip, reproj, hand_err = (m[k] for k in ("add", "add_s", "t_diff", "r_diff", "tip", "reproj", "hand"))
        out["2D_projection"] = float(np.sum(reproj <= 5.0) / num_ann)
        out["2D_projection_distance_mean"] = float(reproj.mean())
        if len(hand_err):
            out["hand_mean"] = float(np.mean(hand_err)); out["hand_std"] = float(np.std(hand_err))
        out.update({"ADD": float(np.sum(add <= thr) / num_ann), "ADD-S": float(np.sum(add_s <= thr) / num_ann),
                    "5cm_5deg": float(np.sum((t_diff <= 50) & (r_diff <= 5)) / num_ann),
                    "translation_mean": float(t_diff.mean()), "translation_std": float(t_diff.std()),
                    "rotation_mean": float(r_diff.mean()), "rotation_std": float(r_diff.std()),
                    "translation_tip_mean": float(tip.mean()),
                    "ADD_distance_mean": float(add.mean()), "ADD_distance_std": float(add.std()),
                    "ADD-S_distance_mean": float(add_s.mean()), "ADD-S_distance_std": float(add_s.std())})
    else:
        out.update({"ADD": 0.0, "ADD-S": 0.0, "5cm_5deg": 0.0, "2D_projection": 0.0})
    if symmetric is not None:
        mixed = "ADD-S" if symmetric else "ADD"
        out["ADD(-S)"] = out[mixed]
        nan = float("nan")                          # the reference's np.mean of nothing
        out["translation_tip_std"] = float(tip.std()) if m else nan
        out["mixed_distance_mean"] = out[mixed + "_distance_mean"] if m else nan
        out["mixed_distance_std"] = out[mixed + "_distance_std"] if m else nan
    return out


# ----------------------------------------------------------------------------------------------------------------
# the same loop with matching and every pose metric on the GPU (hep_score_detections_device, csrc/k_score.hip)
# ----------------------------------------------------------------------------------------------------------------
GT_DOUBLES, RECORD_DOUBLES = _capi.SCORE_GT_DOUBLES, _capi.SCORE_RECORD_DOUBLES


def gt_table(annotations: Sequence[dict], cameras: Sequence[np.ndarray], scale) -> np.ndarray:
    """The ground-truth table of hep_score_detections_device, float64 [n, 88], from ``LinemodFolder``'s annotation dicts
    (``bbox``, ``rotation`` axis-angle, ``translation``, ``drill_tip``, optional ``coords_3d`` [21,3] in metres) and camera
    matrices.  ``scale``: the image scale of every frame (network size / longer image side), one number or one per image.
    Layout: include/hep.h.  One annotation per image."""
    n = len(annotations)
    if len(cameras) != n:
        raise ValueError("gt_table: one camera matrix per annotation")
    scales = np.broadcast_to(np.asarray(scale, np.float64), (n,))
    t = np.zeros((n, GT_DOUBLES), np.float64)
    for i, (ann, K) in enumerate(zip(annotations, cameras)):
        K = np.asarray(K, np.float64)
        t[i, 0] = 1.0
        t[i, 1:5] = np.asarray(ann["bbox"], np.float64).reshape(4)
        t[i, 5:8] = np.asarray(ann["rotation"], np.float64).reshape(3)
        t[i, 8:11] = np.asarray(ann["translation"], np.float64).reshape(3)
        t[i, 11:14] = np.asarray(ann["drill_tip"], np.float64).reshape(-1)[:3]
        t[i, 14:18] = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        t[i, 18] = scales[i]
        if "coords_3d" in ann:
            t[i, 19] = 1.0
            t[i, 20:83] = np.asarray(ann["coords_3d"], np.float64).reshape(63)
    return t


def _check_draw_into(who: str, draw_into, frames, cuboids, dev, max_detections: int) -> None:
    """The ``draw_into`` argument of the evaluators' ``add``, checked before anything is launched."""
    if draw_into is None:
        return
    if cuboids is None:
        raise ValueError(f"{who}: draw_into needs the evaluator's model cuboids")
    if (not isinstance(draw_into, torch.Tensor) or draw_into.dtype != torch.uint8 or draw_into.device != dev or draw_into.dim() != 4
            or draw_into.shape[3] != 3 or not draw_into.is_contiguous() or (isinstance(frames, torch.Tensor) and draw_into.shape[0] != frames.shape[0])):
        raise ValueError(f"{who}: draw_into must be a contiguous uint8 tensor [B,H,W,3] on {dev}, one image per frame")
    if not (16 <= draw_into.shape[1] <= 4096 and 16 <= draw_into.shape[2] <= 4096):
        raise ValueError(f"{who}: draw_into: height and width must be in 16..4096")
    if max_detections > _capi.DRAW_MAX_DETECTIONS:
        raise ValueError(f"{who}: draw_into draws at most {_capi.DRAW_MAX_DETECTIONS} detections per image, max_detections is {max_detections}")


def _check_meshes(who: str, meshes, draw_into, dev, max_detections: int) -> None:
    """The ``meshes`` argument of the evaluators' ``add``, checked before anything is launched."""
    if meshes is None:
        return
    from .render import MeshSet
    if draw_into is None:
        raise ValueError(f"{who}: meshes are blended into draw_into, which is missing")
    if not isinstance(meshes, MeshSet) or meshes.device != dev:
        raise ValueError(f"{who}: meshes must be a render.MeshSet on {dev}")
    if max_detections > _capi.RENDER_MAX_POSES:
        raise ValueError(f"{who}: meshes are rendered for at most {_capi.RENDER_MAX_POSES} detections per image, max_detections is {max_detections}")


def _blend_models(draw_into, meshes, gt0, d, score_threshold: float, max_detections: int) -> None:
    """The filled models of the kept detections blended into ``draw_into`` (hep_render_models_device) - before the lines are drawn.
    ``gt0``: row 0 of each image's ground-truth rows [B,88], whose slots 14-18 are the camera the draw call uses too."""
    from .render import poses_from_detections, render_models
    poses = poses_from_detections(dict(scores=d[1], labels=d[2], rotation=d[3], translation=d[4]), score_threshold, max_detections)
    render_models(poses, gt0[:, 14:19].contiguous(), meshes, int(draw_into.shape[1]), int(draw_into.shape[2]), mask=False, blend_into=draw_into)


def _folder_meshes(who: str, model_path: str, object_ids, device):
    """The ``draw_model`` argument of the folder evaluations: the triangle meshes of the folder's PLY files, one label per object."""
    from .render import MeshSet, load_ply_mesh
    meshes = []
    for o in object_ids:
        try:
            meshes.append(load_ply_mesh(os.path.join(model_path, f"obj_{o:02}.ply")))
        except ValueError as e:
            raise ValueError(f"{who}: draw_model needs triangle faces in the folder's PLY files ({e})") from None
    return MeshSet(meshes, device=device)


def _check_bop(who: str, bop, depth_test, frames, dev, num_labels: int):
    """The ``bop`` and ``depth_test`` arguments of the evaluators' ``add``, checked before anything is launched: the image size, or None."""
    if bop is None and depth_test is None:
        return None
    from .bop import check_settings
    return check_settings(who, bop, depth_test, frames, dev, num_labels)


def _score_bop(ev, bop, size, gt, d, records, diameters, depth_test, o: int) -> None:
    """MSSD, MSPD and VSD of a batch's matched pairs (``records`` [B,A,16]) into the evaluator's second buffer [capacity,A,2+T] at image offset ``o``."""
    from .bop import score_batch
    B, A, T = int(records.shape[0]), int(records.shape[1]), int(bop.tau_fractions.size)
    if ev._bop_buf is None or ev._bop_buf.shape[2] != 2 + T:
        ev._bop_buf = torch.full((ev.capacity, A, 2 + T), float("nan"), dtype=torch.float64, device=ev.device)
    score_batch(bop, size, gt, dict(rotation=d[3], translation=d[4]), records, diameters, depth_test, ev._bop_buf[o:o + B])
    ev._bop_count += B
    ev._bop_width = int(size[1])


def _bop_result(ev, who: str, rec: np.ndarray, diameters) -> Dict[str, dict]:
    """The ``"bop"`` entry of ``result``: one extra copy, then ``bop.summarise_bop``."""
    from .bop import summarise_bop
    if ev._bop_count != ev.count:
        raise ValueError(f"{who}: bop= was given for {ev._bop_count} of the {ev.count} images: give it to every add of an evaluation, or to none")
    return summarise_bop(rec, ev._bop_buf.cpu().numpy()[:ev.count], diameters, ev._bop_width)


def _matched_metrics(r: np.ndarray) -> Optional[dict]:
    """``metric_summary``'s ``m`` from the matched records [n,16] of either scoring kernel, or None without a match."""
    if not r.shape[0]:
        return None
    return dict(add=r[:, 5], add_s=r[:, 6], t_diff=r[:, 7], r_diff=r[:, 8], tip=r[:, 9], reproj=r[:, 10], hand=r[:, 11][~np.isnan(r[:, 11])])


_DETECTION_KEYS = ("boxes", "scores", "labels", "rotation", "translation", "hand")
_NUMPY = {torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32}          # the dtypes of the evaluators' buffer layouts


class _Evaluator:
    """What ``DeviceEvaluator`` and ``SceneEvaluator`` share: the settings, ONE allocation cut by a declared layout, and ``add`` - every
    check, preprocess, ``model.detect``, the scoring launch, then BOP, the mesh blend and the draw.  A subclass supplies ``_gt_shape`` (the
    per-image shape of ``gt``), ``num_labels``, ``_launch`` (its one library call), ``_bop_records`` and ``result``."""

    def __init__(self, model, image_size: int, capacity: int, score_threshold: float, max_detections: int, iou_threshold: float,
                 diameter_threshold: float, device: Optional[torch.device], max_points: int, draw_layers: int, draw_thickness: int):
        self.model, self.image_size, self.capacity = model, int(image_size), int(capacity)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.diameter_threshold = float(diameter_threshold)
        self.score_threshold, self.max_detections, self.iou_threshold = float(score_threshold), int(max_detections), float(iou_threshold)
        self.max_points = int(max_points)
        # ``add(..., draw_into=)``: the subclass's cuboids float32 [labels,8,3] on the device, the layers (HEP_DRAW_*) and line thickness of both
        # annotations and detections
        self._cuboids = None
        self.draw_layers, self.draw_thickness = int(draw_layers), int(draw_thickness)
        self.count = 0
        self._bop_buf, self._bop_count, self._bop_width = None, 0, 0      # ``add(..., bop=)``: errors [C,amax,2+T] float64, allocated on first use

    def _check_sizes(self, capacity: int, max_detections: int, max_points: int) -> None:
        """A constructor's first refusal, ahead of the subclass's own."""
        if capacity < 1 or max_detections < 1 or not 1 <= max_points <= 1024:
            raise ValueError(f"{type(self).__name__}: capacity and max_detections must be >= 1, max_points in 1..1024")

    def _points(self, points, what: str) -> np.ndarray:
        pts = np.ascontiguousarray(points, dtype=np.float32)
        if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
            raise ValueError(f"{type(self).__name__}: {what} must be [P,3] with P >= 1")
        return pts

    def _allocate(self, layout) -> None:
        """ONE allocation, so that ``result`` is one copy.  ``layout``: (name, torch dtype, per-image shape) in byte order; ``_out[name]`` is the
        device view [capacity, *shape] and ``_host()[name]`` the host view of the images added."""
        self._layout = [(name, dt, (self.capacity, *shape)) for name, dt, shape in layout]
        self._cut = np.cumsum([0] + [math.prod(shape) * dt.itemsize for _, dt, shape in self._layout]).tolist()
        self._buf = torch.zeros((self._cut[-1],), dtype=torch.uint8, device=self.device)
        self._out = {name: self._buf[a:b].view(dt).view(*shape) for (name, dt, shape), a, b in zip(self._layout, self._cut, self._cut[1:])}

    def _host(self) -> Dict[str, np.ndarray]:
        """The one device-to-host copy of an evaluation (which waits for the launches), cut like ``_out``, the images added only."""
        host = self._buf.cpu().numpy()
        return {name: host[a:b].view(_NUMPY[dt]).reshape(shape)[:self.count]
                for (name, dt, shape), a, b in zip(self._layout, self._cut, self._cut[1:])}

    def reset(self) -> None:
        self.count = self._bop_count = 0

    def add(self, frames, camera: torch.Tensor, gt: torch.Tensor, draw_into: Optional[torch.Tensor] = None, meshes=None, bop=None,
            depth_test: Optional[torch.Tensor] = None) -> None:
        """One batch: ``frames`` uint8 [B,H,W,3] (preprocessed here) or the network input float32 [B,3,S,S]; ``camera`` float32 [B,6]
        (``LinemodFolder.camera_input``); ``gt`` float64 [B,88] (``gt_table``) for ``DeviceEvaluator``, [B,amax,88] (``gt_scene_table``) for
        ``SceneEvaluator``; all on the evaluator's device.  Everything is checked on the host before the library sees a pointer; a batch that
        does not fit the remaining capacity raises ValueError.
        ``draw_into``: uint8 [B,H,W,3] on the device that already holds the original frames (it may be ``frames``): after scoring, the
        ground truth - every valid annotation - and the kept detections are drawn into it from the same table and rows, each with its
        label's cuboid, on the same stream (hep_draw_poses_device; needs the evaluator's ``cuboid`` / ``cuboids``).  The scores do not depend on it.
        ``meshes``: a ``render.MeshSet`` next to ``draw_into``, one mesh per label: the filled models of the kept detections are blended in
        first (hep_render_models_device, the labels' colours at half weight), then the lines are drawn on top.
        ``bop``: a ``bop.BopSettings`` over the evaluator's labels (``DeviceEvaluator``: 0..``label``): MSSD, MSPD and VSD (tau = the
        label's diameter times each tau fraction) of every matched (annotation, detection) pair go into a second buffer at the running
        offset, and ``result`` gains a ``"bop"`` entry with one extra copy; ``depth_test``: float32 [B,H,W] measured depth in the model's
        unit, one image per frame, for VSD's visibility.  Without ``bop`` nothing changes: same launches, same bytes."""
        who, dev = type(self).__name__ + ".add", self.device
        _check_draw_into(who, draw_into, frames, self._cuboids, dev, self.max_detections)
        _check_meshes(who, meshes, draw_into, dev, self.max_detections)
        bop_size = _check_bop(who, bop, depth_test, frames, dev, self.num_labels)
        for name, t, dt in (("frames", frames, None), ("camera", camera, torch.float32), ("gt", gt, torch.float64)):
            if not isinstance(t, torch.Tensor) or t.device != dev or (dt is not None and t.dtype != dt):
                raise ValueError(f"{who}: {name} must be a {dt or 'uint8 or float32'} tensor on {dev}")
        if frames.dim() != 4 or frames.shape[0] < 1:
            raise ValueError(f"{who}: frames must be uint8 [B,H,W,3] or float32 [B,3,S,S]")
        B = int(frames.shape[0])
        if frames.dtype == torch.uint8:
            if frames.shape[3] != 3:
                raise ValueError(f"{who}: uint8 frames must be [B,H,W,3]")
        elif frames.dtype != torch.float32 or tuple(frames.shape[1:]) != (3, self.image_size, self.image_size):
            raise ValueError(f"{who}: an image must be float32 [B,3,{self.image_size},{self.image_size}]")
        gt_shape = (B, *self._gt_shape)
        if tuple(camera.shape) != (B, 6) or tuple(gt.shape) != gt_shape:
            raise ValueError(f"{who}: camera must be [{B},6] and gt [{','.join(map(str, gt_shape))}]")
        if self.count + B > self.capacity:
            raise ValueError(f"{who}: {self.count} + {B} images exceed the capacity of {self.capacity}")
        x = self.model.model.session(self.image_size, B, dev).preprocess(frames) if frames.dtype == torch.uint8 else frames
        det = self.model.detect(x, camera)
        rows = int(det["scores"].shape[1]) if det["scores"].dim() == 2 else 0
        for k, w, dt in (("boxes", 4, torch.float32), ("scores", None, torch.float32), ("labels", None, torch.int32), ("rotation", 3, torch.float32),
                         ("translation", 3, torch.float32), ("hand", 63, torch.float32)):
            t = det[k]
            if tuple(t.shape) != ((B, rows) if w is None else (B, rows, w)) or t.dtype != dt or t.device != dev:
                raise ValueError(f"{who}: detection rows '{k}' have shape {tuple(t.shape)} / {t.dtype} on {t.device}")
        if not 1 <= rows <= 256 or self.max_detections > rows:
            raise ValueError(f"{who}: {rows} detection rows: must be 1..256 and >= max_detections {self.max_detections}")
        d = [det[k].contiguous() for k in _DETECTION_KEYS]
        g = gt.contiguous()
        o = self.count
        _capi.check(self._launch([t.data_ptr() for t in d], B, rows, g.data_ptr(), {k: v[o:].data_ptr() for k, v in self._out.items()},
                                 torch.cuda.current_stream(dev).cuda_stream))
        self.count += B
        scene = g.view(B, -1, GT_DOUBLES)                  # [B,amax,88]; row 0 carries the image's camera whichever the class
        if bop is not None:
            records, diameters = self._bop_records(self._out["records"][o:o + B])
            _score_bop(self, bop, bop_size, scene, d, records, diameters, depth_test, o)
        if meshes is not None:
            _blend_models(draw_into, meshes, scene[:, 0], d, self.score_threshold, self.max_detections)
        if draw_into is not None:
            from .draw import draw_poses
            draw_poses(draw_into, cuboids=self._cuboids, gt=g, detections=dict(zip(_DETECTION_KEYS, d)),
                       score_threshold=self.score_threshold, max_detections=self.max_detections, ann_layers=self.draw_layers,
                       det_layers=self.draw_layers, thickness=self.draw_thickness)

    def _with_bop(self, out: dict, records: np.ndarray) -> dict:
        """``result``'s ``"bop"`` entry, where ``add`` was given ``bop=``."""
        if self._bop_count:
            out["bop"] = _bop_result(self, type(self).__name__ + ".result", *self._bop_records(records))
        return out


class DeviceEvaluator(_Evaluator):
    """``evaluate`` with nothing on the host until the end: ``add`` runs preprocess (uint8 frames), ``model.detect`` and ONE launch of
    hep_score_detections_device per batch - per-image matching plus ADD, ADD-S, translation, rotation, tip, reprojection and hand
    errors of the matched pair - into device buffers of ``capacity`` images at a running offset, with no device-to-host copy and no
    synchronisation; ``result`` makes the one copy of an evaluation and finishes on the host like ``evaluate`` (``metric_summary``).

    ``model``: a ``TrainModelWithLoss`` in eval mode on the GPU.  ``points`` [P,3] and ``diameter``: the object model.  The
    dictionary has every key of ``evaluate`` plus ``translation_tip_std``, ``ADD(-S)`` and ``mixed_distance_mean`` / ``_std`` (ADD-S
    values when ``symmetric``, else ADD - what train.py steps ``ReduceLROnPlateau`` with and keeps the best checkpoint by).

    Scope: one annotation per image and one evaluated ``label``, as ``evaluate`` has; several annotations per image and several
    labels in one pass: ``SceneEvaluator``."""

    _gt_shape = (GT_DOUBLES,)

    def __init__(self, model, points, diameter: float, image_size: int, capacity: int, score_threshold: float = 0.05, max_detections: int = 10,
                 iou_threshold: float = 0.5, diameter_threshold: float = 0.1, label: int = 0, symmetric: bool = False,
                 device: Optional[torch.device] = None, max_points: int = 1000, cuboid=None, draw_layers: int = _capi.DRAW_CUBOID,
                 draw_thickness: int = 2):
        self._check_sizes(capacity, max_detections, max_points)
        super().__init__(model, image_size, capacity, score_threshold, max_detections, iou_threshold, diameter_threshold, device, max_points,
                         draw_layers, draw_thickness)
        self.label, self.symmetric, self.diameter = int(label), bool(symmetric), float(diameter)
        self.num_labels = self.label + 1                   # the labels its cuboids, ``meshes`` and ``bop`` sets hold: 0..``label``
        if cuboid is not None:                             # ``LinemodFolder.cuboid``, at every label: the table's rows carry label 0, the detections theirs
            c = np.ascontiguousarray(cuboid, dtype=np.float32)
            if c.shape != (8, 3):
                raise ValueError("DeviceEvaluator: cuboid must be [8,3]")
            self._cuboids = torch.from_numpy(np.repeat(c[None], self.num_labels, axis=0)).to(self.device)
        self.points = torch.from_numpy(self._points(points, "points")).to(self.device)
        M = self.max_detections
        self._allocate([("records", torch.float64, (RECORD_DOUBLES,)), ("scores", torch.float32, (M,)), ("tp", torch.int32, (M,))])

    def _launch(self, det, B, rows, gt, out, stream):
        return _capi.lib().hep_score_detections_device(
            *det, B, rows, gt, self.points.data_ptr(), int(self.points.shape[0]), self.max_points,
            self.label, self.score_threshold, self.max_detections, self.iou_threshold, out["records"], out["scores"], out["tp"], stream)

    def _bop_records(self, records):
        """Records [n,16], device or host, in the scene layout [n,1,16] BOP reads: every image is an annotation of ``label``; slot 1 matched
        and 2 the row as they are.  With the diameter of every label up to it."""
        scene = (records.clone() if isinstance(records, torch.Tensor) else records.copy())[:, None, :]
        scene[..., 0], scene[..., 12] = 1.0, float(self.label)
        return scene, [self.diameter] * self.num_labels

    def result(self) -> Dict[str, float]:
        """The metric dictionary of the images added since the last ``reset``: one device-to-host copy (which waits for the launches),
        then the host arithmetic of ``evaluate``'s tail."""
        host = self._host()
        rec, sc, tp = host["records"], host["scores"], host["tp"]
        keep = np.arange(self.max_detections)[None, :] < rec[:, 0:1]      # the considered detections, image by image, in row order
        out = metric_summary(float(self.count), [float(v) for v in sc[keep]], tp[keep], _matched_metrics(rec[rec[:, 1] == 1.0]),
                             self.diameter * self.diameter_threshold, symmetric=self.symmetric)
        return self._with_bop(out, rec)


def _evaluate_folder(ev: _Evaluator, dataset, table, image_size: int, batch_size: int, save_path: Optional[str], meshes, **add_kw):
    """The folder loop of ``evaluate_device`` and ``evaluate_scene_device``: batch by batch the frames, camera rows and
    ``table(annotations, cameras, scale)`` uploaded and added to ``ev`` (with ``add_kw``), the drawn frames saved; returns ``ev.result()``."""
    n, device = len(dataset), ev.device
    for i0 in range(0, n, batch_size):
        idx = list(range(i0, min(n, i0 + batch_size)))
        frames = [dataset.load_image(i) for i in idx]
        h, w = frames[0].shape[:2]
        if any(f.shape[:2] != (h, w) for f in frames):
            raise ValueError("frames of one batch must share a size")
        scale = image_size / max(h, w)
        u8 = torch.from_numpy(np.stack(frames)).to(device)
        cam = torch.from_numpy(np.stack([dataset.camera_input(i, scale) for i in idx])).to(device)
        gt = torch.from_numpy(table([dataset.annotations[i] for i in idx], [dataset.camera[i] for i in idx], scale)).to(device)
        ev.add(u8, cam, gt, draw_into=u8 if save_path is not None else None, meshes=meshes, **add_kw)
        if save_path is not None:
            save_frames(save_path, idx, u8)
    return ev.result()


def evaluate_device(dataset: LinemodFolder, model, image_size: int, score_threshold: float = 0.05, max_detections: int = 10,
                    iou_threshold: float = 0.5, diameter_threshold: float = 0.1, batch_size: int = 16, device: Optional[torch.device] = None,
                    symmetric: bool = False, save_path: Optional[str] = None, draw_hand: bool = False, draw_bbox_2d: bool = False,
                    draw_model: bool = False) -> Dict[str, float]:
    """``evaluate`` through a ``DeviceEvaluator``: same arguments (the per-detection ``detections_out`` aside - no detection ever reaches
    the host), same dictionary plus the keys train.py steers by.  One host synchronisation for the whole folder.
    ``save_path``: a folder (created if missing) that receives every frame with its ground truth and kept detections drawn in as
    ``<i>.png``, ``i`` the index in dataset order (eval/common.py:452-479): projected cuboid and centre, plus the hand skeleton with
    ``draw_hand`` and the 2D box with ``draw_bbox_2d``.  The frames are drawn on the GPU and each batch is copied down once (one
    synchronisation per batch); the dictionary is the same with and without it.  ``draw_model`` (with ``save_path``): the filled model
    of every kept detection under its pose, blended in beneath the lines; the folder's PLY file must have triangle faces (ValueError)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    layers = _capi.DRAW_CUBOID | (_capi.DRAW_HAND if draw_hand else 0) | (_capi.DRAW_BOX2D if draw_bbox_2d else 0)
    if save_path is not None and dataset.cuboid is None:
        raise ValueError("evaluate_device: save_path needs the model cuboid (min_* / size_* in models_info.yml)")
    if draw_model and save_path is None:
        raise ValueError("evaluate_device: draw_model draws into the saved frames: it needs save_path")
    meshes = _folder_meshes("evaluate_device", dataset.model_path, [dataset.object_id], device) if draw_model else None
    ev = DeviceEvaluator(model, dataset.points, dataset.diameter, image_size, max(len(dataset), 1), score_threshold, max_detections, iou_threshold,
                         diameter_threshold, symmetric=symmetric, device=device, cuboid=dataset.cuboid if save_path is not None else None,
                         draw_layers=layers)
    return _evaluate_folder(ev, dataset, gt_table, image_size, batch_size, save_path, meshes)


def save_frames(save_path: str, indices: Sequence[int], frames: torch.Tensor) -> None:
    """One copy of a drawn batch (uint8 [B,H,W,3], RGB) to the host, then ``<save_path>/<i>.png`` per frame (eval/common.py:479)."""
    from PIL import Image
    os.makedirs(save_path, exist_ok=True)
    host = frames.cpu().numpy()
    for i, img in zip(indices, host):
        Image.fromarray(img).save(os.path.join(save_path, f"{i}.png"))


# ----------------------------------------------------------------------------------------------------------------
# scenes: several annotations per image and several labels in one launch (hep_score_scene_device, csrc/k_score.hip)
# ----------------------------------------------------------------------------------------------------------------
MAX_ANNOTATIONS, MAX_LABELS = _capi.SCORE_MAX_ANNOTATIONS, _capi.SCORE_MAX_LABELS
FRACTION_KEYS = ("AP", "ADD", "ADD-S", "ADD(-S)", "5cm_5deg", "2D_projection")


def gt_scene_table(annotations_per_image: Sequence[Sequence[dict]], cameras: Sequence[np.ndarray], scale, amax: Optional[int] = None) -> np.ndarray:
    """The ground-truth table of hep_score_scene_device, float64 [n, amax, 88]: one list of annotation dicts per image (``gt_table``'s
    keys plus ``label``, an integer >= 0), one camera matrix per image.  Row layout: ``gt_table``'s with slot 83 = label; padding
    rows have slot 0 == 0; camera and scale are repeated in every row of an image.  ``amax``: the slot count, by default the largest
    annotation count (at least 1).  ValueError for more than 16 annotations in an image (or more than ``amax``), a negative or
    non-integral label, or a missing key."""
    n = len(annotations_per_image)
    if len(cameras) != n:
        raise ValueError("gt_scene_table: one camera matrix per image")
    most = max([len(a) for a in annotations_per_image], default=0)
    if most > MAX_ANNOTATIONS:
        raise ValueError(f"gt_scene_table: {most} annotations in one image, at most {MAX_ANNOTATIONS} are supported")
    amax = max(1, most) if amax is None else int(amax)
    if not 1 <= amax <= MAX_ANNOTATIONS or most > amax:
        raise ValueError(f"gt_scene_table: amax {amax} must be in 1..{MAX_ANNOTATIONS} and hold the {most} annotations of the fullest image")
    scales = np.broadcast_to(np.asarray(scale, np.float64), (n,))
    t = np.zeros((n, amax, GT_DOUBLES), np.float64)
    for i, (anns, K) in enumerate(zip(annotations_per_image, cameras)):
        K = np.asarray(K, np.float64)
        t[i, :, 14:18] = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        t[i, :, 18] = scales[i]
        for k, ann in enumerate(anns):
            missing = [q for q in ("bbox", "rotation", "translation", "drill_tip", "label") if q not in ann]
            if missing:
                raise ValueError(f"gt_scene_table: annotation {k} of image {i} lacks {missing}")
            label = ann["label"]
            if label != int(label) or int(label) < 0:
                raise ValueError(f"gt_scene_table: annotation {k} of image {i} has label {label!r}: must be an integer >= 0")
            t[i, k, :14] = gt_table([ann], [K], scales[i])[0, :14]
            if "coords_3d" in ann:
                t[i, k, 19] = 1.0
                t[i, k, 20:83] = np.asarray(ann["coords_3d"], np.float64).reshape(63)
            t[i, k, 83] = float(int(label))
    return t


def scene_mean(per_label: Dict[int, Dict[str, float]]) -> Dict[str, float]:
    """evaluate_model's averaging of the per-label dictionaries (eval/common.py:92-265): the fraction keys are summed over ALL labels
    and divided by the number of labels that have annotations; every other key is the plain average over the labels that have
    annotations (the ones the reference's metric dictionaries hold) - a label with annotations and no match contributes NaN, the
    reference's np.mean of nothing.  ``num_annotations`` / ``num_matched`` are totals."""
    with_ann = [l for l, d in per_label.items() if d["num_annotations"] > 0]
    out = {"num_annotations": float(sum(d["num_annotations"] for d in per_label.values())),
           "num_matched": float(sum(d["num_matched"] for d in per_label.values())), "num_labels": float(len(with_ann))}
    if not with_ann:
        return out
    nan = float("nan")
    for k in FRACTION_KEYS:
        out[k] = sum(d[k] for d in per_label.values()) / len(with_ann)
    keys = sorted({k for l in with_ann for k in per_label[l]} - set(FRACTION_KEYS) - {"num_annotations", "num_matched"})
    for k in keys:
        out[k] = sum(per_label[l].get(k, nan) for l in with_ann) / len(with_ann)
    return out


class SceneEvaluator(_Evaluator):
    """``DeviceEvaluator`` for scenes: up to ``amax`` annotations per image over ``len(models)`` labels.  ``add`` runs preprocess,
    ``model.detect`` (ONE forward per batch, whatever the number of labels) and ONE launch of hep_score_scene_device per batch into
    ONE allocation at a running offset, with no device-to-host copy; ``result`` makes the one copy of an evaluation.

    ``models``: a sequence indexed by label of ``(points [P,3], diameter, symmetric)``.  ``result()`` returns ``{"labels": {l: dict},
    "mean": dict}``: each per-label dictionary is ``metric_summary`` of that label's annotation count, considered scores and flags
    (image, then row order) and matched records (image, then slot order); ``"mean"`` is ``scene_mean`` of them -
    ``result()["mean"]["mixed_distance_mean"]`` is the reference's ``mean_mixed_transformed_mean``, what train.py:273 steps the
    scheduler with."""

    def __init__(self, model, models, image_size: int, capacity: int, amax: int, score_threshold: float = 0.05, max_detections: int = 10,
                 iou_threshold: float = 0.5, diameter_threshold: float = 0.1, device: Optional[torch.device] = None, max_points: int = 1000,
                 cuboids=None, draw_layers: int = _capi.DRAW_CUBOID, draw_thickness: int = 2):
        self._check_sizes(capacity, max_detections, max_points)
        if not 1 <= amax <= MAX_ANNOTATIONS:
            raise ValueError(f"SceneEvaluator: amax must be in 1..{MAX_ANNOTATIONS}")
        if not 1 <= len(models) <= MAX_LABELS:
            raise ValueError(f"SceneEvaluator: 1..{MAX_LABELS} object models, one per label")
        super().__init__(model, image_size, capacity, score_threshold, max_detections, iou_threshold, diameter_threshold, device, max_points,
                         draw_layers, draw_thickness)
        self.amax, self.num_labels = int(amax), len(models)
        self._gt_shape = (self.amax, GT_DOUBLES)
        if cuboids is not None:                            # ``SceneFolder.cuboids``
            c = np.ascontiguousarray(cuboids, dtype=np.float32)
            if c.shape != (len(models), 8, 3):
                raise ValueError(f"SceneEvaluator: cuboids must be [{len(models)},8,3], one per label")
            self._cuboids = torch.from_numpy(c).to(self.device)
        clouds = [self._points(points, f"the points of label {l}") for l, (points, _, _) in enumerate(models)]
        self.diameters, self.symmetric = [float(m[1]) for m in models], [bool(m[2]) for m in models]
        self._offsets = (ctypes.c_int32 * (self.num_labels + 1))(*np.concatenate(([0], np.cumsum([len(c) for c in clouds]))).tolist())
        self.points = torch.from_numpy(np.concatenate(clouds)).to(self.device)
        M = self.max_detections
        self._allocate([("records", torch.float64, (self.amax, RECORD_DOUBLES)), ("scores", torch.float32, (M,)), ("tp", torch.int32, (M,)),
                        ("labels", torch.int32, (M,)), ("counts", torch.int32, ())])

    def _launch(self, det, B, rows, gt, out, stream):
        return _capi.lib().hep_score_scene_device(
            *det, B, rows, gt, self.amax, self.points.data_ptr(), self._offsets, self.num_labels, self.max_points,
            self.score_threshold, self.max_detections, self.iou_threshold, out["records"], out["scores"], out["tp"], out["labels"], out["counts"],
            stream)

    def _bop_records(self, records):
        return records, self.diameters

    def result(self) -> Dict[str, dict]:
        """``{"labels": {l: dict}, "mean": dict}`` of the images added since the last ``reset``: one device-to-host copy (which waits
        for the launches), then the host arithmetic."""
        host = self._host()
        out = summarise_scene(host["records"], host["scores"], host["tp"], host["labels"], host["counts"], self.diameters, self.symmetric,
                              self.diameter_threshold)
        return self._with_bop(out, host["records"])


def summarise_scene(rec: np.ndarray, sc: np.ndarray, tp: np.ndarray, labels: np.ndarray, counts: np.ndarray, diameters: Sequence[float],
                    symmetric: Sequence[bool], diameter_threshold: float = 0.1) -> Dict[str, dict]:
    """The host tail of ``SceneEvaluator.result`` on the five outputs of hep_score_scene_device (records [n,amax,16], scores / flags /
    labels [n,M], counts [n]): per label ``metric_summary``, and ``scene_mean`` of the labels."""
    keep = np.arange(sc.shape[1])[None, :] < counts[:, None] if sc.shape[0] else np.zeros(sc.shape, bool)
    flat = rec.reshape(-1, RECORD_DOUBLES)                                # image, then slot
    per_label = {}
    for l, (diameter, sym) in enumerate(zip(diameters, symmetric)):
        own = keep & (labels == l)
        r = flat[(flat[:, 0] == 1.0) & (flat[:, 12] == l)]
        num_ann = float(r.shape[0])
        r = r[r[:, 1] == 1.0]
        per_label[l] = metric_summary(num_ann, [float(v) for v in sc[own]], tp[own], _matched_metrics(r), diameter * diameter_threshold, symmetric=sym)
    return {"labels": per_label, "mean": scene_mean(per_label)}


class SceneFolder(_Folder):
    """One scene folder of a Linemod-format dataset (``<root>/data/<NN>/`` as ``LinemodFolder`` reads it) with EVERY ground-truth entry of
    a frame whose ``obj_id`` is in ``object_ids``; the label of an entry is the index of its object in that list.  ``scene_id``: the
    folder number (default: the first object id).  Boxes come from ``obj_bb`` (x, y, w, h) or, for the objects ``mask_values`` maps to
    their byte in the frame's merged mask ``mask/<frame>.png``, from the pixels equal to that byte.  ``models``: per label
    ``(points, diameter, symmetric)`` from ``models/`` (symmetric: models_info.yml lists symmetries for the object)."""

    def __init__(self, dataset_path: str, object_ids: Sequence[int], scene_id: Optional[int] = None, fold: int = 0, split: str = "test",
                 mask_values: Optional[Dict[int, int]] = None, image_extension: str = ".png"):
        self.object_ids = [int(o) for o in object_ids]
        if not self.object_ids or len(set(self.object_ids)) != len(self.object_ids):
            raise ValueError("SceneFolder: object_ids must be a non-empty list without repeats")
        self._mask_values = mask_values or {}
        super().__init__(dataset_path, self.object_ids[0] if scene_id is None else int(scene_id), fold, split, image_extension)
        self.amax = max([len(e) for e in self.annotations] + [1])

    def _read_models(self, models: dict) -> None:
        self.models = [(load_ply_vertices(os.path.join(self.model_path, f"obj_{o:02}.ply")), float(models[o]["diameter"]),
                        any(k.startswith("symmetries") for k in models[o])) for o in self.object_ids]
        self.models_info = [models[o] for o in self.object_ids]                              # ``bop.symmetry_transforms`` reads the symmetries
        boxes = [_model_cuboid(models[o]) for o in self.object_ids]
        self.cuboids = np.stack(boxes) if all(c is not None for c in boxes) else None      # float32 [labels,8,3], or None without min_* / size_*

    def _annotation(self, n: str, entries: list, image_extension: str) -> List[dict]:
        """EVERY entry of a listed object, in the file's order; the boxes of the objects ``mask_values`` names from the frame's merged mask."""
        mask = None
        out = []
        for a in entries:
            if a["obj_id"] not in self.object_ids:
                continue
            entry = {"label": self.object_ids.index(a["obj_id"]), **self._pose(a)}
            if a["obj_id"] in self._mask_values:
                if mask is None:
                    from PIL import Image
                    mask = np.asarray(Image.open(os.path.join(self.object_path, "mask", n)))
                    mask = mask.reshape(mask.shape[0], mask.shape[1], -1)[:, :, 0]
                entry["bbox"] = self._mask_box(mask == self._mask_values[a["obj_id"]])
            else:
                entry["bbox"] = self._obj_bb(a)
            out.append(entry)
        if len(out) > MAX_ANNOTATIONS:
            raise ValueError(f"SceneFolder: frame {n} holds {len(out)} annotations, at most {MAX_ANNOTATIONS} are supported")
        return out


def evaluate_scene_device(dataset: SceneFolder, model, image_size: int, score_threshold: float = 0.05, max_detections: int = 10,
                          iou_threshold: float = 0.5, diameter_threshold: float = 0.1, batch_size: int = 16,
                          device: Optional[torch.device] = None, save_path: Optional[str] = None, draw_hand: bool = False,
                          draw_bbox_2d: bool = False, draw_model: bool = False, bop: bool = False, max_sym_disc_step: float = 0.01) -> Dict[str, dict]:
    """A ``SceneFolder`` through a ``SceneEvaluator``, driven like ``evaluate_device``: one forward and one scoring launch per batch,
    one host synchronisation for the whole folder.  Returns ``SceneEvaluator.result()``.  ``save_path``, ``draw_hand``,
    ``draw_bbox_2d``, ``draw_model``: as for ``evaluate_device`` - every annotation and every kept detection of a frame, each with its
    label's cuboid (and, with ``draw_model``, every kept detection's filled model).  ``bop``: MSSD, MSPD and VSD of every matched pair
    and their average recalls as ``result()["bop"]`` (``bop.BopSettings`` built from the folder's ``models/``: the PLY meshes, which
    need triangle faces, and the symmetries of models_info.yml in steps of ``max_sym_disc_step``; no measured depth is read)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    settings = None
    if bop:
        from .bop import folder_settings
        settings = folder_settings("evaluate_scene_device", dataset.model_path, dataset.object_ids, dataset.models_info, device, max_sym_disc_step)
    layers = _capi.DRAW_CUBOID | (_capi.DRAW_HAND if draw_hand else 0) | (_capi.DRAW_BOX2D if draw_bbox_2d else 0)
    if save_path is not None and dataset.cuboids is None:
        raise ValueError("evaluate_scene_device: save_path needs the model cuboids (min_* / size_* in models_info.yml)")
    if draw_model and save_path is None:
        raise ValueError("evaluate_scene_device: draw_model draws into the saved frames: it needs save_path")
    meshes = _folder_meshes("evaluate_scene_device", dataset.model_path, dataset.object_ids, device) if draw_model else None
    ev = SceneEvaluator(model, dataset.models, image_size, max(len(dataset), 1), dataset.amax, score_threshold, max_detections, iou_threshold,
                        diameter_threshold, device=device, cuboids=dataset.cuboids if save_path is not None else None, draw_layers=layers)
    return _evaluate_folder(ev, dataset, lambda annotations, cameras, scale: gt_scene_table(annotations, cameras, scale, dataset.amax),
                            image_size, batch_size, save_path, meshes, bop=settings)


def main(argv=None):
    """The reference's ``evaluate.py`` entry point for this path (evaluate.py:18-128; its argument names)."""
    ap = argparse.ArgumentParser(description="Evaluate an HMD-EgoPose checkpoint on a Linemod-format object folder (MI355X)")
    ap.add_argument("--dataset-path", required=True, help="folder holding data/<NN>/ and models/ (reference: --dataset-path)")
    ap.add_argument("--object-id", type=int, default=1)
    ap.add_argument("--object-ids", default=None, help="comma-separated object ids of one scene folder, e.g. 1,5,6: every listed object is a label "
                    "and every annotation of a frame is scored (evaluate_scene_device); the folder is data/<first id>/")
    ap.add_argument("--fold", type=int, default=0)
    ap.add_argument("--phi", type=int, default=0)
    ap.add_argument("--img-size", default="256,256")
    ap.add_argument("--weights", required=True, help=".pth state_dict (model. / model.module. prefixes are stripped) or a HEPW pack")
    ap.add_argument("--score-threshold", type=float, default=0.5)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "fp8"])
    ap.add_argument("--save-images", default=None, metavar="DIR", help="write every frame with its ground truth and kept detections drawn in (on the GPU) "
                    "as DIR/<i>.png (reference: --validation-image-save-path); a single object then runs through evaluate_device")
    ap.add_argument("--draw-hand", action="store_true", help="with --save-images: the hand skeletons as well")
    ap.add_argument("--draw-bbox-2d", action="store_true", help="with --save-images: the 2D boxes as well")
    ap.add_argument("--draw-model", action="store_true", help="with --save-images: the filled model of every kept detection under its pose, beneath the "
                    "lines (the folder's PLY files need triangle faces)")
    ap.add_argument("--bop", action="store_true", help="with --object-ids: MSSD, MSPD and VSD of every matched pair and their average recalls "
                    "(the folder's PLY files need triangle faces; symmetries from models_info.yml)")
    ap.add_argument("--max-sym-disc-step", type=float, default=0.01, help="with --bop: the step of continuous symmetries (at most 64 transforms per object)")
    a = ap.parse_args(argv)
    from . import HMDEgoPose, TrainModelWithLoss, load_pack, strip_checkpoint_prefix
    size = int(str(a.img_size).split(",")[0])
    if a.weights.endswith(".hepw"):
        state = {k: torch.from_numpy(np.array(v)) for k, v in load_pack(open(a.weights, "rb").read()).items()}
    else:
        state = strip_checkpoint_prefix(torch.load(a.weights, map_location="cpu", weights_only=True))
    ids = [int(v) for v in a.object_ids.split(",")] if a.object_ids else None
    m = HMDEgoPose({"iter": 0}, num_classes=len(ids) if ids else 1, compound_coef=a.phi, onnx_export=True, input_sizes=[size] * 9, precision=a.precision)
    m.load_state_dict(state, strict=False)
    model = TrainModelWithLoss(m.to("cuda").eval()).eval()
    if ids:
        res = evaluate_scene_device(SceneFolder(a.dataset_path, ids, fold=a.fold), model, size, score_threshold=a.score_threshold, batch_size=a.batch_size,
                                    save_path=a.save_images, draw_hand=a.draw_hand, draw_bbox_2d=a.draw_bbox_2d, draw_model=a.draw_model,
                                    bop=a.bop, max_sym_disc_step=a.max_sym_disc_step)
        for name, d in [(f"object {o}", res["labels"][l]) for l, o in enumerate(ids)] + [("mean", res["mean"])]:
            print(name)
            for k, v in d.items():
                print(f"{k:>28s}: {v:.6g}")
        if a.bop:
            for name, d in [(f"object {o} (BOP)", res["bop"]["labels"][l]) for l, o in enumerate(ids)] + [("mean (BOP)", res["bop"]["mean"])]:
                print(name)
                for k, v in d.items():
                    print(f"{k:>28s}: {v:.6g}")
        return res
    if a.save_images or a.draw_model:             # the drawing runs on the GPU path (the host ``evaluate`` does not draw)
        res = evaluate_device(LinemodFolder(a.dataset_path, a.object_id, a.fold), model, size, score_threshold=a.score_threshold, batch_size=a.batch_size,
                              save_path=a.save_images, draw_hand=a.draw_hand, draw_bbox_2d=a.draw_bbox_2d, draw_model=a.draw_model)
    else:
        res = evaluate(LinemodFolder(a.dataset_path, a.object_id, a.fold), model, size, score_threshold=a.score_threshold, batch_size=a.batch_size)
    for k, v in res.items():
        print(f"{k:>24s}: {v:.6g}")
    return res


if __name__ == "__main__":
    main()
