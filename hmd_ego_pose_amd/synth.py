"""Synthetic training frames on the GPU: coloured meshes under drawn poses, shaded by one light per image, composited over the caller's
backgrounds - and, from the same call, the labels ``augment.augment_6dof`` takes: the instance mask, the visible box of every object from
the pixels it actually won, and the padded annotation tensors with hidden and off-frame objects dropped (hep_synth_frames_device,
csrc/k_render.hip: the renderer's rasteriser with the winning fragment shaded).  With it the training loop has no host-side piece:

    draw_poses -> synth_frames -> augment.colour_augment -> augment.augment_6dof -> training.anchor_targets_device -> Trainer.step(gt_hand=None)

The shading is this project's own definition - flat normals, two-sided, float64 with every rounding stated; include/hep.h states it,
tests/_synth.py states it in numpy and the kernels match it bit for bit.  No textures, smooth shading, shadows, anti-aliasing or hands."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _capi
from .augment import pad_annotations
from .render import MAX_POSES, MeshSet, _read_ply, _workspace, poses_from_annotations

LIGHT_DOUBLES, VISIBLE_INTS = 8, 5


def load_ply_coloured_mesh(path: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(vertices float32 [V,3], faces int32 [F,3], colours uint8 [V,3]) of an ASCII or binary-little-endian PLY file: ``load_ply_mesh``
    (the same parser, the same refusals) plus the vertex element's uchar properties red, green and blue.  A file without one of them
    raises ValueError naming the file."""
    return _read_ply(path, True)


def face_normals(vertices: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """float64 [F,3], on the host: cross(v1 - v0, v2 - v0) / length of the float32 vertices widened; a zero-length cross product gives zeros."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    length = np.sqrt((c * c).sum(axis=1))
    return np.where(length[:, None] > 0, c / np.where(length > 0, length, 1.0)[:, None], 0.0)


class ShadedMeshSet(MeshSet):
    """A ``MeshSet`` plus what the shading reads: ``vertex_colours`` uint8 [V,3] and ``face_normals`` float64 [F,3] on the device (and
    ``host_vertex_colours``, ``host_face_normals``).  ``meshes_per_label``: a sequence of (vertices [v,3], faces [f,3], colours uint8 [v,3])
    triples, e.g. ``load_ply_coloured_mesh`` results.  The normals are computed here, once, in float64 (``face_normals``): the kernel has
    no sqrt and takes them as data."""

    def __init__(self, meshes_per_label: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray]], device: Optional[torch.device] = None):
        if any(len(m) != 3 for m in meshes_per_label):
            raise ValueError("ShadedMeshSet: every label needs (vertices, faces, colours)")
        super().__init__([(m[0], m[1]) for m in meshes_per_label], device)
        cols = []
        for l, m in enumerate(meshes_per_label):
            c = np.asarray(m[2])
            if c.dtype != np.uint8 or c.shape != (np.asarray(m[0]).shape[0], 3):
                raise ValueError(f"ShadedMeshSet: colours of label {l} must be uint8 [{np.asarray(m[0]).shape[0]},3], one per vertex")
            cols.append(c)
        self.host_vertex_colours = np.ascontiguousarray(np.concatenate(cols))
        self.host_face_normals = np.ascontiguousarray(face_normals(self.host_vertices, self.host_faces))
        self.vertex_colours = torch.from_numpy(self.host_vertex_colours).to(self.device)
        self.face_normals = torch.from_numpy(self.host_face_normals).to(self.device)


def draw_poses(rng, batch: int, objects: int, camera_k, height: int, width: int, distance_range: Tuple[float, float], labels: Sequence[int],
               mask_values: Optional[Sequence[int]] = None, margin: float = 0.1, symmetric: Optional[Sequence[int]] = None) -> List[dict]:
    """Random poses of ``objects`` objects in each of ``batch`` images, on the host.  ``rng`` needs a ``random()`` in [0, 1) (a
    ``random.Random(seed)`` reproduces a sequence); it is called exactly SIX times per object, image by image and object by object:
      u1, u2, u3   a uniform rotation by Shoemake's method: the quaternion (x, y, z, w) = (sqrt(1 - u1) sin 2 pi u2, sqrt(1 - u1) cos 2 pi u2,
                   sqrt(u1) sin 2 pi u3, sqrt(u1) cos 2 pi u3), stored as the axis-angle 2 atan2(|xyz|, w) xyz / |xyz|;
      a, b         the projected centre, uniform inside the frame less the margin: u = width (margin + a (1 - 2 margin)), v alike with height;
      c            Z = z0 + c (z1 - z0) with (z0, z1) = ``distance_range``.
    tvec = ((u - cx) Z / fx, (v - cy) Z / fy, Z) with ``camera_k`` = fx, fy, cx, cy ([4] or [batch,4], host).  ``labels``: the label of
    object k, one per object; ``mask_values``: its mask value in 1..255, default k + 1 (distinct per object); ``symmetric``: 0 / 1 per
    object, default 0.  Returns the reference-style annotation dicts ``augment.pad_annotations`` takes - ``bboxes`` zeros [K,4] (the
    visible boxes come from ``synth_frames``), ``labels`` [K], ``rotations`` [K,5] = axis-angle, is_symmetric, class, ``translations``
    [K,3], ``mask_values`` [K] - one per image."""
    B, K = int(batch), int(objects)
    if B < 1 or not 1 <= K <= MAX_POSES:
        raise ValueError(f"draw_poses: batch >= 1 and objects in 1..{MAX_POSES}")
    cam = np.asarray(camera_k, np.float64)
    cam = np.broadcast_to(cam, (B, 4)) if cam.shape == (4,) else cam
    if cam.shape != (B, 4) or not np.isfinite(cam).all() or (cam[:, :2] <= 0).any():
        raise ValueError("draw_poses: camera_k must be finite [4] or [batch,4] = fx, fy, cx, cy with positive focal lengths")
    z0, z1 = (float(v) for v in distance_range)
    if not 0.0 < z0 <= z1 or not math.isfinite(z1):
        raise ValueError("draw_poses: distance_range must be 0 < near <= far")
    if not 0.0 <= float(margin) < 0.5:
        raise ValueError("draw_poses: margin must be in [0, 0.5)")
    lab = np.asarray(labels, np.int64).reshape(-1)
    mv = np.arange(1, K + 1) if mask_values is None else np.asarray(mask_values, np.int64).reshape(-1)
    sym = np.zeros(K, np.int64) if symmetric is None else np.asarray(symmetric, np.int64).reshape(-1)
    if lab.shape[0] != K or mv.shape[0] != K or sym.shape[0] != K or (lab < 0).any() or (mv < 1).any() or (mv > 255).any():
        raise ValueError("draw_poses: labels, mask_values and symmetric need one entry per object; labels >= 0, mask values in 1..255")
    out = []
    for b in range(B):
        rot, trn = np.zeros((K, 5), np.float64), np.zeros((K, 3), np.float64)
        for k in range(K):
            u1, u2, u3 = rng.random(), rng.random(), rng.random()
            a, c, d = rng.random(), rng.random(), rng.random()
            s1, s2 = math.sqrt(1.0 - u1), math.sqrt(u1)
            q = np.array([s1 * math.sin(2 * math.pi * u2), s1 * math.cos(2 * math.pi * u2), s2 * math.sin(2 * math.pi * u3), s2 * math.cos(2 * math.pi * u3)])
            n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
            if n > 0.0:
                rot[k, :3] = q[:3] * (2.0 * math.atan2(n, q[3]) / n)
            rot[k, 3], rot[k, 4] = sym[k], lab[k]
            u = width * (margin + a * (1.0 - 2.0 * margin))
            v = height * (margin + c * (1.0 - 2.0 * margin))
            Z = z0 + d * (z1 - z0)
            trn[k] = ((u - cam[b, 2]) * Z / cam[b, 0], (v - cam[b, 3]) * Z / cam[b, 1], Z)
        out.append(dict(bboxes=np.zeros((K, 4), np.float64), labels=lab.copy(), rotations=rot, translations=trn, mask_values=mv.copy()))
    return out


def draw_lights(rng, batch: int, ambient: Tuple[float, float] = (0.3, 0.6), diffuse: Tuple[float, float] = (0.4, 0.8),
                gain: Tuple[float, float] = (0.9, 1.1)) -> np.ndarray:
    """float64 [batch,8] = lx, ly, lz, ambient, diffuse, gain0, gain1, gain2, on the host.  ``rng.random()`` is called seven times per image:
    two for a direction uniform on the sphere (z = 2 r - 1, azimuth 2 pi r; normalised to unit length in float64 - the kernel does not),
    then ambient, diffuse and the three channel gains, each uniform in its range."""
    out = np.zeros((int(batch), LIGHT_DOUBLES), np.float64)
    span = lambda r, t: float(r[0]) + t * (float(r[1]) - float(r[0]))
    for b in range(int(batch)):
        z, az = 2.0 * rng.random() - 1.0, 2.0 * math.pi * rng.random()
        h = math.sqrt(max(0.0, 1.0 - z * z))
        d = np.array([h * math.cos(az), h * math.sin(az), z], np.float64)
        out[b, :3] = d / math.sqrt(float((d * d).sum()))
        out[b, 3], out[b, 4] = span(ambient, rng.random()), span(diffuse, rng.random())
        out[b, 5:8] = [span(gain, rng.random()) for _ in range(3)]
    return out


_GROUP = (("boxes", torch.float64, (4,)), ("labels", torch.int32, ()), ("mask_values", torch.int32, ()), ("rvec", torch.float32, (3,)),
          ("tvec", torch.float32, (3,)), ("extra", torch.float32, (2,)))


def synth_frames(backgrounds_u8: torch.Tensor, annotations: Union[Dict[str, torch.Tensor], Sequence[dict]], camera: torch.Tensor, meshes: ShadedMeshSet,
                 lights, alpha: int = 256, min_pixels: int = 16, mask: bool = True, depth: bool = False) -> Dict[str, object]:
    """``backgrounds_u8``: contiguous uint8 [B,H,W,3] on the meshes' device, composited IN PLACE at ``alpha`` / 256.  ``annotations``: the
    padded tensors of ``augment.pad_annotations`` (labels, mask_values int32 [B,K], rvec, tvec float32 [B,K,3], extra float32 [B,K,2],
    num_gt int32 [B]; boxes are not read) or a list of annotation dicts (``draw_poses``), padded and uploaded once; the pose table is
    ``render.poses_from_annotations`` of them.  ``camera``: float64 [B,5] fx, fy, cx, cy, scale on the device (``render_models``'s).
    ``lights``: float64 [B,8] (``draw_lights``), host array or device tensor.  Returns a dict: ``frames`` (= ``backgrounds_u8``),
    ``mask`` uint8 [B,H,W] and ``depth`` float32 [B,H,W] when asked for, ``visible`` int32 [B,K,5] (min_x, min_y, max_x, max_y, count of
    the pixels each slot won) and ``annotations``: boxes float64 [B,K,4], labels, mask_values, rvec, tvec, extra, num_gt - what
    ``augment.augment_6dof`` takes directly - plus slot_of int32 [B,K]; an object that won fewer than ``min_pixels`` pixels is dropped.
    Raises ValueError for a wrong dtype, device or shape before the ABI sees a pointer; enqueues on the current stream and does not
    synchronise."""
    who = "synth_frames"
    if not isinstance(meshes, ShadedMeshSet):
        raise ValueError(f"{who}: meshes must be a ShadedMeshSet")
    dev = meshes.device
    f = backgrounds_u8
    if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3 or f.device != dev or not f.is_contiguous():
        raise ValueError(f"{who}: backgrounds_u8 must be a contiguous uint8 tensor [B,H,W,3] on {dev} (it is composited in place)")
    B, H, W = (int(v) for v in f.shape[:3])
    if B < 1 or not (16 <= H <= 4096 and 16 <= W <= 4096):
        raise ValueError(f"{who}: {B} x {H} x {W}: B >= 1, height and width in 16..4096")
    if not 0 <= int(alpha) <= 256:
        raise ValueError(f"{who}: alpha must be in 0..256")
    if int(min_pixels) < 1:
        raise ValueError(f"{who}: min_pixels must be >= 1")
    if not isinstance(camera, torch.Tensor) or camera.dtype != torch.float64 or camera.device != dev or tuple(camera.shape) != (B, 5):
        raise ValueError(f"{who}: camera must be a float64 tensor [{B},5] on {dev}")
    if isinstance(lights, torch.Tensor):
        if lights.dtype != torch.float64 or lights.device != dev or tuple(lights.shape) != (B, LIGHT_DOUBLES):
            raise ValueError(f"{who}: lights must be float64 [{B},{LIGHT_DOUBLES}] on {dev}, or a host array")
        d_lights = lights.contiguous()
    else:
        host = np.asarray(lights)
        if host.dtype != np.float64 or host.shape != (B, LIGHT_DOUBLES):
            raise ValueError(f"{who}: lights must be float64 [{B},{LIGHT_DOUBLES}]")
        d_lights = torch.from_numpy(np.ascontiguousarray(host)).to(dev, non_blocking=True)
    if not isinstance(annotations, dict):
        if len(annotations) != B:
            raise ValueError(f"{who}: {len(annotations)} annotation dicts for {B} frames")
        annotations = pad_annotations(annotations, dev)
    need = [k for k, _, _ in _GROUP[1:]] + ["num_gt"]
    if any(not isinstance(annotations.get(k), torch.Tensor) for k in need) or annotations["labels"].dim() != 2:
        raise ValueError(f"{who}: the annotations need the tensors {need}")
    K = int(annotations["labels"].shape[1])
    if not 1 <= K <= MAX_POSES:
        raise ValueError(f"{who}: at most {MAX_POSES} annotations per image")
    src = {}
    for k, dt, tail in _GROUP[1:] + (("num_gt", torch.int32, None),):
        t, shape = annotations[k], ((B,) if tail is None else (B, K) + tail)
        if t.dtype != dt or t.device != dev or tuple(t.shape) != shape:
            raise ValueError(f"{who}: annotations['{k}'] must be a {dt} tensor {list(shape)} on {dev}")
        src[k] = t.contiguous()
    poses = poses_from_annotations(src).contiguous()
    camera = camera.contiguous()
    out: Dict[str, object] = {"frames": f}
    if mask:
        out["mask"] = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    if depth:
        out["depth"] = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    out["visible"] = torch.empty((B, K, VISIBLE_INTS), dtype=torch.int32, device=dev)
    ann = {k: torch.empty((B, K) + tail, dtype=dt, device=dev) for k, dt, tail in _GROUP}
    ann["num_gt"] = torch.empty((B,), dtype=torch.int32, device=dev)
    ann["slot_of"] = torch.empty((B, K), dtype=torch.int32, device=dev)
    out["annotations"] = ann
    ws = _workspace(dev, B, H, W, K, meshes.num_vertices)
    _capi.check(_capi.lib().hep_synth_frames_device(
        poses.data_ptr(), B, K, camera.data_ptr(), meshes.vertices.data_ptr(), meshes.vertex_colours.data_ptr(), meshes.num_vertices, meshes.faces.data_ptr(),
        meshes.face_normals.data_ptr(), meshes.num_faces, meshes.face_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), meshes.num_labels, d_lights.data_ptr(),
        H, W, f.data_ptr(), int(alpha), _capi.ptr(out.get("mask")), _capi.ptr(out.get("depth")), out["visible"].data_ptr(), src["rvec"].data_ptr(),
        src["tvec"].data_ptr(), src["extra"].data_ptr(), int(min_pixels), ann["boxes"].data_ptr(), ann["labels"].data_ptr(), ann["mask_values"].data_ptr(),
        ann["rvec"].data_ptr(), ann["tvec"].data_ptr(), ann["extra"].data_ptr(), ann["num_gt"].data_ptr(), ann["slot_of"].data_ptr(), ws.data_ptr(), ws.numel(),
        torch.cuda.current_stream(dev).cuda_stream))
    return out
