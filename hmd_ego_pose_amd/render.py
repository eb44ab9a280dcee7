"""Object models rendered under poses on the GPU: the uint8 instance mask (what ``augment.augment_6dof`` takes), the depth of the
model and a filled overlay of every image of a batch from one z-buffered triangle rasteriser (hep_render_models_device,
csrc/k_render.hip).  The rasterisation is this project's own definition - float64 projection and depth, exact integer coverage with a
top-left rule, the nearest (z, slot, face) wins; include/hep.h states it, tests/_render.py states it in numpy and the kernels match it
bit for bit.  No textures, shading, anti-aliasing, near-plane clipping or non-triangle faces."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi

MAX_POSES, MAX_ELEMENTS = _capi.RENDER_MAX_POSES, _capi.RENDER_MAX_ELEMENTS
POSE_DOUBLES = 16
_PLY_CODE = {"float": "f4", "float32": "f4", "double": "f8", "float64": "f8", "uchar": "u1", "uint8": "u1", "char": "i1", "int8": "i1",
             "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4"}


def load_ply_mesh(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(vertices float32 [V,3], faces int32 [F,3]) of an ASCII or binary-little-endian PLY file: ``evaluate.load_ply_vertices`` plus the
    ``face`` element's ``vertex_indices`` / ``vertex_index`` list.  A face that is not a triangle, a file without faces and an index
    outside the vertices raise ValueError naming the file."""
    return _read_ply(path, False)[:2]


def _read_ply(path: str, want_colours: bool):
    """The parser behind ``load_ply_mesh`` and ``synth.load_ply_coloured_mesh``: (vertices, faces, colours uint8 [V,3] or None).  With
    ``want_colours`` the vertex element must have the uchar properties red, green and blue."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []                      # elements: [name, count, [(property name, type) or (name, count type, item type)]]
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
                elements.append([tok[1], int(tok[2]), []])
            elif tok[0] == "property" and elements:
                elements[-1][2].append((tok[4], tok[2], tok[3]) if tok[1] == "list" else (tok[2], tok[1]))
            elif tok[0] == "end_header":
                break
        names = [e[0] for e in elements]
        if names[:1] != ["vertex"] or "face" not in names:
            raise ValueError(f"{path}: a mesh needs a vertex element followed by a face element")
        if names[1] != "face":
            raise ValueError(f"{path}: an element between vertex and face is not supported")
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError(f"{path}: unsupported PLY format {fmt}")
        (_, nv, vprops), (_, nf, fprops) = elements[0], elements[1]
        vnames = [p[0] for p in vprops]
        if any(len(p) != 2 for p in vprops) or not all(k in vnames for k in "xyz"):
            raise ValueError(f"{path}: vertex element has no plain x/y/z")
        if want_colours:
            for k in ("red", "green", "blue"):
                if k not in vnames or _PLY_CODE.get(vprops[vnames.index(k)][1]) != "u1":
                    raise ValueError(f"{path}: vertex element has no uchar property '{k}' (a coloured mesh needs red, green and blue)")
        colours = None
        lists = [i for i, p in enumerate(fprops) if len(p) == 3]
        if len(lists) != 1 or fprops[lists[0]][0] not in ("vertex_indices", "vertex_index"):
            raise ValueError(f"{path}: face element needs exactly one list property, vertex_indices or vertex_index")
        if nf < 1:
            raise ValueError(f"{path}: no faces")
        li = lists[0]
        if fmt == "ascii":
            rows = [f.readline().split() for _ in range(nv)]              # line by line: the faces follow in the same stream
            if any(len(r) != len(vprops) for r in rows):
                raise ValueError(f"{path}: truncated vertex element")
            rows = np.array(rows, dtype=np.float64).reshape(nv, len(vprops))
            vertices = np.stack([rows[:, vnames.index(k)] for k in "xyz"], axis=-1).astype(np.float32)
            if want_colours:
                colours = np.stack([rows[:, vnames.index(k)] for k in ("red", "green", "blue")], axis=-1).astype(np.uint8)
            faces = np.empty((nf, 3), np.int64)
            for i in range(nf):
                tok = f.readline().split()
                if len(tok) <= li or int(tok[li]) != 3:       # scalar properties in front of the list take one token each
                    raise ValueError(f"{path}: face {i} is not a triangle")
                faces[i] = [int(t) for t in tok[li + 1:li + 4]]
        else:
            vdt = np.dtype([(nm, "<" + _PLY_CODE[ty]) for nm, ty in vprops])
            v = np.frombuffer(f.read(nv * vdt.itemsize), dtype=vdt, count=nv)
            vertices = np.stack([v["x"], v["y"], v["z"]], axis=-1).astype(np.float32)
            if want_colours:
                colours = np.stack([v["red"], v["green"], v["blue"]], axis=-1).astype(np.uint8)
            fields = []
            for p in fprops:                                   # the record of a triangle; a face of another size breaks the count check
                fields += [("_n", "<" + _PLY_CODE[p[1]]), ("_i", "<" + _PLY_CODE[p[2]], (3,))] if len(p) == 3 else [(p[0], "<" + _PLY_CODE[p[1]])]
            fdt = np.dtype(fields)
            raw = f.read(nf * fdt.itemsize)
            if len(raw) >= fdt.itemsize and np.frombuffer(raw[:fdt.itemsize], dtype=fdt, count=1)["_n"][0] != 3:
                raise ValueError(f"{path}: face 0 is not a triangle")
            if len(raw) != nf * fdt.itemsize:
                raise ValueError(f"{path}: truncated face element")
            rec = np.frombuffer(raw, dtype=fdt, count=nf)
            bad = np.nonzero(rec["_n"] != 3)[0]
            if bad.size:
                raise ValueError(f"{path}: face {int(bad[0])} is not a triangle")
            faces = rec["_i"].astype(np.int64)
    if faces.min() < 0 or faces.max() >= nv:
        raise ValueError(f"{path}: a face index lies outside the {nv} vertices")
    return vertices, faces.astype(np.int32), colours


class MeshSet:
    """The triangle meshes of labels 0..L-1 concatenated and uploaded once: ``vertices`` float32 [V,3] and ``faces`` int32 [F,3] on the
    device (face indices offset into the common vertex array), ``face_start`` and ``vertex_start`` host int32 [L+1].  ``meshes_per_label``: a sequence of
    (vertices [v,3], faces [f,3]) pairs, e.g. ``load_ply_mesh`` results.  Every index is checked here, on the host."""

    def __init__(self, meshes_per_label: Sequence[Tuple[np.ndarray, np.ndarray]], device: Optional[torch.device] = None):
        if not 1 <= len(meshes_per_label) <= _capi.SCORE_MAX_LABELS:
            raise ValueError(f"MeshSet: {len(meshes_per_label)} labels: must be 1..{_capi.SCORE_MAX_LABELS}")
        vs, fs, start, vstart, off = [], [], [0], [0], 0
        for l, (v, f) in enumerate(meshes_per_label):
            v, f = np.asarray(v), np.asarray(f)
            if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1 or not np.issubdtype(v.dtype, np.floating):
                raise ValueError(f"MeshSet: vertices of label {l} must be floating point [V,3] with V >= 1")
            if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not np.issubdtype(f.dtype, np.integer):
                raise ValueError(f"MeshSet: faces of label {l} must be integers [F,3] with F >= 1")
            if f.min() < 0 or f.max() >= v.shape[0]:
                raise ValueError(f"MeshSet: a face index of label {l} lies outside its {v.shape[0]} vertices")
            vs.append(v.astype(np.float32))
            fs.append(f.astype(np.int64) + off)
            off += v.shape[0]
            start.append(start[-1] + f.shape[0])
            vstart.append(off)
        if off > MAX_ELEMENTS or start[-1] > MAX_ELEMENTS:
            raise ValueError(f"MeshSet: {off} vertices and {start[-1]} faces: at most {MAX_ELEMENTS} of each")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.host_vertices = np.ascontiguousarray(np.concatenate(vs))
        self.host_faces = np.ascontiguousarray(np.concatenate(fs).astype(np.int32))
        self.face_start = np.ascontiguousarray(np.asarray(start, np.int32))
        self.vertex_start = np.ascontiguousarray(np.asarray(vstart, np.int32))      # label l owns vertices [vertex_start[l], vertex_start[l+1])
        self.num_labels, self.num_vertices, self.num_faces = len(meshes_per_label), off, int(start[-1])
        self.vertices = torch.from_numpy(self.host_vertices).to(self.device)
        self.faces = torch.from_numpy(self.host_faces).to(self.device)


def _rodrigues(rv: torch.Tensor) -> torch.Tensor:
    """float64 [...,3] axis-angle -> [...,9] row-major rotation matrices, the statements of rodrigues_f64 (csrc/eval_dev.h): identity below
    an angle of 1e-12.  Computed HERE, once: the kernel takes the matrix."""
    x, y, z = rv[..., 0], rv[..., 1], rv[..., 2]
    th = torch.sqrt((x * x + y * y) + z * z)
    small = th < 1e-12
    d = torch.where(small, torch.ones_like(th), th)
    kx, ky, kz, c, s = x / d, y / d, z / d, torch.cos(th), torch.sin(th)
    v = 1.0 - c
    R = torch.stack([c + v * kx * kx, v * kx * ky - s * kz, v * kx * kz + s * ky,
                     v * ky * kx + s * kz, c + v * ky * ky, v * ky * kz - s * kx,
                     v * kz * kx - s * ky, v * kz * ky + s * kx, c + v * kz * kz], dim=-1)
    eye = torch.eye(3, dtype=torch.float64, device=rv.device).reshape(9)      # made on the device: a host list would be a blocking upload
    return torch.where(small[..., None], eye.expand_as(R), R)


def _pose_table(valid, labels, mask_values, rvec, tvec) -> torch.Tensor:
    B, K = valid.shape
    out = torch.zeros((B, K, POSE_DOUBLES), dtype=torch.float64, device=valid.device)
    out[..., 0], out[..., 1], out[..., 2] = valid.to(torch.float64), labels.to(torch.float64), mask_values.to(torch.float64)
    out[..., 4:13] = _rodrigues(rvec.to(torch.float64))
    out[..., 13:16] = tvec.to(torch.float64)
    return out


def poses_from_annotations(annotations, mask_values=None) -> torch.Tensor:
    """The pose table float64 [B,K,16] on the device, with torch float64 operations and no synchronisation, from either
    the padded tensors of ``augment.pad_annotations`` (a dict with labels, mask_values int32 [B,K], rvec, tvec float32 [B,K,3] widened,
    num_gt int32 [B]: the first num_gt[b] slots are valid), or the evaluators' ground-truth table float64 [B,amax,88] / [B,88]
    (``evaluate.gt_scene_table`` / ``gt_table``: slot 0 valid, 5-7 axis-angle, 8-10 translation, 83 label).  The table carries no mask
    value: ``mask_values`` (a sequence, one per label) gives it, default label + 1."""
    who = "poses_from_annotations"
    if isinstance(annotations, dict):
        need = ("labels", "mask_values", "rvec", "tvec", "num_gt")
        if any(k not in annotations or not isinstance(annotations[k], torch.Tensor) for k in need):
            raise ValueError(f"{who}: the annotations need the tensors {need}")
        lab = annotations["labels"]
        if lab.dim() != 2 or not 1 <= lab.shape[1] <= MAX_POSES:
            raise ValueError(f"{who}: labels must be [B,K] with K in 1..{MAX_POSES}")
        B, K = lab.shape
        for k, shape in (("mask_values", (B, K)), ("rvec", (B, K, 3)), ("tvec", (B, K, 3)), ("num_gt", (B,))):
            if tuple(annotations[k].shape) != shape or annotations[k].device != lab.device:
                raise ValueError(f"{who}: annotations['{k}'] must be {list(shape)} on {lab.device}")
        valid = torch.arange(K, device=lab.device)[None, :] < annotations["num_gt"][:, None]
        return _pose_table(valid, lab, annotations["mask_values"], annotations["rvec"], annotations["tvec"])
    gt = annotations
    if not isinstance(gt, torch.Tensor) or gt.dtype != torch.float64 or gt.dim() not in (2, 3) or gt.shape[-1] != _capi.SCORE_GT_DOUBLES:
        raise ValueError(f"{who}: a dict of padded annotation tensors or a float64 table [B,amax,{_capi.SCORE_GT_DOUBLES}] / [B,{_capi.SCORE_GT_DOUBLES}]")
    if gt.dim() == 2:
        gt = gt[:, None, :]
    if not 1 <= gt.shape[1] <= MAX_POSES:
        raise ValueError(f"{who}: amax must be in 1..{MAX_POSES}")
    lab = gt[..., 83]
    if mask_values is None:
        mv = lab + 1.0
    else:
        table = torch.as_tensor(np.asarray(mask_values, np.float64), device=gt.device)
        inside = (lab >= 0) & (lab < table.numel())                            # NaN fails: the row is skipped by its label anyway
        mv = torch.where(inside, table[torch.where(inside, lab, torch.zeros_like(lab)).long()], torch.zeros_like(lab))
    return _pose_table(gt[..., 0] != 0, lab, mv, gt[..., 5:8], gt[..., 8:11])


def poses_from_detections(det: Dict[str, torch.Tensor], score_threshold: float = 0.5, max_detections: int = 10, mask_values=None) -> torch.Tensor:
    """The pose table float64 [B,max_detections,16] of the kept detections, on the device and without synchronisation, under the
    candidate rule and roundings ``hep_draw_poses_device`` states: a row with score > ``score_threshold`` (float32 compare; padding and
    NaN are none) is a candidate, the first ``max_detections`` candidates in row order are kept (slot k: the k-th), rotation =
    float32(r) * float32(pi) in float32, then Rodrigues in float64; the translation is widened.  A kept row whose label is out of range
    stays in the table and is skipped by the renderer, as the draw call skips it.  Mask value: ``mask_values[label]``, default label + 1."""
    who = "poses_from_detections"
    for k in ("scores", "labels", "rotation", "translation"):
        if not isinstance(det.get(k), torch.Tensor):
            raise ValueError(f"{who}: detections lack '{k}'")
    sc, lab, rot, trn = det["scores"], det["labels"], det["rotation"], det["translation"]
    if sc.dim() != 2 or sc.dtype != torch.float32 or lab.dtype != torch.int32 or rot.dtype != torch.float32 or trn.dtype != torch.float32:
        raise ValueError(f"{who}: scores float32 [B,rows], labels int32, rotation and translation float32")
    B, rows = sc.shape
    if tuple(lab.shape) != (B, rows) or tuple(rot.shape) != (B, rows, 3) or tuple(trn.shape) != (B, rows, 3):
        raise ValueError(f"{who}: labels [B,rows], rotation and translation [B,rows,3] with B, rows = {B}, {rows}")
    M = int(max_detections)
    if not 1 <= M <= min(rows, MAX_POSES):
        raise ValueError(f"{who}: max_detections {M}: must be 1..min(rows, {MAX_POSES})")
    cand = sc > torch.tensor(float(score_threshold), dtype=torch.float32, device=sc.device)
    rank = torch.cumsum(cand.to(torch.int64), dim=1) - 1                      # the candidate's position among the candidates
    keep = cand & (rank < M)
    # slot k of an image takes its k-th candidate: scatter row indices by rank (rows that are not kept go to a spare slot M)
    slot = torch.where(keep, rank, torch.full_like(rank, M))
    row_of = torch.zeros((B, M + 1), dtype=torch.int64, device=sc.device)
    row_of.scatter_(1, slot, torch.arange(rows, device=sc.device).expand(B, rows))
    row_of = row_of[:, :M]
    valid = torch.arange(M, device=sc.device)[None, :] < keep.sum(dim=1, keepdim=True)
    lab_k = torch.gather(lab.to(torch.int64), 1, row_of)
    rv = torch.gather(rot, 1, row_of[..., None].expand(B, M, 3)) * torch.tensor(math.pi, dtype=torch.float32, device=sc.device)      # float32
    tv = torch.gather(trn, 1, row_of[..., None].expand(B, M, 3))
    if mask_values is None:
        mv = lab_k + 1
    else:
        table = torch.as_tensor(np.asarray(mask_values, np.int64), device=sc.device)
        inside = (lab_k >= 0) & (lab_k < table.numel())
        mv = torch.where(inside, table[torch.where(inside, lab_k, torch.zeros_like(lab_k))], torch.zeros_like(lab_k))
    return _pose_table(valid, lab_k, mv, rv, tv)


_workspaces: Dict[tuple, torch.Tensor] = {}


def _workspace(dev, B, H, W, pmax, V) -> torch.Tensor:
    """The caller-owned workspace of one shape, kept: launches on one stream are ordered, so successive calls may share it."""
    key = (dev, B, H, W, pmax, V)
    ws = _workspaces.get(key)
    if ws is None:
        if len(_workspaces) >= 8:
            _workspaces.clear()
        need = _capi.check(_capi.lib().hep_render_workspace_bytes(B, H, W, pmax, V))
        ws = _workspaces[key] = torch.empty((need,), dtype=torch.uint8, device=dev)
    return ws


def render_models(poses: torch.Tensor, camera: torch.Tensor, meshes: MeshSet, height: int, width: int, *, mask: bool = True, depth: bool = False,
                  blend_into: Optional[torch.Tensor] = None, colours=None, alpha: int = 128) -> Dict[str, torch.Tensor]:
    """Render the meshes under ``poses`` (float64 [B,pmax,16]: ``poses_from_annotations`` / ``poses_from_detections``; include/hep.h has
    the layout) through ``camera`` (float64 [B,5] fx, fy, cx, cy, scale; scale unused), both on the meshes' device.  Returns a dict with
    ``mask`` uint8 [B,H,W] (0, or the nearest pose's mask value), ``depth`` float32 [B,H,W] (0, or the nearest surface's Z) and
    ``frames`` = ``blend_into`` (uint8 [B,H,W,3], contiguous, blended in place with ``colours`` - host uint8 [L,3], default
    ``draw.label_colours`` - at ``alpha`` / 256) - those that were asked for.  Raises ValueError for a wrong dtype, device or shape
    before the ABI sees a pointer; enqueues on the current stream and does not synchronise."""
    who = "render_models"
    if not isinstance(meshes, MeshSet):
        raise ValueError(f"{who}: meshes must be a MeshSet")
    dev = meshes.device
    if not isinstance(poses, torch.Tensor) or poses.dtype != torch.float64 or poses.dim() != 3 or poses.shape[2] != POSE_DOUBLES or poses.device != dev:
        raise ValueError(f"{who}: poses must be a float64 tensor [B,pmax,{POSE_DOUBLES}] on {dev}")
    B, pmax = int(poses.shape[0]), int(poses.shape[1])
    if B < 1 or not 1 <= pmax <= MAX_POSES:
        raise ValueError(f"{who}: poses [{B},{pmax},16]: B >= 1 and pmax in 1..{MAX_POSES}")
    if not isinstance(camera, torch.Tensor) or camera.dtype != torch.float64 or camera.device != dev or tuple(camera.shape) != (B, 5):
        raise ValueError(f"{who}: camera must be a float64 tensor [{B},5] on {dev}")
    H, W = int(height), int(width)
    if not (16 <= H <= 4096 and 16 <= W <= 4096):
        raise ValueError(f"{who}: {H} x {W}: height and width must be in 16..4096")
    if not mask and not depth and blend_into is None:
        raise ValueError(f"{who}: nothing to render: mask, depth and blend_into are all off")
    col = None
    if blend_into is not None:
        f = blend_into
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or tuple(f.shape) != (B, H, W, 3) or f.device != dev or not f.is_contiguous():
            raise ValueError(f"{who}: blend_into must be a contiguous uint8 tensor [{B},{H},{W},3] on {dev} (it is blended in place)")
        if colours is None:
            from .draw import label_colours
            colours = label_colours(meshes.num_labels)
        col = np.asarray(colours)
        if col.dtype != np.uint8 or col.shape != (meshes.num_labels, 3):
            raise ValueError(f"{who}: colours must be a host uint8 array [{meshes.num_labels},3]")
        col = np.ascontiguousarray(col)
        if not 0 <= int(alpha) <= 256:
            raise ValueError(f"{who}: alpha must be in 0..256")
    poses, camera = poses.contiguous(), camera.contiguous()
    out: Dict[str, torch.Tensor] = {}
    if mask:
        out["mask"] = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    if depth:
        out["depth"] = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    if blend_into is not None:
        out["frames"] = blend_into
    ws = _workspace(dev, B, H, W, pmax, meshes.num_vertices)
    _capi.check(_capi.lib().hep_render_models_device(
        poses.data_ptr(), B, pmax, camera.data_ptr(), meshes.vertices.data_ptr(), meshes.num_vertices, meshes.faces.data_ptr(), meshes.num_faces,
        meshes.face_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), meshes.num_labels, H, W, _capi.ptr(out.get("mask")), _capi.ptr(out.get("depth")),
        _capi.ptr(out.get("frames")), None if col is None else col.ctypes.data, int(alpha), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return out
