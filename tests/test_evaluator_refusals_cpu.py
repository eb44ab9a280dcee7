"""Every refusal of the device evaluators, their folder drivers and the folder readers, held to the recorded (exception type, message)
pairs of tests/golden/evaluator_refusals.json (written by tests/golden/make_golden_evaluator.py on the commit before the evaluators got
their common core): what ``DeviceEvaluator`` / ``SceneEvaluator`` refuse, in which order and in which words, is part of their interface.

No GPU: both evaluators are built on ``torch.device("cpu")`` with ``model=None`` or a stub whose ``detect`` returns host tensors, and
every case ends in a ValueError BEFORE the library call - which would see host pointers - so no case may pass its last check."""
import json
import os

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import evaluate as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluator_refusals.json")
CPU = torch.device("cpu")
S = 16                                                    # the network size of every case
PTS = np.arange(12, dtype=np.float32).reshape(4, 3)
CUBE = np.zeros((8, 3), np.float32)
KINDS = ("device", "scene")
NUM_CASES = 125                                           # counted: len(CASES), asserted below


def evaluator(kind, **kw):
    if kind == "device":
        a = dict(model=None, points=PTS, diameter=100.0, image_size=S, capacity=4, device=CPU)
        return E.DeviceEvaluator(**dict(a, **kw))
    a = dict(model=None, models=[(PTS, 100.0, False), (PTS[:2], 90.0, True)], image_size=S, capacity=4, amax=3, device=CPU)
    if "cuboid" in kw:
        kw["cuboids"] = np.stack([kw.pop("cuboid")] * 2)      # the same one for both labels
    return E.SceneEvaluator(**dict(a, **kw))


def batch(kind, B=2, **change):
    """A valid batch of network inputs (no preprocess, so no session), with ``change`` laid over it."""
    b = dict(frames=torch.zeros((B, 3, S, S), dtype=torch.float32), camera=torch.zeros((B, 6), dtype=torch.float32),
             gt=torch.zeros((B, 88) if kind == "device" else (B, 3, 88), dtype=torch.float64))
    return dict(b, **change)


class Stub:
    """``model.detect`` of six padded host tensors with ``rows`` rows; ``change``: name -> f(B, rows) replacing one of them."""

    def __init__(self, rows=12, **change):
        self.rows, self.change = rows, change

    def detect(self, x, camera):
        B, R = int(x.shape[0]), self.rows
        det = dict(boxes=torch.zeros((B, R, 4)), scores=torch.zeros((B, R)), labels=torch.zeros((B, R), dtype=torch.int32),
                   rotation=torch.zeros((B, R, 3)), translation=torch.zeros((B, R, 3)), hand=torch.zeros((B, R, 63)))
        det.update({k: f(B, R) for k, f in self.change.items()})
        return det


def u8(B=2, h=S, w=S, c=3):
    return torch.zeros((B, h, w, c), dtype=torch.uint8)


def mesh_set(labels):
    from hmd_ego_pose_amd.render import MeshSet
    return MeshSet([(PTS, np.array([[0, 1, 2]], np.int32))] * labels, device=CPU)


CASES = {}


def case(name, both=True):
    """Registers f(kind) once per evaluator class, or f(folders) once."""
    def deco(f):
        for kind in (KINDS if both else (None,)):
            key = f"{kind}:{name}" if both else name
            assert key not in CASES, key
            CASES[key] = (f, kind)
        return f
    return deco


# ---- the constructors --------------------------------------------------------------------------------------------------------------
for _name, _kw in (("capacity_0", dict(capacity=0)), ("max_detections_0", dict(max_detections=0)), ("max_points_0", dict(max_points=0)),
                   ("max_points_1025", dict(max_points=1025))):
    case("init_" + _name)(lambda kind, kw=_kw: evaluator(kind, **kw))
case("init_cuboid_shape")(lambda kind: evaluator(kind, cuboid=np.zeros((7, 3), np.float32)))
case("init_amax_0", both=False)(lambda f: evaluator("scene", amax=0))
case("init_amax_17", both=False)(lambda f: evaluator("scene", amax=17))
case("init_no_models", both=False)(lambda f: evaluator("scene", models=[]))
case("init_64_models", both=False)(lambda f: evaluator("scene", models=[(PTS, 1.0, False)] * 64))
case("init_cuboids_one_short", both=False)(lambda f: evaluator("scene", cuboids=np.zeros((1, 8, 3), np.float32)))
case("init_points_flat", both=False)(lambda f: evaluator("device", points=np.zeros(6, np.float32)))
case("init_points_width", both=False)(lambda f: evaluator("device", points=np.zeros((5, 2), np.float32)))
case("init_points_empty", both=False)(lambda f: evaluator("device", points=np.zeros((0, 3), np.float32)))
case("init_points_of_label_1_width", both=False)(lambda f: evaluator("scene", models=[(PTS, 1.0, False), (np.zeros((5, 4)), 1.0, False)]))
case("init_points_of_label_0_empty", both=False)(lambda f: evaluator("scene", models=[(np.zeros((0, 3)), 1.0, False)]))


# ---- add: draw_into ----------------------------------------------------------------------------------------------------------------
def add(kind, ev_kw=None, **change):
    evaluator(kind, **(ev_kw or {})).add(**batch(kind, **change))


case("draw_into_without_cuboids")(lambda kind: add(kind, draw_into=u8()))
for _name, _t in (("not_a_tensor", lambda: np.zeros((2, S, S, 3), np.uint8)), ("float", lambda: u8().float()), ("three_dims", lambda: u8()[0]),
                  ("four_channels", lambda: u8(c=4)), ("strided", lambda: u8(w=2 * S)[:, :, ::2]), ("other_batch", lambda: u8(B=3))):
    case("draw_into_" + _name)(lambda kind, t=_t: add(kind, dict(cuboid=CUBE), draw_into=t()))
case("draw_into_other_batch_than_uint8_frames")(lambda kind: add(kind, dict(cuboid=CUBE), frames=u8(B=2), draw_into=u8(B=1)))
for _name, _hw in (("height_15", (15, S)), ("height_4097", (4097, S)), ("width_15", (S, 15)), ("width_4097", (S, 4097))):
    case("draw_into_" + _name)(lambda kind, hw=_hw: add(kind, dict(cuboid=CUBE), draw_into=u8(h=hw[0], w=hw[1])))
case("draw_into_65_detections")(lambda kind: add(kind, dict(cuboid=CUBE, max_detections=65), draw_into=u8()))

# ---- add: meshes -------------------------------------------------------------------------------------------------------------------
case("meshes_without_draw_into")(lambda kind: add(kind, meshes=mesh_set(1)))
case("meshes_not_a_mesh_set")(lambda kind: add(kind, dict(cuboid=CUBE), draw_into=u8(), meshes=[(PTS, np.array([[0, 1, 2]]))]))
case("meshes_17_detections")(lambda kind: add(kind, dict(cuboid=CUBE, max_detections=17), draw_into=u8(), meshes=mesh_set(2)))

# ---- add: bop (bop.check_settings words them; the prefix is the evaluator's) ----------------------------------------------------------
case("depth_test_without_bop")(lambda kind: add(kind, depth_test=torch.zeros((2, S, S))))
case("bop_not_settings")(lambda kind: add(kind, bop=object()))

# ---- add: tensors, shapes, capacity --------------------------------------------------------------------------------------------------
case("frames_not_a_tensor")(lambda kind: add(kind, frames=np.zeros((2, 3, S, S), np.float32)))
case("camera_float64")(lambda kind: add(kind, camera=torch.zeros((2, 6), dtype=torch.float64)))
case("camera_not_a_tensor")(lambda kind: add(kind, camera=[[0.0] * 6] * 2))
case("gt_float32")(lambda kind: add(kind, gt=batch(kind)["gt"].float()))
case("frames_three_dims")(lambda kind: add(kind, frames=torch.zeros((3, S, S))))
case("frames_empty_batch")(lambda kind: add(kind, frames=torch.zeros((0, 3, S, S))))
case("uint8_frames_four_channels")(lambda kind: add(kind, frames=u8(c=4)))
case("frames_float64")(lambda kind: add(kind, frames=torch.zeros((2, 3, S, S), dtype=torch.float64)))
case("frames_other_size")(lambda kind: add(kind, frames=torch.zeros((2, 3, S, S + 1))))
case("frames_channels_last")(lambda kind: add(kind, frames=torch.zeros((2, S, S, 3))))
case("camera_five_columns")(lambda kind: add(kind, camera=torch.zeros((2, 5))))
case("camera_other_batch")(lambda kind: add(kind, camera=torch.zeros((3, 6))))
case("gt_other_batch")(lambda kind: add(kind, gt=batch(kind, B=1)["gt"]))
case("gt_87_doubles")(lambda kind: add(kind, gt=batch(kind)["gt"][..., :87]))
case("gt_shape_of_the_other_class")(lambda kind: add(kind, gt=batch("scene" if kind == "device" else "device")["gt"]))
case("gt_other_amax", both=False)(lambda f: add("scene", gt=torch.zeros((2, 2, 88), dtype=torch.float64)))
case("capacity_exceeded")(lambda kind: add(kind, dict(capacity=1)))
case("capacity_exceeded_by_uint8_frames")(lambda kind: add(kind, dict(capacity=1), frames=u8()))


@case("capacity_is_checked_before_the_model_is_used")
def _(kind):
    ev = evaluator(kind, capacity=5)
    ev.count = 4                                           # as after two batches of two
    ev.add(**batch(kind))


# ---- add: the detection rows -------------------------------------------------------------------------------------------------------
def detect(kind, stub, **ev_kw):
    evaluator(kind, model=stub, **ev_kw).add(**batch(kind))


case("rows_boxes_width")(lambda kind: detect(kind, Stub(boxes=lambda B, R: torch.zeros((B, R, 5)))))
case("rows_scores_three_dims")(lambda kind: detect(kind, Stub(scores=lambda B, R: torch.zeros((B, R, 1)))))
case("rows_scores_float64")(lambda kind: detect(kind, Stub(scores=lambda B, R: torch.zeros((B, R), dtype=torch.float64))))
case("rows_labels_int64")(lambda kind: detect(kind, Stub(labels=lambda B, R: torch.zeros((B, R), dtype=torch.int64))))
case("rows_labels_other_rows")(lambda kind: detect(kind, Stub(labels=lambda B, R: torch.zeros((B, R + 1), dtype=torch.int32))))
case("rows_rotation_other_batch")(lambda kind: detect(kind, Stub(rotation=lambda B, R: torch.zeros((B + 1, R, 3)))))
case("rows_translation_half")(lambda kind: detect(kind, Stub(translation=lambda B, R: torch.zeros((B, R, 3), dtype=torch.float16))))
case("rows_hand_width")(lambda kind: detect(kind, Stub(hand=lambda B, R: torch.zeros((B, R, 42)))))
case("rows_0")(lambda kind: detect(kind, Stub(rows=0)))
case("rows_257")(lambda kind: detect(kind, Stub(rows=257)))
case("rows_fewer_than_max_detections")(lambda kind: detect(kind, Stub(rows=9)))
case("rows_fewer_than_max_detections_11")(lambda kind: detect(kind, Stub(rows=10), max_detections=11))


# ---- the folder drivers and the folder readers ---------------------------------------------------------------------------------------
def make_folders(root):
    """``plain``: tests/_util.make_linemod_folder as tests/test_draw_cpu.py calls it; ``bare``: its models_info.yml without the cuboid;
    ``other``: frame 0 annotated for object 2 only; ``crowded``: frame 0 with 17 entries of object 1."""
    import yaml
    from tests._util import make_linemod_folder
    out = {}
    for name in ("plain", "bare", "other", "crowded"):
        out[name] = os.path.join(root, name)
        make_linemod_folder(out[name], n=2, size=64)
        gt_path = os.path.join(out[name], "data", "01", "gt_0.yml")
        with open(gt_path) as f:
            gt = yaml.safe_load(f)
        if name == "bare":
            with open(os.path.join(out[name], "models", "models_info.yml"), "w") as f:
                yaml.safe_dump({1: {"diameter": 180.0}}, f)
        elif name == "other":
            gt[0][0]["obj_id"] = 2
        elif name == "crowded":
            gt[0] = gt[0] * 17
        with open(gt_path, "w") as f:
            yaml.safe_dump(gt, f)
    return out


case("evaluate_device_save_path_without_cuboid", both=False)(
    lambda f: E.evaluate_device(E.LinemodFolder(f["bare"]), None, 64, device=CPU, save_path=os.path.join(f["bare"], "out")))
case("evaluate_device_draw_model_without_save_path", both=False)(
    lambda f: E.evaluate_device(E.LinemodFolder(f["plain"]), None, 64, device=CPU, draw_model=True))
case("evaluate_scene_device_save_path_without_cuboids", both=False)(
    lambda f: E.evaluate_scene_device(E.SceneFolder(f["bare"], [1]), None, 64, device=CPU, save_path=os.path.join(f["bare"], "out")))
case("evaluate_scene_device_draw_model_without_save_path", both=False)(
    lambda f: E.evaluate_scene_device(E.SceneFolder(f["plain"], [1]), None, 64, device=CPU, draw_model=True))
case("linemod_folder_frame_without_its_object", both=False)(lambda f: E.LinemodFolder(f["other"]))
case("scene_folder_no_object_ids", both=False)(lambda f: E.SceneFolder(f["plain"], []))
case("scene_folder_repeated_object_id", both=False)(lambda f: E.SceneFolder(f["plain"], [1, 1]))
case("scene_folder_17_annotations", both=False)(lambda f: E.SceneFolder(f["crowded"], [1]))


def run_case(name, folders):
    """(exception type, message) of one case; a case that raises nothing says so."""
    f, kind = CASES[name]
    try:
        f(kind if kind is not None else folders)
    except Exception as e:                                  # noqa: BLE001 - the type is what is recorded
        return [type(e).__name__, str(e)]
    return ["no exception", ""]


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    return make_folders(str(tmp_path_factory.mktemp("refusals")))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_case_list_is_the_recorded_one(golden):
    assert len(CASES) == NUM_CASES >= 30 and sorted(golden) == sorted(CASES)
    assert all(t == "ValueError" and m for t, m in golden.values())          # none got past its last check when it was recorded
    for cls, kind in (("DeviceEvaluator", "device"), ("SceneEvaluator", "scene")):          # every class's own prefix, on every one of its cases
        own = [golden[k][1] for k in CASES if k.startswith(kind + ":")]
        assert len(own) >= 30 and all(m.startswith(cls + ":") or m.startswith(cls + ".add:") for m in own)


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal_is_the_recorded_one(name, folders, golden):
    assert run_case(name, folders) == golden[name]
