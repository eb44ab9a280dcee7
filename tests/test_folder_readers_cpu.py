"""``LinemodFolder`` and ``SceneFolder`` on the synthetic folders of tests/test_host_cpu.py, tests/test_draw_cpu.py and
tests/test_score_scene_cpu.py: every public attribute equals, bit for bit, what tests/golden/folder_readers.npz holds (recorded by
tests/golden/make_golden_evaluator.py on the commit before the two readers got their common part)."""
import hashlib
import json
import os

import numpy as np
import pytest

from hmd_ego_pose_amd import evaluate as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "folder_readers.npz")


def make_folders(root):
    """name -> folder: the calls of the three test files."""
    from tests._util import make_linemod_folder
    from tests.test_score_scene_cpu import _write_scene_folder
    out = {k: os.path.join(root, k) for k in ("host", "host_ascii", "draw", "scene")}
    make_linemod_folder(out["host"], n=4)
    make_linemod_folder(out["host_ascii"], n=1, binary_ply=False)
    make_linemod_folder(out["draw"], n=2, size=64)
    _write_scene_folder(out["scene"])
    return out


READERS = {                                               # name -> (folder, reader)
    "host": ("host", lambda p: E.LinemodFolder(p)),
    "host_ascii": ("host_ascii", lambda p: E.LinemodFolder(p)),
    "draw": ("draw", lambda p: E.LinemodFolder(p)),
    "draw_as_scene": ("draw", lambda p: E.SceneFolder(p, [1])),
    "scene_5_1": ("scene", lambda p: E.SceneFolder(p, [5, 1], scene_id=1)),
    "scene_5_1_mask_of_1": ("scene", lambda p: E.SceneFolder(p, [5, 1], scene_id=1, mask_values={1: 40})),
    "scene_1_5_both_masks": ("scene", lambda p: E.SceneFolder(p, [1, 5], mask_values={1: 40, 5: 90})),
    "scene_1_5_absent_byte": ("scene", lambda p: E.SceneFolder(p, [1, 5], mask_values={5: 7})),
    "scene_6_1": ("scene", lambda p: E.SceneFolder(p, [6, 1], scene_id=1)),
    "scene_as_object_1": ("scene", lambda p: E.LinemodFolder(p, 1)),          # first annotation of object 1, box of ANY non-zero mask pixel
}


def snapshot(ds, root):
    """Every public attribute of a reader as name -> array; paths relative to the folder; one entry per annotation key."""
    out = {}

    def put(k, v):
        v = np.asarray(v)
        if v.nbytes > 4096:                               # the point clouds: their digest keeps the fixture small and is as strict
            v = np.asarray(f"{v.dtype}{v.shape}sha256:" + hashlib.sha256(v.tobytes()).hexdigest())
        out[k] = v
    scene = isinstance(ds, E.SceneFolder)
    put("len", len(ds))
    for k in ("object_path", "model_path"):
        put(k, os.path.relpath(getattr(ds, k), root))
    put("image_paths", [os.path.relpath(p, root) for p in ds.image_paths])
    put("camera", np.stack(ds.camera))
    put("camera_input", np.stack([ds.camera_input(i, 0.5) for i in range(len(ds))]))
    for i, a in enumerate(ds.annotations):
        entries = a if scene else [a]
        put(f"annotations/{i}/count", len(entries))
        for k, e in enumerate(entries):
            for key, v in e.items():
                put(f"annotations/{i}/{k}/{key}", v)
    if scene:
        put("object_ids", ds.object_ids)
        put("amax", ds.amax)
        put("models_info", json.dumps(ds.models_info, sort_keys=True))
        put("cuboids", np.zeros(0) if ds.cuboids is None else ds.cuboids)
        for l, (points, diameter, symmetric) in enumerate(ds.models):
            put(f"models/{l}/points", points); put(f"models/{l}/diameter", diameter); put(f"models/{l}/symmetric", symmetric)
        put("models/count", len(ds.models))
    else:
        put("object_id", ds.object_id)
        put("points", ds.points)
        put("diameter", ds.diameter)
        put("cuboid", np.zeros(0) if ds.cuboid is None else ds.cuboid)
    return out


def record(root):
    folders = make_folders(root)
    return {f"{name}|{k}": v for name, (folder, read) in READERS.items() for k, v in snapshot(read(folders[folder]), folders[folder]).items()}


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    return make_folders(str(tmp_path_factory.mktemp("readers")))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_every_reader_is_recorded(golden):
    assert {k.split("|")[0] for k in golden} == set(READERS)


@pytest.mark.parametrize("name", sorted(READERS))
def test_reader_gives_the_recorded_attributes(name, folders, golden):
    folder, read = READERS[name]
    got = snapshot(read(folders[folder]), folders[folder])
    want = {k.split("|", 1)[1]: v for k, v in golden.items() if k.startswith(name + "|")}
    assert sorted(got) == sorted(want)
    for k, v in got.items():
        assert v.dtype == want[k].dtype and v.shape == want[k].shape and v.tobytes() == want[k].tobytes(), k
