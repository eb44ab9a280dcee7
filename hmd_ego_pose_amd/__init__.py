"""hmd_ego_pose_amd - MI355X-native (gfx950) EfficientPose / HMD-EgoPose inference path.

Only what the hot path needs: ``csrc/`` (HIP kernels + the C ABI of ``libhep.so``),
the ctypes binding, and the host-side mirror of the reference's operator interface
(``HMDEgoPose``, ``TrainModelWithLoss``).  See DESIGN.md.
"""
from .arch import get_arch, level_sizes, num_anchors_total, param_spec  # noqa: F401
from .weights import load_pack, pack_bytes, save_pack, seeded_state_dict, strip_checkpoint_prefix  # noqa: F401


def __getattr__(name):   # torch custom-op registration happens on first use of the model API
    if name in ("HMDEgoPose", "TrainModelWithLoss", "Session", "tile_windows", "window_cameras", "window_from_box",
                "rectify_windows", "rectified_point_to_frame", "window_from_box_rectified"):
        from . import model
        return getattr(model, name)
    if name == "TrainableHeads":
        from .heads import TrainableHeads
        return TrainableHeads
    if name in ("TrainableNeck", "backbone_taps"):
        from . import neck
        return getattr(neck, name)
    if name == "TrainableBackbone":
        from .backbone import TrainableBackbone
        return TrainableBackbone
    if name == "Trainer":
        from .trainer import Trainer
        return Trainer
    if name == "PlateauSchedule":
        from .trainer import PlateauSchedule
        return PlateauSchedule
    if name in ("DeviceEvaluator", "evaluate_device", "gt_table", "SceneEvaluator", "SceneFolder", "evaluate_scene_device", "gt_scene_table"):
        from . import evaluate
        return getattr(evaluate, name)
    if name == "InflightPool":
        from .pipeline import InflightPool
        return InflightPool
    if name in ("augment_6dof", "draw_6dof", "rotation_matrices", "colour_augment", "draw_colour", "COLOUR_OPS"):
        from . import augment
        return getattr(augment, name)
    if name in ("draw_poses", "cuboid_corners", "label_colours", "detections_from_records"):
        from . import draw
        return getattr(draw, name)
    if name in ("render_models", "MeshSet", "load_ply_mesh", "poses_from_annotations", "poses_from_detections"):
        from . import render
        return getattr(render, name)
    if name in ("synth_frames", "ShadedMeshSet", "load_ply_coloured_mesh", "draw_lights"):      # (synth.draw_poses: by its module, draw_poses is the overlay's)
        from . import synth
        return getattr(synth, name)
    if name in ("bop_errors", "pairs_from_scene", "symmetry_transforms", "SymmetrySet", "BopSettings"):
        from . import bop
        return getattr(bop, name)
    raise AttributeError(name)
