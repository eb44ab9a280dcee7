"""Shared helpers for the tests: seeded inputs (same recipe as tests/golden/make_golden.py)
and golden-digest comparison."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {  # tag -> (phi, size, batch, seed, input kind)
    "phi0_s256_b2_seed0": (0, 256, 2, 0, "normal"),
    "phi0_s256_b1_seed1": (0, 256, 1, 1, "uniform"),
    "phi3_s512_b1_seed0": (3, 512, 1, 0, "normal"),
    # the BENCHMARKED shapes (BASELINE configs[1] and configs[3]): the launch plan depends on the batch (multi-pass fronts by
    # rounds of workgroups, two tiles per workgroup in the boundary kernels, the split-K tile of the project GEMMs)
    "phi0_s256_b16_seed0": (0, 256, 16, 0, "normal"),
    "phi3_s512_b8_seed0": (3, 512, 8, 0, "normal"),
    # the regime of the reference's only published latency ("effnet_b0_512", FP32, batch 1: unity-sandbox/WebRTCNetCoreSandbox/Program.cs:24-33),
    # what bench.py's latency_b1 block times
    "phi0_s512_b1_seed0": (0, 512, 1, 0, "normal"),
}
CLASS_CASES = {  # tag -> (phi, size, batch, seed, input kind, num_classes): the classifier header with more than one class
    "phi0_s256_b2_seed0_k3": (0, 256, 2, 0, "normal", 3),
}

# ---- what the GPU parity suite compares with a reference -------------------------------------------------------------------
# One entry per session that a test of tests/test_gpu_parity.py holds against the CPU oracle:
#   (phi, size, batch, dtype, knob environment, kind)
# kind "stages":     teacher-forced stage by stage with FLAG_KEEP_INTERMEDIATES (_teacher_forced_fp32 / _teacher_forced_bf16 and
#                    test_planner_variants_match_oracle_stage_by_stage, which checks the stages that hold a variant nothing else reaches);
# kind "end_to_end": the head outputs within the fp32 1e-3 gate of the oracle.
# Sessions that are only compared bit for bit with another plan (the fragment-order and bf16 plan-variant tests), the bf16 loop
# of test_other_input_sizes (finite and loosely close) and the several-class sessions are not listed: they pin no variant to a
# reference.  The tests take their parameters from these groups; tests/test_plan_coverage_cpu.py plans every entry on the host
# and requires that each variant the planner can select over its support matrix is reached by at least one of them.
def _e2e(cfgs, env=None):
    return [(phi, size, batch, "fp32", dict(env or {}), "end_to_end") for phi, size, batch in cfgs]


def _stages(cfgs, dtype):
    return [(phi, size, batch, dtype, {}, "stages") for phi, size, batch in cfgs]


OTHER_WIDTHS = [(phi, 256, 2) for phi in (1, 2, 4, 5, 6)]            # test_other_widths_match_oracle
RAGGED_TILES = [(0, 384, 3), (0, 640, 1)]                             # test_ragged_tiles_match_oracle
OTHER_SIZES = [(0, 128, 5), (0, 384, 2)]                              # test_other_input_sizes
BF16_BASELINE = [(0, 256, 16), (3, 512, 8)]                           # test_bf16_matches_bf16_emulating_oracle
FP32_STAGEWISE = [(0, 256, 16)]                                       # test_fp32_stage_by_stage_at_rounding_level
ALT_PLAN_CONFIG = (0, 256, 3)                                         # test_alternative_plans_keep_parity, under each environment of:
ALT_PLAN_ENVS = [{"HEP_MBF_MP": "force"}, {"HEP_LANES": "2"}, {"HEP_SE_MAXMB": "0"}, {"HEP_SE_MAXMB": "1000"}, {"HEP_TOWER_COOP": "0"},
                 {"HEP_XBF_GENERIC": "1"}, {"HEP_STEM_MFMA": "1"}]
# test_planner_variants_match_oracle_stage_by_stage: (phi, size, batch, dtype, the variants the case is there for).  The smallest set of
# configurations found (greedy by variants per cost, redundant picks dropped: tools/plan_variants.py --uncovered --without variant_cover)
# that reaches every variant of the support matrix that no entry above selects; the test checks the stages that hold a listed variant
VARIANT_COVER = [
    (0, 128, 1, 'bf16', ("pw_gemm_kernel<1, 1, 1, 2, 0, 1, 4>", "pw_gemm_kernel<1, 1, 1, 2, 0, 2, 4>")),
    (1, 128, 16, 'fp32', ("pw_gemm_kernel<0, 2, 1, 0, 0, 1, 4>",)),
    (3, 128, 1, 'bf16', ("pw_gemm_kernel<1, 1, 1, 2, 0, 3, 4>", "sep_kernel<true, 2, true, false>")),
    (3, 128, 1, 'fp32', ("pw_gemm_kernel<0, 1, 1, 2, 0, 2, 4>", "pw_gemm_kernel<0, 2, 1, 1, 0, 2, 4>", "pw_gemm_kernel<0, 2, 1, 2, 0, 1, 4>")),
    (0, 384, 1, 'fp32', ("pw_gemm_kernel<0, 2, 1, 1, 1, 0, 4>",)),
    (0, 256, 64, 'fp32', ("pw_gemm_kernel<0, 1, 5, 0, 0, 2, 4>", "pw_gemm_kernel<0, 1, 5, 0, 0, 3, 4>", "pw_gemm_kernel<0, 1, 7, 0, 0, 3, 4>", "pw_gemm_kernel<0, 2, 3, 0, 0, 1, 4>", "pw_gemm_kernel<0, 2, 3, 0, 0, 3, 4>")),
    (2, 128, 64, 'bf16', ("pw_gemm_kernel<1, 1, 3, 0, 0, 2, 4>", "pw_gemm_kernel<1, 2, 1, 0, 0, 1, 4>")),
    (0, 384, 32, 'fp32', ("pw_gemm_kernel<0, 1, 7, 0, 1, 0, 4>", "pw_gemm_kernel<0, 1, 8, 0, 1, 0, 4>")),
    (4, 128, 64, 'bf16', ("pw_gemm_kernel<1, 1, 4, 0, 0, 1, 4>", "pw_gemm_kernel<1, 1, 4, 0, 0, 2, 4>")),
    (4, 128, 64, 'fp32', ("pw_gemm_kernel<0, 1, 4, 0, 0, 1, 4>", "pw_gemm_kernel<0, 1, 4, 0, 0, 3, 4>")),
    (0, 640, 16, 'bf16', ("mbf_kernel<true, 5, 1, 8, false, 1>", "pw_gemm_kernel<1, 1, 5, 0, 0, 1, 4>", "pw_gemm_kernel<1, 1, 5, 0, 0, 3, 4>", "pw_gemm_kernel<1, 1, 7, 0, 0, 3, 4>", "pw_gemm_kernel<1, 1, 7, 0, 1, 0, 4>", "pw_gemm_kernel<1, 1, 8, 0, 1, 0, 4>", "pw_gemm_kernel<1, 2, 3, 0, 0, 3, 4>")),
    (2, 384, 1, 'fp32', ("dw_kernel<false, 3, 1, 1>",)),
    (5, 128, 64, 'fp32', ("pw_gemm_kernel<0, 1, 4, 0, 0, 2, 4>",)),
    (2, 256, 64, 'bf16', ("pw_gemm_kernel<1, 1, 6, 0, 0, 2, 4>", "pw_gemm_kernel<1, 1, 6, 0, 0, 3, 4>", "pw_gemm_kernel<1, 1, 8, 0, 0, 3, 4>", "pw_gemm_kernel<1, 2, 1, 0, 0, 3, 4>", "pw_gemm_kernel<1, 2, 3, 0, 0, 1, 4>")),
    (2, 256, 64, 'fp32', ("pw_gemm_kernel<0, 1, 6, 0, 0, 3, 4>", "pw_gemm_kernel<0, 1, 8, 0, 0, 3, 4>", "pw_gemm_kernel<0, 2, 1, 0, 0, 3, 4>")),
    (5, 256, 1, 'fp32', ("pw_gemm_kernel<0, 1, 2, 2, 1, 0, 4>",)),
    (2, 512, 1, 'bf16', ("pw_gemm_kernel<1, 2, 1, 2, 0, 2, 4>", "pw_gemm_kernel<1, 2, 2, 2, 0, 2, 4>")),
    (4, 256, 32, 'bf16', ("mbf_kernel<true, 5, 2, 8, false, 1>", "pw_gemm_kernel<1, 1, 4, 0, 0, 3, 4>")),
    (3, 512, 3, 'fp32', ("pw_gemm_kernel<0, 1, 2, 0, 0, 3, 4>",)),
    (4, 256, 64, 'bf16', ("pw_gemm_kernel<1, 1, 7, 0, 0, 2, 4>", "pw_gemm_kernel<1, 2, 4, 0, 0, 1, 4>", "pw_gemm_kernel<1, 2, 4, 0, 0, 3, 4>")),
    (4, 256, 64, 'fp32', ("pw_gemm_kernel<0, 2, 4, 0, 0, 1, 4>", "pw_gemm_kernel<0, 2, 4, 0, 0, 3, 4>")),
    (5, 256, 64, 'bf16', ("pw_gemm_kernel<1, 1, 8, 0, 0, 2, 4>",)),
    (6, 640, 1, 'bf16', ("dw_kernel<true, 3, 1, 2>", "dw_kernel<true, 5, 1, 4>", "pw_gemm_kernel<1, 2, 2, 2, 1, 0, 4>")),
]

PARITY_GROUPS = {
    "golden": _e2e([c[:3] for c in CASES.values()]),
    "other_widths": _e2e(OTHER_WIDTHS) + _stages(OTHER_WIDTHS, "fp32") + _stages(OTHER_WIDTHS, "bf16"),
    "ragged_tiles": _e2e(RAGGED_TILES) + _stages(RAGGED_TILES, "bf16"),
    "other_sizes": _e2e(OTHER_SIZES),
    "bf16_baseline": _stages(BF16_BASELINE, "bf16"),
    "fp32_stagewise": _stages(FP32_STAGEWISE, "fp32"),
    "alt_plans": [e for env in ALT_PLAN_ENVS for e in _e2e([ALT_PLAN_CONFIG], env)],
    "variant_cover": [(phi, size, batch, dtype, {}, "stages") for phi, size, batch, dtype, _variants in VARIANT_COVER],
}
PARITY_CONFIGS = [e for group in PARITY_GROUPS.values() for e in group]

CAMS = np.array([[480, 480, 128, 128, 1000, 1.0],
                 [572.4114, 573.57043, 325.2611, 242.04899, 1000, 0.8]], dtype=np.float32)


def seeded_input(shape, seed, kind="normal"):
    rng = np.random.Generator(np.random.PCG64([seed, 0x1234]))
    a = rng.standard_normal(shape) if kind == "normal" else rng.random(shape)
    return a.astype(np.float32)


@functools.lru_cache(maxsize=8)
def seeded_state_dict_once(phi, seed=0, num_classes=1):
    """hmd_ego_pose_amd.seeded_state_dict, kept for the next caller: at phi 5 one call draws 34 M values (1 to 2 s) and a
    gradient case needs the same weights for the module, both oracle evaluations and its checks.  Read-only for every caller."""
    from hmd_ego_pose_amd import seeded_state_dict
    return seeded_state_dict(phi, seed, num_classes=num_classes)


def golden_meta():
    with open(os.path.join(GOLDEN, "golden_meta.json")) as f:
        return json.load(f)


def golden_case(tag):
    return golden_meta()[tag], np.load(os.path.join(GOLDEN, f"net_{tag}.npz"))


def strides_for(size, key, batch=1):
    """Stride of the committed slice of a flattened tensor (primes; the batch-8 / batch-16 cases keep every ~16th sample of
    the small-batch ones so that their fixtures stay small)."""
    big = batch >= 8
    if key.startswith("trace_"):
        return (16139 if big else 1009) if size == 256 else (131071 if big else 8191)
    return (1543 if big else 97) if size == 256 else (6353 if big else 397)


ARCH_DIGEST_PHI = (1, 2, 4, 5, 6, 7)     # the phi without a net_*.npz of their own: forward digests in tests/golden/arch_all_phi.npz
ARCH_DIGEST_SIZE = 128


def arch_digest_stride(key, n):
    """Slice stride of tests/golden/arch_all_phi.npz (size 128, batch 1): ``strides_for`` where that keeps at least 16 samples
    of the n elements, else 7 (the top-level maps and taps hold a few hundred elements)."""
    s = strides_for(ARCH_DIGEST_SIZE, key, 1)
    return s if n >= 16 * s else 7


def golden_arch():
    """(meta of tests/golden/arch_all_phi.json, the slices of arch_all_phi.npz): tests/golden/make_golden_arch.py."""
    with open(os.path.join(GOLDEN, "arch_all_phi.json")) as f:
        return json.load(f), np.load(os.path.join(GOLDEN, "arch_all_phi.npz"))


GUARD_BYTES = 1 << 20
GUARD_PATTERN = 0x5AC3A53C               # as a float 2.75e16: nothing a kernel computes here


class GuardedWorkspace:
    """An exact-size, 16-byte aligned workspace window inside a larger device buffer of the test's own, GUARD_BYTES of guard on
    each side.  The window starts out as NaN (a read of scratch that nothing wrote poisons the result), the guards as a fixed
    bit pattern; ``changed()`` lists the guards a kernel wrote into.  The guards are this buffer's memory, so an overrun of
    up to GUARD_BYTES is seen as a changed byte and touches nothing else."""

    def __init__(self, nbytes, device):
        import torch
        assert nbytes > 0 and nbytes % 16 == 0
        self.buf = torch.empty((GUARD_BYTES + nbytes + GUARD_BYTES + 16,), dtype=torch.uint8, device=device)
        lo = (-self.buf.data_ptr()) % 16
        self.nbytes = nbytes
        self.below = self.buf[lo:lo + GUARD_BYTES].view(torch.int32)
        self.window = self.buf[lo + GUARD_BYTES:lo + GUARD_BYTES + nbytes]
        self.above = self.buf[lo + GUARD_BYTES + nbytes:lo + 2 * GUARD_BYTES + nbytes].view(torch.int32)
        self.below.fill_(GUARD_PATTERN)
        self.above.fill_(GUARD_PATTERN)
        self.window.view(torch.float32).fill_(float("nan"))
        self.ptr = self.window.data_ptr()
        assert self.ptr % 16 == 0 and self.above.data_ptr() == self.ptr + nbytes and self.below.data_ptr() + GUARD_BYTES == self.ptr

    def changed(self):
        """[(which guard, changed 32-bit words, byte offset of the first from the guard's start)]; empty when both are intact."""
        out = []
        for name, g in (("below", self.below), ("above", self.above)):
            bad = (g != GUARD_PATTERN).nonzero()
            if bad.numel():
                out.append((name, int(bad.numel()), 4 * int(bad[0])))
        return out


def check_digest(name, arr, info, ref_slice, stride, atol, rtol=0.0):
    """Compare a full tensor against the committed strided slice (elementwise) and the
    float64 sum / abs-sum (global)."""
    a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
    assert list(np.shape(arr)) == info["shape"], (name, np.shape(arr), info["shape"])
    got = a[::stride]
    err = np.abs(got.astype(np.float64) - ref_slice.astype(np.float64))
    tol = atol + rtol * np.abs(ref_slice.astype(np.float64))
    assert np.all(err <= tol), f"{name}: max err {err.max():.3e} (tol {atol:g}+{rtol:g}*|ref|) at {int(err.argmax())}"
    n = a.size
    s = float(a.astype(np.float64).sum())
    sa = float(np.abs(a.astype(np.float64)).sum())
    assert abs(sa - info["abssum"]) <= n * atol + rtol * info["abssum"] + 1e-6, (name, sa, info["abssum"])
    assert abs(s - info["sum"]) <= n * atol + rtol * info["abssum"] + 1e-6, (name, s, info["sum"])
    return float(err.max())


def make_linemod_folder(root, n=5, size=256, seed=0, binary_ply=True):
    """A tiny synthetic dataset in the Linemod layout the reference's ColibriGenerator reads (data/01/{rgb,mask}/*.png,
    gt_0.yml, info_0.yml, test_0.txt, models/obj_01.ply, models_info.yml).  Returns the ground truth it wrote."""
    import os
    import yaml
    from PIL import Image
    from scipy.spatial.transform import Rotation
    rng = np.random.Generator(np.random.PCG64(seed))
    obj = os.path.join(root, "data", "01")
    for d in ("rgb", "mask", "hands"):
        os.makedirs(os.path.join(obj, d), exist_ok=True)
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    pts = (rng.standard_normal((1500, 3)) * np.array([40.0, 25.0, 60.0])).astype(np.float32)
    with open(os.path.join(root, "models", "obj_01.ply"), "wb") as f:
        if binary_ply:
            f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n" % len(pts))
            rec = np.zeros(len(pts), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1")])
            rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
            f.write(rec.tobytes())
        else:
            f.write(b"ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(pts))
            for p in pts:
                f.write(("%r %r %r\n" % (float(p[0]), float(p[1]), float(p[2]))).encode())
    with open(os.path.join(root, "models", "models_info.yml"), "w") as f:
        yaml.safe_dump({1: {"diameter": 180.0, "min_x": -100.0, "min_y": -80.0, "min_z": -150.0, "size_x": 200.0, "size_y": 160.0, "size_z": 300.0}}, f)
    gt, info, names, truth = {}, {}, [], []
    for i in range(n + 1):                        # one extra frame that is NOT in the split
        img = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(obj, "rgb", f"{i:06d}.png"))
        m = np.zeros((size, size), np.uint8)
        x0, y0 = int(rng.integers(5, 100)), int(rng.integers(5, 100))
        x1, y1 = x0 + int(rng.integers(30, 120)), y0 + int(rng.integers(30, 120))
        m[y0:y1 + 1, x0:x1 + 1] = 255
        Image.fromarray(m).save(os.path.join(obj, "mask", f"{i:06d}.png"))
        R = Rotation.from_rotvec(rng.standard_normal(3)).as_matrix()
        t = np.array([rng.normal(0, 40), rng.normal(0, 40), 500 + rng.normal(0, 50)])
        joints = (rng.standard_normal((21, 3)) * 0.05).astype(np.float64)          # hand joints in metres (generators/colibri.py:430-436)
        np.save(os.path.join(obj, "hands", f"{i:06d}_coords_3d.npy"), joints)
        gt[i] = [{"cam_R_m2c": [float(v) for v in R.reshape(-1)], "cam_t_m2c": [float(v) for v in t], "obj_bb": [x0, y0, x1 - x0, y1 - y0],
                  "obj_id": 1, "drill_tip_transform": [10.0, -20.0, 30.0, 1.0]}]
        info[i] = {"cam_K": [480.0, 0.0, 128.0, 0.0, 480.0, 128.0, 0.0, 0.0, 1.0], "depth_scale": 1.0}
        if i < n:
            names.append(f"{i:06d}")
            truth.append(dict(image=img, bbox=np.array([x0, y0, x1, y1], np.float32), R=R, t=t, joints=joints))
    with open(os.path.join(obj, "gt_0.yml"), "w") as f:
        yaml.safe_dump(gt, f)
    with open(os.path.join(obj, "info_0.yml"), "w") as f:
        yaml.safe_dump(info, f)
    with open(os.path.join(obj, "test_0.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return pts, truth


def loss_cases():
    """Seeded predictions / targets for the training-side losses (hmdegopose/loss.py:54-428): name -> dict of float32
    arrays.  Shared by tests/golden/make_golden_losses.py (the real reference), the oracle test and the GPU test."""
    out = {}
    for name, B, N, K, P, npos, seed in (("typical", 3, 2000, 2, 60, 24, 1), ("empty", 2, 500, 1, 20, 0, 2),
                                         ("full", 2, 12276, 1, 500, 40, 3), ("one_positive", 1, 777, 1, 33, 1, 4)):
        rng = np.random.Generator(np.random.PCG64([seed, 0x10555]))
        state = np.zeros((B, N), np.float32)
        for b in range(B):
            state[b, rng.choice(N, size=N // 10, replace=False)] = -1.0          # ignore
            if npos:
                state[b, rng.choice(N, size=npos + b, replace=False)] = 1.0       # object (a different count per image)
        cls = rng.integers(0, K, size=(B, N))
        labels = np.zeros((B, N, K), np.float32)
        pos = state == 1
        labels[pos, cls[pos]] = 1.0
        gt_classification = np.concatenate([labels, state[..., None]], axis=2)
        gt_regression = np.concatenate([rng.standard_normal((B, N, 4)).astype(np.float32) * 0.3, state[..., None]], axis=2)
        rot_t = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
        tr_t = (rng.standard_normal((B, N, 3)) * 100).astype(np.float32)
        sym = rng.integers(0, 2, size=(B, N, 1)).astype(np.float32)
        gt_transformation = np.concatenate([rot_t, tr_t, sym, cls[..., None].astype(np.float32), state[..., None]], axis=2)
        gt_hand = np.concatenate([(rng.standard_normal((B, N, 63)) * 0.2).astype(np.float32), state[..., None]], axis=2)
        out[name] = dict(
            gt_classification=gt_classification.astype(np.float32),
            classification=(1.0 / (1.0 + np.exp(-rng.standard_normal((B, N, K)) * 3))).astype(np.float32),
            gt_regression=gt_regression.astype(np.float32),
            regression=(gt_regression[..., :4] + rng.standard_normal((B, N, 4)) * 0.15).astype(np.float32),
            gt_transformation=gt_transformation.astype(np.float32),
            transformation=np.concatenate([rot_t + rng.standard_normal((B, N, 3)).astype(np.float32) * 0.1,
                                           tr_t + rng.standard_normal((B, N, 3)).astype(np.float32) * 5], axis=2).astype(np.float32),
            gt_hand=gt_hand.astype(np.float32),
            hand=(gt_hand[..., :63] + rng.standard_normal((B, N, 63)) * 0.1).astype(np.float32),
            model_points=(rng.standard_normal((K, P, 3)) * np.array([40, 25, 60])).astype(np.float32))
    return out


def rebuilt_real_onnx_export():
    """tests/golden/onnx_eval_phi0.structure.gz (the reference model as torch.onnx.export wrote it, eval mode, opset 9, payloads blanked:
    tests/golden/make_golden_onnx.py) with its tensor payloads rebuilt from ``seeded_state_dict(0, 0)``: tensors that kept their names
    verbatim, BatchNorm-folded convolutions through the numpy restatement of the fold (2.4e-7 from the real payloads).
    Returns (file bytes, meta dict, {initialiser name: array written})."""
    import gzip
    import json
    import os
    from hmd_ego_pose_amd import seeded_state_dict
    from hmd_ego_pose_amd.arch import BN_EPS
    from hmd_ego_pose_amd.onnx_init import conv_exec_order, initializer_spans, read_nodes
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    meta = json.load(open(os.path.join(gdir, "onnx_eval_phi0.json")))
    blob = bytearray(gzip.decompress(open(os.path.join(gdir, "onnx_eval_phi0.structure.gz"), "rb").read()))
    sd = seeded_state_dict(meta["phi"], 0)
    convs = [n for n in read_nodes(bytes(blob)) if n[0] == "Conv"]
    want = {}
    for (_op, ins, _o, _n), (wk, bk, bn) in zip(convs, conv_exec_order(meta["phi"])):
        if ins[1] in sd:
            continue
        g, b, m, v = (sd[bn + k].numpy() for k in (".weight", ".bias", ".running_mean", ".running_var"))
        sc = (g / np.sqrt(v + np.float32(BN_EPS))).astype(np.float32)
        want[ins[1]] = (sd[wk].numpy() * sc[:, None, None, None]).astype(np.float32)
        want[ins[2]] = (((sd[bk].numpy() if bk else np.zeros_like(m)) - m) * sc + b).astype(np.float32)
    written = {}
    for name, lo, hi in initializer_spans(bytes(blob)):
        if name not in meta["tensors"]:
            continue
        a = sd[name].numpy() if name in sd else want[name]
        raw = np.ascontiguousarray(a, "<f4").tobytes()
        assert len(raw) == hi - lo, name
        blob[lo:hi] = raw
        written[name] = a
    return bytes(blob), meta, written
