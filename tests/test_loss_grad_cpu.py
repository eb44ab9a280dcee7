"""CPU side of the loss backward (hep_losses_backward_device, training.losses' grad_fn).

* the float64 restatement of tests/_loss_grad.py reproduces the gradients the REAL reference's autograd returned
  (tests/golden/loss_grads.npz, tests/golden/make_golden_loss_grads.py) - it is the yardstick of the GPU edge tests;
* the C ABI exports the entry point and refuses bad arguments before any HIP call (no device here).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from hmd_ego_pose_amd import _capi
from tests._loss_grad import expand_golden, restated_grads
from tests._util import loss_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_grads.npz")


def _split(g):
    """Named gradient tensors, the transformation split into rotation and translation columns (scales 1e5 apart)."""
    return {"classification": g["classification"], "regression": g["regression"], "rotation": g["transformation"][..., :3],
            "translation": g["transformation"][..., 3:], "hand": g["hand"]}


@pytest.mark.parametrize("name", list(loss_cases()))
def test_restatement_reproduces_reference_gradients(name):
    c = loss_cases()[name]
    B, N, _K = c["classification"].shape
    fx = np.load(GOLDEN)
    want = _split(expand_golden(fx, name, {"regression": (B, N, 4), "transformation": (B, N, 6), "hand": (B, N, 63)}))
    got = _split(restated_grads(c))
    for k, w in want.items():
        assert np.isfinite(w).all() and np.isfinite(got[k]).all(), (name, k)
        m = np.abs(w).max()
        err = np.abs(got[k] - w).max()
        assert err <= 1e-5 * max(m, 1e-30), (name, k, err, m)
        assert (got[k][w == 0] == 0).all(), (name, k, "non-zero where the reference is exactly zero")


def test_golden_gradient_fixture_is_small_and_complete():
    fx = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) <= 300 * 1024
    for name, c in loss_cases().items():
        assert fx[f"{name}.classification"].shape == c["classification"].shape
        for key, gt_key in (("regression", "gt_regression"), ("transformation", "gt_transformation"), ("hand", "gt_hand")):
            state = c[gt_key][..., -1].reshape(-1)
            obj = np.nonzero((np.round(state) == 1) if key == "transformation" else (state == 1))[0]
            assert np.array_equal(fx[f"{name}.{key}_rows"], obj), (name, key)


def test_backward_entry_point_refuses_bad_arguments_without_a_device():
    """hep_losses_backward_device is exported and applies the forward's argument rules (HEP_ERR_INVALID = -1,
    HEP_ERR_UNSUPPORTED = -4) before any HIP call - this machine has no GPU, a HIP call would fail with -3."""
    l = _capi.lib()
    assert hasattr(l, "hep_losses_backward_device")
    f = l.hep_losses_backward_device
    buf = ctypes.create_string_buffer(4096)                       # never dereferenced: validation comes first
    p = ctypes.addressof(buf)
    ws = p

    def call(gh=p, hand=p, B=2, N=10, K=1, R=3, H=63, C=1, P=50, u=p, g_hand=p, ws=ws):
        return f(p, p, p, p, p, p, gh, hand, p, B, N, K, R, H, C, P, u, p, p, p, g_hand, ws, None)

    cases = {
        "gt_hand without hand": (call(hand=None, g_hand=None), -1),
        "hand without gt_hand": (call(gh=None), -1),
        "grad_hand without hand": (call(gh=None, hand=None), -1),
        "num_rotation 4": (call(R=4), -1),
        "num_rotation 6": (call(R=6), -1),
        "batch 0": (call(B=0), -1),
        "no anchors": (call(N=0), -1),
        "no workspace": (call(ws=None), -1),
        "no upstream gradient": (call(u=None), -1),
        "2049 points": (call(P=2049), -4),
        "0 points": (call(P=0), -4),
    }
    for what, (rc, want) in cases.items():
        assert rc == want, (what, rc, l.hep_last_error())
        assert l.hep_last_error(), what
    # the forward refuses the same sizes with the same codes
    assert l.hep_losses_device(p, p, p, p, p, p, p, p, p, 2, 10, 1, 3, 63, 1, 2049, p, p, None) == -4


def test_python_layer_refuses_host_predictions():
    from hmd_ego_pose_amd.training import batch_iterate, losses
    c = loss_cases()["one_positive"]
    t = {k: torch.from_numpy(v) for k, v in c.items() if k != "model_points"}
    args = (t["gt_classification"], t["classification"].requires_grad_(True), t["gt_regression"], t["regression"], t["gt_transformation"],
            t["transformation"], t["gt_hand"], t["hand"], c["model_points"], 3)
    with pytest.raises(ValueError, match="ROCm tensor"):
        losses(*args)
    with pytest.raises(ValueError, match="ROCm tensor"):
        batch_iterate(*args)
