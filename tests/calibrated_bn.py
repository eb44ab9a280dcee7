#!/usr/bin/env python3
"""BatchNorm running statistics CALIBRATED on seeded frames - used by tests/precision_calibrated.py.

The plain seeded recipe (hmd_ego_pose_amd.weights.seeded_state_dict) draws running_mean / running_var at random, so a BatchNorm
output is whatever the random statistics make of it and the network amplifies a rounding error ~1000 x on its way to the heads
(DESIGN.md section 3).  A trained network's statistics are those of its own activations: every BatchNorm output is ~N(beta, gamma^2).
This script makes such a recipe without training: one pass of the CPU oracle (oracle/efficientpose_ref.py) over calibration
frames in which every BatchNorm measures the per-channel mean / variance of ITS input - behind the already calibrated layers in front
of it - and normalises with them (what `model.train()` + momentum 1 would record).  Only the statistics are stored (~20k channels);
`hmd_ego_pose_amd.weights.calibrated_state_dict` overlays them on the seeded weights.  TEST INFRASTRUCTURE (it runs the oracle).

    python tests/golden/make_calibrated_bn.py            # phi 0, seed 0
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def calibrate(phi, seed, size, frames):
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from tests import _hard_values
    # (the measuring pass itself lives in tests/_hard_values.py, which calibrates any state dict)
    return {k: v.numpy().copy() for k, v in _hard_values.calibrate(seeded_state_dict(phi, seed), phi, size, frames, seed).items()}


def calibrated_state_dict(phi, seed=0, size=256, frames=8):
    import torch
    from hmd_ego_pose_amd.weights import seeded_state_dict
    sd = seeded_state_dict(phi, seed)
    for k, v in calibrate(phi, seed, size, frames).items():
        sd[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return sd
