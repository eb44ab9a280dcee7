#!/usr/bin/env python3
"""Golden GRADIENTS of the training-side losses from the REAL reference.

Runs only in the build container (needs /root/reference, read-only).  ``hmdegopose/loss.py`` is imported unchanged with the
stubs of make_golden_losses.py, ``batch_iterate`` is run on the seeded cases of ``tests/_util.py::loss_cases`` with the
predictions requiring grad, and the weighting of train.py:61-65 (cls + reg + 100 rot + 0.1 tr + hand) is backpropagated.
The five terms touch disjoint inputs, so this one backward pins all five gradients.  Stored per case (float32):
``<case>.classification`` dense [B, N, K]; ``<case>.regression`` / ``.transformation`` / ``.hand`` only on the object-anchor
rows of each tensor's own state column, with their flat row indices b * N + n in ``<case>.<name>_rows`` (every other row is
exactly zero in the reference).  The archive is written like np.savez_compressed but with fixed member timestamps, so a
rerun is byte-identical.

    python tests/golden/make_golden_loss_grads.py       # writes tests/golden/loss_grads.npz
"""
import io
import os
import sys
import types
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/pytorch-sandbox"
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    import torch
    warnings.filterwarnings("ignore", category=UserWarning)        # the reference's deprecated list indexing
    torch.set_num_threads(1)                                         # one summation order for the CPU reductions
    _stub("torchvision"); _stub("torchvision.ops"); _stub("torchvision.ops.boxes", nms=None)
    tf = _stub("tensorflow"); tf.keras = _stub("tensorflow.keras")
    _stub("generators.utils.compute_overlap", compute_overlap=None, wrapper_c_min_distances=None)
    sys.path.insert(0, REF)
    from hmdegopose.loss import batch_iterate                        # noqa: E402
    from tests._util import loss_cases
    out = {}
    for name, c in loss_cases().items():
        t = {k: torch.from_numpy(v) for k, v in c.items() if k != "model_points"}
        preds = {k: t[k].clone().requires_grad_(True) for k in ("classification", "regression", "transformation", "hand")}
        cls, reg, rot, tr, hand = batch_iterate(t["gt_classification"], preds["classification"], t["gt_regression"], preds["regression"],
                                                t["gt_transformation"], preds["transformation"], t["gt_hand"], preds["hand"], c["model_points"], 3)
        loss = cls.mean() + reg.mean() + 100 * rot.mean() + 0.1 * tr.mean() + hand.mean()     # train.py:55-65
        loss.backward()
        B, N = c["classification"].shape[:2]
        out[f"{name}.classification"] = preds["classification"].grad.numpy().astype(np.float32)
        for key, gt_key in (("regression", "gt_regression"), ("transformation", "gt_transformation"), ("hand", "gt_hand")):
            state = c[gt_key][..., -1].reshape(-1)
            obj = (np.round(state) == 1) if key == "transformation" else (state == 1)
            g = preds[key].grad.numpy().reshape(B * N, -1)
            assert not g[~obj].any(), (name, key, "non-zero gradient on a non-object row")
            rows = np.nonzero(obj)[0].astype(np.int32)
            out[f"{name}.{key}"] = g[rows].astype(np.float32)
            out[f"{name}.{key}_rows"] = rows
        print(name, {k.split(".", 1)[1]: float(np.abs(v).max()) if v.size else 0.0 for k, v in out.items() if k.startswith(name + ".")
                     and not k.endswith("_rows")})
    _write_npz(os.path.join(HERE, "loss_grads.npz"), out)


if __name__ == "__main__":
    main()
