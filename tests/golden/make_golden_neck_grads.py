#!/usr/bin/env python3
"""Golden values and GRADIENTS of the BiFPN neck from the REAL reference.

Runs only in the build container (needs /root/reference, read-only).  The reference ``HMDEgoPose({'iter': 0}, ...)`` is
imported unchanged (stubs of make_golden.py), loaded with ``seeded_state_dict`` and put in ``eval()`` (running-statistics
BatchNorm, the semantics of ``hmd_ego_pose_amd.neck``); its ``bifpn`` sub-module is called on seeded taps that require grad,
each of the five maps is contracted with a seeded cotangent (``tests/_neck_grad.py::seeded_inputs``, input seed 0: the one
generator whose cases were checked to hold REF_F32_TOL), and the sum is backpropagated.  Stored per case
(``tests/_neck_grad.py::GOLDEN_CASES``) for the five maps, the three tap gradients and every trainable ``bifpn.*`` tensor, in
the order of ``golden_names``: ``<case>/shapes``, ``/sums`` (float64 sum and abs-sum), ``/slices`` (a prime-strided slice of
every tensor, float32, concatenated) and ``/offsets`` - digests, not the dense tensors.  Only data goes into the archive; it
is written with fixed member timestamps, so a rerun is byte-identical.

    python tests/golden/make_golden_neck_grads.py       # writes tests/golden/neck_grads.npz
"""
import io
import os
import sys
import types
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
    torch.set_num_threads(1)                                         # one summation order for the CPU reductions
    _stub("torchvision"); _stub("torchvision.ops"); _stub("torchvision.ops.boxes", nms=None)
    tf = _stub("tensorflow"); tf.keras = _stub("tensorflow.keras")
    _stub("generators.utils.compute_overlap", compute_overlap=None, wrapper_c_min_distances=None)
    sys.path.insert(0, REF)
    from backbone import HMDEgoPose                                  # noqa: E402
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from tests import _neck_grad as N
    out = {}
    for tag, (phi, size, batch, seed) in N.GOLDEN_CASES.items():
        model = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=phi, onnx_export=True, input_sizes=[size] * 9)
        model.load_state_dict(seeded_state_dict(phi, seed), strict=True)
        model.eval()
        taps_np, cots_np = N.seeded_inputs(phi, size, batch)
        taps = tuple(torch.from_numpy(a).requires_grad_(True) for a in taps_np)
        maps = model.bifpn(taps)
        sum((m * torch.from_numpy(c)).sum() for m, c in zip(maps, cots_np)).backward()
        named = dict(model.named_parameters())
        tensors = {f"map.{l}": m.detach() for l, m in enumerate(maps)}
        tensors.update({f"tap.{t}": a.grad for t, a in enumerate(taps)})
        for k, _ in N.neck_keys(phi):
            if N.trainable(k):
                assert named[k].grad is not None, k
                tensors["param." + k] = named[k].grad
        names = N.golden_names(phi)
        assert sorted(names) == sorted(tensors), "golden_names drifted from what the reference returns"
        for part, v in N.pack_digests({k: t.numpy() for k, t in tensors.items()}, names).items():
            out[f"{tag}/{part}"] = v
        print(tag, len(tensors), "tensors; max |grad| of the taps", [float(a.grad.abs().max()) for a in taps])
    _write_npz(os.path.join(HERE, "neck_grads.npz"), out)
    print("wrote", os.path.getsize(os.path.join(HERE, "neck_grads.npz")), "bytes")


if __name__ == "__main__":
    main()
