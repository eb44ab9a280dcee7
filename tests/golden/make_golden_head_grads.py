#!/usr/bin/env python3
"""Golden GRADIENTS of the five head nets from the REAL reference.

Runs only in the build container (needs /root/reference, read-only).  The reference ``HMDEgoPose({'iter': 0}, ...)`` is
imported unchanged (stubs of make_golden.py), loaded with ``seeded_state_dict`` and put in ``eval()`` (running-statistics
BatchNorm, the semantics of ``hmd_ego_pose_amd.heads``); its five head sub-modules are called on seeded maps that require
grad, each output is contracted with a seeded cotangent, and the sum is backpropagated.  Stored per case
(``tests/_head_grad.py::GOLDEN_CASES``) for every trainable head tensor, every map gradient and every head output, in the
order of ``golden_names``: ``<case>/shapes``, ``/sums`` (float64 sum and abs-sum), ``/slices`` (a prime-strided slice of
every tensor, float32, concatenated) and ``/offsets`` - digests, not the dense tensors.  Only data goes into the archive; it
is written with fixed member timestamps, so a rerun is byte-identical.

    python tests/golden/make_golden_head_grads.py       # writes tests/golden/head_grads.npz
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
    from tests import _head_grad as H
    out = {}
    for tag, (phi, classes, size, batch, seed) in H.GOLDEN_CASES.items():
        model = HMDEgoPose({"iter": 0}, num_classes=classes, compound_coef=phi, onnx_export=True, input_sizes=[size] * 9)
        model.load_state_dict(seeded_state_dict(phi, seed, num_classes=classes), strict=True)
        model.eval()
        feats = tuple(torch.from_numpy(a).requires_grad_(True) for a in H.seeded_maps(phi, size, batch, seed + 1))
        cots = [torch.from_numpy(a) for a in H.seeded_cotangents(classes, size, batch, seed + 2)]
        outs = (model.regressor(feats), model.classifier(feats), model.rotation_net(feats), model.translation_net(feats), model.hand_net(feats))
        sum((o * c).sum() for o, c in zip(outs, cots)).backward()
        named = dict(model.named_parameters())
        tensors = {f"out.{n}": o.detach() for n, o in zip(H.OUT_NAMES, outs)}
        tensors.update({f"feat.{l}": f.grad for l, f in enumerate(feats)})
        for k, _ in H.head_keys(phi, classes):
            if H.trainable(k):
                assert named[k].grad is not None, k
                tensors["param." + k] = named[k].grad
        names = H.golden_names(phi, classes)
        assert sorted(names) == sorted(tensors), "golden_names drifted from what the reference returns"
        for part, v in H.pack_digests({k: t.numpy() for k, t in tensors.items()}, names).items():
            out[f"{tag}/{part}"] = v
        print(tag, len(tensors), "tensors; max |grad| of the maps", [float(f.grad.abs().max()) for f in feats])
    _write_npz(os.path.join(HERE, "head_grads.npz"), out)
    print("wrote", os.path.getsize(os.path.join(HERE, "head_grads.npz")), "bytes")


if __name__ == "__main__":
    main()
