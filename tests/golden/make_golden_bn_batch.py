#!/usr/bin/env python3
"""Golden values of BATCH-STATISTICS BatchNorm training from the REAL reference: outputs, input gradients, gradients of every
trainable tensor and the running statistics after one forward, for the heads, the BiFPN and the backbone.

Runs only in the build container (needs /root/reference, read-only).  The reference ``HMDEgoPose({'iter': 0}, ...)`` is imported
unchanged (stubs of make_golden.py), loaded with ``seeded_state_dict``, cast to float64 and put in ``eval()``; then the part under
test goes to training mode: the five head sub-modules and ``bifpn`` through ``.train()``, the backbone through ``.train()`` of
each of its ``nn.BatchNorm2d`` only, so that drop-connect stays off (rate 0) while every BatchNorm normalises with the statistics
of the batch (momentum 0.01, eps 1e-3) and moves its running statistics.  The part is called on the seeded inputs of
tests/_head_grad.py / _neck_grad.py / _backbone_grad.py, each output is contracted with its seeded cotangent and the sum is
backpropagated.  Stored per case (``tests/_bn_batch.py::GOLDEN``, tag ``<part>.<case>``) in the order of
``_bn_batch.golden_names`` with the digest convention of tests/_head_grad.py::pack_digests: ``/shapes``, ``/sums``, ``/slices``,
``/offsets``.  Only data goes into the archive; it is written with fixed member timestamps, so a rerun is byte-identical.

    python tests/golden/make_golden_bn_batch.py       # writes tests/golden/bn_batch_grads.npz
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
    from torch import nn
    torch.set_num_threads(1)                                         # one summation order for the CPU reductions
    _stub("torchvision"); _stub("torchvision.ops"); _stub("torchvision.ops.boxes", nms=None)
    tf = _stub("tensorflow"); tf.keras = _stub("tensorflow.keras")
    _stub("generators.utils.compute_overlap", compute_overlap=None, wrapper_c_min_distances=None)
    sys.path.insert(0, REF)
    from backbone import HMDEgoPose                                  # noqa: E402
    from hmd_ego_pose_amd.weights import seeded_state_dict
    from tests import _bn_batch as BB
    from tests._head_grad import pack_digests
    out = {}
    for part in BB.PARTS:
        tag = BB.GOLDEN[part]
        case = BB.CASES[part][tag]
        phi, size, batch, seed, classes, drop = case
        assert drop is None
        model = HMDEgoPose({"iter": 0}, num_classes=classes or 1, compound_coef=phi, onnx_export=True, input_sizes=[size] * 9)
        model.load_state_dict(seeded_state_dict(phi, seed, num_classes=classes or 1), strict=True)
        model = model.double().eval()
        x_np, cots_np = BB.inputs(part, case)
        x = [torch.from_numpy(a).double().requires_grad_(True) for a in x_np]
        if part == "heads":
            subs = (model.regressor, model.classifier, model.rotation_net, model.translation_net, model.hand_net)
            for s in subs:
                s.train()
            outs = [s(tuple(x)) for s in subs]
        elif part == "neck":
            model.bifpn.train()
            outs = list(model.bifpn(tuple(x)))
        else:
            norms = [m for m in model.backbone_net.modules() if isinstance(m, nn.BatchNorm2d)]
            for m in norms:
                m.train()
            # efficientnet/model.py: momentum = 1 - batch_norm_momentum (0.99) = 0.01 up to one double rounding
            assert norms and all(abs(m.momentum - BB.MOMENTUM) < 1e-12 and m.eps == BB.EPS for m in norms)
            outs = list(model.backbone_net(x[0])[-3:])
        sum((o * torch.from_numpy(c).double()).sum() for o, c in zip(outs, cots_np)).backward()
        named, state = dict(model.named_parameters()), model.state_dict()
        res = dict(outs=[o.detach() for o in outs], gin=[a.grad for a in x], grads={}, stats={})
        for k, _ in BB.keys(part, case):
            if BB.trainable(k):
                assert named[k].grad is not None, k
                res["grads"][k] = named[k].grad
            else:
                res["stats"][k] = state[k]
        tracked = [v for k, v in state.items() if k.endswith("num_batches_tracked") and k.rsplit(".", 1)[0] + ".running_mean" in res["stats"]]
        assert tracked and all(int(v) == 1 for v in tracked), "every BatchNorm of the part saw exactly one training forward"
        names = BB.golden_names(part, case)
        tensors = BB.golden_tensors(part, case, res)
        assert sorted(names) == sorted(tensors), "golden_names drifted from what the reference returns"
        for piece, v in pack_digests(tensors, names).items():
            out[f"{part}.{tag}/{piece}"] = v
        print(part, tag, len(tensors), "tensors; max |grad| of the inputs", [float(a.grad.abs().max()) for a in x])
    path = os.path.join(HERE, "bn_batch_grads.npz")
    _write_npz(path, out)
    print("wrote", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
