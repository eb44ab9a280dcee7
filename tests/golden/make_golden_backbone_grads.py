#!/usr/bin/env python3
"""Golden values and GRADIENTS of the EfficientNet trunk from the REAL reference.

Runs only in the build container (needs /root/reference, read-only).  The reference ``HMDEgoPose({'iter': 0}, ...)`` is
imported unchanged (stubs of make_golden.py) and loaded with ``seeded_state_dict``; its ``backbone_net`` sub-module is called
on a seeded image that requires grad, each of the three taps P3 / P4 / P5 is contracted with a seeded cotangent
(``tests/_backbone_grad.py::seeded_inputs``, input seed 0) and the sum is backpropagated.

Deterministic cases (``GOLDEN_CASES``): ``eval()`` - running-statistics BatchNorm and no drop-connect, the semantics of
``hmd_ego_pose_amd.backbone``.  The drop-connect case (``DROP_TAG``): ``model.train()`` with every BatchNorm put back in
``eval()`` and ``torch.manual_seed(DROP_TORCH_SEED)`` right before the forward; the scale table is re-created by re-seeding and
drawing in block order (``reference_scales``), stored as data (``<case>/scales``, float32 [blocks, B]), and the script asserts
that the oracle's restated block loop with those scales reproduces the reference's taps within REF_F32_TOL = 1e-5.

Stored per case for the three taps, the image gradient and every trainable ``backbone_net.*`` tensor, in the order of
``golden_names``: ``<case>/shapes``, ``/sums`` (float64 sum and abs-sum), ``/slices`` (a prime-strided slice of every tensor,
float32, concatenated) and ``/offsets`` - digests, not the dense tensors.  Only data goes into the archive; it is written with
fixed member timestamps, so a rerun is byte-identical.

    python tests/golden/make_golden_backbone_grads.py       # writes tests/golden/backbone_grads.npz
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
    from tests import _backbone_grad as G
    out = {}
    cases = [(tag, case, False) for tag, case in G.GOLDEN_CASES.items()] + [(G.DROP_TAG, G.DROP_CASE, True)]
    for tag, (phi, size, batch, seed), drop in cases:
        model = HMDEgoPose({"iter": 0}, num_classes=1, compound_coef=phi, onnx_export=True, input_sizes=[size] * 9)
        sd = seeded_state_dict(phi, seed)
        model.load_state_dict(sd, strict=True)
        model.eval()
        if drop:
            model.train()
            model.freeze_bn()                                        # every BatchNorm back in eval(): running statistics
            assert model.backbone_net.model._global_params.drop_connect_rate == G.DROP_RATE
            torch.manual_seed(G.DROP_TORCH_SEED)
        image_np, cots_np = G.seeded_inputs(phi, size, batch)
        image = torch.from_numpy(image_np).requires_grad_(True)
        taps = model.backbone_net(image)[-3:]
        sum((m * torch.from_numpy(c)).sum() for m, c in zip(taps, cots_np)).backward()
        named = dict(model.named_parameters())
        tensors = {f"tap.{t}": m.detach() for t, m in enumerate(taps)}
        tensors["image"] = image.grad
        for k, _ in G.backbone_keys(phi):
            if G.trainable(k):
                assert named[k].grad is not None, k                  # the reference leaves no backbone parameter without a gradient
                tensors["param." + k] = named[k].grad
        names = G.golden_names(phi)
        assert sorted(names) == sorted(tensors), "golden_names drifted from what the reference returns"
        if drop:
            scales = G.reference_scales(phi, G.DROP_RATE, batch, G.DROP_TORCH_SEED)
            assert (scales == 0).any() and (scales > 1).any(), "the seed must drop a branch and keep one"
            with torch.no_grad():
                mine = G.oracle_backbone({k: v.double() for k, v in sd.items() if v.dtype == torch.float32}, torch.from_numpy(image_np).double(), phi, scales.double())
            for t, (a, b) in enumerate(zip(mine, taps)):
                err = float((a - b.detach().double()).abs().max() / b.detach().abs().max())
                assert err <= 1e-5, (t, err)
                print(tag, f"tap {t}: oracle with the re-created scales against the reference, {err:.2e}")
            out[f"{tag}/scales"] = scales.numpy().astype(np.float32)
        for part, v in G.pack_digests({k: t.numpy() for k, t in tensors.items()}, names).items():
            out[f"{tag}/{part}"] = v
        print(tag, len(tensors), "tensors; max |grad| of the image", float(image.grad.abs().max()),
              "; smallest max |g| over the parameters", min(float(named[k].grad.abs().max()) for k, _ in G.backbone_keys(phi) if G.trainable(k)))
    _write_npz(os.path.join(HERE, "backbone_grads.npz"), out)
    print("wrote", os.path.getsize(os.path.join(HERE, "backbone_grads.npz")), "bytes")


if __name__ == "__main__":
    main()
