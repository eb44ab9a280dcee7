"""GPU (MI355X): every inference kernel against the CPU oracle on saturating, trained-like values (tests/_hard_values.py).

The seeded weights of the other parity suites keep activations O(1), so none of them reaches exp overflow in an epilogue
(hep_dev.h rcp_newton / rcp2_t clamp the denominator for that case; the bf16 FAST forms rely on rcp(inf) == 0), a dead or
negated BatchNorm channel, a fusion node with no live weight, a saturated squeeze-excite gate or a score of exactly 0 or 1.
Here the sessions of tests/_hard_values.py SESSIONS run the recipe's weights at the benchmarked batch sizes (the launch plan
depends on the batch; tests/test_hard_values_cpu.py holds the table to the planner) and every stage is compared, on the device's
own stage input, with the oracle on the images tests/test_gpu_parity.py _images_to_check picks.  Image 0 is a constant frame.

fp32: the float64 oracle; max |hip - f64| / max(1, max |f64|) within FP32_STAGE_TOL (heads FP32_HEAD_TOL) and the same per
output channel within 4 x the float32 CPU oracle's own per-channel error on that input (floor 2e-6).  An underflowing tail that
comes out as a tiny normal (the clamp turns ~1e-40 into ~1e-36) is below both metrics: they are absolute under magnitude 1.
bf16: the bf16-emulating oracle at the strict gates of the BASELINE configurations."""
import numpy as np
import pytest
import torch

from tests import _hard_values as HV
from tests._util import CAMS
from tests.test_gpu_parity import (BF16_TOL_MAX, BF16_TOL_MEAN, FP32_HEAD_TOL, FP32_STAGE_TOL, HEADS, _teacher_forced_bf16,
                                   _teacher_forced_fp32, api)  # noqa: F401  (api: the module fixture of the parity suite)

pytestmark = pytest.mark.gpu

FP32_SESSIONS = [c for c in HV.SESSIONS if c[3] == "fp32"]
BF16_SESSIONS = [c for c in HV.SESSIONS if c[3] == "bf16"]
_id = lambda c: f"phi{c[0]}-{c[1]}-b{c[2]}-{c[3]}-k{c[4]}"


@pytest.mark.parametrize("phi,size,batch,dtype,classes", FP32_SESSIONS, ids=[_id(c) for c in FP32_SESSIONS])
def test_fp32_stages_match_the_float64_oracle_on_hard_values(api, phi, size, batch, dtype, classes):
    """Every stage of the whole batch finite; tensor_err against the float64 oracle within FP32_STAGE_TOL / FP32_HEAD_TOL (asserted
    by _teacher_forced_fp32, which is given the float64 weights as the oracle's); channel_err within channel_bound.  Three classes at
    batch 2 reach the classifier header's other width."""
    R = api["R"]
    sd, x = HV.hard_state_dict(phi, 0, classes), HV.hard_input(size, batch)
    ident = lambda t: t
    st32 = R.emulated_stages(sd, phi, q_act=ident, q_w=ident)
    over = []

    def on_stage(kind, index, inputs, got, want64):
        want32 = HV.stage_outputs(st32, kind, index, inputs)
        dim = -1 if kind == "heads" else 1
        for k, w64 in want64.items():
            assert w64.dtype == torch.float64 and want32[k].dtype == torch.float32
            te, ce, cb = HV.tensor_err(got[k], w64), HV.channel_err(got[k], w64, dim), HV.channel_bound(want32[k], w64, dim)
            print(f"phi {phi} @ {size} b{batch} fp32 k{classes} {k}: images {got[k].shape[0]}, tensor_err {te:.2e}, channel_err {ce:.2e}, channel_bound {cb:.2e}")
            if ce > cb:
                over.append((k, ce, cb))

    body, head = _teacher_forced_fp32(api, sd, phi, size, batch, x, images="plan", on_stage=on_stage, oracle_sd=HV.as_double(sd))
    assert body <= FP32_STAGE_TOL and head <= FP32_HEAD_TOL
    assert not over, f"channel_err above channel_bound (stage, err, bound): {over}"


@pytest.mark.parametrize("phi,size,batch,dtype,classes", BF16_SESSIONS, ids=[_id(c) for c in BF16_SESSIONS])
def test_bf16_stages_match_the_emulating_oracle_on_hard_values(api, phi, size, batch, dtype, classes):
    """The benchmarked bf16 sessions at the strict gates of test_bf16_matches_bf16_emulating_oracle, unchanged: BF16_TOL_MAX /
    BF16_TOL_MEAN per stage, 2.5 x on the heads' max; every device value of the whole batch finite."""
    sd, x = HV.hard_state_dict(phi, 0, classes), HV.hard_input(size, batch)
    assert (BF16_TOL_MAX, BF16_TOL_MEAN) == (1e-2, 2e-3)
    _teacher_forced_bf16(api, sd, phi, size, batch, x, None, strict=True, images="plan")


def _filter_equals_oracle(D, s, out, batch, cases, images):
    _, reg, cls, rot, trn, hand = out
    cam = torch.from_numpy(np.repeat(CAMS[:1], batch, 0)).cuda()
    boxes, trans = s.decode(reg, trn, cam)
    host = [t.cpu().numpy() for t in (boxes, cls, rot, trans, hand)]
    for thr, nms, M, specific in cases:
        det = s.filter(boxes, cls, rot, trans, hand, score_threshold=thr, nms_threshold=nms, max_detections=M, class_specific_filter=specific)
        torch.cuda.synchronize()
        for i in images:
            o = D.filter_detections(*[a[i] for a in host], score_threshold=thr, max_detections=M, nms_threshold=nms, class_specific_filter=specific)
            ctx = (thr, nms, M, specific, i)
            assert np.array_equal(det["index"][i].cpu().numpy(), o[6]), ctx
            assert np.array_equal(det["scores"][i].cpu().numpy(), o[1]), ctx
            assert np.array_equal(det["labels"][i].cpu().numpy(), o[2]), ctx
            assert int(det["count"][i]) == int((o[6] >= 0).sum()), ctx
    return host[1]


def test_filter_on_the_devices_own_saturated_scores(api):
    """Session.filter on what the fp32 batch-16 session itself produced - thousands of scores of exactly 1.0f (all tied: the order is
    the anchor index) and thousands from logits beyond exp overflow - equals oracle.decode_ref.filter_detections on the same arrays bit for bit: index, score,
    label, count.  Once more on the three-class session with the best-class filter."""
    D = api["D"]
    for (phi, size, batch, _dtype, classes), cases in ((HV.SESSIONS[0], [(0.05, 0.5, 100, True), (0.5, 0.0, 256, True)]),
                                                       (HV.SESSIONS[3], [(0.05, 0.5, 100, False)])):
        sd, x = HV.hard_state_dict(phi, 0, classes), HV.hard_input(size, batch)
        s = api["Session"](sd, phi, size, batch, "fp32")
        out = s.forward(x.cuda())
        scores = _filter_equals_oracle(D, s, out, batch, cases, range(batch))
        s.close()
        # (where the oracle's sigmoid underflows to exactly 0.0f the device's clamped denominator gives 2^-126, a tiny normal: the
        #  low extreme is counted as "exp overflowed", at or below 1e-37, and the exact zeros are reported)
        ones, lows, zeros = int((scores == 1.0).sum()), int((scores <= 1e-37).sum()), int((scores == 0.0).sum())
        print(f"phi {phi} @ {size} b{batch} k{classes}: of {scores.size} device scores {ones} are 1.0f, {lows} are <= 1e-37, {zeros} are 0.0f")
        assert ones >= 1000 and lows >= 1000


def test_nan_input_reaches_every_bf16_head_as_nan(api):
    """test_nan_input_reaches_every_fp32_head_as_nan (which runs both dtypes at 256 x 256, batch 2) at the plan of a single
    128 x 128 frame in bf16: the FAST activations (v_rcp_f32 of 1 + exp, no Newton step, no clamp) must carry a NaN through every
    stage into all five heads, most classification scores of the frame are NaN, and the clean frame run through the same session
    afterwards is finite and bit-identical to its run before."""
    phi, size = 0, 128
    sd = api["sd"](phi, 3)
    from tests._util import seeded_input
    clean = torch.from_numpy(seeded_input((1, 3, size, size), 5))
    bad = clean.clone()
    bad[0, :, 50:70, 30:100] = float("nan")
    s = api["Session"](sd, phi, size, 1, "bf16")
    before = [t.cpu() for t in s.forward(clean.cuda())[1:]]
    out = [t.cpu() for t in s.forward(bad.cuda())[1:]]
    after = [t.cpu() for t in s.forward(clean.cuda())[1:]]
    s.close()
    for name, t, b, a in zip(HEADS, out, before, after):
        assert torch.isnan(t[0]).any(), (name, "the poisoned frame came out finite")
        assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0]), name
    assert torch.isnan(out[1][0]).float().mean().item() > 0.5, "classification scores of the poisoned frame"


# ---- training: the three trainable parts on hard values, at the smallest shapes ----------------------------------------------------
# Reference, routing of the neck's max-pools and the bound rule are those of tests/test_gpu_bn_batch.py (4 x the float32 CPU oracle's
# own error, floor 2e-6; tests/_bn_batch.py), here with the hard weights handed to the same helpers and the rule applied PER TENSOR:
# on these values single tensors nearly cancel (float32 itself is 0.4 off on one of them) and a group bound would take its size from them.
TRAIN_MODES = {"running": 2, "batch": 8}           # mode -> batch at phi 0, 128 x 128 (batch statistics need 8 rows at every BatchNorm)
# (part, mode, input variant).  Heads in batch mode run twice, see the test's docstring.
TRAIN_CASES = [(part, "running", None) for part in ("heads", "neck", "backbone")] + \
              [("heads", "batch", "constant_top"), ("heads", "batch", "offset_top"), ("neck", "batch", None), ("backbone", "batch", None)]


F32_THREADS = 8                                    # the second summation order of the float32 CPU oracle (the first is one thread)


def _with_threads(n, fn, *args):
    threads = torch.get_num_threads()
    torch.set_num_threads(n)
    try:
        return fn(*args)
    finally:
        torch.set_num_threads(threads)


def _train_weights(mode):
    """running: the calibrated recipe.  batch: the hard edits alone - batch statistics renormalise by themselves."""
    from tests._util import seeded_state_dict_once
    return HV.hard_state_dict(0, 0, 1) if mode == "running" else HV.hard_edits(seeded_state_dict_once(0, 0), 0)


@pytest.mark.parametrize("part,mode,variant", TRAIN_CASES, ids=["-".join(filter(None, c)) for c in TRAIN_CASES])
def test_training_parts_match_float64_autograd_on_hard_values(part, mode, variant, monkeypatch):
    """Forward outputs, every parameter and input gradient and (batch mode) the updated running statistics of TrainableHeads /
    TrainableNeck / TrainableBackbone against float64 autograd of the oracle: the backward of swish in both tails, gamma == 0 and
    negated, relu-dead and all-zero fusion nodes, and in batch mode BatchNorm channels that are constant (var == 0, rstd =
    1 / sqrt(eps)) or whose mean is more than 50 x their spread - asserted on the float64 side first.  The analytically zero tensors
    (behind a relu-dead fusion entry, behind gamma == 0, a bias in front of a batch-statistics BatchNorm) are derived from the
    float64 gradient with ZERO_REL; the device is held there to 4 x the float32 CPU oracle's largest value, or to ZERO_REL x the
    scale that defines the set where that is larger (then the device's tensor is itself zero by the rule that made the set).
    Heads in batch mode: no BatchNorm of the heads follows a depthwise conv, so none of them sees a constant channel from the
    weights alone, and the mean of a pointwise conv's output over unit-normal maps is of the size of its spread.  Their inputs are
    the test's to choose, so the two classes come from the top-level map (1 x 1, one row per image: the only level without a
    padded border), in two runs: "constant_top" makes it the same for every image, so every channel of that level's BatchNorms is
    constant; "offset_top" scales that common map by 100 and adds the seeded unit-normal one, a mean of 100 x the spread."""
    from tests import _bn_batch as BB
    from tests import _head_grad as H
    from tests import _neck_grad as N
    from tests.test_gpu_bn_batch import _buffers, _module, _run
    case = (0, 128, TRAIN_MODES[mode], 0, 1, None)
    tag = " ".join(filter(None, (part, mode, variant)))
    if variant is not None:
        plain = H.seeded_maps

        def maps_with_a_hard_top_level(*args):
            maps = plain(*args)
            maps[-1][:] = maps[-1][:1] if variant == "constant_top" else 100.0 * maps[-1][:1] + maps[-1]
            return maps
        monkeypatch.setattr(H, "seeded_maps", maps_with_a_hard_top_level)
    sd = _train_weights(mode)
    seen = {}

    def observe(p, x):
        v, mean = x.var(dim=(0, 2, 3), unbiased=False), x.mean(dim=(0, 2, 3))
        live = v >= 1e-12
        seen[p] = (float(v.min()), float((mean.abs() / v.sqrt())[live].max()) if live.any() else 0.0)

    # first, on the float64 side and before the device is touched: the value classes are there (the oracle routing its own max-pools)
    r64 = BB.oracle(part, sd, case, torch.float64, None, mode, observe)
    if mode == "batch":
        dead, far = sum(v[0] < 1e-12 for v in seen.values()), sum(v[1] > 50 for v in seen.values())
        print(f"{tag}: of {len(seen)} BatchNorms {dead} see a channel with batch variance < 1e-12, {far} one with |mean| > 50 sqrt(var)")
        assert (dead >= 1 or variant == "offset_top") and (far >= 1 or variant == "constant_top")
    m = _module(part, case, batch_norm="batch" if mode == "batch" else None, sd=sd)
    m = m.train() if mode == "batch" else m.eval()
    before = _buffers(m)
    dev = _run(part, m, case)
    after = _buffers(m)
    if part == "neck":                                           # ... now with the device's pool routing
        r64 = BB.oracle(part, sd, case, torch.float64, dev["argmax"], mode)
    # The float32 oracle's own error is a noisy statistic on these values (cancellation behind the 1e3 : 1e-3 fusion vector and the
    # dead channels): two correct float32 evaluations that differ only in summation order lie up to 5 x apart (measured on the CPU:
    # the neck's fusion scalars, 1.9e-5 with one thread against 9.0e-5 with eight).  So it is evaluated in both orders, with one
    # thread and with F32_THREADS, and a tensor's float32 error is the larger of the two.
    r32s = [_with_threads(n, BB.oracle, part, sd, case, torch.float32, dev["argmax"], mode) for n in (1, F32_THREADS)]
    for r in (r64, dev, *r32s):
        assert all(torch.isfinite(t).all() for t in list(r["outs"]) + list(r["grads"].values()) + list(r["gin"])), "non-finite value"
    assert set(dev["grads"]) == set(r64["grads"])
    zeros = BB.zero_set(r64["grads"])
    top = max(float(v.abs().max()) for k, v in r64["grads"].items() if BB.is_bn_bias(k))
    larger = lambda dicts: {k: max(d[k] for d in dicts) for k in dicts[0]}
    # PER TENSOR: each output, input gradient and trainable tensor against 4 x its float32 error, floor 2e-6.  A tensor's float32
    # error is the larger of its own and the median over the part's tensors of that kind: its own is ONE draw of a noisy statistic
    # (measured on the CPU, running-statistics backbone: the four squeeze-excite tensors of block 1 are 8.9e-5 off float64 with one
    # thread and 2.9e-6 with two or more, a factor of 31 between two correct evaluations, while every other tensor of that block and
    # the part's median sit at 1e-4: the tensors of a part share their upstream gradients and with them an error level).  That is
    # never wider than the rule of the seeded cases, which gives every tensor the group's LARGEST float32 error; a tensor that
    # nearly cancels (float32 0.4 off on one of the neck's) widens only its own bound, and a gradient of zeros (e = 1) fails.
    e, e32 = BB.tensor_errors(dev, r64, zeros), larger([BB.tensor_errors(r, r64, zeros) for r in r32s])
    bound, bad = {}, {}
    for kind, names in (("outputs", [k for k in e if k.startswith("out.")]), ("gradients", [k for k in e if not k.startswith("out.")])):
        typical = float(np.median([e32[k] for k in names]))
        bound.update({k: BB.bound(max(e32[k], typical)) for k in names})
        worst = sorted(names, key=lambda k: e[k] / bound[k])[-3:][::-1]
        print(f"{tag} {kind}: {len(names)} tensors; median device {np.median([e[k] for k in names]):.2e} | float32 torch on the CPU {typical:.2e} | bound of a typical"
              f" tensor {BB.bound(typical):.2e}; {sum(e32[k] > typical for k in names)} tensors on their own, the largest at {max(bound[k] for k in names):.2e};"
              f" closest to their bounds: " + "; ".join(f"{k} {e[k]:.2e} / {bound[k]:.2e}" for k in worst))
    bad = {k: (e[k], bound[k]) for k in e if not e[k] <= bound[k]}
    zero32 = max(float(BB.group_errors(r, r64, zeros)["zeros"]) for r in r32s)
    zdev = max([float(dev["grads"][k].abs().max()) for k in zeros] or [0.0])
    zbound = max(BB.BOUND_FACTOR * zero32, BB.ZERO_REL * top)
    print(f"{tag} zeros: {len(zeros)} tensors, device max |g| {zdev:.3e} | float32 torch on the CPU {zero32:.3e} | bound {zbound:.3e}")
    if not zdev <= zbound:
        bad["zeros"] = (zdev, zbound)
    if mode == "batch":
        s, s32 = BB.stat_errors({k: after[k] for k in r64["stats"]}, r64["stats"]), larger([BB.stat_errors(r["stats"], r64["stats"]) for r in r32s])
        for kind, v in s.items():
            print(f"{tag} {kind}: device {v:.3e} | float32 torch on the CPU {s32[kind]:.3e} | bound {BB.bound(s32[kind]):.3e}")
            if not v <= BB.bound(s32[kind]):
                bad[kind] = (v, BB.bound(s32[kind]))
    else:
        assert all(torch.equal(v, before[k]) for k, v in after.items())          # running mode writes no statistics
    assert not bad, (tag, len(bad), bad)
    if part == "neck":                                           # legitimacy of the routing, the condition of tests/test_gpu_neck_grads.py
        pool = r64["pool"]
        for name, slack, scale in zip(N.pool_names(case[0]), pool.slack, pool.scale):
            assert slack <= 4e-5 * max(1.0, scale), (name, slack, scale)
