#!/usr/bin/env python3
"""Time the frame-to-pose calls against the compositions they replace, through the C ABI as a C# host would call it, in the regime of
bench.py's latency_b1: phi 0 @ 512, fp32, batch 1, a 1280x720 I420 frame, the classifier bias shifted as latency_b1 does (about 30
candidates).  Host clock around calls that end in a synchronise; 300 calls after 20 warm-ups; p50 / p99, back to back and paced at
60 Hz (one call per 16.7 ms: the device idles between frames).

  (a) host array in:  old = hep_run -> hep_decode -> hep_filter on host arrays     new = hep_pose_from_input
  (b) frame bytes in: old = the frame composition exactly as latency_b1 builds it   new = hep_pose_from_i420
      (torch H2D of the frame, hep_preprocess_i420_device, hep_run_device, hep_decode_device, hep_filter_device, D2H of the rows)

Every measurement runs in a child process; old and new alternate, twice each (old, new, old, new).  Then the new calls once each with
HEP_POSE_UPLOAD=pinned and =direct: camera and payload copied into the handle's pinned buffer and sent as one copy, against two
copies straight from the caller's pageable memory (the library's default is the second: it measured faster).
A child that fails ends the run: nothing further is started on the device.

Acceptance (the rule of NOTEBOOK.md section 15), stated per regime: spread = |old run 1 - old run 2| of the p50;
  (b) the new call's slower run is not above the old composition's slower run by more than that spread;
  (a) the new call's slower run is below the old composition's faster run by more than that spread.

    python tools/pose_call_time.py [--calls 300] [--warmup 20] [--json FILE]

--labels K: the same regime with seeded K-class weights, for the calls that return the top detection of EVERY label:
  (a) old = hep_run -> hep_decode -> hep_filter on host arrays, the rows then searched by label   new = hep_poses_from_input
  (b) old = the frame composition above, the rows searched by label                               new = hep_poses_from_i420
old and new alternate twice; both (a) and (b) must have the new call's slower run below the old path's faster run by more than the old
path's spread.  With K = 1 a third child, "top1" (hep_pose_from_input / hep_pose_from_i420), runs between them: the two kernels on the
same scores should be level.  No upload A/B in this mode.

    python tools/pose_call_time.py --labels 3 [--calls 300] [--warmup 20] [--json FILE]

--tiles NXxNY: the whole-frame search on one 896 x 504 frame with crop 256, resized 512, phi 0 @ 512 and @ 256, fp32, seeded weights:
  tiled    = one hep_pose_from_i420_tiled call (one upload, one forward at batch NX * NY, best-of-windows on the device, one download)
  composed = what a caller could do without it: the same windows cut on the host into 256 x 256 I420 frames, one hep_pose_from_i420 each with
             the window's camera row, the maximum taken on the host
composed and tiled alternate, twice each per size, in child processes under the same limits.  No ratio is fixed in advance: the tool prints both
medians, both run-to-run spreads, and whether the one call is faster than the composed path by more than the composed path's own spread.

    python tools/pose_call_time.py --tiles 4x2 [--calls 300] [--warmup 20] [--json FILE]

--tiles NXxNY --rectified: the same frame and sessions, the one call on RECTIFIED windows against the one call on plain windows:
  tiled     = hep_pose_from_i420_tiled, as above (unchanged code: its figures show that nothing else moved)
  rectified = hep_pose_from_i420_tiled_rectified (the table computed on the host and uploaded with the rest, four clamped taps and a float64
              chain per crop pixel where the plain kernel reads one pixel, and the back-rotation launch)
tiled and rectified alternate, twice each per size.  The tool prints both medians, both run-to-run spreads, and whether the rectified call costs
more than the plain call's own spread.

    python tools/pose_call_time.py --tiles 4x2 --rectified [--calls 300] [--warmup 20] [--json FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLS_BIAS_KEY = "classifier.header.pointwise_conv.conv.bias"


def child(args):
    import numpy as np
    import torch

    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd.model import Session
    from hmd_ego_pose_amd.weights import seeded_state_dict
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = _capi.lib()
    dev = torch.device("cuda", 0)
    phi, S, M, thr = 0, 512, 100, 0.5
    K = args.labels or 1
    sd = seeded_state_dict(phi, 0, num_classes=K)
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.standard_normal((1, 3, S, S)).astype(np.float32)
    shift = 0.0                                       # latency_b1's load knob: the quantile of the logits that leaves ~30 candidates
    for _ in range(6):
        sd_l = dict(sd); sd_l[CLS_BIAS_KEY] = sd[CLS_BIAS_KEY] - shift
        s = Session(sd_l, phi, S, 1, "fp32", dev)
        p = s.forward(torch.from_numpy(x).to(dev), want_features=False)[2].double().flatten()
        n_pass = int((p > thr).sum())
        if 10 <= n_pass <= 60:
            break
        pc = p.clamp(1e-6, 1 - 1e-6)
        shift += float(torch.quantile(torch.log(pc / (1 - pc)), 1.0 - 30.0 / p.numel()))
        s.close()
    N = s.num_anchors
    cam = np.array([[480, 480, 128, 128, 1000, 1.0]], np.float32)
    FH, FW = 720, 1280
    frame = rng.integers(0, 256, (1, FH * FW * 3 // 2), dtype=np.uint8)
    top = {"found": np.empty(1, np.int32), "score": np.empty(1, np.float32), "label": np.empty(1, np.int32), "index": np.empty(1, np.int32),
           "box": np.empty((1, 4), np.float32), "rotation": np.empty((1, 3), np.float32), "translation": np.empty((1, 3), np.float32),
           "hand": np.empty((1, 63), np.float32)}
    top_ptrs = [top[k].ctypes.data for k in Session._POSE_KEYS]
    per = {k: np.empty((1, K) + v.shape[1:], v.dtype) for k, v in top.items() if k != "label"}      # hep_poses_from_*: slot c = label c
    per_ptrs = [per[k].ctypes.data for k in Session._POSE_KEYS if k != "label"]
    row0 = {}

    def by_label(labels, index, scores):
        """what the caller of the old path does with the filter's rows: the first row of every label"""
        out = []
        for c in range(K):
            r = np.nonzero(np.asarray(labels) == c)[0]
            out.append((int(index[r[0]]), float(scores[r[0]])) if len(r) else (-1, -1.0))
        return out

    if args.child == "old":
        ho = [np.empty((1, N, k), np.float32) for k in s.out_width]
        hb, ht = np.empty((1, N, 4), np.float32), np.empty((1, N, 3), np.float32)
        hd_ = [np.empty((1, M, 4), np.float32), np.empty((1, M), np.float32), np.empty((1, M), np.int32), np.empty((1, M, 3), np.float32),
               np.empty((1, M, 3), np.float32), np.empty((1, M, 63), np.float32), np.empty((1, M), np.int32), np.empty((1,), np.int32)]

        def call_a():
            _capi.check(lib.hep_run(s.handle, x.ctypes.data, 1, None, *[o.ctypes.data for o in ho]))
            _capi.check(lib.hep_decode(s.handle, ho[0].ctypes.data, ho[3].ctypes.data, cam.ctypes.data, 1, hb.ctypes.data, ht.ctypes.data))
            _capi.check(lib.hep_filter(s.handle, hb.ctypes.data, ho[1].ctypes.data, ho[2].ctypes.data, ht.ctypes.data, ho[4].ctypes.data, 1, thr, 0.5, M,
                                       *[a.ctypes.data for a in hd_]))
            row0["a"] = by_label(hd_[2][0], hd_[6][0], hd_[1][0]) if args.labels else (int(hd_[6][0, 0]), float(hd_[1][0, 0]))

        tframe = torch.from_numpy(frame)
        st = torch.cuda.Stream(dev)
        cam_d = torch.from_numpy(cam).to(dev)
        pre = torch.empty((1, S, S, 3), dtype=torch.float32, device=dev)
        xv = pre.permute(0, 3, 1, 2)
        xstr = (ctypes.c_int64 * 4)(*xv.stride())
        bx, tr = torch.empty((1, N, 4), device=dev), torch.empty((1, N, 3), device=dev)
        f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        i = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)
        det = [f(1, M, 4), f(1, M), i(1, M), f(1, M, 3), f(1, M, 3), f(1, M, 63), i(1, M), i(1)]

        def call_b():
            with torch.cuda.stream(st):
                fd = tframe.to(dev, non_blocking=True)
                _capi.check(lib.hep_preprocess_i420_device(s.handle, fd.data_ptr(), 1, FH, FW, 256, 512, pre.data_ptr(), st.cuda_stream))
                _capi.check(lib.hep_run_device(s.handle, xv.data_ptr(), xstr, 1, None, None, st.cuda_stream))
                _capi.check(lib.hep_decode_device(s.handle, None, None, cam_d.data_ptr(), 1, bx.data_ptr(), tr.data_ptr(), st.cuda_stream))
                _capi.check(lib.hep_filter_device(s.handle, bx.data_ptr(), None, None, tr.data_ptr(), None, 1, thr, 0.5, M, *[d.data_ptr() for d in det], st.cuda_stream))
                rows = [d.cpu() for d in det]                # D2H of the detection rows (synchronises the stream)
            row0["b"] = by_label(rows[2][0].numpy(), rows[6][0].numpy(), rows[1][0].numpy()) if args.labels else (int(rows[6][0, 0]), float(rows[1][0, 0]))
    elif args.labels and args.child == "new":
        def call_a():
            _capi.check(lib.hep_poses_from_input(s.handle, x.ctypes.data, 1, cam.ctypes.data, thr, *per_ptrs))
            row0["a"] = [(int(per["index"][0, c]), float(per["score"][0, c])) for c in range(K)]

        def call_b():
            _capi.check(lib.hep_poses_from_i420(s.handle, frame.ctypes.data, 1, FH, FW, 256, 512, cam.ctypes.data, thr, *per_ptrs))
            row0["b"] = [(int(per["index"][0, c]), float(per["score"][0, c])) for c in range(K)]
    else:                                             # "new" without --labels, "top1" with it: the single-detection calls
        def call_a():
            _capi.check(lib.hep_pose_from_input(s.handle, x.ctypes.data, 1, cam.ctypes.data, thr, *top_ptrs))
            row0["a"] = [(int(top["index"][0]), float(top["score"][0]))] if args.labels else (int(top["index"][0]), float(top["score"][0]))

        def call_b():
            _capi.check(lib.hep_pose_from_i420(s.handle, frame.ctypes.data, 1, FH, FW, 256, 512, cam.ctypes.data, thr, *top_ptrs))
            row0["b"] = [(int(top["index"][0]), float(top["score"][0]))] if args.labels else (int(top["index"][0]), float(top["score"][0]))

    out = {"path": args.child, "upload": os.environ.get("HEP_POSE_UPLOAD", "default"), "candidates": n_pass,
           "a": back_to_back(call_a, args), "a_60hz": paced(call_a, 60.0, args), "b": back_to_back(call_b, args), "b_60hz": paced(call_b, 60.0, args),
           "row0": row0, "forward_launches": lib.hep_kernel_count(s.handle, 1)}
    s.close()
    print("RESULT " + json.dumps(out), flush=True)


def stats(ts):
    ts = sorted(ts)
    return {"p50_ms": round(ts[len(ts) // 2], 4), "p99_ms": round(ts[min(len(ts) - 1, int(len(ts) * 0.99))], 4), "min_ms": round(ts[0], 4)}


def back_to_back(fn, args):
    import torch
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.calls):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def paced(fn, hz, args):
    ts, period = [], 1.0 / hz
    nxt = time.perf_counter() + period
    for _ in range(args.calls):
        while time.perf_counter() < nxt:
            time.sleep(max(0.0, min(0.002, nxt - time.perf_counter())))
        nxt += period
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def child_tiles(args):
    """--tiles: one frame searched whole.  "tiled" = one hep_pose_from_i420_tiled call; "composed" = what a caller could do before it: every
    window of the same grid cut out of the frame on the host into a crop x crop I420 frame (chroma planes at half offsets - an odd offset loses
    its last chroma column: the composed path cannot express it), one hep_pose_from_i420 each with the window's camera, the maximum on the host."""
    import numpy as np
    import torch

    import hmd_ego_pose_amd as H
    from hmd_ego_pose_amd import _capi
    from hmd_ego_pose_amd.model import Session
    from hmd_ego_pose_amd.weights import seeded_state_dict
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = _capi.lib()
    nx, ny = args.tiles
    S, T, thr = args.size, nx * ny, 0.0               # threshold 0: every window reports its best anchor, so the two paths' answers can be compared
    FH, FW, crop, rs = 504, 896, 256, 512
    s = Session(seeded_state_dict(0, 0), 0, S, T, "fp32", torch.device("cuda", 0))
    rng = np.random.Generator(np.random.PCG64(5))
    frame = rng.integers(0, 256, (1, FH * FW * 3 // 2), dtype=np.uint8)
    cam = np.array([[480, 480, S / 2, S / 2, 1000, S / rs]], np.float32)
    grid = H.tile_windows(FH, FW, crop, nx, ny, 1)
    wcam = H.window_cameras(cam, grid, FH, FW, crop, rs)
    top = {"found": np.empty(1, np.int32), "score": np.empty(1, np.float32), "label": np.empty(1, np.int32), "index": np.empty(1, np.int32),
           "box": np.empty((1, 4), np.float32), "rotation": np.empty((1, 3), np.float32), "translation": np.empty((1, 3), np.float32),
           "hand": np.empty((1, 63), np.float32)}
    top_ptrs = [top[k].ctypes.data for k in Session._POSE_KEYS]
    window = np.empty(1, np.int32)
    answer = {}
    if args.child == "rectified":
        def call():
            _capi.check(lib.hep_pose_from_i420_tiled_rectified(s.handle, frame.ctypes.data, 1, FH, FW, crop, rs, nx, ny, cam.ctypes.data, thr, *top_ptrs,
                                                               window.ctypes.data))
            answer["row"] = (int(window[0]), int(top["index"][0]), float(top["score"][0]))
    elif args.child == "tiled":
        def call():
            _capi.check(lib.hep_pose_from_i420_tiled(s.handle, frame.ctypes.data, 1, FH, FW, crop, rs, nx, ny, cam.ctypes.data, thr, *top_ptrs, window.ctypes.data))
            answer["row"] = (int(window[0]), int(top["index"][0]), float(top["score"][0]))
    else:
        hw, q = FH * FW, (FH // 2) * (FW // 2)
        yp, p1, p2 = frame[0, :hw].reshape(FH, FW), frame[0, hw:hw + q].reshape(FH // 2, FW // 2), frame[0, hw + q:].reshape(FH // 2, FW // 2)
        sub = np.empty((1, crop * crop * 3 // 2), np.uint8)
        c2 = crop // 2

        def call():
            best = (-1, -1, -1.0)
            for i, (_f, ox, oy) in enumerate(grid):
                sub[0, :crop * crop].reshape(crop, crop)[:] = yp[oy:oy + crop, ox:ox + crop]
                sub[0, crop * crop:crop * crop + c2 * c2].reshape(c2, c2)[:] = p1[oy // 2:oy // 2 + c2, ox // 2:ox // 2 + c2]
                sub[0, crop * crop + c2 * c2:].reshape(c2, c2)[:] = p2[oy // 2:oy // 2 + c2, ox // 2:ox // 2 + c2]
                _capi.check(lib.hep_pose_from_i420(s.handle, sub.ctypes.data, 1, crop, crop, crop, rs, wcam[i:i + 1].ctypes.data, thr, *top_ptrs))
                if top["found"][0] == 1 and float(top["score"][0]) > best[2]:
                    best = (i, int(top["index"][0]), float(top["score"][0]))
            answer["row"] = best
    out = {"path": args.child, "size": S, "tiles": [nx, ny], "call": back_to_back(call, args), "call_60hz": paced(call, 60.0, args), "row": answer["row"],
           "even_offsets": bool((grid[:, 1:] % 2 == 0).all()), "forward_launches": lib.hep_kernel_count(s.handle, T)}
    s.close()
    print("RESULT " + json.dumps(out), flush=True)


def tiles_child(args, path, size):
    """one measuring child of the --tiles modes: its result, printed; a child that fails ends the run"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--calls", str(args.calls), "--warmup", str(args.warmup),
           "--tiles", f"{args.tiles[0]}x{args.tiles[1]}", "--size", str(size)]
    r = subprocess.run(cmd, timeout=args.timeout, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
        sys.exit(f"the {path} child failed (exit status {r.returncode}): nothing further is started")
    d = json.loads(line[0][7:])
    print(f"{path:<9} size {size}  " + "  ".join(f"{k}: p50 {d[k]['p50_ms']:.4f} p99 {d[k]['p99_ms']:.4f}" for k in ("call", "call_60hz")) +
          f"  (window, anchor, score) = {d['row']}", flush=True)
    return d


def main_tiles_rectified(args):
    """tiled and rectified alternate, twice each, at phi 0 @ 512 and @ 256; medians and run-to-run spread of both, and what the rectification costs"""
    runs, verdict = [], {}
    for size in (512, 256):
        for path in ("tiled", "rectified") * 2:
            runs.append(tiles_child(args, path, size))
        mine = [r for r in runs if r["size"] == size]
        for k in ("call", "call_60hz"):
            t, c = ([r[k]["p50_ms"] for r in mine if r["path"] == p] for p in ("tiled", "rectified"))
            ts, cs = abs(t[0] - t[1]), abs(c[0] - c[1])
            cost = sum(c) / 2 - sum(t) / 2
            beyond = min(c) > max(t) + ts
            verdict[f"{size} {k}"] = {"tiled_p50": t, "rectified_p50": c, "tiled_spread": round(ts, 4), "rectified_spread": round(cs, 4),
                                      "cost_ms": round(cost, 4), "cost_beyond_spread": bool(beyond)}
            print(f"size {size} {k:<9} tiled p50 {t} (spread {ts:.4f})  rectified p50 {c} (spread {cs:.4f})  -> the rectification costs {cost:+.4f} ms, "
                  f"{'more' if beyond else 'NOT more'} than the plain call's run-to-run spread")
    T = args.tiles[0] * args.tiles[1]
    print(f"tiled:     per frame H2D 3 (cameras, table, frame), preprocess 3 launches at batch {T}, forward at batch {T}, top-1 1, best-of-windows 1, D2H 1")
    print(f"rectified: per frame H2D 4 (cameras, table, float64 table, frame), the same launches with the warp in place of the crop, back-rotation 1, D2H 1")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": runs, "verdict": verdict}, f, indent=1)


def main_tiles(args):
    """composed and tiled alternate, twice each, at phi 0 @ 512 and @ 256; medians and run-to-run spread of both, and whether the one call is
    faster than the composed path by more than the composed path's own spread"""
    runs, verdict = [], {}
    for size in (512, 256):
        for path in ("composed", "tiled") * 2:
            runs.append(tiles_child(args, path, size))
        mine = [r for r in runs if r["size"] == size]
        rows = {tuple(r["row"][:2]) for r in mine}
        if mine[0]["even_offsets"]:                      # the composed path is exact only then
            assert len(rows) == 1, [r["row"] for r in mine]
        elif len(rows) != 1:
            print(f"size {size}: the grid has odd offsets, which the host cut rounds down in the chroma planes - the two paths' answers differ: {sorted(rows)}")
        for k in ("call", "call_60hz"):
            c, t = ([r[k]["p50_ms"] for r in mine if r["path"] == p] for p in ("composed", "tiled"))
            cs, ts = abs(c[0] - c[1]), abs(t[0] - t[1])
            faster = max(t) < min(c) - cs
            verdict[f"{size} {k}"] = {"composed_p50": c, "tiled_p50": t, "composed_spread": round(cs, 4), "tiled_spread": round(ts, 4), "tiled_faster_beyond_spread": bool(faster)}
            print(f"size {size} {k:<9} composed p50 {c} (spread {cs:.4f})  tiled p50 {t} (spread {ts:.4f})  -> the one call is "
                  f"{'faster than' if faster else 'NOT faster than'} the composed path by more than the composed path's spread ({min(c) / max(t):.2f} x)")
    T = args.tiles[0] * args.tiles[1]
    print(f"composed: per frame {T} host cuts, {T} x (H2D 2, preprocess 3 launches, forward at batch 1, top-1 1, D2H 1, synchronise)")
    print(f"tiled:    per frame H2D 3 (cameras, table, frame), preprocess 3 launches at batch {T}, forward at batch {T}, top-1 1, best-of-windows 1, D2H 1, one synchronise")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": runs, "verdict": verdict}, f, indent=1)


# per call, beside the forward's own launches (hep_kernel_count; one eager stem launch + one graph replay)
LAUNCHES = {
    "old a": "kernels: decode 1, filter 1; copies: H2D 1 + 3 + 5 (input; regression, translation, camera; boxes and four heads), D2H 5 + 2 + 8; three synchronises",
    "new a": "kernels: top-1 1; copies: H2D 2 (camera, input), D2H 1 (320 bytes); one synchronise",
    "old b": "kernels: preprocess 3, decode 1, filter 1; copies: H2D 1 (frame), D2H 8 (rows, each synchronising)",
    "new b": "kernels: preprocess 3, top-1 1; copies: H2D 2 (camera, frame), D2H 1 (320 bytes); one synchronise",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None, help="also write every child's result to this file")
    ap.add_argument("--timeout", type=int, default=180, help="time limit of one measuring child process, seconds")
    ap.add_argument("--labels", type=int, default=0, help="K: time hep_poses_from_* with seeded K-class weights (see above)")
    ap.add_argument("--tiles", default=None, help="NXxNY: time hep_pose_from_i420_tiled against the composed whole-frame search (see above)")
    ap.add_argument("--rectified", action="store_true", help="with --tiles: time hep_pose_from_i420_tiled_rectified against hep_pose_from_i420_tiled")
    ap.add_argument("--size", type=int, default=512, help=argparse.SUPPRESS)
    ap.add_argument("--child", default=None, choices=["old", "new", "top1", "composed", "tiled", "rectified"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not 0 <= args.labels <= 63:
        sys.exit("--labels must be in 1..63")
    if args.tiles:
        try:
            args.tiles = tuple(int(v) for v in args.tiles.lower().split("x"))
            assert len(args.tiles) == 2 and min(args.tiles) >= 1
        except (ValueError, AssertionError):
            sys.exit("--tiles takes NXxNY, e.g. 4x2")
        return child_tiles(args) if args.child else (main_tiles_rectified if args.rectified else main_tiles)(args)
    if args.rectified:
        sys.exit("--rectified goes with --tiles")
    if args.child:
        return child(args)
    runs = []
    plan = (("old", None), ("new", None), ("old", None), ("new", None), ("new", "pinned"), ("new", "direct"))
    if args.labels:
        plan = (("old", None), ("top1", None), ("new", None)) * 2 if args.labels == 1 else (("old", None), ("new", None)) * 2
    for path, upload in plan:
        env = dict(os.environ)
        env.pop("HEP_POSE_UPLOAD", None)
        if upload:
            env["HEP_POSE_UPLOAD"] = upload
        cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--calls", str(args.calls), "--warmup", str(args.warmup), "--labels", str(args.labels)]
        r = subprocess.run(cmd, timeout=args.timeout, env=env, capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
            sys.exit(f"the {path} child failed (exit status {r.returncode}): nothing further is started")
        runs.append(json.loads(line[0][7:]))
        d = runs[-1]
        print(f"{path:<4} upload={d['upload']:<7} candidates={d['candidates']}  " + "  ".join(
            f"{k}: p50 {d[k]['p50_ms']:.4f} p99 {d[k]['p99_ms']:.4f}" for k in ("a", "a_60hz", "b", "b_60hz")), flush=True)
    old = [r for r in runs if r["path"] == "old"]
    new = [r for r in runs if r["path"] == "new" and r["upload"] == "default"]
    assert all(r["row0"] == runs[0]["row0"] for r in runs), [r["row0"] for r in runs]      # every path returns the same top detection
    verdict = {}
    for k in ("a", "a_60hz", "b", "b_60hz"):
        o, n = [r[k]["p50_ms"] for r in old], [r[k]["p50_ms"] for r in new]
        spread = abs(o[0] - o[1])
        ok = (max(n) < min(o) - spread) if k.startswith("a") or args.labels else (max(n) <= max(o) + spread)
        verdict[k] = {"old_p50": o, "new_p50": n, "old_spread": round(spread, 4), "met": bool(ok)}
        print(f"{k:<7} old p50 {o}  new p50 {n}  old spread {spread:.4f} ms  -> {'met' if ok else 'NOT met'}")
    top1 = [r for r in runs if r["path"] == "top1"]
    if top1:                                          # K = 1: hep_poses_from_* against hep_pose_from_* on the same scores
        for k in ("a", "a_60hz", "b", "b_60hz"):
            t, n = [r[k]["p50_ms"] for r in top1], [r[k]["p50_ms"] for r in new]
            verdict[k]["top1_p50"] = t
            print(f"{k:<7} hep_pose_from_* p50 {t}  hep_poses_from_* p50 {n}  difference of the means {sum(n) / len(n) - sum(t) / len(t):+.4f} ms")
    print(f"forward: {runs[0]['forward_launches']} launches (one eager, the rest one graph replay)")
    for k, v in LAUNCHES.items():
        print(f"{k}: {v.replace('top-1', 'top-per-label').replace('320 bytes', f'{args.labels} x 320 bytes') if args.labels else v}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": runs, "verdict": verdict, "launches": LAUNCHES}, f, indent=1)


if __name__ == "__main__":
    main()
