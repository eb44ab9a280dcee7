"""The whole-frame search stated in numpy: the definitions of hep_tile_windows, hep_window_cameras, hep_window_from_box, of a window's blob
(hep_preprocess_i420_windows_device) and of the best-of-windows rule (hep_best_window_device), and the helpers their CPU and GPU tests share.

A window is {frame, ox, oy} (int32): the crop x crop square of frame ``frame`` whose top-left pixel is (ox, oy), 0 <= ox <= width - crop,
0 <= oy <= height - crop, any parity.  Its pixels are those of the converted FULL frame (chroma at (sy / 2, sx / 2) of the frame), so a window's
blob is ``oracle.decode_ref.webrtc_frame_preprocess`` with the slice taken at (ox, oy) in place of the centre."""
import numpy as np

from oracle import decode_ref as D

RECORD_WORDS = 80


def tile_offsets(side, crop, cells):
    """offsets of a grid's cells along one axis: integer division; one cell sits at the centre crop, several reach both borders"""
    span = side - crop
    return [span // 2] if cells == 1 else [(i * span) // (cells - 1) for i in range(cells)]


def tile_windows(height, width, crop, nx, ny, frames=1):
    """[frames * ny * nx, 3] int32 {frame, ox, oy}: frame-major, then row, then column"""
    xs, ys = tile_offsets(width, crop, nx), tile_offsets(height, crop, ny)
    return np.array([[f, ox, oy] for f in range(frames) for oy in ys for ox in xs], np.int32).reshape(-1, 3)


def window_cameras(camera, windows, height, width, crop, resized):
    """camera [F,6] float32: the rows of the CENTRE window of every frame -> [n,6]: window i's frame's row with the principal point moved by the
    window's offset from the centre crop in pixels of the resized image - float64, rounded once; the other four entries bit for bit"""
    camera, windows = np.asarray(camera, np.float32), np.asarray(windows, np.int32)
    out = camera[windows[:, 0]].copy()
    for col, side, k in ((1, width, 2), (2, height, 3)):
        d = (windows[:, col].astype(np.int64) - (side - crop) // 2).astype(np.float64)
        out[:, k] = (camera[windows[:, 0], k].astype(np.float64) - d * np.float64(resized) / np.float64(crop)).astype(np.float32)
    return out


def window_from_box(box, ox, oy, height, width, crop, size):
    """the window centred on a detection: box = xmin, ymin, xmax, ymax (float32) in network-input pixels of the window (ox, oy); float64"""
    b = np.asarray(box, np.float32).astype(np.float64)

    def around(o, lo, hi, side):
        c = np.float64(o) + np.float64(0.5) * (lo + hi) * np.float64(crop) / np.float64(size)
        return int(min(max(np.floor(c - np.float64(0.5) * np.float64(crop) + np.float64(0.5)), 0.0), float(side - crop)))
    return around(ox, b[0], b[2], width), around(oy, b[1], b[3], height)


def window_blobs(frames, height, width, windows, image_size, crop, resized):
    """frames [F, height * width * 3 / 2] uint8, windows [n,3] -> [n, S, S, 3] float32 (B, G, R): yv12_to_bgr of the whole frame, the slice at
    (ox, oy), resize_bilinear_u8 to resized and ResizeAndNormalizeMat - webrtc_frame_preprocess line by line with another slice"""
    bgr = [D.yv12_to_bgr(f, height, width) for f in frames]            # each frame converted once
    out = np.zeros((len(windows), image_size, image_size, 3), np.float32)
    scale = np.float32(image_size) / np.float32(resized)
    nw, nh = image_size, int(np.float32(resized) * scale)
    for i, (f, ox, oy) in enumerate(np.asarray(windows)):
        roi = np.ascontiguousarray(bgr[f][oy: oy + crop, ox: ox + crop])
        img = D.resize_bilinear_u8(roi, resized, resized) if resized != crop else roi
        if (nh, nw) != (resized, resized):
            img = D.resize_bilinear_u8(img, nw, nh)
        x = img.astype(np.float32) / np.float32(255.0)
        x = (x - np.array([0.485, 0.456, 0.406], np.float32)) / np.array([0.229, 0.224, 0.225], np.float32)
        out[i, :nh, :nw] = x.astype(np.float32)
    return out


def cut_window_i420(frame, height, width, ox, oy, crop):
    """what a caller without the windowed calls does: the window cut out of an I420 frame on the host into a crop x crop I420 frame (Y slice,
    chroma slices at half offsets).  Exact for even ox, oy and crop only - the composed path cannot express an odd offset."""
    assert ox % 2 == 0 and oy % 2 == 0 and crop % 2 == 0
    f = np.asarray(frame, np.uint8).ravel()
    hw, q = height * width, (height // 2) * (width // 2)
    y = f[:hw].reshape(height, width)[oy: oy + crop, ox: ox + crop]
    p1 = f[hw: hw + q].reshape(height // 2, width // 2)[oy // 2: (oy + crop) // 2, ox // 2: (ox + crop) // 2]
    p2 = f[hw + q: hw + 2 * q].reshape(height // 2, width // 2)[oy // 2: (oy + crop) // 2, ox // 2: (ox + crop) // 2]
    return np.concatenate([y.ravel(), p1.ravel(), p2.ravel()])


def not_found_record():
    """the record the top-detection launches write without a candidate: found 0; words 3, 78, 79 zero; the filter's padding elsewhere"""
    rec = np.zeros(RECORD_WORDS, np.int32)
    rec[1] = rec[2] = -1
    rec.view(np.float32)[4:78] = -1.0
    return rec


def best_window_rule(records, windows, frames):
    """records [n, slots, 80] int32, windows [n,3] -> (out_records [frames, slots, 80], out_window [frames, slots]): per frame and slot the found
    record with the largest score (word 4, float32 comparison) among the windows of the frame, ties to the lowest window, copied bit for bit;
    none: the not-found record and -1.  Windows of a frame need not be adjacent."""
    records, windows = np.asarray(records, np.int32), np.asarray(windows, np.int32)
    n, slots = records.shape[0], records.shape[1]
    out = np.tile(not_found_record(), (frames, slots, 1))
    win = np.full((frames, slots), -1, np.int32)
    for f in range(frames):
        for c in range(slots):
            best = -1
            for i in range(n):
                if windows[i, 0] != f or records[i, c, 0] != 1:
                    continue
                if best < 0 or records[i, c].view(np.float32)[4] > records[best, c].view(np.float32)[4]:
                    best = i
            if best >= 0:
                out[f, c], win[f, c] = records[best, c], best
    return out, win


def records_of(p):
    """the dict of numpy arrays of Session.pose_from_* / poses_from_* as int32 records [rows..., 80] (label word: the slot for per-label arrays)"""
    found = np.asarray(p["found"])
    rec = np.zeros(found.shape + (RECORD_WORDS,), np.int32)
    f = rec.view(np.float32)
    rec[..., 0] = found
    if "label" in p:
        rec[..., 1] = p["label"]
    else:
        rec[..., 1] = np.where(found == 1, np.arange(found.shape[-1], dtype=np.int32), -1)
    rec[..., 2] = p["index"]
    f[..., 4] = p["score"]
    f[..., 5:9], f[..., 9:12], f[..., 12:15], f[..., 15:78] = p["box"], p["rotation"], p["translation"], p["hand"]
    return rec
