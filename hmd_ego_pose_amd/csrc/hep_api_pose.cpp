// hep_api_pose.cpp - frame to pose: the entry points of the C ABI of libhep.so (include/hep.h) that turn a handle's head outputs into pose
// records (hep_top1_device, hep_top_labels_device), the twelve hep_pose(s)_from_* host calls ("host bytes in, pose records out") and the
// whole-frame search around them: window tables, rectified windows, best of the windows.  The twelve calls are ONE staged call (PoseCall,
// pose_run_locked); their wrappers only check arguments.  (Sessions, forward, preprocess, decode and filter: hep_api.cpp.)
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "hep_api_util.h"
#include "hep_plan.h"

using namespace hep;

// ---- top detection ----
static int top1_locked(Session& s, const float* regression, const float* classification, const float* rotation,
                       const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                       uint32_t* records, hipStream_t st, bool per_label = false) {
  Top1Args a;
  a.regression = regression ? regression : s.d_out[0];         // NULL = the handle's own last outputs
  a.scores = classification ? classification : s.d_out[1];
  a.rotation = rotation ? rotation : s.d_out[2];
  a.translation_raw = translation_raw ? translation_raw : s.d_out[3];
  a.hand = hand ? hand : s.d_out[4];
  a.camera = camera; a.anchors = s.d_anchors; a.t_anchors = s.d_tanchors;
  a.B = batch; a.N = s.num_anchors; a.K = s.num_classes; a.any_class = s.class_specific_filter ? 0 : 1;
  a.score_thr = score_threshold; a.clip_max = (float)(s.size - 1);
  a.records = records;                                         // per_label: [batch][num_classes] records, class-specific whatever the handle's mode
  if (per_label) launch_toplabel(a, st); else launch_top1(a, st);
  HIPRET(hipGetLastError());
  return 0;
}

// the body of hep_top1_device and hep_top_labels_device: `who` is the prefix of the entry point's messages
static int top_device(const char* who, bool per_label, hep_handle* h, const float* regression, const float* classification, const float* rotation,
                      const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                      uint32_t* records, void* stream) {
  const Check c{who};
  CHECKED(c.ptrs({{h, "handle"}, {camera, "camera"}, {records, "records"}}));      // (the handle is not read before the pointers are checked)
  Session& s = h->s; CHECKED(c.range("batch", batch, 1, s.max_batch, HEP_ERR_INVALID, "max_batch"));
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  return top1_locked(s, regression, classification, rotation, translation_raw, hand, camera, batch, score_threshold, records, (hipStream_t)stream, per_label);
}

// ---- frame to pose: one staged call ----
namespace {
struct PoseOut { int32_t* found; float* scores; int32_t* labels; int32_t* index; float* boxes; float* rotation; float* translation; float* hand; };
constexpr size_t kRecBytes = (size_t)HEP_POSE_RECORD_WORDS * 4;
static_assert(HEP_POSE_RECORD_WORDS == POSE_RECORD_WORDS, "the record of include/hep.h is the kernel's");
static_assert(HEP_RECTIFY_ROW_DOUBLES == RECTIFY_ROW_DOUBLES, "the table row of include/hep.h and of the kernels");

// One host call, every argument checked.  Exactly one of `input` and `yuv` is set; everything that may be NULL is a stage the call leaves out.
struct PoseCall {
  bool per_label = false;             // hep_poses_from_*: num_classes records per image, output row b * num_classes + c
  const float* input = nullptr;       // the float blob [n,3,S,S]: no preprocess
  const uint8_t* yuv = nullptr;       // `frames` I420 frames of height x width: the frame path with this crop and resized
  int frames = 0, height = 0, width = 0, crop = 0, resized = 0;
  int n = 0;                          // images through the network: the frames themselves, or the windows
  const float* camera = nullptr;      // [n,6], one row per image (the rectified calls: every window's frame's CENTRE row)
  const int32_t* windows = nullptr;   // [n,3] host table: the windowed preprocess in place of the centre crop
  const double* rect = nullptr;       // [n,HEP_RECTIFY_ROW_DOUBLES] host table: the rectified preprocess, and the back-rotation behind the top detection
  float score_threshold = 0.f;
  PoseOut out{};
  int32_t* window_out = nullptr;      // the best-of-windows launch follows: `frames` (x num_classes) winners and their window indices come back
};
}  // namespace

// the records of a download -> the caller's arrays, row by row
static void pose_scatter(const uint32_t* hr, int rows, const PoseOut& o) {
  for (int b = 0; b < rows; b++) {
    const uint32_t* r = hr + (size_t)b * HEP_POSE_RECORD_WORDS;
    memcpy(&o.found[b], r + 0, 4);
    if (o.labels) memcpy(&o.labels[b], r + 1, 4);
    if (o.index) memcpy(&o.index[b], r + 2, 4);
    if (o.scores) memcpy(&o.scores[b], r + 4, 4);
    if (o.boxes) memcpy(o.boxes + (size_t)b * 4, r + 5, 16);
    if (o.rotation) memcpy(o.rotation + (size_t)b * 3, r + 9, 12);
    if (o.translation) memcpy(o.translation + (size_t)b * 3, r + 12, 12);
    if (o.hand) memcpy(o.hand + (size_t)b * 63, r + 15, 63 * 4);
  }
}

// Runs `c`; s.mu is held.  Every buffer is the handle's, allocated at first use for max_batch images (d_pose_in / h_pose_in: for max_batch payloads
// of this call's per-image size, only ever grown), so a repeated shape allocates nothing.
// Staging: the sections [camera rows | window table | float64 table | payload] that the call has, each but the last reserved for max_batch rows
// rounded up to 256 bytes, on the device.  Direct (the default): one hipMemcpyAsync per section from the caller's pageable memory.  Pinned
// (HEP_POSE_UPLOAD=pinned, read at the handle's first call; kept for the A/B of tools/pose_call_time.py and held equal to direct by
// tests/test_gpu_pose_upload.py): the sections are copied into a pinned buffer of the handle and go up as ONE hipMemcpyAsync.  Measured twice
// (NOTEBOOK.md section 24): the 3 MB float blob is 0.05 ms faster direct (the host copy into the pinned buffer costs more than the runtime's own
// staging), the 1.4 MB frame 0.02 ms faster back to back and level at 60 Hz.
// Then: preprocess (frames only), forward at batch n, top-detection launch on the handle's own head outputs, back-rotation (rect), best of the
// windows (window_out), ONE download through a pinned buffer, synchronise, scatter.
static int pose_run_locked(Session& s, const PoseCall& c) {
  HIPRET(hipSetDevice(s.device));
  const size_t most = (size_t)s.max_batch, in_floats = (size_t)3 * s.size * s.size;
  const int slots = c.per_label ? s.num_classes : 1;
  if (c.yuv && !s.d_in) HIPRET(hipMalloc((void**)&s.d_in, in_floats * most * 4));
  if (c.per_label) {
    if (!s.d_recs) HIPRET(hipMalloc((void**)&s.d_recs, kRecBytes * most * s.num_classes));
    if (!s.h_recs) HIPRET(hipHostMalloc((void**)&s.h_recs, kRecBytes * most * s.num_classes, hipHostMallocDefault));
  }
  if (c.window_out) {                 // records and window indices of max_batch x num_classes rows: one size for the single and the per-label call
    if (!s.d_best) HIPRET(hipMalloc((void**)&s.d_best, (kRecBytes + 4) * most * s.num_classes));
    if (!s.h_best) HIPRET(hipHostMalloc((void**)&s.h_best, (kRecBytes + 4) * most * s.num_classes, hipHostMallocDefault));
  }
  if (!s.d_rec) {
    const char* e = getenv("HEP_POSE_UPLOAD");
    s.pose_upload_pinned = e && !strcmp(e, "pinned");
    HIPRET(hipMalloc((void**)&s.d_rec, kRecBytes * most));
  }
  if (!s.h_rec) HIPRET(hipHostMalloc((void**)&s.h_rec, kRecBytes * most, hipHostMallocDefault));

  const size_t per_image = c.yuv ? (size_t)c.height * c.width * 3 / 2 : in_floats * 4, row_bytes = HEP_RECTIFY_ROW_DOUBLES * sizeof(double);
  auto rows256 = [&](size_t row) { return (most * row + 255) & ~(size_t)255; };
  struct Section { const void* host; size_t used, reserved, at; } sec[4] = {
      {c.camera, (size_t)c.n * 24, rows256(24), 0},
      {c.windows, (size_t)c.n * 12, rows256(12), 0},
      {c.rect, (size_t)c.n * row_bytes, rows256(row_bytes), 0},
      {c.yuv ? (const void*)c.yuv : (const void*)c.input, per_image * (size_t)c.frames, per_image * most, 0}};
  size_t need = 0, used = 0;          // the reservation, and the end of the last section's bytes of this call
  for (Section& x : sec) {
    if (!x.host) continue;
    x.at = need; used = need + x.used; need += x.reserved;
  }
  if (s.pose_in_bytes < need) {
    HIPRET(hipStreamSynchronize(s.stream));
    hipFree(s.d_pose_in); s.d_pose_in = nullptr; s.pose_in_bytes = 0;
    HIPRET(hipMalloc((void**)&s.d_pose_in, need)); s.pose_in_bytes = need;
  }
  if (s.pose_upload_pinned && s.pose_pin_bytes < need) {
    HIPRET(hipStreamSynchronize(s.stream));
    hipHostFree(s.h_pose_in); s.h_pose_in = nullptr; s.pose_pin_bytes = 0;
    HIPRET(hipHostMalloc((void**)&s.h_pose_in, need, hipHostMallocDefault)); s.pose_pin_bytes = need;
  }
  for (const Section& x : sec) {
    if (!x.host) continue;
    if (s.pose_upload_pinned) memcpy(s.h_pose_in + x.at, x.host, x.used);
    else HIPRET(hipMemcpyAsync(s.d_pose_in + x.at, x.host, x.used, hipMemcpyHostToDevice, s.stream));
  }
  if (s.pose_upload_pinned) HIPRET(hipMemcpyAsync(s.d_pose_in, s.h_pose_in, used, hipMemcpyHostToDevice, s.stream));
  const float* d_camera = (const float*)s.d_pose_in;
  const int32_t* d_windows = c.windows ? (const int32_t*)(s.d_pose_in + sec[1].at) : nullptr;
  const double* d_rect = c.rect ? (const double*)(s.d_pose_in + sec[2].at) : nullptr;      // (256-byte aligned)
  const unsigned char* d_payload = s.d_pose_in + sec[3].at;

  std::string err;
  if (c.yuv) {
    CHECKED(preprocess_i420_locked(s, d_payload, c.n, c.height, c.width, c.crop, c.resized, s.d_in, s.stream, d_windows, d_rect));
    const int64_t S = s.size; const int64_t nhwc[4] = {3 * S * S, 1, 3 * S, 3};      // the NCHW view of the [n,S,S,3] images
    if (int rc = run_forward(&s, s.d_in, nhwc, c.n, s.stream, &err)) return fail(rc, err);
  } else if (int rc = run_forward(&s, (const float*)d_payload, nullptr, c.n, s.stream, &err)) return fail(rc, err);

  uint32_t* d = c.per_label ? s.d_recs : s.d_rec;
  uint32_t* hr = c.per_label ? s.h_recs : s.h_rec;
  int rows = c.n * slots;
  CHECKED(top1_locked(s, nullptr, nullptr, nullptr, nullptr, nullptr, d_camera, c.n, c.score_threshold, d, s.stream, c.per_label));
  if (c.rect) {
    DerotateArgs a; a.records = d; a.table = d_rect; a.n = c.n; a.slots = slots;
    launch_derotate_records(a, s.stream);
    HIPRET(hipGetLastError());
  }
  if (c.window_out) {                 // [rows records | rows window indices] in d_best
    rows = c.frames * slots;
    BestWindowArgs a; a.records = d; a.windows = d_windows; a.out_records = s.d_best; a.out_window = (int32_t*)(s.d_best + (size_t)rows * HEP_POSE_RECORD_WORDS);
    a.n = c.n; a.slots = slots; a.frames = c.frames;
    launch_best_window(a, s.stream);
    HIPRET(hipGetLastError());
    d = s.d_best; hr = s.h_best;
  }
  HIPRET(hipMemcpyAsync(hr, d, (kRecBytes + (c.window_out ? 4 : 0)) * rows, hipMemcpyDeviceToHost, s.stream));
  HIPRET(hipStreamSynchronize(s.stream));
  pose_scatter(hr, rows, c.out);
  if (c.window_out) memcpy(c.window_out, hr + (size_t)rows * HEP_POSE_RECORD_WORDS, (size_t)rows * 4);
  return 0;
}

// ---- the wrappers: argument checks, then the call ----
// what the host entry points refuse first, without reading the handle: NULL pointers and a batch below 1 (check_pose); then, behind the frame
// geometry where there is one, the batch against the handle's max_batch (check_pose_batch)
static int check_pose_batch(const Check& c, int batch, int most) { return c.range("batch", batch, 1, most, HEP_ERR_INVALID, "max_batch given to hep_create"); }
static int check_pose(const Check& c, const hep_handle* h, const void* input, const char* input_name, int batch, const float* camera, const int32_t* found) {
  CHECKED(c.ptrs({{h, "handle"}, {input, input_name}, {camera, "camera"}, {found, "found"}}));
  return check_pose_batch(c, batch, INT_MAX);
}

// the bodies of hep_pose_from_input / hep_poses_from_input and of hep_pose_from_i420 / hep_poses_from_i420: `who` is the prefix of the entry point's messages
static int pose_from_input(const char* who, bool per_label, hep_handle* h, const float* input_nchw, int batch, const float* camera,
                           float score_threshold, const PoseOut& o) {
  const Check c{who};
  CHECKED(check_pose(c, h, input_nchw, "input_nchw", batch, camera, o.found)); CHECKED(check_pose_batch(c, batch, h->s.max_batch));
  Session& s = h->s;
  PoseCall p; p.per_label = per_label; p.input = input_nchw; p.frames = p.n = batch; p.camera = camera; p.score_threshold = score_threshold; p.out = o;
  std::lock_guard<std::mutex> lk(s.mu);
  return pose_run_locked(s, p);
}
// the frame calls' description: `frames` frames in, n images through the network
static PoseCall frame_call(bool per_label, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int n, float score_threshold, const PoseOut& o) {
  PoseCall p; p.per_label = per_label; p.yuv = yuv; p.frames = frames; p.height = height; p.width = width; p.crop = crop; p.resized = resized;
  p.n = n; p.score_threshold = score_threshold; p.out = o;
  return p;
}
static int pose_from_i420(const char* who, bool per_label, hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop,
                          int resized, const float* camera, float score_threshold, const PoseOut& o) {
  const Check c{who};
  CHECKED(check_pose(c, h, yuv, "yuv", batch, camera, o.found)); CHECKED(check_i420(height, width, crop, resized)); CHECKED(check_pose_batch(c, batch, h->s.max_batch));
  Session& s = h->s;
  CHECKED(check_fits(s, resized));                  // refused here, before any HIP call
  PoseCall p = frame_call(per_label, yuv, batch, height, width, crop, resized, batch, score_threshold, o); p.camera = camera;
  std::lock_guard<std::mutex> lk(s.mu);
  return pose_run_locked(s, p);
}

// ---- whole-frame search: windows of a frame, best of the windows (include/hep.h) ----
// a grid offset along one axis: span = side - crop; one cell sits at the centre (the frame path's crop), several reach both borders
static int tile_offset(int i, int cells, int span) { return cells == 1 ? span / 2 : (int)(((int64_t)i * span) / (cells - 1)); }
static void tile_windows(int height, int width, int crop, int nx, int ny, int frames, int32_t* w) {
  for (int f = 0; f < frames; f++)
    for (int r = 0; r < ny; r++)
      for (int i = 0; i < nx; i++, w += 3) { w[0] = f; w[1] = tile_offset(i, nx, width - crop); w[2] = tile_offset(r, ny, height - crop); }
}
// camera row of window {frame, ox, oy}: the frame's row with the principal point moved by the window's offset from the centre crop, in pixels
// of the resized image; every rounding stated (tests/_windows.py restates it)
static void window_camera(const float* camera, const int32_t* w, int height, int width, int crop, int resized, float* out) {
  const float* row = camera + (size_t)w[0] * 6;
  memcpy(out, row, 24);
  out[2] = (float)((double)row[2] - (double)(w[1] - (width - crop) / 2) * (double)resized / (double)crop);
  out[3] = (float)((double)row[3] - (double)(w[2] - (height - crop) / 2) * (double)resized / (double)crop);
}
// the offset along one axis of the crop-wide window around `centre` (frame pixels), kept inside a frame `side` wide (compared in double: no
// cast of a value an int cannot hold; a NaN - a ray that points backwards - gives 0)
static int window_around(double centre, int crop, int side) {
  const double v = floor(centre - 0.5 * (double)crop + 0.5);
  return !(v > 0.0) ? 0 : (v > (double)(side - crop) ? side - crop : (int)v);
}
// a host table: every window inside its frame; frames < 0: the frame index has no upper limit to hold (hep_window_cameras)
static int check_windows(const Check& c, const int32_t* windows, int n, int frames, int height, int width, int crop) {
  for (int i = 0; i < n; i++) {
    const int32_t* w = windows + (size_t)i * 3;
    if (w[0] < 0 || (frames >= 0 && w[0] >= frames) || w[1] < 0 || w[1] > width - crop || w[2] < 0 || w[2] > height - crop)
      return c.fail(HEP_ERR_INVALID, "window " + std::to_string(i) + " {" + std::to_string(w[0]) + ", " + std::to_string(w[1]) + ", " + std::to_string(w[2]) +
                                     "} lies outside the frame (frame index or offsets)");
  }
  return 0;
}
// rectified windows: the host arithmetic is hep_rectify.cpp's (built without contraction), the checks are here
// every window's frame has a camera row whose focal lengths are finite and positive
static int check_rectify_camera(const Check& c, const float* camera, const int32_t* windows, int n) {
  for (int i = 0; i < n; i++) {
    const float* row = camera + (size_t)windows[(size_t)i * 3] * 6;
    if (!(row[0] > 0.f && row[0] <= FLT_MAX && row[1] > 0.f && row[1] <= FLT_MAX))
      return c.fail(HEP_ERR_INVALID, "camera row " + std::to_string(windows[(size_t)i * 3]) + ": fx and fy must be finite and positive");
  }
  return 0;
}
static int check_rectify_row(const Check& c, const double* row) {
  return row[9] > 0.0 && row[9] <= DBL_MAX && row[10] > 0.0 && row[10] <= DBL_MAX ? 0 : c.fail(HEP_ERR_INVALID, "row: fx and fy must be finite and positive");
}

// the host tables of the tiled and of the rectified calls, built under the mutex: sized once, max_batch rows
static void win_buffers(Session& s) {
  if (s.win_table.empty()) { s.win_table.resize((size_t)s.max_batch * 3); s.win_cam.resize((size_t)s.max_batch * 6); s.win_rect.resize((size_t)s.max_batch * HEP_RECTIFY_ROW_DOUBLES); }
}
// the rectified calls' host side: s.win_cam = every window's frame's centre row as it is, s.win_rect = the table of hep_rectify_windows
static void rectify_tables(Session& s, const float* camera, const int32_t* windows, int n, int height, int width, int crop, int resized) {
  for (int i = 0; i < n; i++) {
    const float* row = camera + (size_t)windows[(size_t)i * 3] * 6;
    memcpy(s.win_cam.data() + (size_t)i * 6, row, 24);
    rectify_row(row, windows + (size_t)i * 3, height, width, crop, resized, s.win_rect.data() + (size_t)i * HEP_RECTIFY_ROW_DOUBLES);
  }
}

// the bodies of the windows and of the tiled calls.  rectified: camera is [frames,6], the centre rows
static int pose_from_i420_windows(const char* who, bool per_label, hep_handle* h, const uint8_t* yuv, int frames, int height, int width,
                                  const int32_t* windows, int n, int crop, int resized, const float* camera, float score_threshold, const PoseOut& o,
                                  bool rectified = false) {
  const Check c{who};
  CHECKED(c.ptrs({{h, "handle"}, {yuv, "yuv"}, {windows, "windows"}, {camera, "camera"}, {o.found, "found"}}));
  CHECKED(c.range("n", n, 1, INT_MAX, HEP_ERR_INVALID, "max_batch given to hep_create")); CHECKED(c.at_least("frames", frames, 1));
  CHECKED(check_i420(height, width, crop, resized)); CHECKED(check_windows(c, windows, n, frames, height, width, crop));
  if (rectified) CHECKED(check_rectify_camera(c, camera, windows, n));
  Session& s = h->s;      // (the handle is read from here on)
  CHECKED(c.range("n", n, 1, s.max_batch, HEP_ERR_INVALID, "max_batch given to hep_create"));
  CHECKED(c.range("frames", frames, 1, s.max_batch, HEP_ERR_INVALID, "max_batch given to hep_create")); CHECKED(check_fits(s, resized));
  PoseCall p = frame_call(per_label, yuv, frames, height, width, crop, resized, n, score_threshold, o); p.camera = camera; p.windows = windows;
  std::lock_guard<std::mutex> lk(s.mu);
  if (rectified) {
    win_buffers(s);
    rectify_tables(s, camera, windows, n, height, width, crop, resized);
    p.camera = s.win_cam.data(); p.rect = s.win_rect.data();
  }
  return pose_run_locked(s, p);
}

static int pose_from_i420_tiled(const char* who, bool per_label, hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop,
                                int resized, int nx, int ny, const float* camera, float score_threshold, const PoseOut& o, int32_t* window,
                                bool rectified = false) {
  const Check c{who};
  CHECKED(c.ptrs({{h, "handle"}, {yuv, "yuv"}, {camera, "camera"}, {o.found, "found"}, {window, "window"}}));
  CHECKED(c.at_least("nx", nx, 1)); CHECKED(c.at_least("ny", ny, 1)); CHECKED(c.at_least("frames", frames, 1));
  CHECKED(check_i420(height, width, crop, resized));
  Session& s = h->s;      // (the handle is read from here on)
  int64_t n = (int64_t)nx * ny;                     // (two factors at a time: neither product can pass int64)
  if (n <= s.max_batch) n *= frames;
  if (n > s.max_batch) return c.fail(HEP_ERR_INVALID, "frames * nx * ny outside 1..max_batch given to hep_create");
  CHECKED(check_fits(s, resized));
  if (rectified)
    for (int f = 0; f < frames; f++) { const int32_t w[3] = {f, 0, 0}; CHECKED(check_rectify_camera(c, camera, w, 1)); }
  PoseCall p = frame_call(per_label, yuv, frames, height, width, crop, resized, (int)n, score_threshold, o); p.window_out = window;
  std::lock_guard<std::mutex> lk(s.mu);
  win_buffers(s);
  tile_windows(height, width, crop, nx, ny, frames, s.win_table.data());
  p.windows = s.win_table.data(); p.camera = s.win_cam.data();
  if (rectified) { rectify_tables(s, camera, p.windows, p.n, height, width, crop, resized); p.rect = s.win_rect.data(); }
  else for (int i = 0; i < p.n; i++) window_camera(camera, p.windows + (size_t)i * 3, height, width, crop, resized, s.win_cam.data() + (size_t)i * 6);
  return pose_run_locked(s, p);
}

extern "C" {

int hep_top1_device(hep_handle* h, const float* regression, const float* classification, const float* rotation,
                    const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                    uint32_t* records, void* stream) try {
  return top_device("hep_top1_device: ", false, h, regression, classification, rotation, translation_raw, hand, camera, batch, score_threshold, records, stream);
} HEP_CATCH_INT

int hep_top_labels_device(hep_handle* h, const float* regression, const float* classification, const float* rotation,
                          const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                          uint32_t* records, void* stream) try {
  return top_device("hep_top_labels_device: ", true, h, regression, classification, rotation, translation_raw, hand, camera, batch, score_threshold, records, stream);
} HEP_CATCH_INT

int hep_pose_from_input(hep_handle* h, const float* input_nchw, int batch, const float* camera, float score_threshold,
                        int32_t* found, float* scores, int32_t* labels, int32_t* index, float* boxes, float* rotation,
                        float* translation, float* hand) try {
  return pose_from_input("hep_pose_from_input: ", false, h, input_nchw, batch, camera, score_threshold,
                         PoseOut{found, scores, labels, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

int hep_pose_from_i420(hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop, int resized,
                       const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels,
                       int32_t* index, float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420("hep_pose_from_i420: ", false, h, yuv, batch, height, width, crop, resized, camera, score_threshold,
                        PoseOut{found, scores, labels, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

// several objects: [batch][num_classes] rows per output, slot c = label c (no labels array)
int hep_poses_from_input(hep_handle* h, const float* input_nchw, int batch, const float* camera, float score_threshold,
                         int32_t* found, float* scores, int32_t* index, float* boxes, float* rotation, float* translation,
                         float* hand) try {
  return pose_from_input("hep_poses_from_input: ", true, h, input_nchw, batch, camera, score_threshold,
                         PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

int hep_poses_from_i420(hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop, int resized,
                        const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index, float* boxes,
                        float* rotation, float* translation, float* hand) try {
  return pose_from_i420("hep_poses_from_i420: ", true, h, yuv, batch, height, width, crop, resized, camera, score_threshold,
                        PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

int hep_tile_windows(int height, int width, int crop, int nx, int ny, int frames, int32_t* windows_out) try {
  const Check c{"hep_tile_windows: "};
  CHECKED(c.ptrs({{windows_out, "windows_out"}}));
  CHECKED(c.at_least("nx", nx, 1)); CHECKED(c.at_least("ny", ny, 1)); CHECKED(c.at_least("frames", frames, 1));
  CHECKED(check_i420(height, width, crop, 1));
  tile_windows(height, width, crop, nx, ny, frames, windows_out);
  return 0;
} HEP_CATCH_INT

int hep_window_cameras(const float* camera, const int32_t* windows, int n, int height, int width, int crop, int resized, float* camera_out) try {
  const Check c{"hep_window_cameras: "};
  CHECKED(c.ptrs({{camera, "camera"}, {windows, "windows"}, {camera_out, "camera_out"}}));
  CHECKED(c.at_least("n", n, 1)); CHECKED(check_i420(height, width, crop, resized)); CHECKED(check_windows(c, windows, n, -1, height, width, crop));
  for (int i = 0; i < n; i++) window_camera(camera, windows + (size_t)i * 3, height, width, crop, resized, camera_out + (size_t)i * 6);
  return 0;
} HEP_CATCH_INT

int hep_window_from_box(const float* box, int ox, int oy, int height, int width, int crop, int size, int32_t* ox_out, int32_t* oy_out) try {
  const Check c{"hep_window_from_box: "};
  CHECKED(c.ptrs({{box, "box"}, {ox_out, "ox_out"}, {oy_out, "oy_out"}}));
  CHECKED(check_i420(height, width, crop, 1)); CHECKED(c.at_least("size", size, 1));
  const int32_t w[3] = {0, ox, oy};
  CHECKED(check_windows(c, w, 1, 1, height, width, crop));
  // the centre of the box in frame pixels, then the window around it
  auto centre = [&](int o, float lo, float hi) { return (double)o + 0.5 * ((double)lo + (double)hi) * (double)crop / (double)size; };
  *ox_out = window_around(centre(ox, box[0], box[2]), crop, width); *oy_out = window_around(centre(oy, box[1], box[3]), crop, height);
  return 0;
} HEP_CATCH_INT

int hep_best_window_device(const uint32_t* records, int slots, const int32_t* windows, int n, int frames, uint32_t* out_records,
                           int32_t* out_window, void* stream) try {
  const Check c{"hep_best_window_device: "};
  CHECKED(c.ptrs({{records, "records"}, {windows, "windows"}, {out_records, "out_records"}, {out_window, "out_window"}}));
  CHECKED(c.range("slots", slots, 1, 63)); CHECKED(c.at_least("n", n, 1)); CHECKED(c.range("frames", frames, 1, INT_MAX / 64));
  BestWindowArgs a; a.records = records; a.windows = windows; a.out_records = out_records; a.out_window = out_window; a.n = n; a.slots = slots; a.frames = frames;
  launch_best_window(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

int hep_rectify_windows(const float* camera, int frames, const int32_t* windows, int n, int height, int width, int crop, int resized,
                        double* table_out) try {
  const Check c{"hep_rectify_windows: "};
  CHECKED(c.ptrs({{camera, "camera"}, {windows, "windows"}, {table_out, "table_out"}}));
  CHECKED(c.at_least("frames", frames, 1)); CHECKED(c.at_least("n", n, 1)); CHECKED(check_i420(height, width, crop, resized));
  CHECKED(check_windows(c, windows, n, frames, height, width, crop)); CHECKED(check_rectify_camera(c, camera, windows, n));
  for (int i = 0; i < n; i++)
    rectify_row(camera + (size_t)windows[(size_t)i * 3] * 6, windows + (size_t)i * 3, height, width, crop, resized, table_out + (size_t)i * HEP_RECTIFY_ROW_DOUBLES);
  return 0;
} HEP_CATCH_INT

int hep_rectified_point_to_frame(const double* row, double x, double y, int height, int width, int crop, int resized, int size, double* xy_out) try {
  const Check c{"hep_rectified_point_to_frame: "};
  CHECKED(c.ptrs({{row, "row"}, {xy_out, "xy_out"}}));
  CHECKED(check_i420(height, width, crop, resized)); CHECKED(c.at_least("size", size, 1)); CHECKED(check_rectify_row(c, row));
  rectified_point(row, x, y, height, width, crop, resized, size, xy_out);
  return 0;
} HEP_CATCH_INT

int hep_window_from_box_rectified(const double* row, const float* box, int height, int width, int crop, int resized, int size, int32_t* ox_out,
                                  int32_t* oy_out) try {
  const Check c{"hep_window_from_box_rectified: "};
  CHECKED(c.ptrs({{row, "row"}, {box, "box"}, {ox_out, "ox_out"}, {oy_out, "oy_out"}}));
  CHECKED(check_i420(height, width, crop, resized)); CHECKED(c.at_least("size", size, 1)); CHECKED(check_rectify_row(c, row));
  double xy[2];
  rectified_point(row, 0.5 * ((double)box[0] + (double)box[2]), 0.5 * ((double)box[1] + (double)box[3]), height, width, crop, resized, size, xy);
  *ox_out = window_around(xy[0], crop, width); *oy_out = window_around(xy[1], crop, height);      // the window around that frame position
  return 0;
} HEP_CATCH_INT

int hep_derotate_records_device(uint32_t* records, int slots, const double* table, int n, void* stream) try {
  const Check c{"hep_derotate_records_device: "};
  CHECKED(c.ptrs({{records, "records"}, {table, "table"}}));
  CHECKED(c.range("slots", slots, 1, 63)); CHECKED(c.range("n", n, 1, INT_MAX / 64));
  DerotateArgs a; a.records = records; a.table = table; a.n = n; a.slots = slots;
  launch_derotate_records(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

int hep_pose_from_i420_windows(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                               int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels,
                               int32_t* index, float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420_windows("hep_pose_from_i420_windows: ", false, h, yuv, frames, height, width, windows, n, crop, resized, camera, score_threshold,
                                PoseOut{found, scores, labels, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

int hep_poses_from_i420_windows(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                                int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index,
                                float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420_windows("hep_poses_from_i420_windows: ", true, h, yuv, frames, height, width, windows, n, crop, resized, camera, score_threshold,
                                PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

int hep_pose_from_i420_tiled(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                             const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels, int32_t* index,
                             float* boxes, float* rotation, float* translation, float* hand, int32_t* window) try {
  return pose_from_i420_tiled("hep_pose_from_i420_tiled: ", false, h, yuv, frames, height, width, crop, resized, nx, ny, camera, score_threshold,
                              PoseOut{found, scores, labels, index, boxes, rotation, translation, hand}, window);
} HEP_CATCH_INT

int hep_poses_from_i420_tiled(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                              const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index, float* boxes,
                              float* rotation, float* translation, float* hand, int32_t* window) try {
  return pose_from_i420_tiled("hep_poses_from_i420_tiled: ", true, h, yuv, frames, height, width, crop, resized, nx, ny, camera, score_threshold,
                              PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand}, window);
} HEP_CATCH_INT

// the rectified forms of the four calls above (include/hep.h): camera is [frames,6], the centre rows, for all four
int hep_pose_from_i420_windows_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                                         int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels,
                                         int32_t* index, float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420_windows("hep_pose_from_i420_windows_rectified: ", false, h, yuv, frames, height, width, windows, n, crop, resized, camera, score_threshold,
                                PoseOut{found, scores, labels, index, boxes, rotation, translation, hand}, true);
} HEP_CATCH_INT

int hep_poses_from_i420_windows_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                                          int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index,
                                          float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420_windows("hep_poses_from_i420_windows_rectified: ", true, h, yuv, frames, height, width, windows, n, crop, resized, camera, score_threshold,
                                PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand}, true);
} HEP_CATCH_INT

int hep_pose_from_i420_tiled_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                                       const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels, int32_t* index,
                                       float* boxes, float* rotation, float* translation, float* hand, int32_t* window) try {
  return pose_from_i420_tiled("hep_pose_from_i420_tiled_rectified: ", false, h, yuv, frames, height, width, crop, resized, nx, ny, camera, score_threshold,
                              PoseOut{found, scores, labels, index, boxes, rotation, translation, hand}, window, true);
} HEP_CATCH_INT

int hep_poses_from_i420_tiled_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                                        const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index, float* boxes,
                                        float* rotation, float* translation, float* hand, int32_t* window) try {
  return pose_from_i420_tiled("hep_poses_from_i420_tiled_rectified: ", true, h, yuv, frames, height, width, crop, resized, nx, ny, camera, score_threshold,
                              PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand}, window, true);
} HEP_CATCH_INT

}  // extern "C"
