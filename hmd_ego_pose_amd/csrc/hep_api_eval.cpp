// hep_api_eval.cpp - the evaluation and visualisation side of the C ABI of libhep.so (include/hep.h), none of it taking a hep_handle: every argument check
// (hep_api_util.h: Check) precedes the first HIP call, then the kernels run on the caller's stream.  (Sessions: hep_api.cpp; training: hep_api_train.cpp.)
#include <math.h>
#include <string.h>

#include "hep_api_util.h"
#include "hep_eval.h"

using namespace hep;

static_assert(SCORE_MAX_LABELS == 63, "Check::labels (hep_api_util.h) states the kernels' label limit");

extern "C" {

// ---- pose errors (evaluator) ----
int hep_pose_errors_device(const float* points, int num_points, const float* rvec_gt, const float* t_gt, const float* rvec_pred,
                           const float* t_pred, int num_pairs, int max_points, double* add, double* add_s, void* stream) try {
  if (!points || !rvec_gt || !t_gt || !rvec_pred || !t_pred || !add || !add_s) return fail(HEP_ERR_INVALID, "bad argument");
  if (num_points < 1 || num_pairs < 0) return fail(HEP_ERR_INVALID, "num_points must be >= 1 and num_pairs >= 0");
  CHECKED(Check{""}.max_points(max_points, HEP_ERR_UNSUPPORTED));
  if (num_pairs == 0) return 0;
  PoseErrArgs a; a.points = points; a.rvec_gt = rvec_gt; a.t_gt = t_gt; a.rvec_pr = rvec_pred; a.t_pr = t_pred;
  a.add = add; a.add_s = add_s; a.P = num_points; a.D = num_pairs; a.max_points = max_points;
  launch_pose_errors(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

int hep_pose_errors(int device, const float* points, int num_points, const float* rvec_gt, const float* t_gt, const float* rvec_pred,
                    const float* t_pred, int num_pairs, int max_points, double* add, double* add_s) try {
  if (!points || !rvec_gt || !t_gt || !rvec_pred || !t_pred || !add || !add_s) return fail(HEP_ERR_INVALID, "bad argument");
  if (num_points < 1 || num_pairs < 0) return fail(HEP_ERR_INVALID, "num_points must be >= 1 and num_pairs >= 0");
  if (num_pairs == 0) return 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(HEP_ERR_DEVICE, "no HIP device visible: libhep has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(HEP_ERR_INVALID, "device index out of range");
  HIPRET(hipSetDevice(device));
  const size_t pb = (size_t)num_points * 12, db = (size_t)num_pairs * 12, ob = (size_t)num_pairs * 8;
  unsigned char* buf = nullptr;
  HIPRET(hipMalloc((void**)&buf, pb + 4 * db + 2 * ob + 64));
  struct Free { unsigned char* p; ~Free() { hipFree(p); } } guard{buf};
  float* d_pts = (float*)buf; float* d_rg = (float*)(buf + pb); float* d_tg = d_rg + 3 * num_pairs; float* d_rp = d_tg + 3 * num_pairs; float* d_tp = d_rp + 3 * num_pairs;
  double* d_add = (double*)(buf + ((pb + 4 * db + 7) & ~(size_t)7)); double* d_adds = d_add + num_pairs;
  HIPRET(hipMemcpy(d_pts, points, pb, hipMemcpyHostToDevice));
  HIPRET(hipMemcpy(d_rg, rvec_gt, db, hipMemcpyHostToDevice)); HIPRET(hipMemcpy(d_tg, t_gt, db, hipMemcpyHostToDevice));
  HIPRET(hipMemcpy(d_rp, rvec_pred, db, hipMemcpyHostToDevice)); HIPRET(hipMemcpy(d_tp, t_pred, db, hipMemcpyHostToDevice));
  if (int rc = hep_pose_errors_device(d_pts, num_points, d_rg, d_tg, d_rp, d_tp, num_pairs, max_points, d_add, d_adds, nullptr)) return rc;
  HIPRET(hipMemcpy(add, d_add, ob, hipMemcpyDeviceToHost));
  HIPRET(hipMemcpy(add_s, d_adds, ob, hipMemcpyDeviceToHost));
  return 0;
} HEP_CATCH_INT

// ---- evaluator: matching and pose metrics of a batch in one launch ----
static_assert(HEP_SCORE_GT_DOUBLES == SCORE_GT_DOUBLES && HEP_SCORE_RECORD_DOUBLES == SCORE_RECORD_DOUBLES, "the tables of include/hep.h are the kernel's");
int hep_score_detections_device(const float* det_boxes, const float* det_scores, const int32_t* det_labels, const float* det_rotation,
                                const float* det_translation, const float* det_hand, int batch, int rows, const double* gt,
                                const float* points, int num_points, int max_points, int label, float score_threshold,
                                int max_detections, double iou_threshold, double* records, float* out_scores, int32_t* out_tp,
                                void* stream) try {
  const Check c{"hep_score_detections_device: "};
  CHECKED(c.ptrs({{det_boxes, "det_boxes"}, {det_scores, "det_scores"}, {det_labels, "det_labels"}, {det_rotation, "det_rotation"},
                       {det_translation, "det_translation"}, {gt, "gt"}, {points, "points"}, {records, "records"}, {out_scores, "out_scores"},
                       {out_tp, "out_tp"}}));
  CHECKED(c.at_least("batch", batch, 1)); CHECKED(c.range("rows", rows, 1, SCORE_MAX_ROWS));
  CHECKED(c.range("max_detections", max_detections, 1, rows, HEP_ERR_INVALID, "rows"));
  CHECKED(c.at_least("num_points", num_points, 1)); CHECKED(c.max_points(max_points, HEP_ERR_INVALID));
  ScoreArgs a;
  a.boxes = det_boxes; a.scores = det_scores; a.labels = det_labels; a.rotation = det_rotation; a.translation = det_translation; a.hand = det_hand;
  a.gt = gt; a.points = points; a.records = records; a.out_scores = out_scores; a.out_tp = out_tp;
  a.B = batch; a.rows = rows; a.P = num_points; a.max_points = max_points; a.label = label; a.max_det = max_detections;
  a.score_thr = score_threshold; a.iou_thr = iou_threshold;
  launch_score(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

static_assert(HEP_SCORE_MAX_ANNOTATIONS == SCORE_MAX_ANN, "the annotation limit of include/hep.h is the kernel's");
int hep_score_scene_device(const float* det_boxes, const float* det_scores, const int32_t* det_labels, const float* det_rotation,
                           const float* det_translation, const float* det_hand, int batch, int rows, const double* gt, int amax,
                           const float* points, const int32_t* point_offsets, int num_labels, int max_points, float score_threshold,
                           int max_detections, double iou_threshold, double* records, float* out_scores, int32_t* out_tp,
                           int32_t* out_labels, int32_t* out_count, void* stream) try {
  const Check c{"hep_score_scene_device: "};
  CHECKED(c.ptrs({{det_boxes, "det_boxes"}, {det_scores, "det_scores"}, {det_labels, "det_labels"}, {det_rotation, "det_rotation"},
                       {det_translation, "det_translation"}, {gt, "gt"}, {points, "points"}, {point_offsets, "point_offsets"}, {records, "records"},
                       {out_scores, "out_scores"}, {out_tp, "out_tp"}, {out_labels, "out_labels"}, {out_count, "out_count"}}));
  CHECKED(c.at_least("batch", batch, 1)); CHECKED(c.range("rows", rows, 1, SCORE_MAX_ROWS));
  CHECKED(c.range("max_detections", max_detections, 1, rows, HEP_ERR_INVALID, "rows"));
  CHECKED(c.range("amax", amax, 1, SCORE_MAX_ANN)); CHECKED(c.labels(num_labels));
  if (point_offsets[0] != 0) return c.fail(HEP_ERR_INVALID, "point_offsets[0] must be 0");
  CHECKED(c.start_table("point_offsets", point_offsets, num_labels, INT32_MAX, 0, "point"));      // (the clouds' total length is not an argument)
  CHECKED(c.max_points(max_points, HEP_ERR_INVALID));
  SceneScoreArgs a;
  a.boxes = det_boxes; a.scores = det_scores; a.labels = det_labels; a.rotation = det_rotation; a.translation = det_translation; a.hand = det_hand;
  a.gt = gt; a.points = points; a.records = records; a.out_scores = out_scores; a.out_tp = out_tp; a.out_labels = out_labels; a.out_count = out_count;
  a.B = batch; a.rows = rows; a.amax = amax; a.num_labels = num_labels; a.max_points = max_points; a.max_det = max_detections;
  a.score_thr = score_threshold; a.iou_thr = iou_threshold;
  for (int l = 0; l <= SCORE_MAX_LABELS; l++) a.offsets[l] = l <= num_labels ? point_offsets[l] : point_offsets[num_labels];
  launch_score_scene(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

// ---- pose overlays: annotations and kept detections drawn into the frames in one launch ----
static_assert(HEP_DRAW_MAX_DETECTIONS == DRAW_MAX_DET && HEP_DRAW_BOX2D == DRAW_BOX2D && HEP_DRAW_CUBOID == DRAW_CUBOID && HEP_DRAW_HAND == DRAW_HAND,
              "the limits and layer bits of include/hep.h are the kernel's");
int hep_draw_poses_device(uint8_t* frames, int batch, int height, int width, const double* gt, int amax, const double* camera,
                          const float* det_boxes, const float* det_scores, const int32_t* det_labels, const float* det_rotation,
                          const float* det_translation, const float* det_hand, int rows, float score_threshold, int max_detections,
                          const float* cuboids, const uint8_t* colours, int num_labels, int ann_layers, int det_layers, int thickness,
                          void* stream) try {
  const Check c{"hep_draw_poses_device: "};
  CHECKED(c.ptrs({{frames, "frames"}, {cuboids, "cuboids"}, {colours, "colours"}}));
  if (!gt && !camera) return c.fail(HEP_ERR_INVALID, "gt and camera are both NULL (the camera comes from one of them)");
  CHECKED(c.at_least("batch", batch, 1)); if (gt) CHECKED(c.range("amax", amax, 1, SCORE_MAX_ANN));
  const int given = (det_boxes != nullptr) + (det_scores != nullptr) + (det_labels != nullptr) + (det_rotation != nullptr) + (det_translation != nullptr);
  if (given != 0 && given != 5)
    return c.fail(HEP_ERR_INVALID, "det_boxes, det_scores, det_labels, det_rotation and det_translation must all be given or all be NULL");
  if (given == 0 && det_hand) return c.fail(HEP_ERR_INVALID, "det_hand without the other det_* arrays");
  if (given == 5) {
    CHECKED(c.range("rows", rows, 1, SCORE_MAX_ROWS));
    CHECKED(c.range("max_detections", max_detections, 1, std::min(rows, DRAW_MAX_DET), HEP_ERR_INVALID, "min(rows, 64)"));
  }
  CHECKED(c.labels(num_labels)); CHECKED(c.range("thickness", thickness, 1, 8));
  const int all_layers = DRAW_BOX2D | DRAW_CUBOID | DRAW_HAND;
  if ((ann_layers & ~all_layers) || (det_layers & ~all_layers))
    return c.fail(HEP_ERR_INVALID, "layer bits outside HEP_DRAW_BOX2D | HEP_DRAW_CUBOID | HEP_DRAW_HAND");
  CHECKED(c.frame(height, width));
  DrawArgs a;
  a.frames = frames; a.gt = gt; a.camera = camera;
  a.boxes = det_boxes; a.scores = det_scores; a.labels = det_labels; a.rotation = det_rotation; a.translation = det_translation; a.hand = det_hand;
  a.cuboids = cuboids;
  a.B = batch; a.H = height; a.W = width; a.amax = gt ? amax : 0; a.rows = given ? rows : 0; a.max_det = given ? max_detections : 0;
  a.num_labels = num_labels; a.ann_layers = ann_layers; a.det_layers = det_layers; a.thickness = thickness; a.score_thr = score_threshold;
  memset(a.colours, 0, sizeof(a.colours));
  memcpy(a.colours, colours, (size_t)num_labels * 3);
  launch_draw(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

// ---- object models under poses: mask, depth and filled overlays from one z-buffered rasteriser ----
static_assert(HEP_RENDER_MAX_POSES == RENDER_MAX_POSES && HEP_RENDER_MAX_ELEMENTS == RENDER_MAX_ELEMS, "the limits of include/hep.h are the kernel's");
// what both entry points of the rasteriser refuse, worded once (c: the entry point's prefix); the workspace holds the vertex records, then one bounding box per (image, slot)
static int64_t render_workspace_bytes(const Check& c, int batch, int height, int width, int pmax, int num_vertices) {
  CHECKED(c.at_least("batch", batch, 1)); CHECKED(c.range("pmax", pmax, 1, RENDER_MAX_POSES));
  CHECKED(c.range("num_vertices", num_vertices, 1, RENDER_MAX_ELEMS)); CHECKED(c.frame(height, width));
  return (int64_t)batch * pmax * ((int64_t)num_vertices + 1) * (int64_t)sizeof(RenderVertex);
}
static int render_face_tables(const Check& c, int num_faces, const int32_t* face_start, int num_labels) {
  CHECKED(c.range("num_faces", num_faces, 1, RENDER_MAX_ELEMS)); CHECKED(c.labels(num_labels));
  if (face_start[0] < 0 || face_start[num_labels] > num_faces) return c.fail(HEP_ERR_INVALID, "face_start leaves 0..num_faces");
  for (int l = 0; l < num_labels; l++) if (face_start[l] > face_start[l + 1]) return c.fail(HEP_ERR_INVALID, "face_start decreases");      // (a label without faces draws nothing)
  return 0;
}

int64_t hep_render_workspace_bytes(int batch, int height, int width, int pmax, int num_vertices) try {
  return render_workspace_bytes(Check{"hep_render_models_device: "}, batch, height, width, pmax, num_vertices);      // (hep_render_models_device takes these refusals from here, with the figure)
} HEP_CATCH_INT

int hep_render_models_device(const double* poses, int batch, int pmax, const double* camera, const float* vertices, int num_vertices,
                             const int32_t* faces, int num_faces, const int32_t* face_start, int num_labels, int height, int width,
                             uint8_t* mask, float* depth, uint8_t* frames, const uint8_t* colours, int alpha,
                             void* workspace, int64_t workspace_bytes, void* stream) try {
  const Check c{"hep_render_models_device: "};
  CHECKED(c.ptrs({{poses, "poses"}, {camera, "camera"}, {vertices, "vertices"}, {faces, "faces"}, {face_start, "face_start"},
                       {workspace, "workspace"}}));
  if (!mask && !depth && !frames) return c.fail(HEP_ERR_INVALID, "mask, depth and frames are all NULL");
  const int64_t need = render_workspace_bytes(c, batch, height, width, pmax, num_vertices); if (need < 0) return (int)need;
  CHECKED(render_face_tables(c, num_faces, face_start, num_labels));
  if (frames && !colours) return c.fail(HEP_ERR_INVALID, "frames without colours");
  if (frames) CHECKED(c.range("alpha", alpha, 0, 256));
  CHECKED(c.workspace(workspace, workspace_bytes, need, "hep_render_workspace_bytes"));
  RenderArgs a;
  a.poses = poses; a.camera = camera; a.vertices = vertices; a.faces = faces; a.mask = mask; a.depth = depth; a.frames = frames;
  a.ws = (RenderVertex*)workspace;
  a.boxes = (int4*)(a.ws + (int64_t)batch * pmax * num_vertices);
  a.B = batch; a.H = height; a.W = width; a.pmax = pmax; a.V = num_vertices; a.F = num_faces; a.num_labels = num_labels; a.alpha = frames ? alpha : 0;
  memset(a.face_start, 0, sizeof(a.face_start));
  memcpy(a.face_start, face_start, (size_t)(num_labels + 1) * sizeof(int32_t));
  memset(a.colours, 0, sizeof(a.colours));
  if (frames) memcpy(a.colours, colours, (size_t)num_labels * 3);
  launch_render(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

// ---- synthetic training frames: shaded models composited over backgrounds, visible boxes and the padded annotations ----
int64_t hep_synth_workspace_bytes(int batch, int height, int width, int pmax, int num_vertices) try {
  return render_workspace_bytes(Check{"hep_synth_frames_device: "}, batch, height, width, pmax, num_vertices);
} HEP_CATCH_INT

int hep_synth_frames_device(const double* poses, int batch, int pmax, const double* camera, const float* vertices, const uint8_t* vertex_colours,
                            int num_vertices, const int32_t* faces, const double* face_normals, int num_faces, const int32_t* face_start,
                            int num_labels, const double* lights, int height, int width, uint8_t* frames, int alpha, uint8_t* mask, float* depth,
                            int32_t* visible, const float* rvec, const float* tvec, const float* extra, int min_pixels, double* boxes,
                            int32_t* labels, int32_t* mask_values, float* out_rvec, float* out_tvec, float* out_extra, int32_t* num_gt,
                            int32_t* slot_of, void* workspace, int64_t workspace_bytes, void* stream) try {
  const Check c{"hep_synth_frames_device: "};
  CHECKED(c.ptrs({{poses, "poses"}, {camera, "camera"}, {vertices, "vertices"}, {vertex_colours, "vertex_colours"}, {faces, "faces"},
                  {face_normals, "face_normals"}, {face_start, "face_start"}, {lights, "lights"}, {frames, "frames"}, {visible, "visible"},
                  {workspace, "workspace"}}));
  const void* group[11] = {rvec, tvec, extra, boxes, labels, mask_values, out_rvec, out_tvec, out_extra, num_gt, slot_of};
  int given = 0;
  for (const void* p : group) given += p != nullptr;
  if (given != 0 && given != 11) return c.fail(HEP_ERR_INVALID, "the annotation group (rvec, tvec, extra and the eight outputs) is half given: all or none");
  const int64_t need = render_workspace_bytes(c, batch, height, width, pmax, num_vertices); if (need < 0) return (int)need;
  CHECKED(render_face_tables(c, num_faces, face_start, num_labels));
  CHECKED(c.range("alpha", alpha, 0, 256)); CHECKED(c.at_least("min_pixels", min_pixels, 1));
  CHECKED(c.aligned(poses, 8, "poses")); CHECKED(c.aligned(camera, 8, "camera")); CHECKED(c.aligned(face_normals, 8, "face_normals"));
  CHECKED(c.aligned(lights, 8, "lights")); CHECKED(c.aligned(vertices, 4, "vertices")); CHECKED(c.aligned(faces, 4, "faces"));
  CHECKED(c.aligned(depth, 4, "depth")); CHECKED(c.aligned(visible, 4, "visible"));
  if (given) {
    CHECKED(c.aligned(boxes, 8, "boxes"));
    const std::pair<const void*, const char*> words[] = {{rvec, "rvec"}, {tvec, "tvec"}, {extra, "extra"}, {labels, "labels"}, {mask_values, "mask_values"},
                                                          {out_rvec, "out_rvec"}, {out_tvec, "out_tvec"}, {out_extra, "out_extra"}, {num_gt, "num_gt"}, {slot_of, "slot_of"}};
    for (const auto& w : words) CHECKED(c.aligned(w.first, 4, w.second));
  }
  CHECKED(c.workspace(workspace, workspace_bytes, need, "hep_synth_workspace_bytes"));
  SynthArgs x;
  RenderArgs& a = x.r;
  a.poses = poses; a.camera = camera; a.vertices = vertices; a.faces = faces; a.mask = mask; a.depth = depth; a.frames = frames;
  a.ws = (RenderVertex*)workspace;
  a.boxes = (int4*)(a.ws + (int64_t)batch * pmax * num_vertices);
  a.B = batch; a.H = height; a.W = width; a.pmax = pmax; a.V = num_vertices; a.F = num_faces; a.num_labels = num_labels; a.alpha = alpha;
  memset(a.face_start, 0, sizeof(a.face_start));
  memcpy(a.face_start, face_start, (size_t)(num_labels + 1) * sizeof(int32_t));
  memset(a.colours, 0, sizeof(a.colours));
  x.vertex_colours = vertex_colours; x.face_normals = face_normals; x.lights = lights; x.visible = visible;
  x.rvec = rvec; x.tvec = tvec; x.extra = extra; x.out_boxes = boxes; x.out_labels = labels; x.out_mask_values = mask_values;
  x.out_rvec = out_rvec; x.out_tvec = out_tvec; x.out_extra = out_extra; x.num_gt = num_gt; x.slot_of = slot_of; x.min_pixels = min_pixels;
  launch_synth(x, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

// ---- BOP pose errors of matched pairs: MSSD / MSPD and VSD ----
static_assert(HEP_BOP_PAIR_DOUBLES == BOP_PAIR_DOUBLES && HEP_BOP_MAX_SYMMETRIES == BOP_MAX_SYM && HEP_BOP_MAX_TAUS == BOP_MAX_TAUS,
              "the table and limits of include/hep.h are the kernel's");
int hep_bop_point_errors_device(const double* pairs, int n, const float* vertices, int num_vertices, const int32_t* vertex_start,
                                const double* symmetries, int num_symmetries, const int32_t* symmetry_start, int num_labels,
                                double* errors, void* stream) try {
  const Check c{"hep_bop_point_errors_device: "};
  CHECKED(c.ptrs({{pairs, "pairs"}, {vertices, "vertices"}, {vertex_start, "vertex_start"}, {symmetries, "symmetries"},
                       {symmetry_start, "symmetry_start"}, {errors, "errors"}}));
  CHECKED(c.at_least("n", n, 1)); CHECKED(c.labels(num_labels));
  if (num_vertices < 1 || num_symmetries < 1) return c.fail(HEP_ERR_INVALID, "num_vertices and num_symmetries must be >= 1");
  CHECKED(c.start_table("vertex_start", vertex_start, num_labels, num_vertices, 0));
  CHECKED(c.start_table("symmetry_start", symmetry_start, num_labels, num_symmetries, BOP_MAX_SYM));
  BopPointArgs a;
  a.pairs = pairs; a.vertices = vertices; a.sym = symmetries; a.out = errors; a.n = n; a.num_labels = num_labels;
  for (int l = 0; l <= SCORE_MAX_LABELS; l++) {
    a.vertex_start[l] = vertex_start[l <= num_labels ? l : num_labels];
    a.sym_start[l] = symmetry_start[l <= num_labels ? l : num_labels];
  }
  launch_bop_points(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

int64_t hep_bop_workspace_bytes(int n, int num_taus) try {
  const Check c{"hep_bop_vsd_device: "};      // (hep_bop_vsd_device takes these refusals from here, with the figure)
  CHECKED(c.at_least("n", n, 1)); CHECKED(c.range("num_taus", num_taus, 1, BOP_MAX_TAUS));
  return ((int64_t)n * (2 + num_taus) * (int64_t)sizeof(int32_t) + 15) & ~(int64_t)15;      // the counters, rounded up to the alignment
} HEP_CATCH_INT

int hep_bop_vsd_device(const double* pairs, int n, int num_labels, const float* depth_gt, const float* depth_est, const float* depth_test,
                       int num_images, int height, int width, double delta, const double* taus, int num_taus, double* vsd, int32_t* counts,
                       void* workspace, int64_t workspace_bytes, void* stream) try {
  const Check c{"hep_bop_vsd_device: "};
  CHECKED(c.ptrs({{pairs, "pairs"}, {depth_gt, "depth_gt"}, {depth_est, "depth_est"}, {taus, "taus"}, {vsd, "vsd"}, {counts, "counts"},
                       {workspace, "workspace"}}));
  const int64_t need = hep_bop_workspace_bytes(n, num_taus); if (need < 0) return (int)need;
  CHECKED(c.labels(num_labels));
  if (depth_test && num_images < 1) return c.fail(HEP_ERR_INVALID, "num_images must be >= 1 with a depth_test");
  if (!(std::isfinite(delta) && delta > 0.0)) return c.fail(HEP_ERR_INVALID, "delta must be finite and positive");
  for (int j = 0; j < num_taus; j++)
    if (!(std::isfinite(taus[j]) && taus[j] > 0.0)) return c.fail(HEP_ERR_INVALID, "tau " + std::to_string(j) + " must be finite and positive");
  CHECKED(c.workspace(workspace, workspace_bytes, need, "hep_bop_workspace_bytes")); CHECKED(c.frame(height, width));
  BopVsdArgs a;
  a.pairs = pairs; a.depth_gt = depth_gt; a.depth_est = depth_est; a.depth_test = depth_test; a.ws = (int32_t*)workspace; a.vsd = vsd; a.counts = counts;
  a.n = n; a.H = height; a.W = width; a.T = num_taus; a.images = depth_test ? num_images : 0; a.num_labels = num_labels; a.delta = delta;
  for (int j = 0; j < BOP_MAX_TAUS; j++) a.taus[j] = j < num_taus ? taus[j] : 0.0;
  launch_bop_vsd(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

}  // extern "C"
