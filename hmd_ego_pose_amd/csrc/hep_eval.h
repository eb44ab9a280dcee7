// hep_eval.h - launch arguments, limits and launch functions of the stateless evaluation and visualisation toolkit (hep_api_eval.cpp; k_eval.hip's
// pose errors, k_score.hip, k_draw.hip, k_render.hip, k_bop.hip).  Plan and session: hep_internal.h; training: hep_train.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- pose errors: ADD / ADD-S of D pose pairs over P model points (eval/common.py:682-746) ----
struct PoseErrArgs {
  const float* points;                       // [P,3]
  const float* rvec_gt; const float* t_gt;   // [D,3] axis-angle (radians), [D,3]
  const float* rvec_pr; const float* t_pr;
  double* add; double* add_s;                // [D]
  int P, D, max_points;                      // max_points: 1000 in the reference (ADD-S subsampling)
};
void launch_pose_errors(const PoseErrArgs&, hipStream_t);

// ---- evaluator: per-image matching + all pose metrics of the matched pair (k_score.hip; eval/common.py:866-1121) ----
#define SCORE_GT_DOUBLES 88          // HEP_SCORE_GT_DOUBLES
#define SCORE_RECORD_DOUBLES 16      // HEP_SCORE_RECORD_DOUBLES
#define SCORE_MAX_ROWS 256
struct ScoreArgs {
  const float* boxes; const float* scores; const int32_t* labels;      // [B][rows][4|1|1], the rows of the detection filter
  const float* rotation; const float* translation; const float* hand;  // [B][rows][3|3|63]; hand nullable
  const double* gt;                                                    // [B][SCORE_GT_DOUBLES]
  const float* points;                                                 // [P,3]
  double* records; float* out_scores; int32_t* out_tp;                 // [B][SCORE_RECORD_DOUBLES], [B][max_det], [B][max_det]
  int B, rows, P, max_points, label, max_det;
  float score_thr; double iou_thr;
};
void launch_score(const ScoreArgs&, hipStream_t);
// several annotations per image, several labels (score_scene_kernel): gt and records gain the annotation-slot axis
#define SCORE_MAX_ANN 16             // HEP_SCORE_MAX_ANNOTATIONS
#define SCORE_MAX_LABELS 63
struct SceneScoreArgs {
  const float* boxes; const float* scores; const int32_t* labels;      // [B][rows][4|1|1]
  const float* rotation; const float* translation; const float* hand;  // [B][rows][3|3|63]; hand nullable
  const double* gt;                                                    // [B][amax][SCORE_GT_DOUBLES], slot 83 = label
  const float* points;                                                 // the clouds of all labels, concatenated
  double* records;                                                     // [B][amax][SCORE_RECORD_DOUBLES]
  float* out_scores; int32_t* out_tp; int32_t* out_labels; int32_t* out_count;      // [B][max_det] x 3, [B]
  int B, rows, amax, num_labels, max_points, max_det;
  float score_thr; double iou_thr;
  int32_t offsets[SCORE_MAX_LABELS + 1];                               // label l owns points [offsets[l], offsets[l+1]); checked on the host
};
void launch_score_scene(const SceneScoreArgs&, hipStream_t);

// ---- pose overlays: annotations and kept detections drawn into uint8 frames in place (k_draw.hip; eval/common.py:452-479) ----
#define DRAW_MAX_DET 64              // HEP_DRAW_MAX_DETECTIONS
#define DRAW_BOX2D 1                 // HEP_DRAW_BOX2D / _CUBOID / _HAND
#define DRAW_CUBOID 2
#define DRAW_HAND 4
struct DrawArgs {
  uint8_t* frames;                                                     // [B][H][W][3]
  const double* gt;                                                    // [B][amax][SCORE_GT_DOUBLES], nullable
  const double* camera;                                                // [B][5] fx, fy, cx, cy, scale; nullable when gt is given
  const float* boxes; const float* scores; const int32_t* labels;      // [B][rows][4|1|1]; all five required ones, or none
  const float* rotation; const float* translation; const float* hand;  // [B][rows][3|3|63]; hand nullable
  const float* cuboids;                                                // [num_labels][8][3]
  int B, H, W, amax, rows, max_det, num_labels, ann_layers, det_layers, thickness;
  float score_thr;
  uint8_t colours[SCORE_MAX_LABELS * 3 + 3];                           // [num_labels][3], copied from the host
};
void launch_draw(const DrawArgs&, hipStream_t);

// ---- object models rendered under poses: mask, depth and filled overlays from one z-buffered rasteriser (k_render.hip) ----
#define RENDER_MAX_POSES 16          // HEP_RENDER_MAX_POSES
#define RENDER_MAX_ELEMS (1 << 24)   // HEP_RENDER_MAX_ELEMENTS: vertices and faces; a face index fits the 24 low bits of a winner's key
struct RenderVertex { int32_t sx, sy; double w; };                     // sub-pixel coordinates, 1 / Z; w < 0: invalid
static_assert(sizeof(RenderVertex) == 16 && sizeof(int4) == 16, "the workspace holds 16 bytes per (image, slot, vertex) and per (image, slot)");
struct RenderArgs {
  const double* poses;                                                 // [B][pmax][16]
  const double* camera;                                                // [B][5] fx, fy, cx, cy, (scale)
  const float* vertices; const int32_t* faces;                         // [V][3], [F][3]
  uint8_t* mask; float* depth; uint8_t* frames;                        // [B][H][W], [B][H][W], [B][H][W][3]; each nullable, not all
  RenderVertex* ws;                                                    // [B][pmax][V]
  int4* boxes;                                                         // [B][pmax] sub-pixel x0, y0, x1, y1 of a slot's valid vertices, behind ws
  int B, H, W, pmax, V, F, num_labels, alpha;
  int32_t face_start[SCORE_MAX_LABELS + 1];                            // label l owns faces [face_start[l], face_start[l+1]); checked on the host
  uint8_t colours[SCORE_MAX_LABELS * 3 + 3];                           // [num_labels][3], copied from the host (zeros without frames)
};
void launch_render(const RenderArgs&, hipStream_t);

// ---- synthetic training frames: the same rasteriser with the winning fragment shaded, composited and boxed (k_render.hip) ----
#define SYNTH_LIGHT_DOUBLES 8        // lx, ly, lz, ambient, diffuse, gain0, gain1, gain2
#define SYNTH_VISIBLE_INTS 5         // min_x, min_y, max_x, max_y, count
struct SynthArgs {
  RenderArgs r;                                                        // frames required, colours unused
  const uint8_t* vertex_colours;                                       // [V][3]
  const double* face_normals;                                          // [F][3], plain data: a zero vector is legal
  const double* lights;                                                // [B][SYNTH_LIGHT_DOUBLES]
  int32_t* visible;                                                    // [B][pmax][SYNTH_VISIBLE_INTS], initialised by the bounds launch
  // the annotation group, all given or all NULL: gathered inputs [B][pmax][3|3|2] and the compacted outputs in augment.pad_annotations' layout
  const float* rvec; const float* tvec; const float* extra;
  double* out_boxes; int32_t* out_labels; int32_t* out_mask_values;    // [B][pmax][4], [B][pmax], [B][pmax]
  float* out_rvec; float* out_tvec; float* out_extra;                  // [B][pmax][3|3|2]
  int32_t* num_gt; int32_t* slot_of;                                   // [B], [B][pmax]
  int min_pixels;
};
void launch_synth(const SynthArgs&, hipStream_t);

// ---- BOP pose errors of matched pairs: MSSD / MSPD over vertices and symmetries, VSD over rendered depth maps (k_bop.hip) ----
#define BOP_PAIR_DOUBLES 32          // HEP_BOP_PAIR_DOUBLES
#define BOP_MAX_SYM 64               // HEP_BOP_MAX_SYMMETRIES
#define BOP_MAX_TAUS 16              // HEP_BOP_MAX_TAUS
struct BopPointArgs {
  const double* pairs;                                                 // [n][BOP_PAIR_DOUBLES]
  const float* vertices;                                               // [V][3]
  const double* sym;                                                   // [S_total][12] R row-major, t
  double* out;                                                         // [n][2] MSSD, MSPD
  int n, num_labels;
  int32_t vertex_start[SCORE_MAX_LABELS + 1];                          // label l owns vertices [vertex_start[l], vertex_start[l+1]); checked on the host
  int32_t sym_start[SCORE_MAX_LABELS + 1];                             // ... and symmetries [sym_start[l], sym_start[l+1]), 1..BOP_MAX_SYM of them
};
void launch_bop_points(const BopPointArgs&, hipStream_t);
struct BopVsdArgs {
  const double* pairs;                                                 // [n][BOP_PAIR_DOUBLES]
  const float* depth_gt; const float* depth_est;                       // [n][H][W]
  const float* depth_test;                                             // [images][H][W], nullable
  int32_t* ws;                                                         // [n][2 + T] union, intersection, cost per tau
  double* vsd; int32_t* counts;                                        // [n][T], [n][2 + T]
  int n, H, W, T, images, num_labels;
  double delta;
  double taus[BOP_MAX_TAUS];                                           // copied from the host, zeros behind T
};
void launch_bop_vsd(const BopVsdArgs&, hipStream_t);
