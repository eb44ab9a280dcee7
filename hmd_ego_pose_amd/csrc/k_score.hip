// k_score.hip - the per-image half of the evaluator's metric loop on gfx950: match the detection rows of one image against
// its ground truth and score the matched pose, one launch per batch.  score_kernel: one annotation per image and one label, one
// workgroup per image.  score_scene_kernel (below): up to 16 annotations per image over several labels, one workgroup per
// (image, annotation slot).  Both state the scaled box, the IoU and the metrics of a pair through the same device functions.
//
// reference: evaluate_model, pytorch-sandbox/eval/common.py:866-1121 with _get_detections :419-447 (boxes /= scale,
// rotations *= pi, score > threshold, first max_detections), compute_overlap.pyx:33-73 (float64 IoU, "+1" convention),
// calc_rotation_diff :762-778, check_6d_pose_2d_reprojection :646-679, the hand error :970-982; restated on the host in
// hmd_ego_pose_amd/evaluate.py::evaluate, whose per-image decisions and roundings this kernel mirrors:
//   candidates   rows with score > threshold (float32 compare), the first max_detections of them, then label == label
//   conversion   box = float32(box) / float32(scale), rotation = float32(r) * float32(pi): float32, as numpy does them
//   matching     float64 IoU of the converted box with the ground-truth box; the first candidate with IoU >= iou_threshold
//   ADD, ADD-S   pose_error_pair (eval_dev.h, the body of pose_error_kernel) on the ground truth ROUNDED TO FLOAT32, as
//                evaluate.pose_errors feeds it: bit-identical to hep_pose_errors_device on the same pair
//   the rest     float64 on the table's float64 ground truth: |t_gt - t_pr|, the rotation angle in degrees (clamped arccos of
//                the trace), the drill tip R tip + t under both poses, the mean pinhole reprojection distance over ALL model
//                points, the mean hand-joint distance in mm
// Thread 0 walks the (at most 256) rows: the decisions are sequential by definition and a few hundred cycles long.  Whether
// the image has a match goes through LDS, so the whole workgroup takes the same side of every branch that holds a barrier.
// Sums over the points are reduced in a fixed order: the launch is bit-reproducible.
//
// Contraction: this object is built with the flags of k_eval.o (the Makefile's -ffp-contract=fast, which contracts in the
// back end whatever a pragma says) - only then does the inlined pose_error_pair round like pose_error_kernel's.  The one
// place where a fused product could flip a DECISION, the IoU, keeps its products out of the adder's reach with nofuse().
#include "hep_dev.h"
#include "hep_eval.h"
#include "eval_dev.h"

// an opaque pass through a VGPR pair: the product is rounded before the sum sees it
__device__ __forceinline__ double nofuse(double x) { asm volatile("" : "+v"(x)); return x; }

// compute_overlap of one detection box (float32 values) with the ground-truth box q (float64): 0 without intersection
__device__ __forceinline__ double score_iou(const float* bx, const double* q) {
  const double b0 = bx[0], b1 = bx[1], b2 = bx[2], b3 = bx[3];
  const double iw = fmin(b2, q[2]) - fmax(b0, q[0]) + 1.0;
  const double ih = fmin(b3, q[3]) - fmax(b1, q[1]) + 1.0;
  if (!(iw > 0 && ih > 0)) return 0.0;
  const double inter = nofuse(iw * ih);
  const double ua = nofuse((b2 - b0 + 1.0) * (b3 - b1 + 1.0)) + nofuse((q[2] - q[0] + 1.0) * (q[3] - q[1] + 1.0)) - inter;
  return inter > 0 ? inter / ua : 0.0;
}

// the detection box of one row in original-image pixels: float32(box) / float32(scale), as numpy divides it (post_filter)
__device__ __forceinline__ void score_scaled_box(const float* boxes, int64_t row, float scale, float bx[4]) {
  for (int k = 0; k < 4; k++) bx[k] = boxes[row * 4 + k] / scale;
}

// the operands of ADD / ADD-S of one pair, by one thread: gt rvec, gt t (rounded to float32), predicted rvec (x pi), predicted t
__device__ __forceinline__ void score_load_pose(float* s_pose, const double* gt, const float* rotation, const float* translation, int64_t row) {
  for (int k = 0; k < 3; k++) {
    s_pose[k] = (float)gt[5 + k]; s_pose[3 + k] = (float)gt[8 + k];
    s_pose[6 + k] = rotation[row * 3 + k] * 3.14159274f;          // np.float32(math.pi)
    s_pose[9 + k] = translation[row * 3 + k];
  }
}

// The seven metrics of one matched pair into rec[5..11], by the whole workgroup of EVAL_THREADS threads; every thread must call it
// (it holds barriers, pose_error_pair's included).  gt: the annotation's table row; s_pose: score_load_pose's 12 floats in LDS,
// written before the caller's last barrier; hand_row: the matched row's 63 floats or nullptr; rec[11] must hold NaN on entry.
__device__ __forceinline__ void score_pair_metrics(const float* points, int P, int max_points, const double* gt, const float* s_pose,
                                                   const float* hand_row, double* rec) {
  __shared__ double s_Rg[9], s_Rp[9];
  __shared__ double s_red[EVAL_THREADS];
  const int t = threadIdx.x;
  pose_error_pair(points, P, max_points, s_pose, s_pose + 3, s_pose + 6, s_pose + 9, rec + 5, rec + 6);

  // the float64 metrics: ground truth as the table holds it, the prediction's float32 values widened
  if (t == 0) rodrigues_f64(gt + 5, s_Rg);
  if (t == 64) rodrigues_f64(s_pose + 6, s_Rp);
  __syncthreads();
  const double tg[3] = {gt[8], gt[9], gt[10]};
  const double tp[3] = {(double)s_pose[9], (double)s_pose[10], (double)s_pose[11]};
  const double fx = gt[14], fy = gt[15], cx = gt[16], cy = gt[17];
  double acc = 0.0;
  for (int p = t; p < P; p += EVAL_THREADS) {
    const double x = points[3 * p], y = points[3 * p + 1], z = points[3 * p + 2];
    const double gx = (x * s_Rg[0] + y * s_Rg[1]) + z * s_Rg[2] + tg[0], gy = (x * s_Rg[3] + y * s_Rg[4]) + z * s_Rg[5] + tg[1], gz = (x * s_Rg[6] + y * s_Rg[7]) + z * s_Rg[8] + tg[2];
    const double qx = (x * s_Rp[0] + y * s_Rp[1]) + z * s_Rp[2] + tp[0], qy = (x * s_Rp[3] + y * s_Rp[4]) + z * s_Rp[5] + tp[1], qz = (x * s_Rp[6] + y * s_Rp[7]) + z * s_Rp[8] + tp[2];
    const double du = (fx * gx / gz + cx) - (fx * qx / qz + cx), dv = (fy * gy / gz + cy) - (fy * qy / qz + cy);
    acc += sqrt(du * du + dv * dv);
  }
  s_red[t] = acc;
  __syncthreads();
  for (int o = EVAL_THREADS / 2; o > 0; o >>= 1) { if (t < o) s_red[t] += s_red[t + o]; __syncthreads(); }
  if (t == 0) {
    rec[10] = s_red[0] / (double)P;
    const double dx = tg[0] - tp[0], dy = tg[1] - tp[1], dz = tg[2] - tp[2];
    rec[7] = sqrt((dx * dx + dy * dy) + dz * dz);
    double tr = 0.0;                                // trace(R_pr R_gt^T) = sum of the element-wise products
    for (int k = 0; k < 9; k++) tr += s_Rp[k] * s_Rg[k];
    tr = (tr - 1.0) / 2.0;
    rec[8] = fabs(acos(fmin(1.0, fmax(-1.0, tr))) * (180.0 / 3.141592653589793));
    const double tip[3] = {gt[11], gt[12], gt[13]};
    double s2 = 0.0;
    for (int k = 0; k < 3; k++) {
      const double g = (s_Rg[3 * k] * tip[0] + s_Rg[3 * k + 1] * tip[1]) + s_Rg[3 * k + 2] * tip[2] + tg[k];
      const double q = (s_Rp[3 * k] * tip[0] + s_Rp[3 * k + 1] * tip[1]) + s_Rp[3 * k + 2] * tip[2] + tp[k];
      s2 += (g - q) * (g - q);
    }
    rec[9] = sqrt(s2);
    if (hand_row && gt[19] != 0.0) {
      double sum = 0.0;
      for (int j = 0; j < 21; j++) {
        const double e0 = gt[20 + 3 * j] - (double)hand_row[3 * j], e1 = gt[21 + 3 * j] - (double)hand_row[3 * j + 1], e2 = gt[22 + 3 * j] - (double)hand_row[3 * j + 2];
        sum += sqrt((e0 * e0 + e1 * e1) + e2 * e2);
      }
      rec[11] = sum / 21.0 * 1000.0;
    }
  }
}

__global__ __launch_bounds__(EVAL_THREADS) void score_kernel(ScoreArgs a) {
  __shared__ int s_row;
  __shared__ float s_pose[12];
  const int b = blockIdx.x, t = threadIdx.x;
  const double* gt = a.gt + (int64_t)b * SCORE_GT_DOUBLES;
  double* rec = a.records + (int64_t)b * SCORE_RECORD_DOUBLES;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  if (t == 0) {
    const int64_t r0 = (int64_t)b * a.rows;
    float* os = a.out_scores + (int64_t)b * a.max_det;
    int32_t* ot = a.out_tp + (int64_t)b * a.max_det;
    const bool has = gt[0] != 0.0;
    const float scale = (float)gt[18];
    int cand = 0, considered = 0, m = -1;
    double m_score = nan, m_iou = nan;
    for (int r = 0; r < a.rows && cand < a.max_det; r++) {
      const float sc = a.scores[r0 + r];
      if (!(sc > a.score_thr)) continue;                           // padding (-1) and NaN are no candidates
      cand++;                                                     // the cap counts every label (post_filter), the label cut follows
      if (a.labels[r0 + r] != a.label) continue;
      float bx[4];
      score_scaled_box(a.boxes, r0 + r, scale, bx);
      const double ov = has ? score_iou(bx, gt + 1) : 0.0;
      const bool hit = has && m < 0 && ov >= a.iou_thr;
      os[considered] = sc; ot[considered] = hit ? 1 : 0;
      considered++;
      if (hit) { m = r; m_score = (double)sc; m_iou = ov; }
    }
    for (int k = considered; k < a.max_det; k++) { os[k] = -1.0f; ot[k] = -1; }
    rec[0] = (double)considered; rec[1] = m >= 0 ? 1.0 : 0.0; rec[2] = (double)m; rec[3] = m_score; rec[4] = m_iou;
    for (int k = 5; k < 12; k++) rec[k] = nan;
    for (int k = 12; k < SCORE_RECORD_DOUBLES; k++) rec[k] = 0.0;
    if (m >= 0) score_load_pose(s_pose, gt, a.rotation, a.translation, r0 + m);
    s_row = m;
  }
  __syncthreads();
  const int m = s_row;                              // uniform: decided once, read by everybody
  if (m < 0) return;
  score_pair_metrics(a.points, a.P, a.max_points, gt, s_pose, a.hand ? a.hand + ((int64_t)b * a.rows + m) * 63 : nullptr, rec);
}

void launch_score(const ScoreArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(score_kernel, dim3(a.B), dim3(EVAL_THREADS), 0, s, a);
}

// ---- several annotations per image, several labels (hep_score_scene_device) ----
// One workgroup per (image, annotation slot).  The matching of an image is sequential by definition (eval/common.py:912-1030: each row of
// label l, in row order, goes to the FIRST annotation of label l with the maximal IoU, np.argmax, and is a true positive only if that IoU
// reaches the threshold and the annotation is still free), so thread 0 of EVERY workgroup of the image repeats it - at most 256 rows x 16
// float64 IoUs - and the workgroup then scores its own annotation only: no communication between workgroups, the LDS of score_kernel.
// The workgroup of slot 0 writes the image's score / flag / label rows and its count.  Who took which annotation goes through LDS, so
// the whole workgroup leaves together when its slot is invalid or unmatched, else takes every barrier of score_pair_metrics together.
__global__ __launch_bounds__(EVAL_THREADS) void score_scene_kernel(SceneScoreArgs a) {
  __shared__ int s_row, s_label;
  __shared__ int s_alabel[SCORE_MAX_ANN], s_taken[SCORE_MAX_ANN];      // the slot's label (-1: not a valid annotation), the row that took it (-1: free)
  __shared__ float s_tscore[SCORE_MAX_ANN];
  __shared__ double s_tiou[SCORE_MAX_ANN];
  __shared__ float s_pose[12];
  const int b = blockIdx.x, slot = blockIdx.y, t = threadIdx.x;
  const double* gt0 = a.gt + (int64_t)b * a.amax * SCORE_GT_DOUBLES;   // the image's rows; row 0 carries the scale of the detection boxes
  const double* gt = gt0 + (int64_t)slot * SCORE_GT_DOUBLES;
  double* rec = a.records + ((int64_t)b * a.amax + slot) * SCORE_RECORD_DOUBLES;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  if (t == 0) {
    const int64_t r0 = (int64_t)b * a.rows;
    const bool writer = slot == 0;
    float* os = a.out_scores + (int64_t)b * a.max_det;
    int32_t* ot = a.out_tp + (int64_t)b * a.max_det;
    int32_t* ol = a.out_labels + (int64_t)b * a.max_det;
    for (int k = 0; k < a.amax; k++) {
      const double* g = gt0 + (int64_t)k * SCORE_GT_DOUBLES;
      const double lab = g[83];
      s_alabel[k] = (g[0] != 0.0 && lab >= 0.0 && lab < (double)a.num_labels) ? (int)lab : -1;      // NaN fails both compares
      s_taken[k] = -1;
    }
    const float scale = (float)gt0[18];
    int cand = 0, considered = 0;
    for (int r = 0; r < a.rows && cand < a.max_det; r++) {
      const float sc = a.scores[r0 + r];
      if (!(sc > a.score_thr)) continue;                           // padding (-1) and NaN are no candidates
      cand++;                                                     // the cap counts every label, the label cut follows
      const int l = a.labels[r0 + r];
      if (l < 0 || l >= a.num_labels) continue;
      float bx[4];
      score_scaled_box(a.boxes, r0 + r, scale, bx);
      int best = -1;
      double best_ov = 0.0;
      for (int k = 0; k < a.amax; k++) {
        if (s_alabel[k] != l) continue;
        const double ov = score_iou(bx, gt0 + (int64_t)k * SCORE_GT_DOUBLES + 1);
        if (best < 0 || ov > best_ov) { best = k; best_ov = ov; }   // the first maximum, as np.argmax
      }
      const bool hit = best >= 0 && best_ov >= a.iou_thr && s_taken[best] < 0;
      if (hit) { s_taken[best] = r; s_tscore[best] = sc; s_tiou[best] = best_ov; }
      if (writer) { os[considered] = sc; ot[considered] = hit ? 1 : 0; ol[considered] = l; }
      considered++;
    }
    if (writer) {
      for (int k = considered; k < a.max_det; k++) { os[k] = -1.0f; ot[k] = -1; ol[k] = -1; }
      a.out_count[b] = considered;
    }
    const int lab = s_alabel[slot], m = lab >= 0 ? s_taken[slot] : -1;
    rec[0] = lab >= 0 ? 1.0 : 0.0; rec[1] = m >= 0 ? 1.0 : 0.0; rec[2] = (double)m;
    rec[3] = m >= 0 ? (double)s_tscore[slot] : nan; rec[4] = m >= 0 ? s_tiou[slot] : nan;
    for (int k = 5; k < 12; k++) rec[k] = nan;
    rec[12] = (double)lab;
    for (int k = 13; k < SCORE_RECORD_DOUBLES; k++) rec[k] = 0.0;
    if (m >= 0) score_load_pose(s_pose, gt, a.rotation, a.translation, r0 + m);
    s_row = m; s_label = lab;
  }
  __syncthreads();
  const int m = s_row;                              // uniform: decided once, read by everybody
  if (m < 0) return;
  const int lab = __builtin_amdgcn_readfirstlane(s_label);      // uniform by construction; said so, the offsets stay in the kernel argument
  const int off = a.offsets[lab];
  score_pair_metrics(a.points + (int64_t)3 * off, a.offsets[lab + 1] - off, a.max_points, gt, s_pose,
                     a.hand ? a.hand + ((int64_t)b * a.rows + m) * 63 : nullptr, rec);
}

void launch_score_scene(const SceneScoreArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(score_scene_kernel, dim3(a.B, a.amax), dim3(EVAL_THREADS), 0, s, a);
}
