// eval_dev.h - the ADD / ADD-S arithmetic of one (ground truth, prediction) pose pair as device functions: the body of
// pose_error_kernel (k_eval.hip), shared with score_kernel (k_score.hip) so that both kernels run the same statements in
// the same order.  See k_eval.hip for the definition and the reference lines.
// The contract(off) pragma below is the one pose_error_kernel has always carried; the library's -ffp-contract=fast contracts
// in the back end all the same (Makefile), so these statements run with fused multiply-adds, in both kernels alike: the two
// objects are built with the same flags, and that is what makes their ADD / ADD-S bit-identical.
#pragma once
#include "hep_dev.h"

#define EVAL_THREADS 256
#define EVAL_MAX_SUB 1024

// Rodrigues: R = cos(th) I + (1 - cos(th)) k k^T + sin(th) [k]x, th = |r|, k = r / th; identity below 1e-12
// (T = float: the operands of ADD / ADD-S; T = double: the float64 ground truth of the other metrics)
template <typename T>
__device__ void rodrigues_f64(const T* rv, double R[9]) {
  const double x = rv[0], y = rv[1], z = rv[2];
  const double th = sqrt(x * x + y * y + z * z);
  if (th < 1e-12) { for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
  const double kx = x / th, ky = y / th, kz = z / th, c = cos(th), s = sin(th), v = 1.0 - c;
  R[0] = c + v * kx * kx;      R[1] = v * kx * ky - s * kz; R[2] = v * kx * kz + s * ky;
  R[3] = v * ky * kx + s * kz; R[4] = c + v * ky * ky;      R[5] = v * ky * kz - s * kx;
  R[6] = v * kz * kx - s * ky; R[7] = v * kz * ky + s * kx; R[8] = c + v * kz * kz;
}

// ADD and ADD-S of ONE pose pair by the whole workgroup of EVAL_THREADS threads; every thread must call it (it holds
// barriers).  rvec_* / t_*: 3 floats each, in global memory or LDS.  Thread 0 stores the two results.
__device__ __forceinline__ void pose_error_pair(const float* points, int P, int max_points, const float* rvec_gt, const float* t_gt,
                                                const float* rvec_pr, const float* t_pr, double* add, double* add_s) {
#pragma clang fp contract(off)
  __shared__ double Rg[9], Rp[9], tg[3], tp[3];
  __shared__ float sub_g[EVAL_MAX_SUB][3], sub_p[EVAL_MAX_SUB][3];
  __shared__ double red[EVAL_THREADS];
  const int t = threadIdx.x;
  if (t == 0) { rodrigues_f64(rvec_gt, Rg); for (int i = 0; i < 3; i++) tg[i] = t_gt[i]; }
  if (t == 64) { rodrigues_f64(rvec_pr, Rp); for (int i = 0; i < 3; i++) tp[i] = t_pr[i]; }
  __syncthreads();
  const int step = P / max_points + 1, nsub = (P + step - 1) / step;
  double acc = 0.0;
  for (int p = t; p < P; p += EVAL_THREADS) {
    const double x = points[3 * p], y = points[3 * p + 1], z = points[3 * p + 2];
    // np.dot(points, R.T) + t: row-vector times R^T = R applied to the point, accumulated x, y, z in order
    const double gx = (x * Rg[0] + y * Rg[1]) + z * Rg[2] + tg[0], gy = (x * Rg[3] + y * Rg[4]) + z * Rg[5] + tg[1], gz = (x * Rg[6] + y * Rg[7]) + z * Rg[8] + tg[2];
    const double qx = (x * Rp[0] + y * Rp[1]) + z * Rp[2] + tp[0], qy = (x * Rp[3] + y * Rp[4]) + z * Rp[5] + tp[1], qz = (x * Rp[6] + y * Rp[7]) + z * Rp[8] + tp[2];
    const double dx = gx - qx, dy = gy - qy, dz = gz - qz;
    acc += sqrt((dx * dx + dy * dy) + dz * dz);
    if (p % step == 0) {
      const int i = p / step;
      sub_g[i][0] = (float)gx; sub_g[i][1] = (float)gy; sub_g[i][2] = (float)gz;
      sub_p[i][0] = (float)qx; sub_p[i][1] = (float)qy; sub_p[i][2] = (float)qz;
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int o = EVAL_THREADS / 2; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
  if (t == 0) *add = red[0] / (double)P;
  __syncthreads();
  // ADD-S: float arithmetic exactly as calc_min_distances.h (the minimum of the squared distances first: the
  // final (float) sqrt((double) .) is monotone, so the minimum commutes with it)
  double sacc = 0.0;
  for (int i = t; i < nsub; i += EVAL_THREADS) {
    const float gx = sub_g[i][0], gy = sub_g[i][1], gz = sub_g[i][2];
    float best = 3.4e38f;
    for (int j = 0; j < nsub; j++) {
      const float d1 = gx - sub_p[j][0], d2 = gy - sub_p[j][1], d3 = gz - sub_p[j][2];
      const float s2 = d1 * d1 + d2 * d2 + d3 * d3;
      best = fminf(best, s2);
    }
    sacc += (double)(float)sqrt((double)best);
  }
  red[t] = sacc;
  __syncthreads();
  for (int o = EVAL_THREADS / 2; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
  if (t == 0) *add_s = red[0] / (double)nsub;
}
