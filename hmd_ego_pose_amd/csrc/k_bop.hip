// k_bop.hip - the three BOP pose-error functions for matched (ground truth, estimate) pairs: MSSD and MSPD over a model's vertices and its
// set of symmetry transforms (hep_bop_point_errors_device), VSD over rendered depth maps (hep_bop_vsd_device).  The definition is the
// project's own restatement - include/hep.h states it in full, tests/_bop.py states it in numpy and the kernels reproduce it: the
// integer counts exactly, the float64 errors bit for bit up to the final sqrt.  Parity with bop_toolkit itself is UNPINNED (it is not
// part of this project's environment), as it is for cv2.  The file is built with -ffp-contract=off (Makefile): every rounding is stated.
//
//   PAIR ROW (BOP_PAIR_DOUBLES = 32 float64): 0 valid, 1 label, 2 image index, 3 reserved, 4-12 R_gt row-major, 13-15 t_gt, 16-24 R_est,
//     25-27 t_est, 28-31 fx fy cx cy.  A row is skipped (NaN outputs, counts -1) when slot 0 is 0, when the label is outside
//     0..num_labels-1 (NaN included) or when a NaN sits in slots 4-27; VSD with a depth_test also skips an image index outside 0..images-1.
//   POINT ERRORS, float64: R' = R_gt R_s, t' = R_gt t_s + t_gt, each element ((a0 b0 + a1 b1) + a2 b2) [+ t]; p = ((R0 v0 + R1 v1) + R2 v2) + t
//     under the estimate, q alike under (R', t'); mssd2(s) = max_v ((dx dx + dy dy) + dz dz), MSSD = sqrt(min_s mssd2(s)); MSPD the same on
//     u = (fx X) / Z + cx, v = (fy Y) / Z + cy with (du du + dv dv).  A vertex with not Z > 0 under the estimate or any (R', t') makes the
//     pair's MSPD NaN; a NaN squared distance makes the error it belongs to NaN.  Only max and min cross threads: the result does not
//     depend on the split.
//   VSD: see bop_vsd_kernel.
//
// bop_points_kernel: one workgroup of 256 threads per pair; the symmetries in turn, the label's vertices strided over the threads, one
//   LDS tree of (max, max, flags) per symmetry.
// bop_zero_kernel / bop_vsd_kernel / bop_finish_kernel: the caller's workspace holds int32 [n][2 + T] counters (union, intersection, cost
//   per tau), zeroed by a launch; one workgroup per (block of 2048 pixels, pair) counts in registers, adds per wave into LDS and per
//   workgroup into the workspace with vector integer atomics - integer sums: the result does not depend on the order; one thread per
//   pair then writes the counts and the T divisions.
#include "hep_dev.h"
#include "hep_eval.h"

#define BOP_THREADS 256
#define BOP_PPT 8                                                  // pixels of a thread in bop_vsd_kernel

// the row of a pair table: is it scored, and with which label
__device__ __forceinline__ bool bop_row(const double* P, int num_labels, int& lab) {
  const double l = P[1];
  if (!(P[0] != 0.0) || !(l >= 0.0 && l < (double)num_labels)) return false;      // NaN label fails
  bool nan = false;
  for (int k = 4; k < 28; k++) nan |= P[k] != P[k];
  if (nan) return false;
  lab = (int)l;
  return true;
}

__global__ __launch_bounds__(BOP_THREADS) void bop_points_kernel(BopPointArgs a) {
  __shared__ double s_m[2][BOP_THREADS];
  __shared__ int s_bad[BOP_THREADS];
  const int t = threadIdx.x;
  const double nan = __builtin_nan("");
  for (int i = blockIdx.x; i < a.n; i += gridDim.x) {
    const double* P = a.pairs + (int64_t)i * BOP_PAIR_DOUBLES;
    int lab;
    if (!bop_row(P, a.num_labels, lab)) {                         // the same for every thread
      if (t == 0) { a.out[2 * (int64_t)i] = nan; a.out[2 * (int64_t)i + 1] = nan; }
      continue;
    }
    const int v0 = a.vertex_start[lab], v1 = a.vertex_start[lab + 1];      // inside [0, num_vertices], increasing: checked on the host
    const int s0 = a.sym_start[lab], s1 = a.sym_start[lab + 1];            // inside [0, num_symmetries], increasing: checked on the host
    const double* G = P + 4;
    const double* E = P + 16;
    const double fx = P[28], fy = P[29], cx = P[30], cy = P[31];
    double best_s = __builtin_inf(), best_p = __builtin_inf();
    int bad = 0;                                                  // bit 0: a NaN squared distance, bit 1: a vertex behind the camera or a NaN pixel distance
    for (int s = s0; s < s1; s++) {
      const double* S = a.sym + (int64_t)s * 12;
      double R[9], T[3];
#pragma unroll
      for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * r + c] = (G[3 * r] * S[c] + G[3 * r + 1] * S[3 + c]) + G[3 * r + 2] * S[6 + c];
        T[r] = ((G[3 * r] * S[9] + G[3 * r + 1] * S[10]) + G[3 * r + 2] * S[11]) + G[9 + r];
      }
      double ms = 0.0, mp = 0.0;
      int b = 0;
      for (int v = v0 + t; v < v1; v += BOP_THREADS) {
        const double c0 = (double)a.vertices[3 * (int64_t)v], c1 = (double)a.vertices[3 * (int64_t)v + 1], c2 = (double)a.vertices[3 * (int64_t)v + 2];
        const double px = ((E[0] * c0 + E[1] * c1) + E[2] * c2) + E[9], py = ((E[3] * c0 + E[4] * c1) + E[5] * c2) + E[10], pz = ((E[6] * c0 + E[7] * c1) + E[8] * c2) + E[11];
        const double qx = ((R[0] * c0 + R[1] * c1) + R[2] * c2) + T[0], qy = ((R[3] * c0 + R[4] * c1) + R[5] * c2) + T[1], qz = ((R[6] * c0 + R[7] * c1) + R[8] * c2) + T[2];
        const double dx = px - qx, dy = py - qy, dz = pz - qz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 != d2) b |= 1; else if (d2 > ms) ms = d2;
        if (!(pz > 0.0) || !(qz > 0.0)) b |= 2;
        else {
          const double du = ((fx * px) / pz + cx) - ((fx * qx) / qz + cx), dv = ((fy * py) / pz + cy) - ((fy * qy) / qz + cy);
          const double e2 = du * du + dv * dv;
          if (e2 != e2) b |= 2; else if (e2 > mp) mp = e2;
        }
      }
      s_m[0][t] = ms; s_m[1][t] = mp; s_bad[t] = b;
      __syncthreads();
      for (int n = BOP_THREADS / 2; n > 0; n >>= 1) {
        if (t < n) {
          s_m[0][t] = s_m[0][t + n] > s_m[0][t] ? s_m[0][t + n] : s_m[0][t];
          s_m[1][t] = s_m[1][t + n] > s_m[1][t] ? s_m[1][t + n] : s_m[1][t];
          s_bad[t] |= s_bad[t + n];
        }
        __syncthreads();
      }
      ms = s_m[0][0]; mp = s_m[1][0]; bad |= s_bad[0];
      __syncthreads();                                            // the tree is the next symmetry's
      best_s = ms < best_s ? ms : best_s;
      best_p = mp < best_p ? mp : best_p;
    }
    if (t == 0) {                                                 // inside [0, 2 n): i < n
      a.out[2 * (int64_t)i] = (bad & 1) ? nan : sqrt(best_s);
      a.out[2 * (int64_t)i + 1] = (bad & 2) ? nan : sqrt(best_p);
    }
  }
}

void launch_bop_points(const BopPointArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bop_points_kernel, dim3(a.n), dim3(BOP_THREADS), 0, s, a);
}

// ---- VSD ----
// the row of a pair table for VSD: bop_row, and with a depth_test an image index inside 0..images-1
__device__ __forceinline__ bool bop_vsd_row(const BopVsdArgs& a, const double* P, int& img) {
  int lab;
  if (!bop_row(P, a.num_labels, lab)) return false;
  img = 0;
  if (a.depth_test) {
    const double m = P[2];
    if (!(m >= 0.0 && m < (double)a.images)) return false;        // NaN fails
    img = (int)m;
  }
  return true;
}

__global__ __launch_bounds__(BOP_THREADS) void bop_zero_kernel(BopVsdArgs a) {
  const int64_t k = (int64_t)blockIdx.x * BOP_THREADS + threadIdx.x;
  if (k < (int64_t)a.n * (2 + a.T)) a.ws[k] = 0;
}

// Per pixel (x, y) of pair i, float64, with zg, ze, zt the three depths widened (zt = 0 without a depth_test):
//   a = (x - cx) / fx, b = (y - cy) / fy, k2 = (a a + b b) + 1;  far(zm, zr, d): zm - zr > 0 and k2 ((zm - zr)(zm - zr)) > d d
//   visible(zm) = zm > 0 and (zt == 0 or not far(zm, zt, delta));  vis_gt = visible(zg);  vis_est = visible(ze) or (vis_gt and ze > 0)
//   union: vis_gt or vis_est; intersection: vis_gt and vis_est; cost(tau): intersection and k2 ((zg - ze)(zg - ze)) >= tau tau
__global__ __launch_bounds__(BOP_THREADS) void bop_vsd_kernel(BopVsdArgs a) {
  __shared__ int s_cnt[2 + BOP_MAX_TAUS];
  const int t = threadIdx.x, lane = t & 63;
  const int64_t HW = (int64_t)a.H * a.W, base = (int64_t)blockIdx.x * (BOP_THREADS * BOP_PPT);
  const double dd = a.delta * a.delta;
  double tt[BOP_MAX_TAUS];
#pragma unroll
  for (int j = 0; j < BOP_MAX_TAUS; j++) tt[j] = a.taus[j] * a.taus[j];
  for (int i = blockIdx.y; i < a.n; i += gridDim.y) {
    const double* P = a.pairs + (int64_t)i * BOP_PAIR_DOUBLES;
    int img;
    if (!bop_vsd_row(a, P, img)) continue;                        // the same for every thread
    if (t < 2 + BOP_MAX_TAUS) s_cnt[t] = 0;
    __syncthreads();
    const double fx = P[28], fy = P[29], cx = P[30], cy = P[31];
    int cnt[2 + BOP_MAX_TAUS];
#pragma unroll
    for (int j = 0; j < 2 + BOP_MAX_TAUS; j++) cnt[j] = 0;
#pragma unroll
    for (int k = 0; k < BOP_PPT; k++) {
      const int64_t p = base + t + k * BOP_THREADS;
      if (p >= HW) continue;
      const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
      const double zg = (double)a.depth_gt[(int64_t)i * HW + p], ze = (double)a.depth_est[(int64_t)i * HW + p];      // inside [0, n H W): i < n, p < H W
      const double zt = a.depth_test ? (double)a.depth_test[(int64_t)img * HW + p] : 0.0;                            // inside [0, images H W): img < images
      const double ca = ((double)x - cx) / fx, cb = ((double)y - cy) / fy;
      const double k2 = (ca * ca + cb * cb) + 1.0;
      const double dg = zg - zt, de = ze - zt;
      const bool far_g = dg <= 0.0 ? false : k2 * (dg * dg) > dd, far_e = de <= 0.0 ? false : k2 * (de * de) > dd;
      const bool vis_gt = zg > 0.0 && (zt == 0.0 || !far_g);
      const bool vis_est = (ze > 0.0 && (zt == 0.0 || !far_e)) || (vis_gt && ze > 0.0);
      const bool inter = vis_gt && vis_est;
      cnt[0] += (vis_gt || vis_est) ? 1 : 0;
      cnt[1] += inter ? 1 : 0;
      if (inter) {
        const double d = zg - ze;
        const double c = k2 * (d * d);
#pragma unroll
        for (int j = 0; j < BOP_MAX_TAUS; j++) cnt[2 + j] += (j < a.T && c >= tt[j]) ? 1 : 0;
      }
    }
#pragma unroll
    for (int j = 0; j < 2 + BOP_MAX_TAUS; j++) {
      int c = cnt[j];
      for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
      if (lane == 0 && c != 0) atomicAdd(&s_cnt[j], c);
    }
    __syncthreads();
    if (t < 2 + a.T && s_cnt[t] != 0) atomicAdd(&a.ws[(int64_t)i * (2 + a.T) + t], s_cnt[t]);      // inside [0, n (2 + T)): i < n, t < 2 + T
    __syncthreads();                                              // s_cnt is the next pair's
  }
}

__global__ __launch_bounds__(BOP_THREADS) void bop_finish_kernel(BopVsdArgs a) {
  const int i = blockIdx.x * BOP_THREADS + threadIdx.x;
  if (i >= a.n) return;
  int img;
  const bool row = bop_vsd_row(a, a.pairs + (int64_t)i * BOP_PAIR_DOUBLES, img);
  const int32_t* w = a.ws + (int64_t)i * (2 + a.T);
  int32_t* c = a.counts + (int64_t)i * (2 + a.T);
  double* o = a.vsd + (int64_t)i * a.T;
  if (!row) {
    for (int j = 0; j < 2 + a.T; j++) c[j] = -1;
    for (int j = 0; j < a.T; j++) o[j] = __builtin_nan("");
    return;
  }
  const int un = w[0], in = w[1];
  c[0] = un; c[1] = in;
  for (int j = 0; j < a.T; j++) {
    c[2 + j] = w[2 + j];
    o[j] = un == 0 ? 1.0 : (double)(w[2 + j] + (un - in)) / (double)un;
  }
}

void launch_bop_vsd(const BopVsdArgs& a, hipStream_t s) {
  const int64_t words = (int64_t)a.n * (2 + a.T), HW = (int64_t)a.H * a.W;
  hipLaunchKernelGGL(bop_zero_kernel, dim3((unsigned)((words + BOP_THREADS - 1) / BOP_THREADS)), dim3(BOP_THREADS), 0, s, a);
  const int blocks = (int)((HW + BOP_THREADS * BOP_PPT - 1) / (BOP_THREADS * BOP_PPT));
  hipLaunchKernelGGL(bop_vsd_kernel, dim3(blocks, a.n < 65535 ? a.n : 65535), dim3(BOP_THREADS), 0, s, a);
  hipLaunchKernelGGL(bop_finish_kernel, dim3((a.n + BOP_THREADS - 1) / BOP_THREADS), dim3(BOP_THREADS), 0, s, a);
}
