// k_loss_grad.hip - backward of the five training losses of `batch_iterate` (reference hmdegopose/loss.py:54-428) on
// gfx950: the gradients of the four prediction tensors given an upstream gradient u[B][5] of the per-image losses (the
// forward is losses_kernel, k_eval.hip).  Semantics are what the reference's autograd returns (tests/golden/loss_grads.npz):
//   classification  d(fw * bce)/dp, p = clamp(cls, 1e-4, 1 - 1e-4) (0 outside the clamp, bounds inclusive like torch),
//                   on non-ignored anchors and labels != -1, x u0 / max(1, n_c)
//   regression/hand smooth-L1 sigma 3: 9 d for |d| <= 1/9, else sign(d) (0 at d = 0), object anchors, x u / max(1, n)
//   translation     clamp(d, -1, 1) / (3 n_t) x u3 on the object anchors (torch SmoothL1Loss, mean)
//   rotation        chain rule through the axis-angle rotation of the model points: per object anchor the sum over the
//                   points of the unit difference vector to the target point (the first nearest one for symmetric
//                   objects, the forward's distance expression), x pi u2 / (n_t P)
// Three launches, no host synchronisation, no float atomics; every output element is written exactly once:
//   1. loss_grad_count_kernel  one workgroup per image: the four normalisers and the object anchors of the
//                              transformation state compacted in anchor order (wave64 ballots + a scan of the 16 wave
//                              counts), into the caller's int32 workspace [B][4] + [B][N]
//   2. loss_grad_dense_kernel  the element-wise gradients, grid-stride over each output tensor (blockIdx.y = tensor);
//                              a non-object anchor reads its state column only and writes zeros
//   3. loss_grad_rot_kernel    the rotation columns of the object anchors: a grid (sized from the CU count) strides
//                              over the compacted list, one workgroup per anchor, the rotated target cloud in LDS; the
//                              per-anchor sums are reduced in double in a fixed order - bit-reproducible
#include <atomic>

#include "hep_dev.h"
#include "hep_train.h"
#include "loss_dev.h"

#define LG_WAVE 64              // gfx950: wave64 (the ballots below are 64-bit)
#define LG_COUNT_THREADS 1024   // 16 waves
#define LG_DENSE_THREADS 256
#define LG_ROT_THREADS 256      // 4 waves per object anchor

static_assert(LG_COUNT_THREADS / LG_WAVE <= 16, "the wave counts of the compaction are scanned by one loop of <= 16");

__global__ __launch_bounds__(LG_COUNT_THREADS) void loss_grad_count_kernel(LossGradArgs g) {
  const LossArgs& a = g.f;
  __shared__ int wave_cnt[LG_COUNT_THREADS / LG_WAVE];
  __shared__ int cnt[3];
  const int b = blockIdx.x, t = threadIdx.x, lane = t % LG_WAVE, w = t / LG_WAVE, N = a.N, K = a.K, R = a.R, H = a.H;
  const float* gc = a.gt_cls + (int64_t)b * N * (K + 1);
  const float* gr = a.gt_reg + (int64_t)b * N * 5;
  const float* gt = a.gt_tr + (int64_t)b * N * (R + 6);
  const float* gh = a.gt_hand ? a.gt_hand + (int64_t)b * N * (H + 1) : nullptr;
  int32_t* list = g.ws + (int64_t)a.B * 4 + (int64_t)b * N;
  if (t < 3) cnt[t] = 0;
  int c = 0, r = 0, h = 0, carry = 0;
  for (int base = 0; base < N; base += LG_COUNT_THREADS) {
    const int n = base + t;
    bool obj = false;
    if (n < N) {
      c += gc[(int64_t)n * (K + 1) + K] == 1.0f;
      r += gr[(int64_t)n * 5 + 4] == 1.0f;
      if (gh) h += gh[(int64_t)n * (H + 1) + H] == 1.0f;
      obj = (int)rintf(gt[(int64_t)n * (R + 6) + R + 5]) == 1;
    }
    const unsigned long long m = __ballot(obj);
    __syncthreads();                                   // wave_cnt of the previous chunk has been read
    if (lane == 0) wave_cnt[w] = __popcll(m);
    __syncthreads();
    int off = carry;
    for (int i = 0; i < w; i++) off += wave_cnt[i];
    if (obj) list[off + __popcll(m & ((1ull << lane) - 1ull))] = n;
    for (int i = 0; i < LG_COUNT_THREADS / LG_WAVE; i++) carry += wave_cnt[i];
  }
  atomicAdd(&cnt[0], c); atomicAdd(&cnt[1], r); atomicAdd(&cnt[2], h);      // integer counts: order-independent
  __syncthreads();
  if (t == 0) {
    int32_t* o = g.ws + (int64_t)b * 4;
    o[0] = cnt[0]; o[1] = cnt[1]; o[2] = carry; o[3] = cnt[2];                // n_c, n_r, n_t, n_h
  }
}

__device__ __forceinline__ float smooth_l1_sigma3_grad(float d) {
#pragma clang fp contract(off)
  return fabsf(d) <= 1.0f / 9.0f ? 9.0f * d : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
}

// d(fw * bce)/dp of the focal loss (alpha 0.25, gamma 1.5), p already inside the clamp
__device__ __forceinline__ float focal_grad(float p, float l) {
#pragma clang fp contract(off)
  const float gamma = 1.5f;
  if (l == 1.0f) return 0.25f * (gamma * powf(1.0f - p, gamma - 1.0f) * logf(p) - powf(1.0f - p, gamma) / p);
  const float bce = -(l * logf(p) + (1.0f - l) * logf(1.0f - p));
  return 0.75f * (gamma * powf(p, gamma - 1.0f) * bce + powf(p, gamma) * ((1.0f - l) / (1.0f - p) - l / p));
}

// row / column of a flat element index: 32-bit division while the tensor has fewer than 2^31 elements
__device__ __forceinline__ void split(int64_t e, int64_t total, int W, int64_t& row, int& k) {
  row = total < 0x7fffffffLL ? (int64_t)((uint32_t)e / (uint32_t)W) : e / W;
  k = (int)(e - row * W);
}

__global__ __launch_bounds__(LG_DENSE_THREADS) void loss_grad_dense_kernel(LossGradArgs g) {
#pragma clang fp contract(off)
  const LossArgs& a = g.f;
  const int N = a.N, K = a.K, R = a.R, H = a.H;
  const int64_t rows = (int64_t)a.B * N, stride = (int64_t)gridDim.x * LG_DENSE_THREADS;
  const int64_t e0 = (int64_t)blockIdx.x * LG_DENSE_THREADS + threadIdx.x;
  auto image = [&](int64_t row) { return rows < 0x7fffffffLL ? (int64_t)((uint32_t)row / (uint32_t)N) : row / N; };
  auto count = [&](int64_t row, int i) { return (float)g.ws[image(row) * 4 + i]; };
  auto up = [&](int64_t row, int i) { return g.u[image(row) * 5 + i]; };
  switch (blockIdx.y) {
    case 0: {                                          // classification [B][N][K]
      if (!g.g_cls) return;
      const int64_t total = rows * K;
      for (int64_t e = e0; e < total; e += stride) {
        int64_t row; int k; split(e, total, K, row, k);
        const float* gc = a.gt_cls + row * (K + 1);
        float v = 0.f;
        if (gc[K] != -1.0f) {
          const float l = gc[k], x = a.cls[e];
          if (l != -1.0f && x >= 1e-4f && x <= 1.0f - 1e-4f) v = focal_grad(x, l) * (up(row, 0) / fmaxf(1.0f, count(row, 0)));
        }
        g.g_cls[e] = v;
      }
      return;
    }
    case 1: {                                          // regression [B][N][4]
      if (!g.g_reg) return;
      const int64_t total = rows * 4;
      for (int64_t e = e0; e < total; e += stride) {
        int64_t row; int k; split(e, total, 4, row, k);
        const float* gr = a.gt_reg + row * 5;
        float v = 0.f;
        if (gr[4] == 1.0f) v = smooth_l1_sigma3_grad(a.reg[e] - gr[k]) * (up(row, 1) / fmaxf(1.0f, count(row, 1)));
        g.g_reg[e] = v;
      }
      return;
    }
    case 2: {                                          // transformation [B][N][R+3]: translation here, rotation of object anchors in kernel 3
      if (!g.g_tr) return;
      const int W = R + 3;
      const int64_t total = rows * W;
      for (int64_t e = e0; e < total; e += stride) {
        int64_t row; int k; split(e, total, W, row, k);
        const float* gt = a.gt_tr + row * (R + 6);
        const bool obj = (int)rintf(gt[R + 5]) == 1;
        if (obj && k < R) continue;                    // written by loss_grad_rot_kernel
        float v = 0.f;
        if (obj) v = fminf(fmaxf(a.tr[e] - gt[k], -1.0f), 1.0f) * (up(row, 3) / (count(row, 2) * 3.0f));
        g.g_tr[e] = v;
      }
      return;
    }
    default: {                                         // hand [B][N][H]
      if (!g.g_hand) return;
      const int64_t total = rows * H;
      for (int64_t e = e0; e < total; e += stride) {
        int64_t row; int k; split(e, total, H, row, k);
        const float* gh = a.gt_hand + row * (H + 1);
        float v = 0.f;
        if (gh[H] == 1.0f) v = smooth_l1_sigma3_grad(a.hand[e] - gh[k]) * (up(row, 4) / fmaxf(1.0f, count(row, 3)));
        g.g_hand[e] = v;
      }
      return;
    }
  }
}

// fixed-order sum over the workgroup (shuffle tree inside each wave, then the waves in order); thread 0 gets it
__device__ double rot_block_sum(double v, double* red) {
  for (int o = LG_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, LG_WAVE);
  __syncthreads();
  if (threadIdx.x % LG_WAVE == 0) red[threadIdx.x / LG_WAVE] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < LG_ROT_THREADS / LG_WAVE; i++) s += red[i];
  return s;
}

__global__ __launch_bounds__(LG_ROT_THREADS) void loss_grad_rot_kernel(LossGradArgs g) {
#pragma clang fp contract(off)
  const LossArgs& a = g.f;
  __shared__ float tgt[LOSS_MAX_POINTS * 3];
  __shared__ double red[LG_ROT_THREADS / LG_WAVE];
  const int t = threadIdx.x, R = a.R, P = a.P, G = gridDim.x, wg = blockIdx.x;
  const float pi = 3.14159265358979323846f;
  int base = 0;                                        // global position of image b's first object anchor
  for (int b = 0; b < a.B; b++) {
    const int cnt = g.ws[b * 4 + 2];
    const int32_t* list = g.ws + (int64_t)a.B * 4 + (int64_t)b * a.N;
    for (int i = ((wg - base) % G + G) % G; i < cnt; i += G) {
      const int64_t row = (int64_t)b * a.N + list[i];
      const float* pr = a.tr + row * (R + 3);
      const float* gt = a.gt_tr + row * (R + 6);
      const AxisAngle qp = axis_angle(pr), qt = axis_angle(gt);
      const float x = pr[0] * pi, y = pr[1] * pi, z = pr[2] * pi;
      const float theta = sqrtf((x * x + y * y) + z * z);
      const bool sym = (int)rintf(gt[R + 3]) == 1;
      const int cls = min(max((int)rintf(gt[R + 4]), 0), a.classes - 1);
      const float* pts = a.points + (int64_t)cls * P * 3;
      __syncthreads();                                 // the previous anchor's cloud has been read
      for (int j = t; j < P; j += LG_ROT_THREADS) rotate_pt(qt, pts + 3 * j, tgt + 3 * j);
      __syncthreads();
      double ga0 = 0.0, ga1 = 0.0, ga2 = 0.0, gth = 0.0;
      for (int j = t; j < P; j += LG_ROT_THREADS) {
        const float* p = pts + 3 * j;
        float o[3];
        rotate_pt(qp, p, o);
        int m = j;
        if (sym) {                                     // the first nearest target point, as fminf kept it in the forward
          float d = INFINITY;
          m = 0;
          for (int q = 0; q < P; q++) {
            const float dx = o[0] - tgt[3 * q], dy = o[1] - tgt[3 * q + 1], dz = o[2] - tgt[3 * q + 2];
            const float dq = sqrtf((dx * dx + dy * dy) + dz * dz);
            if (dq < d) { d = dq; m = q; }
          }
        }
        const float dx = o[0] - tgt[3 * m], dy = o[1] - tgt[3 * m + 1], dz = o[2] - tgt[3 * m + 2];
        const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float inv = dist > 0.0f ? 1.0f / dist : 0.0f;              // torch.norm's gradient is 0 at distance 0
        const float gx = dx * inv, gy = dy * inv, gz = dz * inv;
        const float ap = (qp.ax * p[0] + qp.ay * p[1]) + qp.az * p[2];
        const float ag = (qp.ax * gx + qp.ay * gy) + qp.az * gz;
        const float pg = (p[0] * gx + p[1] * gy) + p[2] * gz;
        const float cx = qp.ay * p[2] - qp.az * p[1], cy = qp.az * p[0] - qp.ax * p[2], cz = qp.ax * p[1] - qp.ay * p[0];
        const float apg = (cx * gx + cy * gy) + cz * gz;                   // (a x p) . g
        const float omc = 1.0f - qp.c;
        ga0 += (double)(qp.s * (p[1] * gz - p[2] * gy) + omc * (ap * gx + ag * p[0]));
        ga1 += (double)(qp.s * (p[2] * gx - p[0] * gz) + omc * (ap * gy + ag * p[1]));
        ga2 += (double)(qp.s * (p[0] * gy - p[1] * gx) + omc * (ap * gz + ag * p[2]));
        gth += (double)((-qp.s * pg + qp.c * apg) + qp.s * ap * ag);
      }
      ga0 = rot_block_sum(ga0, red); ga1 = rot_block_sum(ga1, red); ga2 = rot_block_sum(ga2, red); gth = rot_block_sum(gth, red);
      if (t == 0) {
        float* out = g.g_tr + row * (R + 3);
        const float tx = gt[0] * pi, ty = gt[1] * pi, tz = gt[2] * pi;
        const float tt = sqrtf((tx * tx + ty * ty) + tz * tz);
        if (!(theta > 0.0f) || !(tt > 0.0f)) {         // an exact-zero rotation vector: no axis, the forward's distance is NaN
          out[0] = out[1] = out[2] = 0.f;
        } else {
          // d theta / dv = a, d a / dv = (I - a a^T) / theta, v = pi r
          const double ax = qp.ax, ay = qp.ay, az = qp.az;
          const double dot = ax * ga0 + ay * ga1 + az * ga2;
          const double scale = (double)pi * ((double)g.u[b * 5 + 2] / ((double)g.ws[b * 4 + 2] * (double)P));
          out[0] = (float)(((ga0 - ax * dot) / theta + ax * gth) * scale);
          out[1] = (float)(((ga1 - ay * dot) / theta + ay * gth) * scale);
          out[2] = (float)(((ga2 - az * dot) / theta + az * gth) * scale);
        }
      }
    }
    base += cnt;
  }
}

static int cu_count() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int c = cache[dev].load();
  if (c <= 0) {
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    cache[dev].store(c);
  }
  return c;
}

void launch_losses_backward(const LossGradArgs& g, hipStream_t s) {
  const int cus = cu_count();
  hipLaunchKernelGGL(loss_grad_count_kernel, dim3(g.f.B), dim3(LG_COUNT_THREADS), 0, s, g);
  if (g.g_cls || g.g_reg || g.g_tr || g.g_hand)
    hipLaunchKernelGGL(loss_grad_dense_kernel, dim3(cus * 4, 4), dim3(LG_DENSE_THREADS), 0, s, g);
  if (g.g_tr)
    hipLaunchKernelGGL(loss_grad_rot_kernel, dim3(cus * 2), dim3(LG_ROT_THREADS), 0, s, g);
}
