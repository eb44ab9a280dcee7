// grad_dev.h - the building blocks shared by the training kernels (k_head_grad.hip, k_neck_grad.hip, k_backbone_grad.hip):
// the fp32 MFMA GEMM tile and its accumulator walk, the rolling 3 x 3 window of the depthwise convs, the fixed-order
// second-pass reduce, and the small pieces around them (sigmoid, swish', the running-statistics BatchNorm load, block and
// split-K slab counts).  Each kernel keeps its own argument struct and epilogue in its own file.  The f32x4 accumulator
// type is hep_dev.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "hep_dev.h"

#define GD_THREADS 256
#define GD_BM 64
#define GD_BN 64
#define GD_BK 16
#define GD_LDS_PITCH 80      // floats: rows of a k-step land 16 banks apart (conflict-free fragment reads)
#define GD_BN_EPS 1e-3f

__device__ __forceinline__ float gd_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
// d swish(v) / d v
__device__ __forceinline__ float gd_swish_grad(float v) { const float sg = gd_sigmoid(v); return sg * (1.0f + v * (1.0f - sg)); }

// BatchNorm with running statistics: bn = gamma, beta, mean, var [4][C]
struct GDBn { float gamma, beta, mean, rstd; };
__device__ __forceinline__ GDBn gd_bn_load(const float* __restrict__ bn, int C, int c) {
  return GDBn{bn[c], bn[C + c], bn[2 * C + c], 1.0f / sqrtf(bn[3 * C + c] + GD_BN_EPS)};
}
// one fma for the scale and shift, whatever the contraction flags (what -ffp-contract=fast makes of the plain product and sum)
__device__ __forceinline__ float gd_bn_apply(const GDBn& q, float z) { return fmaf((z - q.mean) * q.rstd, q.gamma, q.beta); }

// ------------------------------------------------------------------------------------------------------------------
// GEMM tile: acc += A(i0.., k) B(k, j0..) over k in [k_begin, k_end), 64 x 64 per workgroup of 256 threads, wave wv owns
// rows 16 wv .. 16 wv + 15 and four 16-column accumulators (v_mfma_f32_16x16x4_f32).  Operand layouts:
//   GD_K_CONTIG    the operand is [row][k] (pitch ld): a thread stages (row = lane, four k)
//   GD_ROW_CONTIG  the operand is [k][row] (pitch ld): a thread stages (k, four rows)
// Edge tiles are masked at the loads (rows past I / J and k past the end read as zero).  B's row-contiguous form stops at
// kb_end, which may be below k_end (the heads' header product: A's pitch is padded, B has the real row count).
// As / Bs: the workgroup's two [GD_BK][GD_LDS_PITCH] staging arrays, 16-byte aligned.
enum { GD_K_CONTIG = 0, GD_ROW_CONTIG = 1 };
template <int LA, int LB>
__device__ __forceinline__ void gd_gemm_tile(float (&As)[GD_BK][GD_LDS_PITCH], float (&Bs)[GD_BK][GD_LDS_PITCH], f32x4 (&acc)[4],
                                             const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb,
                                             int i0, int I, int j0, int J, int k_begin, int k_end, int kb_end, int t, int lane, int wv) {
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int k0 = k_begin; k0 < k_end; k0 += GD_BK) {
    float4 va = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vb = va;
    if (LA == GD_K_CONTIG) {
      const int i = lane, kq = wv * 4;
      if (i0 + i < I && k0 + kq < k_end) va = *reinterpret_cast<const float4*>(A + (int64_t)(i0 + i) * lda + k0 + kq);
      As[kq + 0][i] = va.x; As[kq + 1][i] = va.y; As[kq + 2][i] = va.z; As[kq + 3][i] = va.w;
    } else {
      const int k = t >> 4, q = (t & 15) * 4;
      if (k0 + k < k_end && i0 + q < I) va = *reinterpret_cast<const float4*>(A + (int64_t)(k0 + k) * lda + i0 + q);
      *reinterpret_cast<float4*>(&As[k][q]) = va;
    }
    if (LB == GD_K_CONTIG) {
      const int j = lane, kq = wv * 4;
      if (j0 + j < J && k0 + kq < k_end) vb = *reinterpret_cast<const float4*>(Bm + (int64_t)(j0 + j) * ldb + k0 + kq);
      Bs[kq + 0][j] = vb.x; Bs[kq + 1][j] = vb.y; Bs[kq + 2][j] = vb.z; Bs[kq + 3][j] = vb.w;
    } else {
      const int k = t >> 4, q = (t & 15) * 4;
      if (k0 + k < kb_end && j0 + q < J) vb = *reinterpret_cast<const float4*>(Bm + (int64_t)(k0 + k) * ldb + j0 + q);
      *reinterpret_cast<float4*>(&Bs[k][q]) = vb;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GD_BK / 4; kk++) {
      const float av = As[kk * 4 + (lane >> 4)][wv * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float bv = Bs[kk * 4 + (lane >> 4)][j * 16 + (lane & 15)];
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
}

// The tile's accumulators, element by element: accumulator j, register reg is row i0 + 16 wv + 4 (lane >> 4) + reg, column
// j0 + 16 j + (lane & 15).  f(m, n, v) for every element inside I x J, columns outermost.  With col: col(n) runs once per
// column inside J (what an epilogue needs per column, e.g. its BatchNorm) and the call is f(m, n, v, col(n)).
struct GDNoCol { __device__ __forceinline__ int operator()(int) const { return 0; } };
template <class F, class Col = GDNoCol>
__device__ __forceinline__ void gd_acc_visit(const f32x4 (&acc)[4], int i0, int I, int j0, int J, int lane, int wv, F f, Col col = Col()) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int n = j0 + j * 16 + (lane & 15);
    if (n >= J) continue;
    const auto q = col(n);
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int m = i0 + wv * 16 + (lane >> 4) * 4 + reg;
      if (m >= I) continue;
      if constexpr (std::is_same<Col, GDNoCol>::value) f(m, n, acc[j][reg]);
      else f(m, n, acc[j][reg], q);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The 3 x 3 window of rows around row r = pixel (y, x) of an s x s map, zeros outside the map.  A thread that walks
// consecutive rows keeps it in registers: one new column (three loads) per step instead of nine, all nine at the start of an
// image row.  SW: the stored map is the pre-activation, the window holds swish of it.
template <bool SW> __device__ __forceinline__ void gd_win_col(float (&v)[3][3], const int j, const float* __restrict__ p, int r, int y, int x, int s, int W, int c) {
  const int xx = x + j - 1;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int yy = y + i - 1;
    float t = (yy >= 0 && yy < s && xx >= 0 && xx < s) ? p[(int64_t)(r + (i - 1) * s + (j - 1)) * W + c] : 0.0f;
    if (SW) t = t * gd_sigmoid(t);
    v[i][j] = t;
  }
}
template <bool SW> __device__ __forceinline__ void gd_win_step(float (&v)[3][3], bool fresh, const float* __restrict__ p, int r, int y, int x, int s, int W, int c) {
  if (fresh) {
    gd_win_col<SW>(v, 0, p, r, y, x, s, W, c);
    gd_win_col<SW>(v, 1, p, r, y, x, s, W, c);
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) { v[i][0] = v[i][1]; v[i][1] = v[i][2]; }
  }
  gd_win_col<SW>(v, 2, p, r, y, x, s, W, c);
}

// depthwise 3 x 3 forward on rows: a thread = (GD_DW_ROWS consecutive rows, channel)
#define GD_DW_ROWS 4
__device__ __forceinline__ void gd_dw_taps(float (&w)[9], const float* __restrict__ wdw, int c) {
#pragma unroll
  for (int tp = 0; tp < 9; tp++) w[tp] = wdw[c * 9 + tp];
}
__device__ __forceinline__ float gd_dw_dot(const float (&w)[9], const float (&v)[3][3]) {
  float acc = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) acc = fmaf(w[i * 3 + j], v[i][j], acc);
  return acc;
}

// ------------------------------------------------------------------------------------------------------------------
// Second pass over partial sums: a gradient element is the sum of its partials src[k * stride], k in [k0, k1), added in
// double in a FIXED order.  A workgroup = 16 consecutive elements (el) x 16 partial lanes (kl): lane kl adds the partials
// k0 + kl, k0 + kl + 16, ... in index order, then lane 0 adds the 16 sums in order 0..15 and rounds once; it alone gets the
// sum.  src == NULL: no partials, zero.  Every thread of the workgroup calls it (it synchronises).
#define GD_RED_E 16
#define GD_RED_K 16
static_assert(GD_RED_E * GD_RED_K == GD_THREADS, "one reduce workgroup = 16 elements x 16 partial lanes");
__device__ __forceinline__ float gd_reduce_core(const float* __restrict__ src, int64_t stride, int k0, int k1, int el, int kl) {
  __shared__ double part[GD_RED_K][GD_RED_E + 1];
  double s = 0.0;
  if (src)
    for (int k = k0 + kl; k < k1; k += GD_RED_K) s += (double)src[k * stride];
  part[kl][el] = s;
  __syncthreads();
  double t = 0.0;
  if (kl == 0) {
#pragma unroll
    for (int j = 0; j < GD_RED_K; j++) t += part[j][el];
  }
  return (float)t;
}

// A list of reduce jobs in one launch (blockIdx.y = job): element e of a job = the sum of src[e + k * stride], k < nparts.
// src == NULL: the element is zero (running statistics).
struct GDRedJob { const float* src; float* dst; int64_t count, stride; int nparts; };
template <int NJOBS> struct GDReduceArgs { GDRedJob j[NJOBS]; };
template <int NJOBS> __global__ __launch_bounds__(GD_THREADS) void gd_reduce_kernel(GDReduceArgs<NJOBS> a) {
  const GDRedJob& job = a.j[blockIdx.y];
  const int el = threadIdx.x % GD_RED_E, kl = threadIdx.x / GD_RED_E;
  const int64_t e = (int64_t)blockIdx.x * GD_RED_E + el;
  if ((int64_t)blockIdx.x * GD_RED_E >= job.count) return;  // uniform over the workgroup
  const bool live = e < job.count;
  const float v = gd_reduce_core(live && job.src ? job.src + e : nullptr, job.stride, 0, job.nparts, el, kl);
  if (kl == 0 && live) job.dst[e] = v;
}

// ------------------------------------------------------------------------------------------------------------------
// host side
static inline unsigned gd_blocks(int64_t n) { return (unsigned)((n + GD_THREADS - 1) / GD_THREADS); }
// split-K of a weight-gradient product over R rows: about 512 rows per slab, at most max_slabs, slabs a multiple of GD_BK
static inline void gd_slabs(int R, int max_slabs, int* slab_rows, int* nslab) {
  int ns = R / 512; if (ns < 1) ns = 1; if (ns > max_slabs) ns = max_slabs;
  *slab_rows = ((R + ns - 1) / ns + GD_BK - 1) / GD_BK * GD_BK;
  *nslab = (R + *slab_rows - 1) / *slab_rows;
}
