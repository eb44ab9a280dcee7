// grad_dev.h - the building blocks shared by the training kernels (k_head_grad.hip, k_neck_grad.hip, k_backbone_grad.hip):
// the fp32 MFMA GEMM tile and its accumulator walk, the rolling 3 x 3 window of the depthwise convs, the fixed-order
// second-pass reduce, the batch-statistics BatchNorm passes, and the small pieces around them (sigmoid, swish', the BatchNorm
// table load, block and split-K slab counts).  Each kernel keeps its own argument struct and epilogue in its own file.  The f32x4 accumulator
// type is hep_dev.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "hep_dev.h"
#include "hep_train.h"

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
// gd_reduce_core_d: the same walk over partials of type T (float or double), the sum before its rounding.
template <class T> __device__ __forceinline__ double gd_reduce_core_d(const T* __restrict__ src, int64_t stride, int k0, int k1, int el, int kl) {
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
  return t;
}
__device__ __forceinline__ float gd_reduce_core(const float* __restrict__ src, int64_t stride, int k0, int k1, int el, int kl) {
  return (float)gd_reduce_core_d(src, stride, k0, k1, el, kl);
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
// Batch-statistics BatchNorm (F.batch_norm(training=True)), shared by the three parts.  One job = one BatchNorm = the rows
// [R][C] of its pre-BatchNorm map z (R = the rows it sees: batch * s * s; in the heads one level); blockIdx.y = job.
//   forward   the producing epilogue stores z only;  stats (per (row tile, channel) the sums of z and z^2, in double, a thread
//             walks its tile in row order);  finish (fixed-order second pass, mean and biased variance in double, the EFFECTIVE
//             table gamma, beta, mean, var [4][C] in the layout gd_bn_load reads, the running-statistics update);  apply (z -> a)
//   backward  every consumer reads the effective table instead of the parameters: that gives x^ and d a, the "frozen"
//             d z = d a gamma rstd and the partials of d beta = sum d a, d gamma = sum d a x^;  once their reduce has run, dz adds
//             - gamma rstd (d beta + x^ d gamma) / R in place, before any product reads d z.
// The variance is (sum z^2 - mean sum z) / R of double sums: no float32 cancellation.
struct GDBnJob {
  const float* z;        // pre-BatchNorm rows [R][C]
  const float* bn;       // the parameters' gamma, beta, running_mean, running_var [4][C]
  float* eff;            // the effective table [4][C] (workspace)
  float* stats;          // this BatchNorm's [4][C] in the statistics output: rows 2 and 3 get the new running statistics, rows 0 and 1
                         // stay untouched; NULL: no update
  double* part;          // [tiles][C][2]
  float* io;             // apply: the output rows;  dz: the d z rows, corrected in place
  const float* dbn;      // dz: the reduced d gamma, d beta [2][C]
  const float* res; const float* scale;   // apply GD_BN_SCALE_SKIP: the rows to add, the per-image scale of bn(z) (NULL: 1); images of ss rows
  int R, C, ss;
  // synchronised statistics only (GDSync below): this BatchNorm's slice [2 C + 2] of the exchange block; the float partials
  // [pn][pstride] of d gamma and d beta that the part's own reduce reads (the same partials, the same order)
  double* xch;
  const float* pg; const float* pb; int pn, pstride;
};
template <int NJOBS> struct GDBnArgs { GDBnJob j[NJOBS]; int tile_rows; float momentum; };

// thread = (row tile, channel): channels contiguous, a wave reads 256 consecutive bytes of every row
template <int NJOBS> __global__ __launch_bounds__(GD_THREADS) void gd_bn_stats_kernel(GDBnArgs<NJOBS> a) {
  const GDBnJob& j = a.j[blockIdx.y];
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int tile = (int)(gid / j.C), c = (int)(gid % j.C);
  const int64_t r0 = (int64_t)tile * a.tile_rows;
  if (r0 >= j.R) return;
  const int r1 = (int)min((int64_t)j.R, r0 + a.tile_rows);
  double s = 0.0, q = 0.0;
  for (int r = (int)r0; r < r1; r++) {
    const double v = (double)j.z[(int64_t)r * j.C + c];
    s += v; q = fma(v, v, q);
  }
  j.part[((int64_t)tile * j.C + c) * 2] = s;
  j.part[((int64_t)tile * j.C + c) * 2 + 1] = q;
}

// mean, biased variance, the effective table and the running-statistics update of channel c from the sums s = sum z, q = sum z^2
// over n rows, all in double (one body for the local and the synchronised finish: the same sums give the same bits)
__device__ __forceinline__ void gd_bn_finish_write(const GDBnJob& j, int c, double s, double q, double n, float momentum) {
  const int C = j.C;
  const double mean = s / n, var = fmax((q - mean * s) / n, 0.0);
  j.eff[c] = j.bn[c]; j.eff[C + c] = j.bn[C + c]; j.eff[2 * C + c] = (float)mean; j.eff[3 * C + c] = (float)var;
  if (j.stats) {
    const double m = (double)momentum;
    j.stats[2 * C + c] = (float)((1.0 - m) * (double)j.bn[2 * C + c] + m * mean);
    j.stats[3 * C + c] = (float)((1.0 - m) * (double)j.bn[3 * C + c] + m * (var * n / (n - 1.0)));
  }
}

// workgroup = 16 channels x 16 partial lanes (gd_reduce_core_d, twice).  SYNC: the sums and the row count go to the job's
// slice of the exchange block instead (sum z [C], sum z^2 [C], R, 0), the finish waits for the other replicas' (below)
template <int NJOBS, bool SYNC = false> __global__ __launch_bounds__(GD_THREADS) void gd_bn_finish_kernel(GDBnArgs<NJOBS> a) {
  const GDBnJob& j = a.j[blockIdx.y];
  const int el = threadIdx.x % GD_RED_E, kl = threadIdx.x / GD_RED_E, C = j.C;
  if ((int)blockIdx.x * GD_RED_E >= C) return;              // uniform over the workgroup
  const int c = blockIdx.x * GD_RED_E + el;
  const bool live = c < C;
  const int tiles = (j.R + a.tile_rows - 1) / a.tile_rows;
  const double s = gd_reduce_core_d(live ? j.part + 2 * c : nullptr, (int64_t)2 * C, 0, tiles, el, kl);
  __syncthreads();                                          // the first sum is read before the second reuses the staging array
  const double q = gd_reduce_core_d(live ? j.part + 2 * c + 1 : nullptr, (int64_t)2 * C, 0, tiles, el, kl);
  if (kl != 0 || !live) return;
  if (SYNC) {
    j.xch[c] = s; j.xch[C + c] = q;
    if (c == 0) { j.xch[2 * C] = (double)j.R; j.xch[2 * C + 1] = 0.0; }
  } else {
    gd_bn_finish_write(j, c, s, q, (double)j.R, a.momentum);
  }
}
// the finish over the GLOBAL sums and row count of the exchange block; thread = channel
template <int NJOBS> __global__ __launch_bounds__(GD_THREADS) void gd_bn_sync_finish_kernel(GDBnArgs<NJOBS> a) {
  const GDBnJob& j = a.j[blockIdx.y];
  const int c = blockIdx.x * GD_THREADS + threadIdx.x, C = j.C;
  if (c >= C) return;
  gd_bn_finish_write(j, c, j.xch[c], j.xch[C + c], j.xch[2 * C], a.momentum);
}

// a = bn(z) with the effective table, then nothing | swish(a) | a * scale[image] + res; thread = (GD_DW_ROWS consecutive rows, channel)
enum { GD_BN_PLAIN = 0, GD_BN_SWISH = 1, GD_BN_SCALE_SKIP = 2 };
template <int NJOBS, int EPI> __global__ __launch_bounds__(GD_THREADS) void gd_bn_apply_kernel(GDBnArgs<NJOBS> a) {
  const GDBnJob& j = a.j[blockIdx.y];
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int64_t ra = gid / j.C * GD_DW_ROWS;
  const int c = (int)(gid % j.C);
  if (ra >= j.R) return;
  const int rb = (int)min((int64_t)j.R, ra + GD_DW_ROWS);
  const GDBn q = gd_bn_load(j.eff, j.C, c);
  for (int r = (int)ra; r < rb; r++) {
    float act = gd_bn_apply(q, j.z[(int64_t)r * j.C + c]);
    if (EPI == GD_BN_SWISH) act = act * gd_sigmoid(act);
    if (EPI == GD_BN_SCALE_SKIP) act = fmaf(act, j.scale ? j.scale[r / j.ss] : 1.0f, j.res[(int64_t)r * j.C + c]);
    j.io[(int64_t)r * j.C + c] = act;
  }
}

// d z -= gamma rstd (d beta + x^ d gamma) / R; thread = (GD_DW_ROWS consecutive rows, channel).  SYNC: the global sums (rounded
// once, here) and the global row count of the exchange block
template <int NJOBS, bool SYNC = false> __global__ __launch_bounds__(GD_THREADS) void gd_bn_dz_kernel(GDBnArgs<NJOBS> a) {
  const GDBnJob& j = a.j[blockIdx.y];
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int64_t ra = gid / j.C * GD_DW_ROWS;
  const int c = (int)(gid % j.C);
  if (ra >= j.R) return;
  const int rb = (int)min((int64_t)j.R, ra + GD_DW_ROWS);
  const GDBn q = gd_bn_load(j.eff, j.C, c);
  const float dg = SYNC ? (float)j.xch[c] : j.dbn[c], db = SYNC ? (float)j.xch[j.C + c] : j.dbn[j.C + c];
  const float k = q.gamma * q.rstd / (SYNC ? (float)j.xch[2 * j.C] : (float)j.R);
  for (int r = (int)ra; r < rb; r++) {
    const float zh = (j.z[(int64_t)r * j.C + c] - q.mean) * q.rstd;
    j.io[(int64_t)r * j.C + c] = fmaf(-k, fmaf(zh, dg, db), j.io[(int64_t)r * j.C + c]);
  }
}
// this replica's d gamma, d beta [C] before their rounding to float, and its row count, into the job's slice of the exchange
// block: the walk of the part's own reduce over the same partials (gd_reduce_core_d); workgroup = 16 channels x 16 partial lanes
template <int NJOBS> __global__ __launch_bounds__(GD_THREADS) void gd_bn_sync_dsums_kernel(GDBnArgs<NJOBS> a) {
  const GDBnJob& j = a.j[blockIdx.y];
  const int el = threadIdx.x % GD_RED_E, kl = threadIdx.x / GD_RED_E, C = j.C;
  if ((int)blockIdx.x * GD_RED_E >= C) return;              // uniform over the workgroup
  const int c = blockIdx.x * GD_RED_E + el;
  const bool live = c < C;
  const double dg = gd_reduce_core_d(live ? j.pg + c : nullptr, (int64_t)j.pstride, 0, j.pn, el, kl);
  __syncthreads();
  const double db = gd_reduce_core_d(live ? j.pb + c : nullptr, (int64_t)j.pstride, 0, j.pn, el, kl);
  if (kl != 0 || !live) return;
  j.xch[c] = dg; j.xch[C + c] = db;
  if (c == 0) { j.xch[2 * C] = (double)j.R; j.xch[2 * C + 1] = 0.0; }
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
// Synchronised statistics: the sums of every BatchNorm of a launch cross the replicas in ONE contiguous block of doubles in
// the caller's workspace, job after job [sum z | sum z^2 | R, 0] (forward) or [d gamma | d beta | R, 0] (backward), through
// the caller's hook (hep_sync of include/hep.h): when the work it enqueued on the stream has run, every element is the sum over
// all replicas.  A hook that fails ends the call: GDSyncFailed leaves the launch function, nothing further is launched.
struct GDSync { int (*sum)(void* ctx, void* data, int64_t count, int is_double, void* stream); void* ctx; double* block; };
template <int NJOBS> static inline void gd_sync_exchange(GDBnArgs<NJOBS>* a, const GDSync& sy, hipStream_t st, bool backward, int max_c) {
  int64_t n = 0;
  for (int k = 0; k < NJOBS; k++) { a->j[k].xch = sy.block + n; n += 2 * (int64_t)a->j[k].C + 2; }
  const dim3 grid((unsigned)((max_c + GD_RED_E - 1) / GD_RED_E), NJOBS);
  if (backward) hipLaunchKernelGGL(gd_bn_sync_dsums_kernel<NJOBS>, grid, dim3(GD_THREADS), 0, st, *a);
  else hipLaunchKernelGGL((gd_bn_finish_kernel<NJOBS, true>), grid, dim3(GD_THREADS), 0, st, *a);
  if (const int rc = sy.sum(sy.ctx, sy.block, n, 1, (void*)st)) throw GDSyncFailed{rc};
}
// doubles of the exchange block of a launch over njobs BatchNorms of at most max_c channels
static inline int64_t gd_sync_doubles(int njobs, int max_c) { return (int64_t)njobs * (2 * (int64_t)max_c + 2); }

// the batch-statistics launches over NJOBS BatchNorms whose largest map has max_rows rows and max_c channels
template <int NJOBS> static inline void gd_bn_forward(GDBnArgs<NJOBS>& a, int max_rows, int max_c, int epi, hipStream_t st, const GDSync* sy = nullptr) {
  const int64_t tiles = (max_rows + a.tile_rows - 1) / a.tile_rows, quads = (max_rows + GD_DW_ROWS - 1) / GD_DW_ROWS;
  hipLaunchKernelGGL(gd_bn_stats_kernel<NJOBS>, dim3(gd_blocks(tiles * max_c), NJOBS), dim3(GD_THREADS), 0, st, a);
  if (sy) {
    gd_sync_exchange(&a, *sy, st, false, max_c);
    hipLaunchKernelGGL(gd_bn_sync_finish_kernel<NJOBS>, dim3(gd_blocks(max_c), NJOBS), dim3(GD_THREADS), 0, st, a);
  } else {
    hipLaunchKernelGGL((gd_bn_finish_kernel<NJOBS, false>), dim3((unsigned)((max_c + GD_RED_E - 1) / GD_RED_E), NJOBS), dim3(GD_THREADS), 0, st, a);
  }
  const dim3 grid(gd_blocks(quads * max_c), NJOBS);
  if (epi == GD_BN_SWISH) hipLaunchKernelGGL((gd_bn_apply_kernel<NJOBS, GD_BN_SWISH>), grid, dim3(GD_THREADS), 0, st, a);
  else if (epi == GD_BN_SCALE_SKIP) hipLaunchKernelGGL((gd_bn_apply_kernel<NJOBS, GD_BN_SCALE_SKIP>), grid, dim3(GD_THREADS), 0, st, a);
  else hipLaunchKernelGGL((gd_bn_apply_kernel<NJOBS, GD_BN_PLAIN>), grid, dim3(GD_THREADS), 0, st, a);
}
// sy: the jobs carry pg / pb / pn / pstride, the partials the part's reduce of d gamma / d beta has just read
template <int NJOBS> static inline void gd_bn_dz(GDBnArgs<NJOBS>& a, int max_rows, int max_c, hipStream_t st, const GDSync* sy = nullptr) {
  const int64_t quads = (max_rows + GD_DW_ROWS - 1) / GD_DW_ROWS;
  const dim3 grid(gd_blocks(quads * max_c), NJOBS);
  if (sy) {
    gd_sync_exchange(&a, *sy, st, true, max_c);
    hipLaunchKernelGGL((gd_bn_dz_kernel<NJOBS, true>), grid, dim3(GD_THREADS), 0, st, a);
  } else {
    hipLaunchKernelGGL((gd_bn_dz_kernel<NJOBS, false>), grid, dim3(GD_THREADS), 0, st, a);
  }
}
