// k_backbone_grad.hip - training forward and backward of the EfficientNet trunk (backbone_net.model.*: stem conv + BN + swish
// and every MBConv block; reference efficientnet/model.py:69-104, efficientdet/model.py:436-458) on gfx950, fp32, as a function
// of (its parameters, the image [B,3,S,S]) with the three taps P3 / P4 / P5 as outputs.  By default the function is the inference
// function: BatchNorm uses the RUNNING statistics in forward and backward; gamma and beta get gradients, the statistics get
// zero.  HEP_BN_BATCH: the stem's BatchNorm and every bn0 / bn1 / bn2 normalise with the statistics of their map's rows (the shared
// passes of grad_dev.h): stem, gemm<FWD> and dw_fwd store z only, then statistics / finish / apply (swish; none; * branch_scale +
// skip for bn2); in the backward the gamma / beta reduce and the d z correction follow out_bwd / act_bwd, ahead of whatever reads
// d z.  Drop-connect enters as data: branch_scale[block][image] multiplies the residual branch of the blocks that add their
// input (NULL: every scale is 1).
//
// Plain layouts, as k_neck_grad.hip has (the GEMM tile and the reduce are grad_dev.h's): every map is rows [B * s * s][C],
// channels contiguous, one buffer per map.  The squeeze-excite biases have 4, 6, 10, ... floats, so the tensors behind them are not 16-byte aligned in the flat
// parameter buffer: the forward first copies the stem, every block up to its se_expand bias and every block's project conv +
// bn2 to 16-byte aligned places in the workspace (the GEMMs' float4 loads); forward and backward read that copy.
//
//   block     x -> [expand: z0 = x . W0^T, a0 = swish(bn0(z0))] -> z1 = depthwise_k_s(a0 | x) (TF-SAME), a1 = swish(bn1(z1))
//             -> m = mean_pixels(a1), r = Wr m + br, l = We swish(r) + be, g = sigmoid(l), xg = a1 * g
//             -> z2 = xg . W2^T, y = bn2(z2) [* scale[b] + x where the block adds its input]
//   forward   pack; copy (the image, for the stem's weight gradient); stem (direct 3x3 stride 2: zs, as); per block gemm<FWD> (z0, a0), dw_fwd (z1, a1), se_sum, se_fc (m, r, g),
//             gate (xg), gemm<FWD> (z2, y); nchw_from_rows (the three taps)
//   backward  per block, last first: out_bwd (d y = data path of the next block + its skip path + the tap's cotangent, in that
//             order; bn2: d z2 and gamma / beta partials), gemm<DATA> (d xg), gemm<WGRAD> (d W2), reduce; se_dsum (partials of
//             sum_pixels d xg * a1), se_bwd (per image: d l, d r, d m / ss), se_wgrad (sums over the images in order, in double),
//             act_bwd (d a1 = d xg * g + d m / ss, swish', bn1: d z1 in place), dw_wgrad (per-tile partials), dw_dgrad (gather
//             form), reduce; [act_bwd (bn0: d z0), gemm<WGRAD> (d W0), gemm<DATA> (d x), reduce].  Then the stem: act_bwd,
//             stem_wgrad, reduce, and stem_dgrad when the image gradient is requested.
// The pointwise products are v_mfma_f32_16x16x4_f32 (gd_gemm_tile of grad_dev.h).  Every reduction is partial sums in a
// fixed order plus a fixed-order second pass in double (gd_reduce_kernel): bit-reproducible, no float atomics.
#include <cstdio>

#include "hep.h"
#include "grad_dev.h"
#include "hep_host.h"
#include "hep_train.h"

#define BG_RED_JOBS 4        // reduce jobs of one launch: a weight, gamma, beta, statistics

// ------------------------------------------------------------------------------------------------------------------
struct BGPackArgs { int64_t src[BG_MAX_SEGMENTS], dst[BG_MAX_SEGMENTS], len[BG_MAX_SEGMENTS]; };
// segment blockIdx.y of the flat parameters to its 16-byte aligned place in the workspace
__global__ __launch_bounds__(GD_THREADS) void bg_pack_kernel(BGPackArgs a, const float* __restrict__ params, float* __restrict__ ws) {
  const int sgm = blockIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= a.len[sgm]) return;
  ws[a.dst[sgm] + idx] = params[a.src[sgm] + idx];
}

// the image, kept for the stem's weight gradient
__global__ __launch_bounds__(GD_THREADS) void bg_copy_kernel(int64_t n, const float* __restrict__ src, float* __restrict__ dst) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx < n) dst[idx] = src[idx];
}

// rows [B * ss][C] -> NCHW [B][C][ss]
__global__ __launch_bounds__(GD_THREADS) void bg_nchw_from_rows_kernel(int B, int C, int ss, const float* __restrict__ rows, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)B * ss * C) return;
  const int r = (int)(idx / C), c = (int)(idx % C), b = r / ss, pix = r % ss;
  out[((int64_t)b * C + c) * ss + pix] = rows[idx];
}

// ------------------------------------------------------------------------------------------------------------------
// stem: 3 x 3 stride 2 over the NCHW image of even side S, TF-SAME = no padding before, one row / column after
__global__ __launch_bounds__(GD_THREADS) void bg_stem_fwd_kernel(int B, int S, int C, const float* __restrict__ img, const float* __restrict__ w,
                                                                 const float* __restrict__ bn, float* __restrict__ Z, float* __restrict__ A, int z_only) {
  const int s = S >> 1;
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)B * s * s * C) return;
  const int r = (int)(idx / C), c = (int)(idx % C), b = r / (s * s), pix = r % (s * s), oy = pix / s, ox = pix % s;
  float acc = 0.0f;
#pragma unroll
  for (int ci = 0; ci < 3; ci++)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int y = 2 * oy + i, x = 2 * ox + j;
        if (y < S && x < S) acc = fmaf(w[c * 27 + ci * 9 + i * 3 + j], img[((int64_t)(b * 3 + ci) * S + y) * S + x], acc);
      }
  Z[idx] = acc;
  if (z_only) return;                                      // batch statistics: the BatchNorm passes of grad_dev.h make A
  const float v = gd_bn_apply(gd_bn_load(bn, C, c), acc);
  A[idx] = v * gd_sigmoid(v);
}

// d W[c][ci][i][j] partials: one thread = (tile of output rows, channel)
__global__ __launch_bounds__(GD_THREADS) void bg_stem_wgrad_kernel(int B, int S, int C, int R, int tile_rows, const float* __restrict__ dZ,
                                                                   const float* __restrict__ img, float* __restrict__ part) {
  const int s = S >> 1, ss = s * s;
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int tile = (int)(gid / C), c = (int)(gid % C);
  const int r0 = tile * tile_rows, r1 = min(R, r0 + tile_rows);
  if (r0 >= R) return;
  float aw[27];
#pragma unroll
  for (int tp = 0; tp < 27; tp++) aw[tp] = 0.0f;
  for (int r = r0; r < r1; r++) {
    const int b = r / ss, pix = r % ss, oy = pix / s, ox = pix % s;
    const float g = dZ[(int64_t)r * C + c];
#pragma unroll
    for (int ci = 0; ci < 3; ci++)
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const int y = 2 * oy + i, x = 2 * ox + j;
          if (y < S && x < S) aw[ci * 9 + i * 3 + j] = fmaf(g, img[((int64_t)(b * 3 + ci) * S + y) * S + x], aw[ci * 9 + i * 3 + j]);
        }
  }
#pragma unroll
  for (int tp = 0; tp < 27; tp++) part[((int64_t)tile * C + c) * 27 + tp] = aw[tp];
}

// image gradient in gather form: every image element adds the outputs whose window holds it, (i, j, channel) in order
__global__ __launch_bounds__(GD_THREADS) void bg_stem_dgrad_kernel(int B, int S, int C, const float* __restrict__ dZ, const float* __restrict__ w,
                                                                   float* __restrict__ dimg) {
  const int s = S >> 1;
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)B * 3 * S * S) return;
  const int x = (int)(idx % S), y = (int)((idx / S) % S), ci = (int)((idx / ((int64_t)S * S)) % 3), b = (int)(idx / ((int64_t)3 * S * S));
  float acc = 0.0f;
  for (int i = 0; i < 3; i++) {
    const int ty = y - i;
    if (ty < 0 || (ty & 1)) continue;
    for (int j = 0; j < 3; j++) {
      const int tx = x - j;
      if (tx < 0 || (tx & 1)) continue;
      const float* __restrict__ g = dZ + ((int64_t)(b * s + (ty >> 1)) * s + (tx >> 1)) * C;
      for (int c = 0; c < C; c++) acc = fmaf(w[c * 27 + ci * 9 + i * 3 + j], g[c], acc);
    }
  }
  dimg[idx] = acc;
}

// ------------------------------------------------------------------------------------------------------------------
// depthwise K x K, stride 1 / 2, TF-SAME (pad rows / columns before; the rest falls after), fused with bn1 + swish
template <int K> __global__ __launch_bounds__(GD_THREADS) void bg_dw_fwd_kernel(int B, int si, int so, int stride, int pad, int C, const float* __restrict__ X,
                                                                                const float* __restrict__ w, const float* __restrict__ bn,
                                                                                float* __restrict__ Z, float* __restrict__ A, int z_only) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)B * so * so * C) return;
  const int r = (int)(idx / C), c = (int)(idx % C), b = r / (so * so), pix = r % (so * so), oy = pix / so, ox = pix % so;
  float acc = 0.0f;
#pragma unroll
  for (int i = 0; i < K; i++) {
    const int y = oy * stride - pad + i;
    if (y < 0 || y >= si) continue;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int x = ox * stride - pad + j;
      if (x < 0 || x >= si) continue;
      acc = fmaf(w[c * K * K + i * K + j], X[((int64_t)(b * si + y) * si + x) * C + c], acc);
    }
  }
  Z[idx] = acc;
  if (z_only) return;                                      // batch statistics: the BatchNorm passes of grad_dev.h make A
  const float v = gd_bn_apply(gd_bn_load(bn, C, c), acc);
  A[idx] = v * gd_sigmoid(v);
}

// depthwise weight gradient: K * K sums per channel over all output pixels; one thread = (tile of output rows, channel)
template <int K> __global__ __launch_bounds__(GD_THREADS) void bg_dw_wgrad_kernel(int si, int so, int stride, int pad, int C, int R, int tile_rows,
                                                                                  const float* __restrict__ dZ, const float* __restrict__ X, float* __restrict__ part) {
  const int ss = so * so;
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int tile = (int)(gid / C), c = (int)(gid % C);
  const int r0 = tile * tile_rows, r1 = min(R, r0 + tile_rows);
  if (r0 >= R) return;
  float aw[K * K];
#pragma unroll
  for (int tp = 0; tp < K * K; tp++) aw[tp] = 0.0f;
  for (int r = r0; r < r1; r++) {
    const int b = r / ss, pix = r % ss, oy = pix / so, ox = pix % so;
    const float g = dZ[(int64_t)r * C + c];
#pragma unroll
    for (int i = 0; i < K; i++) {
      const int y = oy * stride - pad + i;
      const bool yin = y >= 0 && y < si;
#pragma unroll
      for (int j = 0; j < K; j++) {
        const int x = ox * stride - pad + j;
        const float v = (yin && x >= 0 && x < si) ? X[((int64_t)(b * si + y) * si + x) * C + c] : 0.0f;
        aw[i * K + j] = fmaf(g, v, aw[i * K + j]);
      }
    }
  }
#pragma unroll
  for (int tp = 0; tp < K * K; tp++) part[((int64_t)tile * C + c) * (K * K) + tp] = aw[tp];
}

// depthwise data gradient in gather form: input (y, x) belongs to the window of output o at tap i where o * stride = y + pad - i
template <int K> __global__ __launch_bounds__(GD_THREADS) void bg_dw_dgrad_kernel(int B, int si, int so, int stride, int pad, int C, const float* __restrict__ dZ,
                                                                                  const float* __restrict__ w, float* __restrict__ dX) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)B * si * si * C) return;
  const int r = (int)(idx / C), c = (int)(idx % C), b = r / (si * si), pix = r % (si * si), y = pix / si, x = pix % si;
  float acc = 0.0f;
#pragma unroll
  for (int i = 0; i < K; i++) {
    const int ty = y + pad - i, oy = ty / stride;
    if (ty < 0 || ty % stride != 0 || oy >= so) continue;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int tx = x + pad - j, ox = tx / stride;
      if (tx < 0 || tx % stride != 0 || ox >= so) continue;
      acc = fmaf(w[c * K * K + i * K + j], dZ[((int64_t)(b * so + oy) * so + ox) * C + c], acc);
    }
  }
  dX[idx] = acc;
}

// ------------------------------------------------------------------------------------------------------------------
// squeeze-excite.  Per (image, chunk of rows, channel) sums in row order; FWD: of a1, else of d xg * a1 with a1 = swish(bn1(z1))
template <bool FWD> __global__ __launch_bounds__(GD_THREADS) void bg_se_sum_kernel(int B, int ss, int C, int nchunk, int chunk_rows, const float* __restrict__ A,
                                                                                   const float* __restrict__ Z, const float* __restrict__ bn, float* __restrict__ part) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)B * nchunk * C) return;
  const int c = (int)(idx % C), q = (int)((idx / C) % nchunk), b = (int)(idx / ((int64_t)C * nchunk));
  const int r0 = q * chunk_rows, r1 = min(ss, r0 + chunk_rows);
  GDBn n{};
  if (!FWD) n = gd_bn_load(bn, C, c);
  float s = 0.0f;
  for (int r = r0; r < r1; r++) {
    const int64_t at = ((int64_t)b * ss + r) * C + c;
    if (FWD) {
      s += A[at];
    } else {
      const float v = gd_bn_apply(n, Z[at]);
      s = fmaf(A[at], v * gd_sigmoid(v), s);
    }
  }
  part[idx] = s;
}

// butterfly sum over the 64 lanes of a wave: a fixed order, every lane gets the total
__device__ __forceinline__ float bg_wave_sum(float a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
  return a;
}

// one workgroup per image: the means (second pass over the chunks in double), the two small FCs (VALU), the gate
__global__ __launch_bounds__(GD_THREADS) void bg_se_fc_kernel(int ss, int C, int se, int nchunk, const float* __restrict__ part, const float* __restrict__ wr,
                                                              const float* __restrict__ br, const float* __restrict__ we, const float* __restrict__ be,
                                                              float* __restrict__ M, float* __restrict__ Rr, float* __restrict__ G) {
  __shared__ float sm[BG_MAX_CEXP];
  __shared__ float sh[BG_MAX_SE];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (int c = t; c < C; c += GD_THREADS) {
    double s = 0.0;
    for (int q = 0; q < nchunk; q++) s += (double)part[((int64_t)b * nchunk + q) * C + c];
    const float m = (float)(s / (double)ss);
    sm[c] = m;
    M[(int64_t)b * C + c] = m;
  }
  __syncthreads();
  for (int j = wv; j < se; j += GD_THREADS / 64) {
    float a = 0.0f;
    for (int c = lane; c < C; c += 64) a = fmaf(wr[(int64_t)j * C + c], sm[c], a);
    a = bg_wave_sum(a);
    if (lane == 0) {
      const float r = a + br[j];
      Rr[b * se + j] = r;
      sh[j] = r * gd_sigmoid(r);
    }
  }
  __syncthreads();
  for (int c = t; c < C; c += GD_THREADS) {
    float l = be[c];
    for (int j = 0; j < se; j++) l = fmaf(we[(int64_t)c * se + j], sh[j], l);
    G[(int64_t)b * C + c] = gd_sigmoid(l);
  }
}

__global__ __launch_bounds__(GD_THREADS) void bg_gate_kernel(int64_t total, int ss, int C, const float* __restrict__ A, const float* __restrict__ G, float* __restrict__ XG) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int r = (int)(idx / C), c = (int)(idx % C);
  XG[idx] = A[idx] * G[(int64_t)(r / ss) * C + c];
}

// one workgroup per image: d l = (sum d xg * a1) * g (1 - g), d r = (We^T d l) * swish'(r), d m / ss = (Wr^T d r) / ss
__global__ __launch_bounds__(GD_THREADS) void bg_se_bwd_kernel(int ss, int C, int se, int nchunk, const float* __restrict__ part, const float* __restrict__ wr,
                                                               const float* __restrict__ we, const float* __restrict__ Rr, const float* __restrict__ G,
                                                               float* __restrict__ DL, float* __restrict__ DR, float* __restrict__ DM) {
  __shared__ float sdl[BG_MAX_CEXP];
  __shared__ float sdr[BG_MAX_SE];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (int c = t; c < C; c += GD_THREADS) {
    double s = 0.0;
    for (int q = 0; q < nchunk; q++) s += (double)part[((int64_t)b * nchunk + q) * C + c];
    const float g = G[(int64_t)b * C + c], dl = (float)s * (g * (1.0f - g));
    sdl[c] = dl;
    DL[(int64_t)b * C + c] = dl;
  }
  __syncthreads();
  for (int j = wv; j < se; j += GD_THREADS / 64) {
    float a = 0.0f;
    for (int c = lane; c < C; c += 64) a = fmaf(we[(int64_t)c * se + j], sdl[c], a);
    a = bg_wave_sum(a);
    if (lane == 0) {
      const float dr = a * gd_swish_grad(Rr[b * se + j]);
      sdr[j] = dr;
      DR[b * se + j] = dr;
    }
  }
  __syncthreads();
  const float inv = 1.0f / (float)ss;
  for (int c = t; c < C; c += GD_THREADS) {
    float a = 0.0f;
    for (int j = 0; j < se; j++) a = fmaf(wr[(int64_t)j * C + c], sdr[j], a);
    DM[(int64_t)b * C + c] = a * inv;
  }
}

// the four squeeze-excite tensors' gradients (se_reduce weight [se][C], bias [se], se_expand weight [C][se], bias [C], contiguous
// in that order): sums over the images in order, in double
__global__ __launch_bounds__(GD_THREADS) void bg_se_wgrad_kernel(int B, int C, int se, const float* __restrict__ M, const float* __restrict__ Rr,
                                                                 const float* __restrict__ DL, const float* __restrict__ DR, float* __restrict__ dst) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int64_t n0 = (int64_t)se * C, n1 = n0 + se, n2 = n1 + (int64_t)C * se, n3 = n2 + C;
  if (idx >= n3) return;
  double s = 0.0;
  if (idx < n0) {
    const int j = (int)(idx / C), c = (int)(idx % C);
    for (int b = 0; b < B; b++) s += (double)(DR[b * se + j] * M[(int64_t)b * C + c]);
  } else if (idx < n1) {
    const int j = (int)(idx - n0);
    for (int b = 0; b < B; b++) s += (double)DR[b * se + j];
  } else if (idx < n2) {
    const int c = (int)((idx - n1) / se), j = (int)((idx - n1) % se);
    for (int b = 0; b < B; b++) {
      const float r = Rr[b * se + j];
      s += (double)(DL[(int64_t)b * C + c] * (r * gd_sigmoid(r)));
    }
  } else {
    const int c = (int)(idx - n2);
    for (int b = 0; b < B; b++) s += (double)DL[(int64_t)b * C + c];
  }
  dst[idx] = (float)s;
}

// ------------------------------------------------------------------------------------------------------------------
enum { BG_FWD = 0, BG_DATA = 1, BG_WGRAD = 2 };
struct BGGemmArgs {
  const float* A; const float* Bm; float* C; float* C2;
  const float* bn;                               // FWD: gamma, beta, mean, var [4][J]
  const float* res; const float* scale;          // FWD without act: the block's input rows to add (or NULL), the per-image branch scale (or NULL)
  int I, J, K, lda, ldb, ldc, ntn, slab_rows, act, ss;
  int z_only;                                    // FWD with batch statistics: store z, the BatchNorm passes of grad_dev.h make C2
};
// C[i][j] = sum_k A(i,k) B(k,j), 64 x 64 per workgroup, wave w owns rows 16w..16w+15 and four 16-column accumulators; edge
// tiles are masked at the loads and at the stores (channel counts are multiples of 8, not of 64).
//   FWD     A = x rows (k contiguous), B = W [J][K] (k contiguous); z = C -> C, act: swish(bn(z)) -> C2, else bn(z) * scale + res -> C2
//   DATA    A = d z rows (k contiguous), B = W [K][J] (j contiguous, W un-transposed) -> C rows
//   WGRAD   A = d z rows read as (k = row, i = column), B = x rows (k = row); rows [z * slab_rows, ...) of K -> C[z][I][J]
template <int MODE> __global__ __launch_bounds__(GD_THREADS) void bg_gemm_kernel(BGGemmArgs a) {
  __shared__ __attribute__((aligned(16))) float As[GD_BK][GD_LDS_PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[GD_BK][GD_LDS_PITCH];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int I = a.I, J = a.J;
  const int i0 = (int)(blockIdx.x / a.ntn) * GD_BM, j0 = (int)(blockIdx.x % a.ntn) * GD_BN;
  if (i0 >= I || j0 >= J) return;                          // uniform over the workgroup
  int k_begin = 0, k_end = a.K;
  if (MODE == BG_WGRAD) { k_begin = blockIdx.z * a.slab_rows; k_end = min(a.K, k_begin + a.slab_rows); }
  f32x4 acc[4];
  gd_gemm_tile<MODE == BG_WGRAD ? GD_ROW_CONTIG : GD_K_CONTIG, MODE == BG_FWD ? GD_K_CONTIG : GD_ROW_CONTIG>(
      As, Bs, acc, a.A, a.lda, a.Bm, a.ldb, i0, I, j0, J, k_begin, k_end, k_end, t, lane, wv);
  gd_acc_visit(acc, i0, I, j0, J, lane, wv, [=](int m, int n, float v, const GDBn& q) {
    if (MODE == BG_FWD) {
      const int64_t at = (int64_t)m * a.ldc + n;
      a.C[at] = v;
      if (!a.z_only) {
        float y = gd_bn_apply(q, v);
        if (a.act) {
          y = y * gd_sigmoid(y);
        } else if (a.res) {
          y = fmaf(y, a.scale ? a.scale[m / a.ss] : 1.0f, a.res[at]);
        }
        a.C2[at] = y;
      }
    } else if (MODE == BG_DATA) {
      a.C[(int64_t)m * a.ldc + n] = v;
    } else {
      a.C[((int64_t)blockIdx.z * I + m) * J + n] = v;
    }
  }, [=](int n) { return MODE == BG_FWD ? gd_bn_load(a.bn, J, n) : GDBn{}; });
}

// ------------------------------------------------------------------------------------------------------------------
// Gradient of a block's output y and bn2 behind it.  One thread = (tile of rows, channel).
//   d y = gdata (the next block's data path) + gskip (the next block's skip path) + cot (NCHW cotangent of a tap), each or NULL
//   d z2 = d y * scale[b] * gamma * rstd;  gamma / beta partials [tile][C]
struct BGOutArgs {
  int ss, C, R, tile_rows;
  const float* gdata; const float* gskip; const float* cot; const float* scale;
  const float* Z; const float* bn;
  float* dY; float* dZ; float* pgamma; float* pbeta;
};
__global__ __launch_bounds__(GD_THREADS) void bg_out_bwd_kernel(BGOutArgs a) {
  const int C = a.C, ss = a.ss;
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int tile = (int)(gid / C), c = (int)(gid % C);
  const int r0 = tile * a.tile_rows, r1 = min(a.R, r0 + a.tile_rows);
  if (r0 >= a.R) return;
  const GDBn q = gd_bn_load(a.bn, C, c);
  float ag = 0.0f, ab = 0.0f;
  for (int r = r0; r < r1; r++) {
    const int b = r / ss, pix = r % ss;
    const int64_t at = (int64_t)r * C + c;
    float g = 0.0f;
    if (a.gdata) g = a.gdata[at];
    if (a.gskip) g += a.gskip[at];
    if (a.cot) g += a.cot[((int64_t)b * C + c) * ss + pix];
    a.dY[at] = g;
    if (a.scale) g *= a.scale[b];
    ag = fmaf(g, (a.Z[at] - q.mean) * q.rstd, ag);
    ab += g;
    a.dZ[at] = g * q.gamma * q.rstd;
  }
  a.pgamma[(int64_t)tile * C + c] = ag;
  a.pbeta[(int64_t)tile * C + c] = ab;
}

// Backward of swish(bn(z)), in place on the gradient rows: g = G (gate: G * gate[b][c] + dmean[b][c], the squeeze-excite's two
// paths into a1), d v = g * swish'(bn(z)), G <- d z = d v * gamma * rstd; gamma / beta partials [tile][C]
struct BGActArgs {
  int ss, C, R, tile_rows;
  float* G; const float* Z; const float* bn; const float* gate; const float* dmean;
  float* pgamma; float* pbeta;
};
__global__ __launch_bounds__(GD_THREADS) void bg_act_bwd_kernel(BGActArgs a) {
  const int C = a.C, ss = a.ss;
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int tile = (int)(gid / C), c = (int)(gid % C);
  const int r0 = tile * a.tile_rows, r1 = min(a.R, r0 + a.tile_rows);
  if (r0 >= a.R) return;
  const GDBn q = gd_bn_load(a.bn, C, c);
  float ag = 0.0f, ab = 0.0f;
  for (int r = r0; r < r1; r++) {
    const int64_t at = (int64_t)r * C + c;
    float g = a.G[at];
    if (a.gate) { const int64_t bc = (int64_t)(r / ss) * C + c; g = fmaf(g, a.gate[bc], a.dmean[bc]); }
    const float zh = (a.Z[at] - q.mean) * q.rstd, v = fmaf(zh, q.gamma, q.beta);
    const float dv = g * gd_swish_grad(v);
    ag = fmaf(dv, zh, ag);
    ab += dv;
    a.G[at] = dv * q.gamma * q.rstd;
  }
  a.pgamma[(int64_t)tile * C + c] = ag;
  a.pbeta[(int64_t)tile * C + c] = ab;
}

// ------------------------------------------------------------------------------------------------------------------
// host side
static inline int bg_tile_rows(int R) { return R <= 4096 ? 8 : R <= 65536 ? 32 : 64; }
static inline int bg_ntiles(int R) { const int tr = bg_tile_rows(R); return (R + tr - 1) / tr; }
static inline void bg_slabs(int R, int* slab_rows, int* nslab) { gd_slabs(R, BG_MAX_SLABS, slab_rows, nslab); }
static inline void bg_chunks(int ss, int* chunk_rows, int* nchunk) {
  int nc = (ss + 31) / 32; if (nc > 128) nc = 128;
  *chunk_rows = (ss + nc - 1) / nc;
  *nchunk = (ss + *chunk_rows - 1) / *chunk_rows;
}

int backbone_plan(int phi, int, int size, int batch, BGPlan* p, const char** why, int bn_mode, int sync) {
  hep::Arch arch;
  if (bn_mode != HEP_BN_RUNNING && bn_mode != HEP_BN_BATCH) { *why = "backbone: the BatchNorm mode must be HEP_BN_RUNNING or HEP_BN_BATCH"; return HEP_ERR_INVALID; }
  p->bn_batch = bn_mode == HEP_BN_BATCH; p->bn_sync = p->bn_batch && sync;
  if (!hep::make_arch(phi, &arch)) { *why = "backbone: phi must be in 0..7 (phi 8 needs a P8 level)"; return HEP_ERR_UNSUPPORTED; }
  if ((int)arch.blocks.size() > BG_MAX_BLOCKS) { *why = "backbone: too many blocks"; return HEP_ERR_UNSUPPORTED; }
  p->phi = phi; p->nblocks = (int)arch.blocks.size(); p->stem = arch.stem; p->B = 0; p->size = 0;
  for (int t = 0; t < 3; t++) { p->taps[t] = arch.taps[t]; p->tapc[t] = arch.tap_channels[t]; }
  int64_t o = 0;
  p->p_stem = o; o += (int64_t)arch.stem * 27;
  p->p_bn_stem = o; o += 4 * arch.stem;
  for (int i = 0; i < p->nblocks; i++) {
    const hep::MBConv& m = arch.blocks[i];
    BGBlock& b = p->b[i];
    b.cin = m.cin; b.cexp = m.cexp; b.k = m.k; b.stride = m.stride; b.se = m.se; b.cout = m.cout; b.expand = m.expand; b.skip = m.skip;
    if (m.cexp > BG_MAX_CEXP || m.se > BG_MAX_SE || (m.k != 3 && m.k != 5) || (m.stride != 1 && m.stride != 2) || m.cin % 8 || m.cout % 8) {
      *why = "backbone: a block is outside what the kernels are built for"; return HEP_ERR_UNSUPPORTED;
    }
    b.p_first = o;
    b.p_w0 = o; b.p_bn0 = o;
    if (m.expand) { o += (int64_t)m.cexp * m.cin; b.p_bn0 = o; o += 4 * m.cexp; }
    b.p_dw = o; o += (int64_t)m.cexp * m.k * m.k;
    b.p_bn1 = o; o += 4 * m.cexp;
    b.p_wr = o; o += (int64_t)m.se * m.cexp;
    b.p_br = o; o += m.se;
    b.p_we = o; o += (int64_t)m.cexp * m.se;
    b.p_be = o; o += m.cexp;
    b.p_w2 = o; o += (int64_t)m.cout * m.cexp;
    b.p_bn2 = o; o += 4 * m.cout;
    b.p_end = o;
  }
  p->nparams = o;
  if (size == 0 && batch == 0) return 0;                   // layout only
  if (size < 128 || size > 2048 || size % 128 != 0) { *why = "backbone: size must be a multiple of 128 in [128, 2048]"; return HEP_ERR_UNSUPPORTED; }
  if (batch < 1) { *why = "backbone: batch must be at least 1"; return HEP_ERR_UNSUPPORTED; }
  if ((int64_t)batch * (size / 2) * (size / 2) > (1 << 24)) { *why = "backbone: batch * pixels exceeds 16 Mi stem rows"; return HEP_ERR_UNSUPPORTED; }
  p->B = batch; p->size = size; p->s0 = size / 2; p->R0 = batch * p->s0 * p->s0;
  int64_t w = 0;
  auto take = [&](int64_t n) { const int64_t at = w; w += (n + 3) / 4 * 4; return at; };
  p->q_stem = take(p->b[0].p_first);
  p->o_img = take((int64_t)batch * 3 * size * size);
  p->o_zs = take((int64_t)p->R0 * p->stem); p->o_as = take((int64_t)p->R0 * p->stem);
  int s = p->s0;
  int64_t m_a1 = 0, m_y = 0, m_xg = 0, m_a0 = 4, m_x = (int64_t)p->R0 * p->stem, m_pw = 4, m_col = (int64_t)bg_ntiles(p->R0) * p->stem;
  int64_t m_pdw = (int64_t)bg_ntiles(p->R0) * p->stem * 27, m_pse = 0, m_bc = 0, m_bs = 0;
  for (int i = 0; i < p->nblocks; i++) {
    BGBlock& b = p->b[i];
    b.s_in = s; b.s_out = s / b.stride; s = b.s_out;
    b.R_in = batch * b.s_in * b.s_in; b.R_out = batch * b.s_out * b.s_out;
    b.q_a = take(b.p_w2 - b.p_first); b.q_b = take(b.p_end - b.p_w2);
    const int64_t nin = (int64_t)b.R_in * b.cexp, nmid = (int64_t)b.R_out * b.cexp, nout = (int64_t)b.R_out * b.cout;
    b.o_z0 = b.o_a0 = 0;
    if (b.expand) { b.o_z0 = take(nin); b.o_a0 = take(nin); }
    b.o_z1 = take(nmid); b.o_xg = take(nmid); b.o_z2 = take(nout); b.o_y = take(nout);
    b.o_m = take((int64_t)batch * b.cexp); b.o_g = take((int64_t)batch * b.cexp); b.o_r = take((int64_t)batch * b.se);
    int cr, nc, sr, ns;
    bg_chunks(b.s_out * b.s_out, &cr, &nc);
    m_a1 = std::max(m_a1, nmid); m_xg = std::max(m_xg, nmid); m_y = std::max(m_y, nout);
    m_x = std::max(m_x, (int64_t)b.R_in * b.cin);
    if (b.expand) m_a0 = std::max(m_a0, nin);
    bg_slabs(b.R_out, &sr, &ns); m_pw = std::max(m_pw, (int64_t)ns * b.cout * b.cexp);
    if (b.expand) { bg_slabs(b.R_in, &sr, &ns); m_pw = std::max(m_pw, (int64_t)ns * b.cexp * b.cin); }
    m_col = std::max(m_col, (int64_t)bg_ntiles(b.R_out) * std::max(b.cexp, b.cout));
    if (b.expand) m_col = std::max(m_col, (int64_t)bg_ntiles(b.R_in) * b.cexp);
    m_pdw = std::max(m_pdw, (int64_t)bg_ntiles(b.R_out) * b.cexp * b.k * b.k);
    m_pse = std::max(m_pse, (int64_t)batch * nc * b.cexp);
    m_bc = std::max(m_bc, (int64_t)batch * b.cexp); m_bs = std::max(m_bs, (int64_t)batch * b.se);
  }
  p->o_a1 = take(m_a1);
  p->o_dy[0] = take(m_y); p->o_dy[1] = take(m_y); p->o_dz2 = take(m_y);
  p->o_dxg = take(m_xg); p->o_da0 = take(m_a0); p->o_dx = take(m_x);
  p->o_pw = take(m_pw); p->o_pcol[0] = take(m_col); p->o_pcol[1] = take(m_col); p->o_pdw = take(m_pdw); p->o_pse = take(m_pse);
  p->o_dl = take(m_bc); p->o_dm = take(m_bc); p->o_dr = take(m_bs);
  p->o_es = p->o_bnp = 0;
  for (int i = 0; i < p->nblocks; i++) p->b[i].o_e0 = p->b[i].o_e1 = p->b[i].o_e2 = 0;
  if (p->bn_batch) {                                       // an effective table per BatchNorm; [tile][C][2] doubles (the smallest map has 16 rows: never < 2)
    p->o_es = take(4 * p->stem);
    for (int i = 0; i < p->nblocks; i++) {
      BGBlock& b = p->b[i];
      if (b.expand) b.o_e0 = take(4 * b.cexp);
      b.o_e1 = take(4 * b.cexp); b.o_e2 = take(4 * b.cout);
    }
    p->o_bnp = take(4 * m_col);
  }
  p->o_xch = 0;
  if (p->bn_sync) {                                        // the widest BatchNorm's sums
    int cmax = p->stem;
    for (int i = 0; i < p->nblocks; i++) cmax = std::max(cmax, std::max(p->b[i].cexp, p->b[i].cout));
    p->o_xch = take(2 * gd_sync_doubles(1, cmax));
  }
  p->ws_floats = w;
  return 0;
}

int backbone_tensor_count(const BGPlan& p) {
  int n = 5;
  for (int i = 0; i < p.nblocks; i++) n += p.b[i].expand ? 19 : 14;
  return n;
}
// the offset of every tensor of the flat buffer, in state_dict order (num_batches_tracked left out)
void backbone_tensor_offsets(const BGPlan& p, int64_t* out) {
  int k = 0;
  auto bn = [&](int64_t at, int C) { for (int t = 0; t < 4; t++) out[k++] = at + (int64_t)t * C; };
  out[k++] = p.p_stem; bn(p.p_bn_stem, p.stem);
  for (int i = 0; i < p.nblocks; i++) {
    const BGBlock& b = p.b[i];
    if (b.expand) { out[k++] = b.p_w0; bn(b.p_bn0, b.cexp); }
    out[k++] = b.p_dw; bn(b.p_bn1, b.cexp);
    out[k++] = b.p_wr; out[k++] = b.p_br; out[k++] = b.p_we; out[k++] = b.p_be;
    out[k++] = b.p_w2; bn(b.p_bn2, b.cout);
  }
}

int backbone_stage_count(const BGPlan& p) { return 1 + p.nblocks; }
// stage 0: "stem" (after BN + swish), stage 1 + i: "block{i}" (the block's output); dims: [B, s, s, C]
int backbone_stage(const BGPlan& p, int i, char name[32], int64_t dims[4], int64_t* offset_floats) {
  if (i < 0 || i >= backbone_stage_count(p)) return -1;
  dims[0] = p.B;
  if (i == 0) { snprintf(name, 32, "stem"); dims[1] = dims[2] = p.s0; dims[3] = p.stem; *offset_floats = p.o_as; return 0; }
  const BGBlock& b = p.b[i - 1];
  snprintf(name, 32, "block%d", i - 1);
  dims[1] = dims[2] = b.s_out; dims[3] = b.cout; *offset_floats = b.o_y;
  return 0;
}

namespace {
inline const float* bg_pa(const BGPlan& p, const float* ws, int i, int64_t flat) { return ws + p.b[i].q_a + (flat - p.b[i].p_first); }
inline const float* bg_pb(const BGPlan& p, const float* ws, int i, int64_t flat) { return ws + p.b[i].q_b + (flat - p.b[i].p_w2); }

void bg_gemm(int mode, BGGemmArgs m, int nslab, hipStream_t st) {
  const int ntm = (m.I + GD_BM - 1) / GD_BM;
  m.ntn = (m.J + GD_BN - 1) / GD_BN;
  if (mode == BG_FWD) hipLaunchKernelGGL(bg_gemm_kernel<BG_FWD>, dim3(ntm * m.ntn), dim3(GD_THREADS), 0, st, m);
  else if (mode == BG_DATA) hipLaunchKernelGGL(bg_gemm_kernel<BG_DATA>, dim3(ntm * m.ntn), dim3(GD_THREADS), 0, st, m);
  else hipLaunchKernelGGL(bg_gemm_kernel<BG_WGRAD>, dim3(ntm * m.ntn, 1, nslab), dim3(GD_THREADS), 0, st, m);
}

void bg_reduce(const GDReduceArgs<BG_RED_JOBS>& rd, hipStream_t st) {
  int64_t most = 1;
  for (int j = 0; j < BG_RED_JOBS; j++) most = std::max(most, rd.j[j].count);
  hipLaunchKernelGGL(gd_reduce_kernel<BG_RED_JOBS>, dim3((unsigned)((most + GD_RED_E - 1) / GD_RED_E), BG_RED_JOBS), dim3(GD_THREADS), 0, st, rd);
}
// BatchNorm column partials [tile][C] -> gamma, beta, zeros for the statistics
void bg_bn_jobs(const BGPlan& p, float* ws, int R, int C, float* dbn, GDReduceArgs<BG_RED_JOBS>* rd, int at) {
  const int T = bg_ntiles(R);
  rd->j[at + 0] = GDRedJob{ws + p.o_pcol[0], dbn, C, C, T};
  rd->j[at + 1] = GDRedJob{ws + p.o_pcol[1], dbn + C, C, C, T};
  rd->j[at + 2] = GDRedJob{nullptr, dbn + 2 * C, 2 * C, 0, 0};
}

// Batch statistics: one BatchNorm over the rows [R][C] of z as a job of grad_dev.h's kernels, its effective table at ws + eff_at
GDBnArgs<1> bg_bn_job(const BGPlan& p, float* ws, int R, int C, const float* z, const float* bn, int64_t eff_at) {
  GDBnArgs<1> a{};
  a.tile_rows = bg_tile_rows(R);
  a.j[0].z = z; a.j[0].bn = bn; a.j[0].eff = ws + eff_at;
  a.j[0].part = reinterpret_cast<double*>(ws + p.o_bnp);
  a.j[0].R = R; a.j[0].C = C;
  return a;
}
// what follows the kernel that left the "frozen" d z and the gamma / beta partials: their reduce first, then d z corrected in
// place - before any product reads it; the stage's own reduce then has its weight job only
inline GDSync bg_sync(const BGPlan& p, float* ws, const hep_sync* sync) { return GDSync{sync->sum, sync->ctx, reinterpret_cast<double*>(ws + p.o_xch)}; }
void bg_bn_backward(const BGPlan& p, float* ws, int R, int C, const float* z, int64_t eff_at, float* dz, float* dbn, hipStream_t st, const GDSync* sy) {
  GDReduceArgs<BG_RED_JOBS> rd{};
  bg_bn_jobs(p, ws, R, C, dbn, &rd, 1);
  bg_reduce(rd, st);
  GDBnArgs<1> a = bg_bn_job(p, ws, R, C, z, nullptr, eff_at);
  a.j[0].io = dz; a.j[0].dbn = dbn;
  a.j[0].pg = ws + p.o_pcol[0]; a.j[0].pb = ws + p.o_pcol[1]; a.j[0].pn = bg_ntiles(R); a.j[0].pstride = C;
  gd_bn_dz(a, R, C, st, sy);
}
}  // namespace

void launch_backbone_forward(const BGPlan& p, const float* params, const float* image, const float* branch_scale, float* const taps[3], float* ws, hipStream_t st,
                             float momentum, float* stats_out, const hep_sync* sync) {
  const int B = p.B, zo = p.bn_batch;
  GDSync sy{};
  if (p.bn_sync) sy = bg_sync(p, ws, sync);
  // batch statistics: z -> statistics -> the effective table and the running-statistics update -> the activation
  auto bn_forward = [&](int R, int C, const float* z, const float* bn, int64_t eff_at, int64_t table_at, float* out, int epi, const float* res,
                        const float* scale, int ss) {
    GDBnArgs<1> a = bg_bn_job(p, ws, R, C, z, bn, eff_at);
    a.momentum = momentum;
    a.j[0].io = out; a.j[0].stats = stats_out ? stats_out + table_at : nullptr; a.j[0].res = res; a.j[0].scale = scale; a.j[0].ss = ss;
    gd_bn_forward(a, R, C, epi, st, p.bn_sync ? &sy : nullptr);
  };
  {
    BGPackArgs pk{};
    int n = 0;
    int64_t most = p.b[0].p_first;
    pk.src[n] = 0; pk.dst[n] = p.q_stem; pk.len[n] = p.b[0].p_first; n++;
    for (int i = 0; i < p.nblocks; i++) {
      const BGBlock& b = p.b[i];
      pk.src[n] = b.p_first; pk.dst[n] = b.q_a; pk.len[n] = b.p_w2 - b.p_first; most = std::max(most, pk.len[n]); n++;
      pk.src[n] = b.p_w2; pk.dst[n] = b.q_b; pk.len[n] = b.p_end - b.p_w2; most = std::max(most, pk.len[n]); n++;
    }
    hipLaunchKernelGGL(bg_pack_kernel, dim3(gd_blocks(most), n), dim3(GD_THREADS), 0, st, pk, params, ws);
  }
  const float* ps = ws + p.q_stem;
  const int64_t nimg = (int64_t)B * 3 * p.size * p.size;
  hipLaunchKernelGGL(bg_copy_kernel, dim3(gd_blocks(nimg)), dim3(GD_THREADS), 0, st, nimg, image, ws + p.o_img);
  hipLaunchKernelGGL(bg_stem_fwd_kernel, dim3(gd_blocks((int64_t)p.R0 * p.stem)), dim3(GD_THREADS), 0, st, B, p.size, p.stem, image, ps,
                     ps + (p.p_bn_stem - p.p_stem), ws + p.o_zs, ws + p.o_as, zo);
  if (zo) bn_forward(p.R0, p.stem, ws + p.o_zs, ps + (p.p_bn_stem - p.p_stem), p.o_es, p.p_bn_stem, ws + p.o_as, GD_BN_SWISH, nullptr, nullptr, 1);
  const float* x = ws + p.o_as;
  for (int i = 0; i < p.nblocks; i++) {
    const BGBlock& b = p.b[i];
    const int ss = b.s_out * b.s_out, pad = b.stride == 1 ? (b.k - 1) / 2 : (b.k - 2) / 2;
    const float* dwin = x;
    if (b.expand) {
      BGGemmArgs m{}; m.A = x; m.Bm = bg_pa(p, ws, i, b.p_w0); m.bn = bg_pa(p, ws, i, b.p_bn0); m.C = ws + b.o_z0; m.C2 = ws + b.o_a0;
      m.I = b.R_in; m.J = b.cexp; m.K = b.cin; m.lda = b.cin; m.ldb = b.cin; m.ldc = b.cexp; m.act = 1; m.ss = 1; m.z_only = zo;
      bg_gemm(BG_FWD, m, 1, st);
      if (zo) bn_forward(b.R_in, b.cexp, m.C, m.bn, b.o_e0, b.p_bn0, m.C2, GD_BN_SWISH, nullptr, nullptr, 1);
      dwin = ws + b.o_a0;
    }
    const int64_t nmid = (int64_t)b.R_out * b.cexp;
    if (b.k == 3)
      hipLaunchKernelGGL(bg_dw_fwd_kernel<3>, dim3(gd_blocks(nmid)), dim3(GD_THREADS), 0, st, B, b.s_in, b.s_out, b.stride, pad, b.cexp, dwin,
                         bg_pa(p, ws, i, b.p_dw), bg_pa(p, ws, i, b.p_bn1), ws + b.o_z1, ws + p.o_a1, zo);
    else
      hipLaunchKernelGGL(bg_dw_fwd_kernel<5>, dim3(gd_blocks(nmid)), dim3(GD_THREADS), 0, st, B, b.s_in, b.s_out, b.stride, pad, b.cexp, dwin,
                         bg_pa(p, ws, i, b.p_dw), bg_pa(p, ws, i, b.p_bn1), ws + b.o_z1, ws + p.o_a1, zo);
    if (zo) bn_forward(b.R_out, b.cexp, ws + b.o_z1, bg_pa(p, ws, i, b.p_bn1), b.o_e1, b.p_bn1, ws + p.o_a1, GD_BN_SWISH, nullptr, nullptr, 1);
    int cr, nc;
    bg_chunks(ss, &cr, &nc);
    hipLaunchKernelGGL(bg_se_sum_kernel<true>, dim3(gd_blocks((int64_t)B * nc * b.cexp)), dim3(GD_THREADS), 0, st, B, ss, b.cexp, nc, cr,
                       (const float*)(ws + p.o_a1), (const float*)nullptr, (const float*)nullptr, ws + p.o_pse);
    hipLaunchKernelGGL(bg_se_fc_kernel, dim3(B), dim3(GD_THREADS), 0, st, ss, b.cexp, b.se, nc, (const float*)(ws + p.o_pse), bg_pa(p, ws, i, b.p_wr),
                       bg_pa(p, ws, i, b.p_br), bg_pa(p, ws, i, b.p_we), bg_pa(p, ws, i, b.p_be), ws + b.o_m, ws + b.o_r, ws + b.o_g);
    hipLaunchKernelGGL(bg_gate_kernel, dim3(gd_blocks(nmid)), dim3(GD_THREADS), 0, st, nmid, ss, b.cexp, (const float*)(ws + p.o_a1),
                       (const float*)(ws + b.o_g), ws + b.o_xg);
    BGGemmArgs m{}; m.A = ws + b.o_xg; m.Bm = bg_pb(p, ws, i, b.p_w2); m.bn = bg_pb(p, ws, i, b.p_bn2); m.C = ws + b.o_z2; m.C2 = ws + b.o_y;
    m.I = b.R_out; m.J = b.cout; m.K = b.cexp; m.lda = b.cexp; m.ldb = b.cexp; m.ldc = b.cout; m.act = 0; m.ss = ss;
    if (b.skip) { m.res = x; m.scale = branch_scale ? branch_scale + (int64_t)i * B : nullptr; }
    m.z_only = zo;
    bg_gemm(BG_FWD, m, 1, st);
    if (zo) bn_forward(b.R_out, b.cout, m.C, m.bn, b.o_e2, b.p_bn2, m.C2, b.skip ? GD_BN_SCALE_SKIP : GD_BN_PLAIN, m.res, m.scale, ss);
    x = ws + b.o_y;
  }
  for (int t = 0; t < 3; t++) {
    const BGBlock& b = p.b[p.taps[t]];
    hipLaunchKernelGGL(bg_nchw_from_rows_kernel, dim3(gd_blocks((int64_t)b.R_out * b.cout)), dim3(GD_THREADS), 0, st, B, b.cout, b.s_out * b.s_out,
                       (const float*)(ws + b.o_y), taps[t]);
  }
}

void launch_backbone_backward(const BGPlan& p, const float* const grad_taps[3], const float* branch_scale, float* grad_params,
                              float* grad_image, float* ws, hipStream_t st, const hep_sync* sync) {
  const int B = p.B;
  GDSync sy{};
  if (p.bn_sync) sy = bg_sync(p, ws, sync);
  const GDSync* const syp = p.bn_sync ? &sy : nullptr;
  float* pg = ws + p.o_pcol[0];
  float* pb = ws + p.o_pcol[1];
  const bool bb = p.bn_batch;       // batch statistics: the tables are the forward's effective ones; every d z is corrected before it is read
  for (int i = p.nblocks - 1; i >= 0; i--) {
    const BGBlock& b = p.b[i];
    const int ss = b.s_out * b.s_out, pad = b.stride == 1 ? (b.k - 1) / 2 : (b.k - 2) / 2;
    const float* x = i == 0 ? ws + p.o_as : ws + p.b[i - 1].o_y;
    // d y, bn2
    BGOutArgs oa{}; oa.ss = ss; oa.C = b.cout; oa.R = b.R_out; oa.tile_rows = bg_tile_rows(b.R_out);
    if (i + 1 < p.nblocks) { oa.gdata = ws + p.o_dx; if (p.b[i + 1].skip) oa.gskip = ws + p.o_dy[(i + 1) & 1]; }
    for (int t = 0; t < 3; t++) if (p.taps[t] == i) oa.cot = grad_taps[t];
    if (b.skip && branch_scale) oa.scale = branch_scale + (int64_t)i * B;
    oa.Z = ws + b.o_z2; oa.bn = bb ? ws + b.o_e2 : bg_pb(p, ws, i, b.p_bn2); oa.dY = ws + p.o_dy[i & 1]; oa.dZ = ws + p.o_dz2; oa.pgamma = pg; oa.pbeta = pb;
    hipLaunchKernelGGL(bg_out_bwd_kernel, dim3(gd_blocks((int64_t)bg_ntiles(b.R_out) * b.cout)), dim3(GD_THREADS), 0, st, oa);
    if (bb) bg_bn_backward(p, ws, b.R_out, b.cout, oa.Z, b.o_e2, ws + p.o_dz2, grad_params + b.p_bn2, st, syp);
    // project conv
    BGGemmArgs md{}; md.A = ws + p.o_dz2; md.Bm = bg_pb(p, ws, i, b.p_w2); md.C = ws + p.o_dxg; md.I = b.R_out; md.J = b.cexp; md.K = b.cout;
    md.lda = b.cout; md.ldb = b.cexp; md.ldc = b.cexp;
    bg_gemm(BG_DATA, md, 1, st);
    int sr, ns;
    bg_slabs(b.R_out, &sr, &ns);
    BGGemmArgs mw{}; mw.A = ws + p.o_dz2; mw.Bm = ws + b.o_xg; mw.C = ws + p.o_pw; mw.I = b.cout; mw.J = b.cexp; mw.K = b.R_out; mw.lda = b.cout; mw.ldb = b.cexp;
    mw.slab_rows = sr;
    bg_gemm(BG_WGRAD, mw, ns, st);
    {
      GDReduceArgs<BG_RED_JOBS> rd{};
      rd.j[0] = GDRedJob{ws + p.o_pw, grad_params + b.p_w2, (int64_t)b.cout * b.cexp, (int64_t)b.cout * b.cexp, ns};
      if (!bb) bg_bn_jobs(p, ws, b.R_out, b.cout, grad_params + b.p_bn2, &rd, 1);
      bg_reduce(rd, st);
    }
    // squeeze-excite
    int cr, nc;
    bg_chunks(ss, &cr, &nc);
    hipLaunchKernelGGL(bg_se_sum_kernel<false>, dim3(gd_blocks((int64_t)B * nc * b.cexp)), dim3(GD_THREADS), 0, st, B, ss, b.cexp, nc, cr,
                       (const float*)(ws + p.o_dxg), (const float*)(ws + b.o_z1), bb ? (const float*)(ws + b.o_e1) : bg_pa(p, ws, i, b.p_bn1), ws + p.o_pse);
    hipLaunchKernelGGL(bg_se_bwd_kernel, dim3(B), dim3(GD_THREADS), 0, st, ss, b.cexp, b.se, nc, (const float*)(ws + p.o_pse), bg_pa(p, ws, i, b.p_wr),
                       bg_pa(p, ws, i, b.p_we), (const float*)(ws + b.o_r), (const float*)(ws + b.o_g), ws + p.o_dl, ws + p.o_dr, ws + p.o_dm);
    hipLaunchKernelGGL(bg_se_wgrad_kernel, dim3(gd_blocks(b.p_w2 - b.p_wr)), dim3(GD_THREADS), 0, st, B, b.cexp, b.se, (const float*)(ws + b.o_m),
                       (const float*)(ws + b.o_r), (const float*)(ws + p.o_dl), (const float*)(ws + p.o_dr), grad_params + b.p_wr);
    // gate, swish, bn1: d z1 in place of d xg
    BGActArgs aa{}; aa.ss = ss; aa.C = b.cexp; aa.R = b.R_out; aa.tile_rows = bg_tile_rows(b.R_out);
    aa.G = ws + p.o_dxg; aa.Z = ws + b.o_z1; aa.bn = bb ? ws + b.o_e1 : bg_pa(p, ws, i, b.p_bn1); aa.gate = ws + b.o_g; aa.dmean = ws + p.o_dm; aa.pgamma = pg; aa.pbeta = pb;
    hipLaunchKernelGGL(bg_act_bwd_kernel, dim3(gd_blocks((int64_t)bg_ntiles(b.R_out) * b.cexp)), dim3(GD_THREADS), 0, st, aa);
    if (bb) bg_bn_backward(p, ws, b.R_out, b.cexp, aa.Z, b.o_e1, aa.G, grad_params + b.p_bn1, st, syp);
    // depthwise
    const float* dwin = b.expand ? ws + b.o_a0 : x;
    float* ddw = b.expand ? ws + p.o_da0 : ws + p.o_dx;
    const unsigned gw = gd_blocks((int64_t)bg_ntiles(b.R_out) * b.cexp), gd = gd_blocks((int64_t)b.R_in * b.cexp);
    if (b.k == 3) {
      hipLaunchKernelGGL(bg_dw_wgrad_kernel<3>, dim3(gw), dim3(GD_THREADS), 0, st, b.s_in, b.s_out, b.stride, pad, b.cexp, b.R_out, bg_tile_rows(b.R_out),
                         (const float*)(ws + p.o_dxg), dwin, ws + p.o_pdw);
      hipLaunchKernelGGL(bg_dw_dgrad_kernel<3>, dim3(gd), dim3(GD_THREADS), 0, st, B, b.s_in, b.s_out, b.stride, pad, b.cexp, (const float*)(ws + p.o_dxg),
                         bg_pa(p, ws, i, b.p_dw), ddw);
    } else {
      hipLaunchKernelGGL(bg_dw_wgrad_kernel<5>, dim3(gw), dim3(GD_THREADS), 0, st, b.s_in, b.s_out, b.stride, pad, b.cexp, b.R_out, bg_tile_rows(b.R_out),
                         (const float*)(ws + p.o_dxg), dwin, ws + p.o_pdw);
      hipLaunchKernelGGL(bg_dw_dgrad_kernel<5>, dim3(gd), dim3(GD_THREADS), 0, st, B, b.s_in, b.s_out, b.stride, pad, b.cexp, (const float*)(ws + p.o_dxg),
                         bg_pa(p, ws, i, b.p_dw), ddw);
    }
    {
      GDReduceArgs<BG_RED_JOBS> rd{};
      const int64_t n = (int64_t)b.cexp * b.k * b.k;
      rd.j[0] = GDRedJob{ws + p.o_pdw, grad_params + b.p_dw, n, n, bg_ntiles(b.R_out)};
      if (!bb) bg_bn_jobs(p, ws, b.R_out, b.cexp, grad_params + b.p_bn1, &rd, 1);
      bg_reduce(rd, st);
    }
    // expand conv
    if (b.expand) {
      BGActArgs ea{}; ea.ss = b.s_in * b.s_in; ea.C = b.cexp; ea.R = b.R_in; ea.tile_rows = bg_tile_rows(b.R_in);
      ea.G = ws + p.o_da0; ea.Z = ws + b.o_z0; ea.bn = bb ? ws + b.o_e0 : bg_pa(p, ws, i, b.p_bn0); ea.pgamma = pg; ea.pbeta = pb;
      hipLaunchKernelGGL(bg_act_bwd_kernel, dim3(gd_blocks((int64_t)bg_ntiles(b.R_in) * b.cexp)), dim3(GD_THREADS), 0, st, ea);
      if (bb) bg_bn_backward(p, ws, b.R_in, b.cexp, ea.Z, b.o_e0, ea.G, grad_params + b.p_bn0, st, syp);
      bg_slabs(b.R_in, &sr, &ns);
      BGGemmArgs ew{}; ew.A = ws + p.o_da0; ew.Bm = x; ew.C = ws + p.o_pw; ew.I = b.cexp; ew.J = b.cin; ew.K = b.R_in; ew.lda = b.cexp; ew.ldb = b.cin;
      ew.slab_rows = sr;
      bg_gemm(BG_WGRAD, ew, ns, st);
      BGGemmArgs ed{}; ed.A = ws + p.o_da0; ed.Bm = bg_pa(p, ws, i, b.p_w0); ed.C = ws + p.o_dx; ed.I = b.R_in; ed.J = b.cin; ed.K = b.cexp;
      ed.lda = b.cexp; ed.ldb = b.cin; ed.ldc = b.cin;
      bg_gemm(BG_DATA, ed, 1, st);
      GDReduceArgs<BG_RED_JOBS> rd{};
      rd.j[0] = GDRedJob{ws + p.o_pw, grad_params + b.p_w0, (int64_t)b.cexp * b.cin, (int64_t)b.cexp * b.cin, ns};
      if (!bb) bg_bn_jobs(p, ws, b.R_in, b.cexp, grad_params + b.p_bn0, &rd, 1);
      bg_reduce(rd, st);
    }
  }
  // the stem: d as = block 0's data path (block 0 never adds its input)
  const float* ps = ws + p.q_stem;
  BGActArgs sa{}; sa.ss = p.s0 * p.s0; sa.C = p.stem; sa.R = p.R0; sa.tile_rows = bg_tile_rows(p.R0);
  sa.G = ws + p.o_dx; sa.Z = ws + p.o_zs; sa.bn = bb ? ws + p.o_es : ps + (p.p_bn_stem - p.p_stem); sa.pgamma = pg; sa.pbeta = pb;
  hipLaunchKernelGGL(bg_act_bwd_kernel, dim3(gd_blocks((int64_t)bg_ntiles(p.R0) * p.stem)), dim3(GD_THREADS), 0, st, sa);
  if (bb) bg_bn_backward(p, ws, p.R0, p.stem, sa.Z, p.o_es, sa.G, grad_params + p.p_bn_stem, st, syp);
  hipLaunchKernelGGL(bg_stem_wgrad_kernel, dim3(gd_blocks((int64_t)bg_ntiles(p.R0) * p.stem)), dim3(GD_THREADS), 0, st, B, p.size, p.stem, p.R0,
                     bg_tile_rows(p.R0), (const float*)(ws + p.o_dx), (const float*)(ws + p.o_img), ws + p.o_pdw);
  GDReduceArgs<BG_RED_JOBS> rd{};
  rd.j[0] = GDRedJob{ws + p.o_pdw, grad_params + p.p_stem, (int64_t)p.stem * 27, (int64_t)p.stem * 27, bg_ntiles(p.R0)};
  if (!bb) bg_bn_jobs(p, ws, p.R0, p.stem, grad_params + p.p_bn_stem, &rd, 1);
  bg_reduce(rd, st);
  if (grad_image)
    hipLaunchKernelGGL(bg_stem_dgrad_kernel, dim3(gd_blocks((int64_t)B * 3 * p.size * p.size)), dim3(GD_THREADS), 0, st, B, p.size, p.stem,
                       (const float*)(ws + p.o_dx), ps, grad_image);
}
