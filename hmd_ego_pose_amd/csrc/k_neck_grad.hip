// k_neck_grad.hip - training forward and backward of the BiFPN neck (all fpn_cells cells of bifpn.{r}; reference
// efficientdet/model.py:194-266, fast-attention fusion, phi 0..5) on gfx950, fp32, as a function of (its parameters, the
// three backbone taps P3 / P4 / P5).  By default the function is the inference function: BatchNorm uses the RUNNING statistics in
// forward and backward; gamma and beta get gradients, the statistics get zero.  HEP_BN_BATCH: every BatchNorm (laterals and nodes)
// normalises with the statistics of its map's rows (the shared passes of grad_dev.h): gemm<FWD> stores z only, then statistics /
// finish / apply; in the backward the gamma / beta reduce and the d z correction follow the gather, ahead of the products.
//
// Plain layouts, as k_head_grad.hip has (the GEMM tile, the 3 x 3 window and the reduce are grad_dev.h's): every map is
// rows [B * s * s][C], channels contiguous, one buffer per map.  The flat parameter buffer starts every cell with 19 fusion scalars, so no tensor behind them is 16-byte aligned:
// the forward first copies each cell to workspace[4 * k + 1], which puts every conv / BatchNorm tensor on a 16-byte boundary
// for the GEMMs' float4 loads; forward and backward read the parameters from that copy.
//
//   node      s = sum_i w_i * src_i (src: same-size map | nearest x2 of the level above | maxpool_same of the level below),
//             w = relu(p) / (sum relu(p) + 1e-4);  x = swish(s);  u = depthwise3x3(x);  z = u . Wp^T + b;  y = bn(z)
//   forward   pack; rows_from_nchw (taps); 6 lateral gemm<FWD>; 2 pools; per node fuse_fwd (stores s, x and the pool's
//             argmax bytes), dw_fwd, gemm<FWD> (stores z and y); nchw_from_rows (the five maps)
//   backward  per node, last cell first, within a cell 7d 6d 5d 4d 3u 4u 5u 6u:
//             gather (the gradient of the node's OUTPUT map in gather form: every destination element adds, in a fixed
//             order, the cotangent and w_i * d s of each consumer - same element | its 2 x 2 children | the at most four pool
//             windows that contain it and whose argmax it is - then BatchNorm: d z, gamma / beta / bias partials);
//             gemm<DATA> (d u = d z . Wp); gemm<WGRAD> (d Wp = d z^T . u, pixels as K, split into slabs); dw_bwd (depthwise
//             weight partials, d x = the 3x3 with mirrored taps, d s = d x * swish'(s), the partials of <d s, src_i>);
//             reduce (second pass over slabs and tiles); fusion (the dot products' second pass, the Jacobian of the
//             normalisation and the relu gate).  Then the laterals of cell 0 (gather, WGRAD, DATA, reduce) and the taps.
// Max-pool routing: zero padding is one column right and one row at the bottom (pooled sides are even); a window's gradient
// goes to the FIRST maximal element in row-major order of the padded window (strict > while scanning), padding included -
// a padding argmax matches no real element, so that window's gradient is dropped.
// The pointwise products are v_mfma_f32_16x16x4_f32 (gd_gemm_tile of grad_dev.h).  Every reduction is partial sums in a
// fixed order plus a fixed-order second pass in double (gd_reduce_kernel): bit-reproducible, no float atomics.
#include <cstdio>

#include "hep.h"
#include "grad_dev.h"
#include "hep_train.h"

#define NG_FUSION_EPS 1e-4f
#define NG_RED_JOBS 6        // reduce jobs of one launch: pointwise weight, depthwise weight, gamma, beta, statistics, bias

enum { NG_SAME = 0, NG_UP = 1, NG_POOL = 2 };

static const int kNeckWidth[6] = {64, 88, 112, 160, 224, 288};
static const int kNeckCells[6] = {3, 4, 5, 6, 7, 7};
static const int kNeckTaps[6][3] = {{40, 112, 320}, {40, 112, 320}, {48, 120, 352}, {48, 136, 384}, {56, 160, 448}, {64, 176, 512}};
// nodes in state_dict order: conv6_up conv5_up conv4_up conv3_up conv4_down conv5_down conv6_down conv7_down
static const int kNodeLevel[NG_NODES] = {3, 2, 1, 0, 1, 2, 3, 4};
static const int kNodeNsrc[NG_NODES] = {2, 2, 2, 2, 3, 3, 3, 2};
static const int kNodeFw[NG_NODES] = {0, 2, 4, 6, 8, 11, 14, 17};       // offset of the node's fusion vector in the cell
// source maps of a node: 0..4 the cell's inputs P3..P7, 5 / 6 the second P4 / P5 input (cell 0: *_down_channel_2), 8 + j node j
static const int kNodeSrc[NG_NODES][3] = {{3, 4, -1}, {2, 8, -1}, {1, 9, -1}, {0, 10, -1}, {5, 10, 11}, {6, 9, 12}, {3, 8, 13}, {4, 14, -1}};
static const int kNodeMode[NG_NODES][3] = {{NG_SAME, NG_UP, 0}, {NG_SAME, NG_UP, 0}, {NG_SAME, NG_UP, 0}, {NG_SAME, NG_UP, 0},
                                           {NG_SAME, NG_SAME, NG_POOL}, {NG_SAME, NG_SAME, NG_POOL}, {NG_SAME, NG_SAME, NG_POOL}, {NG_SAME, NG_POOL, 0}};
static const int kOutNode[5] = {3, 4, 5, 6, 7};                           // the node whose output is the cell's P3..P7
// laterals in state_dict order: p5_down_channel p4_down_channel p3_down_channel p5_to_p6 p4_down_channel_2 p5_down_channel_2
static const int kLatTap[NG_LATERALS] = {2, 1, 0, 2, 1, 2};
static const int kLatCode[NG_LATERALS] = {2, 1, 0, -1, 5, 6};             // the cell-0 input it is (-1: p6_pre, pooled into P6)

// w_i = relu(p_i) / (sum_k relu(p_k) + 1e-4); p == NULL: 1 (a pool that is not a fusion source)
__device__ __forceinline__ float ng_fusion_weight(const float* __restrict__ p, int n, int i) {
  if (!p) return 1.0f;
  float sum = 0.0f;
  for (int k = 0; k < n; k++) sum += fmaxf(p[k], 0.0f);
  return fmaxf(p[i], 0.0f) / (sum + NG_FUSION_EPS);
}

// maxpool_same(3, 2) window of output (oy, ox) over a map of even side sf: the first maximum in row-major order of the
// padded window (zeros right / below), its position 0..8 in *arg
__device__ __forceinline__ float ng_pool_window(const float* __restrict__ p, int b, int sf, int oy, int ox, int W, int c, int* arg) {
  float best = 0.0f;
  int at = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int yy = 2 * oy + k / 3, xx = 2 * ox + k % 3;
    const float v = (yy < sf && xx < sf) ? p[((int64_t)(b * sf + yy) * sf + xx) * W + c] : 0.0f;
    if (k == 0 || v > best) { best = v; at = k; }
  }
  *arg = at;
  return best;
}
// the pooled value again, from the stored argmax
__device__ __forceinline__ float ng_pool_value(const float* __restrict__ p, const uint8_t* __restrict__ am, int b, int sf, int oy, int ox, int W, int c) {
  const int so = sf >> 1, k = am[((int64_t)(b * so + oy) * so + ox) * W + c];
  const int yy = 2 * oy + k / 3, xx = 2 * ox + k % 3;
  return (yy < sf && xx < sf) ? p[((int64_t)(b * sf + yy) * sf + xx) * W + c] : 0.0f;
}

struct NGSrc { const float* p; const uint8_t* am; int mode; };
// source value of a node element (b, y, x, c) of side s, r its row; the pool's argmax comes from the forward
__device__ __forceinline__ float ng_src_value(const NGSrc& q, int r, int b, int y, int x, int s, int W, int c) {
  if (q.mode == NG_SAME) return q.p[(int64_t)r * W + c];
  if (q.mode == NG_UP) { const int sh = s >> 1; return q.p[((int64_t)(b * sh + (y >> 1)) * sh + (x >> 1)) * W + c]; }
  return ng_pool_value(q.p, q.am, b, 2 * s, y, x, W, c);
}

// ------------------------------------------------------------------------------------------------------------------
struct NGPackArgs { int cells; int64_t src[NG_MAX_CELLS + 1], dst[NG_MAX_CELLS]; };
// the flat parameters, cell by cell, to their 16-byte friendly place in the workspace
__global__ __launch_bounds__(GD_THREADS) void ng_pack_kernel(NGPackArgs a, const float* __restrict__ params, float* __restrict__ ws) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= a.src[a.cells]) return;
  int r = 0;
  for (int i = 1; i < a.cells; i++) r += (idx >= a.src[i]);
  ws[a.dst[r] + (idx - a.src[r])] = params[idx];
}

// NCHW [B][C][s][s] -> rows [B * s * s][C]
__global__ __launch_bounds__(GD_THREADS) void ng_rows_from_nchw_kernel(int B, int C, int ss, const float* __restrict__ in, float* __restrict__ rows) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)B * ss * C) return;
  const int r = (int)(idx / C), c = (int)(idx % C), b = r / ss, pix = r % ss;
  rows[idx] = in[((int64_t)b * C + c) * ss + pix];
}
// rows -> NCHW, summing up to three row buffers in their order (the taps collect the data gradients of their laterals)
struct NGRows3 { const float* p[3]; int n; };
__global__ __launch_bounds__(GD_THREADS) void ng_nchw_from_rows_kernel(int B, int C, int ss, NGRows3 rows, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)B * ss * C) return;
  const int r = (int)(idx / C), c = (int)(idx % C), b = r / ss, pix = r % ss;
  float v = rows.p[0][idx];
  for (int i = 1; i < rows.n; i++) v += rows.p[i][idx];
  out[((int64_t)b * C + c) * ss + pix] = v;
}

// maxpool_same of a map of side sf (cell 0: p6_in = pool(p5_to_p6(P5)), p7_in = pool(p6_in)): values and argmax bytes
__global__ __launch_bounds__(GD_THREADS) void ng_pool_fwd_kernel(int B, int sf, int W, const float* __restrict__ in, float* __restrict__ out, uint8_t* __restrict__ am) {
  const int so = sf >> 1;
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)B * so * so * W) return;
  const int r = (int)(idx / W), c = (int)(idx % W), b = r / (so * so), pix = r % (so * so);
  int arg;
  out[idx] = ng_pool_window(in, b, sf, pix / so, pix % so, W, c, &arg);
  am[idx] = (uint8_t)arg;
}

// ------------------------------------------------------------------------------------------------------------------
struct NGFuseArgs {
  int B, s, W, n;
  NGSrc src[3]; uint8_t* am_out;      // am_out: where the pool source (if any) leaves its argmax
  const float* fw;                    // the node's fusion vector p
  float* S; float* X;                 // the pre-activation sum (kept for the backward) and swish of it (the depthwise input)
};
__global__ __launch_bounds__(GD_THREADS) void ng_fuse_fwd_kernel(NGFuseArgs a) {
  const int W = a.W, s = a.s, ss = s * s;
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)a.B * ss * W) return;
  const int r = (int)(idx / W), c = (int)(idx % W), b = r / ss, pix = r % ss, y = pix / s, x = pix % s;
  float acc = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; i++)
    if (i < a.n) {
      float v;
      if (a.src[i].mode == NG_POOL) {
        int arg;
        v = ng_pool_window(a.src[i].p, b, 2 * s, y, x, W, c, &arg);
        a.am_out[idx] = (uint8_t)arg;
      } else {
        v = ng_src_value(a.src[i], r, b, y, x, s, W, c);
      }
      const float w = ng_fusion_weight(a.fw, a.n, i);
      acc = i == 0 ? w * v : acc + w * v;
    }
  a.S[idx] = acc;
  a.X[idx] = acc * gd_sigmoid(acc);
}

// ------------------------------------------------------------------------------------------------------------------
// depthwise 3x3 SAME on the rows of one map; a thread = (GD_DW_ROWS consecutive rows, channel)
__global__ __launch_bounds__(GD_THREADS) void ng_dw_fwd_kernel(int R, int s, int W, const float* __restrict__ src, const float* __restrict__ wdw, float* __restrict__ dst) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int ra = (int)(idx / W) * GD_DW_ROWS, c = (int)(idx % W);
  if (ra >= R) return;
  const int rb = min(R, ra + GD_DW_ROWS), ss = s * s;
  float w[9], v[3][3];
  gd_dw_taps(w, wdw, c);
  for (int r = ra; r < rb; r++) {
    const int pix = r % ss, y = pix / s, x = pix % s;
    gd_win_step<false>(v, r == ra || x == 0, src, r, y, x, s, W, c);
    dst[(int64_t)r * W + c] = gd_dw_dot(w, v);
  }
}

// ------------------------------------------------------------------------------------------------------------------
enum { NG_FWD = 0, NG_DATA = 1, NG_WGRAD = 2 };
struct NGGemmArgs {
  const float* A; const float* Bm; float* C; float* C2;
  const float* bias; const float* bn;          // FWD: [J]; gamma, beta, mean, var [4][J]
  int I, J, K, lda, ldb, ldc, ntn, slab_rows;
  int z_only;                                  // FWD with batch statistics: store z, the BatchNorm passes of grad_dev.h make y
};
// C[i][j] = sum_k A(i,k) B(k,j), 64 x 64 per workgroup, wave w owns rows 16w..16w+15 and four 16-column accumulators.
//   FWD     A = u rows (k contiguous), B = Wp [J][K] (k contiguous); z = C + bias -> C, bn(z) -> C2
//   DATA    A = d z rows (k contiguous), B = Wp [K][J] (j contiguous) -> C rows
//   WGRAD   A = d z rows read as (k = row, i = column), B = u rows (k = row); rows [z * slab_rows, ...) of K -> C[z][I][J]
template <int MODE> __global__ __launch_bounds__(GD_THREADS) void ng_gemm_kernel(NGGemmArgs a) {
  __shared__ __attribute__((aligned(16))) float As[GD_BK][GD_LDS_PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[GD_BK][GD_LDS_PITCH];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int I = a.I, J = a.J;
  const int i0 = (int)(blockIdx.x / a.ntn) * GD_BM, j0 = (int)(blockIdx.x % a.ntn) * GD_BN;
  if (i0 >= I || j0 >= J) return;                          // uniform over the workgroup
  int k_begin = 0, k_end = a.K;
  if (MODE == NG_WGRAD) { k_begin = blockIdx.z * a.slab_rows; k_end = min(a.K, k_begin + a.slab_rows); }
  f32x4 acc[4];
  gd_gemm_tile<MODE == NG_WGRAD ? GD_ROW_CONTIG : GD_K_CONTIG, MODE == NG_FWD ? GD_K_CONTIG : GD_ROW_CONTIG>(
      As, Bs, acc, a.A, a.lda, a.Bm, a.ldb, i0, I, j0, J, k_begin, k_end, k_end, t, lane, wv);
  gd_acc_visit(acc, i0, I, j0, J, lane, wv, [=](int m, int n, float v, const GDBn& q) {
    if (MODE == NG_FWD) {
      const float z = v + a.bias[n];
      a.C[(int64_t)m * a.ldc + n] = z;
      if (!a.z_only) a.C2[(int64_t)m * a.ldc + n] = gd_bn_apply(q, z);
    } else if (MODE == NG_DATA) {
      a.C[(int64_t)m * a.ldc + n] = v;
    } else {
      a.C[((int64_t)blockIdx.z * I + m) * J + n] = v;
    }
  }, [=](int n) { return MODE == NG_FWD ? gd_bn_load(a.bn, J, n) : GDBn{}; });
}

// ------------------------------------------------------------------------------------------------------------------
// One consumer of a map: the node whose source i it is (d s rows of that node, its fusion vector), or a plain pool
// (fw NULL: weight 1, g = the gradient of the pooled map).  mode as the FORWARD saw it from the consumer.
struct NGContrib { const float* g; const float* fw; const uint8_t* am; int n, idx, mode; };
struct NGGatherArgs {
  int B, s, W, R, nc;
  NGContrib c[NG_MAX_CONTRIB];
  const float* cot;                       // NCHW cotangent of this map (the last cell's outputs), or NULL
  const float* Z; const float* bn;        // the map's pre-BatchNorm rows and gamma, beta, mean, var; NULL: a pooled map, no BatchNorm
  float* out;                             // d z rows (or the map's gradient rows)
  float* pgamma; float* pbeta; float* pbias;   // [tile][W]
};
// Gradient of one map in gather form + the BatchNorm that produced it.  One thread = (tile of NG_TILE_ROWS rows, channel).
__global__ __launch_bounds__(GD_THREADS) void ng_gather_kernel(NGGatherArgs a) {
  const int W = a.W, s = a.s, ss = s * s;
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int tile = (int)(gid / W), c = (int)(gid % W);
  const int r0 = tile * NG_TILE_ROWS, r1 = min(a.R, r0 + NG_TILE_ROWS);
  if (r0 >= a.R) return;
  float wt[NG_MAX_CONTRIB];
#pragma unroll
  for (int i = 0; i < NG_MAX_CONTRIB; i++) wt[i] = i < a.nc ? ng_fusion_weight(a.c[i].fw, a.c[i].n, a.c[i].idx) : 0.0f;
  float gamma = 0.0f, mean = 0.0f, rstd = 0.0f;      // (no beta here, so not gd_bn_load)
  if (a.bn) { gamma = a.bn[c]; mean = a.bn[2 * W + c]; rstd = 1.0f / sqrtf(a.bn[3 * W + c] + GD_BN_EPS); }
  float ag = 0.0f, ab = 0.0f, abias = 0.0f;
  for (int r = r0; r < r1; r++) {
    const int b = r / ss, pix = r % ss, y = pix / s, x = pix % s;
    float g = a.cot ? a.cot[((int64_t)b * W + c) * ss + pix] : 0.0f;
#pragma unroll
    for (int i = 0; i < NG_MAX_CONTRIB; i++)
      if (i < a.nc) {
        const float* __restrict__ G = a.c[i].g;
        float v = 0.0f;
        if (a.c[i].mode == NG_SAME) {
          v = G[(int64_t)r * W + c];
        } else if (a.c[i].mode == NG_UP) {                  // the consumer is the finer level: the 2 x 2 children of (y, x)
          const int sf = 2 * s;
#pragma unroll
          for (int d = 0; d < 4; d++) v += G[((int64_t)(b * sf + 2 * y + (d >> 1)) * sf + 2 * x + (d & 1)) * W + c];
        } else {                                            // the consumer is the coarser level: the windows that contain (y, x)
          const int so = s >> 1;
          const uint8_t* __restrict__ am = a.c[i].am;
          for (int oy = (y >> 1) - ((y & 1) == 0 && y >= 2); oy <= (y >> 1); oy++)
            for (int ox = (x >> 1) - ((x & 1) == 0 && x >= 2); ox <= (x >> 1); ox++) {
              const int64_t o = ((int64_t)(b * so + oy) * so + ox) * W + c;
              if (am[o] == (y - 2 * oy) * 3 + (x - 2 * ox)) v += G[o];
            }
        }
        g = fmaf(wt[i], v, g);
      }
    if (a.bn) {
      const float zh = (a.Z[(int64_t)r * W + c] - mean) * rstd, dz = g * gamma * rstd;
      ag = fmaf(g, zh, ag); ab += g; abias += dz;
      a.out[(int64_t)r * W + c] = dz;
    } else {
      a.out[(int64_t)r * W + c] = g;
    }
  }
  if (a.bn) {
    a.pgamma[(int64_t)tile * W + c] = ag; a.pbeta[(int64_t)tile * W + c] = ab; a.pbias[(int64_t)tile * W + c] = abias;
  }
}

// ------------------------------------------------------------------------------------------------------------------
struct NGDwBwdArgs {
  int B, s, W, R, n;
  const float* G; const float* S; const float* w;     // d u rows, the node's pre-activation rows, depthwise weights [W][1][3][3]
  NGSrc src[3];
  float* DS;                                          // d s rows
  float* pdw; double* pf[3];                          // [tile][W * 9]; per source one double per workgroup (these dot products cancel heavily)
};
// One thread = (tile of NG_TILE_ROWS rows, channel); it walks the rows of its tile in order:
//   depthwise weight gradient  pdw[tap] += d u[r] * x[neighbour(r, tap)],  x = swish(s)
//   depthwise data gradient    d x[r]    = sum_tap w[8 - tap] * d u[neighbour(r, tap)]
//   fusion                     d s = d x * swish'(s);  pf[i] += d s * src_i   (exact products, added in double)
__global__ __launch_bounds__(GD_THREADS) void ng_dw_bwd_kernel(NGDwBwdArgs a) {
  __shared__ double red[3][GD_THREADS];
  const int W = a.W, s = a.s, ss = s * s, t = threadIdx.x;
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + t;
  const int tile = (int)(gid / W), c = (int)(gid % W);
  const int r0 = tile * NG_TILE_ROWS, r1 = min(a.R, r0 + NG_TILE_ROWS);
  double af[3] = {0.0, 0.0, 0.0};
  if (r0 < a.R) {
    float wt[9], aw[9];
#pragma unroll
    for (int tp = 0; tp < 9; tp++) { wt[tp] = a.w[c * 9 + tp]; aw[tp] = 0.0f; }
    float xw[3][3], gw[3][3];
    for (int r = r0; r < r1; r++) {
      const int b = r / ss, pix = r % ss, y = pix / s, x = pix % s;
      const bool fresh = r == r0 || x == 0;
      gd_win_step<true>(xw, fresh, a.S, r, y, x, s, W, c);
      gd_win_step<false>(gw, fresh, a.G, r, y, x, s, W, c);
      const float gk = gw[1][1];
      float dx = 0.0f;
#pragma unroll
      for (int tp = 0; tp < 9; tp++) {
        aw[tp] = fmaf(gk, xw[tp / 3][tp % 3], aw[tp]);
        dx = fmaf(wt[8 - tp], gw[tp / 3][tp % 3], dx);
      }
      const float ds = dx * gd_swish_grad(a.S[(int64_t)r * W + c]);
      a.DS[(int64_t)r * W + c] = ds;
#pragma unroll
      for (int i = 0; i < 3; i++)
        if (i < a.n) af[i] = fma((double)ds, (double)ng_src_value(a.src[i], r, b, y, x, s, W, c), af[i]);
    }
#pragma unroll
    for (int tp = 0; tp < 9; tp++) a.pdw[((int64_t)tile * W + c) * 9 + tp] = aw[tp];
  }
  // the workgroup's share of <d s, src_i>: a fixed-order tree over its 256 threads, one double per source and workgroup
#pragma unroll
  for (int i = 0; i < 3; i++) red[i][t] = af[i];
  __syncthreads();
  for (int h = GD_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int i = 0; i < 3; i++) red[i][t] += red[i][t + h];
    }
    __syncthreads();
  }
  if (t == 0)
    for (int i = 0; i < a.n; i++) a.pf[i][blockIdx.x] = red[i][0];
}

// ------------------------------------------------------------------------------------------------------------------
// The fusion vector's gradient: a_i = <d s, src_i> = the sum of the workgroup sums pf[i][0 .. count) (thread t adds t, t + 256, ... in double,
// thread 0 adds the 256 sums in order), then with r = relu(p), D = sum r + 1e-4, w = r / D:
//   d L / d p_j = (a_j - sum_i a_i w_i) / D  where p_j > 0, else exactly 0.
struct NGFusionArgs { const double* pf[3]; int n; int64_t count; const float* p; float* dp; };
__global__ __launch_bounds__(GD_THREADS) void ng_fusion_kernel(NGFusionArgs a) {
  __shared__ double part[3][GD_THREADS];
  for (int i = 0; i < a.n; i++) {
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < a.count; k += GD_THREADS) s += a.pf[i][k];
    part[i][threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double dot[3] = {0.0, 0.0, 0.0}, D = (double)NG_FUSION_EPS, mix = 0.0;
  for (int i = 0; i < a.n; i++) {
    for (int k = 0; k < GD_THREADS; k++) dot[i] += part[i][k];
    D += (double)fmaxf(a.p[i], 0.0f);
  }
  for (int i = 0; i < a.n; i++) mix += dot[i] * ((double)fmaxf(a.p[i], 0.0f) / D);
  for (int i = 0; i < a.n; i++) a.dp[i] = a.p[i] > 0.0f ? (float)((dot[i] - mix) / D) : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------------
// host side
static inline int64_t ng_node_stride(int W) { return (int64_t)9 * W + (int64_t)W * W + W + 4 * W; }
static inline int64_t ng_lat_stride(int W, int K) { return (int64_t)W * K + W + 4 * W; }

int neck_plan(int phi, int, int size, int batch, NGPlan* p, const char** why, int bn_mode, int sync) {
  if (phi == 6 || phi == 7) { *why = "neck: phi 6 and 7 fuse by plain sums at width 384 (no fast attention): not supported, phi must be in 0..5"; return HEP_ERR_UNSUPPORTED; }
  if (phi < 0 || phi > 5) { *why = "neck: phi must be in 0..5 (phi 8 needs a P8 level)"; return HEP_ERR_UNSUPPORTED; }
  if (bn_mode != HEP_BN_RUNNING && bn_mode != HEP_BN_BATCH) { *why = "neck: the BatchNorm mode must be HEP_BN_RUNNING or HEP_BN_BATCH"; return HEP_ERR_INVALID; }
  const int W = kNeckWidth[phi];
  p->bn_batch = bn_mode == HEP_BN_BATCH; p->bn_sync = p->bn_batch && sync;
  p->phi = phi; p->W = W; p->cells = kNeckCells[phi];
  for (int t = 0; t < 3; t++) p->tapc[t] = kNeckTaps[phi][t];
  int64_t o = 0;
  for (int r = 0; r < p->cells; r++) {
    p->p_cell[r] = o; o += NG_FUSION_FLOATS + NG_NODES * ng_node_stride(W);
    if (r == 0)
      for (int i = 0; i < NG_LATERALS; i++) { p->p_lat[i] = o; o += ng_lat_stride(W, p->tapc[kLatTap[i]]); }
  }
  p->p_cell[p->cells] = o;
  p->nparams = o;
  if (size == 0 && batch == 0) return 0;                   // layout only
  if (size < 128 || size > 2048 || size % 128 != 0) { *why = "neck: size must be a multiple of 128 in [128, 2048]"; return HEP_ERR_UNSUPPORTED; }
  if (batch < 1) { *why = "neck: batch must be at least 1"; return HEP_ERR_UNSUPPORTED; }
  if ((int64_t)batch * (size / 8) * (size / 8) > (1 << 22)) { *why = "neck: batch * pixels exceeds 4 Mi rows"; return HEP_ERR_UNSUPPORTED; }
  p->B = batch;
  if (p->bn_batch && !p->bn_sync && batch * (size / 128) * (size / 128) < 2) { *why = "neck: batch statistics need at least 2 rows per BatchNorm (batch * P7 pixels)"; return HEP_ERR_UNSUPPORTED; }
  for (int l = 0; l < 5; l++) {
    p->s[l] = size / (8 << l); p->R[l] = batch * p->s[l] * p->s[l];
    p->ntiles[l] = (p->R[l] + NG_TILE_ROWS - 1) / NG_TILE_ROWS;
    gd_slabs(p->R[l], NG_MAX_SLABS, &p->slab_rows[l], &p->nslab[l]);
  }
  int64_t w = 0;
  auto take = [&](int64_t n) { const int64_t at = w; w += (n + 3) / 4 * 4; return at; };
  for (int r = 0; r < p->cells; r++) p->o_pp[r] = take(p->p_cell[r + 1] - p->p_cell[r] + 4) + 1;   // + 19 fusion floats = 16-byte aligned
  for (int t = 0; t < 3; t++) p->o_tap[t] = take((int64_t)p->R[t] * p->tapc[t]);
  for (int i = 0; i < NG_LATERALS; i++) { p->o_lz[i] = take((int64_t)p->R[kLatTap[i]] * W); p->o_ly[i] = take((int64_t)p->R[kLatTap[i]] * W); }
  p->o_p6 = take((int64_t)p->R[3] * W); p->o_p7 = take((int64_t)p->R[4] * W);
  p->o_am6 = take(((int64_t)p->R[3] * W + 3) / 4); p->o_am7 = take(((int64_t)p->R[4] * W + 3) / 4);
  for (int r = 0; r < p->cells; r++)
    for (int j = 0; j < NG_NODES; j++) {
      const int64_t n = (int64_t)p->R[kNodeLevel[j]] * W;
      p->o_s[r][j] = take(n); p->o_u[r][j] = take(n); p->o_z[r][j] = take(n); p->o_y[r][j] = take(n);
      p->o_am[r][j] = j >= 4 ? take((n + 3) / 4) : 0;      // the down-path nodes pool the level below
    }
  const int64_t n0 = (int64_t)p->R[0] * W;
  p->o_x = take(n0); p->o_dz = take(n0); p->o_du = take(n0);
  for (int k = 0; k < 2; k++)
    for (int j = 0; j < NG_NODES; j++) p->o_ds[k][j] = take((int64_t)p->R[kNodeLevel[j]] * W);
  p->o_g6 = take((int64_t)p->R[3] * W); p->o_g7 = take((int64_t)p->R[4] * W);
  int kmax = W;
  for (int t = 0; t < 3; t++) if (p->tapc[t] > kmax) kmax = p->tapc[t];
  p->o_pw = take((int64_t)NG_MAX_SLABS * W * kmax);
  p->o_pdw = take((int64_t)p->ntiles[0] * W * 9);
  for (int k = 0; k < 3; k++) { p->o_pb[k] = take((int64_t)p->ntiles[0] * W); p->o_pf[k] = take((int64_t)2 * p->ntiles[0] * W); }
  for (int i = 0; i < NG_LATERALS; i++) p->o_dtap[i] = take((int64_t)p->R[kLatTap[i]] * p->tapc[kLatTap[i]]);
  p->o_bne = p->o_bnp = 0;
  if (p->bn_batch) {                                       // an effective table per BatchNorm (laterals, then cell by cell); [tile][W][2] doubles
    p->o_bne = take((int64_t)(NG_LATERALS + p->cells * NG_NODES) * 4 * W);
    p->o_bnp = take((int64_t)p->ntiles[0] * W * 4);
  }
  p->o_xch = p->bn_sync ? take(2 * gd_sync_doubles(1, W)) : 0;
  p->ws_floats = w;
  return 0;
}

// the tensors of the flat buffer in state_dict order: per cell 8 fusion vectors, per node (depthwise, pointwise, bias, BatchNorm's 4); behind cell 0 the laterals' 6
int neck_tensor_count(const NGPlan& p) { return p.cells * (NG_NODES + NG_NODES * 7) + NG_LATERALS * 6; }
void neck_tensor_offsets(const NGPlan& p, int64_t* out) {
  const int W = p.W;
  int k = 0;
  auto vectors = [&](int64_t at) { for (int t = 0; t < 5; t++) out[k++] = at + (int64_t)t * W; };      // bias, then the BatchNorm
  for (int r = 0; r < p.cells; r++) {
    for (int j = 0; j < NG_NODES; j++) out[k++] = p.p_cell[r] + kNodeFw[j];
    for (int j = 0; j < NG_NODES; j++) {
      const int64_t o = p.p_cell[r] + NG_FUSION_FLOATS + j * ng_node_stride(W);
      out[k++] = o; out[k++] = o + 9 * W; vectors(o + 9 * W + (int64_t)W * W);
    }
    if (r == 0)
      for (int i = 0; i < NG_LATERALS; i++) { out[k++] = p.p_lat[i]; vectors(p.p_lat[i] + (int64_t)W * p.tapc[kLatTap[i]]); }
  }
}

int neck_stage_count(const NGPlan& p) { return 2 + 5 * p.cells; }
// stage i: 0 p6_pre (the p5_to_p6 lateral's output), 1 bifpn0_p6_in, then bifpn{r}_p{3..7}; dims: [B, s, s, W] of the stage's level
int neck_stage(const NGPlan& p, int i, char name[32], int64_t dims[4], int64_t* offset_floats) {
  if (i < 0 || i >= neck_stage_count(p)) return -1;
  int level;
  if (i == 0) { snprintf(name, 32, "p6_pre"); level = 2; *offset_floats = p.o_ly[3]; }
  else if (i == 1) { snprintf(name, 32, "bifpn0_p6_in"); level = 3; *offset_floats = p.o_p6; }
  else {
    const int r = (i - 2) / 5, l = (i - 2) % 5;
    snprintf(name, 32, "bifpn%d_p%d", r, l + 3);
    level = l; *offset_floats = p.o_y[r][kOutNode[l]];
  }
  dims[0] = p.B; dims[1] = dims[2] = p.s[level]; dims[3] = p.W;
  return 0;
}

namespace {
// the maps a cell's nodes read, by source code (kNodeSrc)
const float* ng_map(const NGPlan& p, const float* ws, int cell, int code) {
  if (code >= 8) return ws + p.o_y[cell][code - 8];
  if (cell > 0) return ws + p.o_y[cell - 1][kOutNode[code == 5 ? 1 : code == 6 ? 2 : code]];
  switch (code) {
    case 0: return ws + p.o_ly[2];
    case 1: return ws + p.o_ly[1];
    case 2: return ws + p.o_ly[0];
    case 3: return ws + p.o_p6;
    case 4: return ws + p.o_p7;
    case 5: return ws + p.o_ly[4];
    default: return ws + p.o_ly[5];
  }
}
inline const float* ng_node_params(const NGPlan& p, const float* ws, int cell, int j) { return ws + p.o_pp[cell] + NG_FUSION_FLOATS + j * ng_node_stride(p.W); }
inline const float* ng_lat_params(const NGPlan& p, const float* ws, int i) { return ws + p.o_pp[0] + (p.p_lat[i] - p.p_cell[0]); }
inline uint8_t* ng_bytes(float* ws, int64_t off) { return reinterpret_cast<uint8_t*>(ws + off); }

void ng_node_sources(const NGPlan& p, float* ws, int cell, int j, NGSrc src[3]) {
  for (int i = 0; i < kNodeNsrc[j]; i++) {
    src[i].p = ng_map(p, ws, cell, kNodeSrc[j][i]);
    src[i].mode = kNodeMode[j][i];
    src[i].am = src[i].mode == NG_POOL ? ng_bytes(ws, p.o_am[cell][j]) : nullptr;
  }
}

void ng_gemm(int mode, const NGGemmArgs& m, int nslab, hipStream_t st) {
  const int ntm = (m.I + GD_BM - 1) / GD_BM;
  if (mode == NG_FWD) hipLaunchKernelGGL(ng_gemm_kernel<NG_FWD>, dim3(ntm * m.ntn), dim3(GD_THREADS), 0, st, m);
  else if (mode == NG_DATA) hipLaunchKernelGGL(ng_gemm_kernel<NG_DATA>, dim3(ntm * m.ntn), dim3(GD_THREADS), 0, st, m);
  else hipLaunchKernelGGL(ng_gemm_kernel<NG_WGRAD>, dim3(ntm * m.ntn, 1, nslab), dim3(GD_THREADS), 0, st, m);
}

// consumers of the map `code` among the nodes of `cell`, in node order
void ng_collect(const NGPlan& p, float* ws, int cell, int code, NGGatherArgs* ga) {
  for (int j = 0; j < NG_NODES; j++)
    for (int i = 0; i < kNodeNsrc[j]; i++) {
      int sc = kNodeSrc[j][i];
      if (cell > 0 && sc == 5) sc = 1;
      if (cell > 0 && sc == 6) sc = 2;
      if (sc != code) continue;
      NGContrib& c = ga->c[ga->nc++];
      c.g = ws + p.o_ds[cell & 1][j]; c.fw = ws + p.o_pp[cell] + kNodeFw[j]; c.n = kNodeNsrc[j]; c.idx = i; c.mode = kNodeMode[j][i];
      c.am = c.mode == NG_POOL ? ng_bytes(ws, p.o_am[cell][j]) : nullptr;
    }
}
void ng_collect_pool(float* g, uint8_t* am, NGGatherArgs* ga) {
  NGContrib& c = ga->c[ga->nc++];
  c.g = g; c.fw = nullptr; c.am = am; c.n = 0; c.idx = 0; c.mode = NG_POOL;
}

// BatchNorm partials [tile][W] -> gamma, beta, zeros for the statistics, and the conv bias (batch statistics: analytically
// zero, written as zero)
void ng_bn_jobs(const NGPlan& p, float* ws, int level, float* dbias, float* dbn, GDReduceArgs<NG_RED_JOBS>* rd, int at) {
  const int W = p.W, T = p.ntiles[level];
  rd->j[at + 0] = GDRedJob{ws + p.o_pb[0], dbn, W, W, T};
  rd->j[at + 1] = GDRedJob{ws + p.o_pb[1], dbn + W, W, W, T};
  rd->j[at + 2] = GDRedJob{nullptr, dbn + 2 * W, 2 * W, 0, 0};
  rd->j[at + 3] = p.bn_batch ? GDRedJob{nullptr, dbias, W, 0, 0} : GDRedJob{ws + p.o_pb[2], dbias, W, W, T};
}

// Batch statistics.  BatchNorm k (laterals 0..5, then 6 + 8 cell + node) as a job of grad_dev.h's kernels: its effective table,
// and where its gamma, beta, mean, var lie in the flat parameter layout (table_at).
inline float* ng_bn_eff(const NGPlan& p, float* ws, int k) { return ws + p.o_bne + (int64_t)k * 4 * p.W; }
GDBnArgs<1> ng_bn_job(const NGPlan& p, float* ws, int k, int level, const float* z, const float* bn) {
  GDBnArgs<1> a{};
  a.tile_rows = NG_TILE_ROWS;
  a.j[0].z = z; a.j[0].bn = bn; a.j[0].eff = ng_bn_eff(p, ws, k);
  a.j[0].part = reinterpret_cast<double*>(ws + p.o_bnp);
  a.j[0].R = p.R[level]; a.j[0].C = p.W;
  return a;
}
// what follows a map's gather in the backward: its gamma / beta reduce first, then d z (ws + o_dz) corrected in place - before
// any product reads it; the stage's own reduce then has the weight jobs only
inline GDSync ng_sync(const NGPlan& p, float* ws, const hep_sync* sync) { return GDSync{sync->sum, sync->ctx, reinterpret_cast<double*>(ws + p.o_xch)}; }
void ng_bn_backward(const NGPlan& p, float* ws, int k, int level, const float* z, float* dbias, float* dbn, hipStream_t st, const GDSync* sy) {
  GDReduceArgs<NG_RED_JOBS> rd{};
  ng_bn_jobs(p, ws, level, dbias, dbn, &rd, 2);
  hipLaunchKernelGGL(gd_reduce_kernel<NG_RED_JOBS>, dim3((unsigned)((2 * p.W + GD_RED_E - 1) / GD_RED_E), NG_RED_JOBS), dim3(GD_THREADS), 0, st, rd);
  GDBnArgs<1> a = ng_bn_job(p, ws, k, level, z, nullptr);
  a.j[0].io = ws + p.o_dz; a.j[0].dbn = dbn;
  a.j[0].pg = ws + p.o_pb[0]; a.j[0].pb = ws + p.o_pb[1]; a.j[0].pn = p.ntiles[level]; a.j[0].pstride = p.W;
  gd_bn_dz(a, p.R[level], p.W, st, sy);
}
}  // namespace

void launch_neck_forward(const NGPlan& p, const float* params, const float* const taps[3], float* const feats[5], float* ws, hipStream_t st,
                         float momentum, float* stats_out, const hep_sync* sync) {
  const int W = p.W, B = p.B;
  GDSync sy{};
  if (p.bn_sync) sy = ng_sync(p, ws, sync);
  // batch statistics: z (what the GEMM left) -> statistics -> the effective table and the running-statistics update -> y
  auto bn_forward = [&](int k, int level, const NGGemmArgs& m, int64_t table_at) {
    GDBnArgs<1> a = ng_bn_job(p, ws, k, level, m.C, m.bn);
    a.momentum = momentum;
    a.j[0].io = m.C2; a.j[0].stats = stats_out ? stats_out + table_at : nullptr;
    gd_bn_forward(a, p.R[level], W, GD_BN_PLAIN, st, p.bn_sync ? &sy : nullptr);
  };
  NGPackArgs pk{}; pk.cells = p.cells;
  for (int r = 0; r < p.cells; r++) { pk.src[r] = p.p_cell[r]; pk.dst[r] = p.o_pp[r]; }
  pk.src[p.cells] = p.nparams;
  hipLaunchKernelGGL(ng_pack_kernel, dim3(gd_blocks(p.nparams)), dim3(GD_THREADS), 0, st, pk, params, ws);
  for (int t = 0; t < 3; t++)
    hipLaunchKernelGGL(ng_rows_from_nchw_kernel, dim3(gd_blocks((int64_t)p.R[t] * p.tapc[t])), dim3(GD_THREADS), 0, st, B, p.tapc[t], p.s[t] * p.s[t], taps[t], ws + p.o_tap[t]);
  for (int i = 0; i < NG_LATERALS; i++) {
    const int t = kLatTap[i], K = p.tapc[t];
    const float* lp = ng_lat_params(p, ws, i);
    NGGemmArgs m{}; m.A = ws + p.o_tap[t]; m.Bm = lp; m.bias = lp + (int64_t)W * K; m.bn = lp + (int64_t)W * K + W;
    m.C = ws + p.o_lz[i]; m.C2 = ws + p.o_ly[i]; m.I = p.R[t]; m.J = W; m.K = K; m.lda = K; m.ldb = K; m.ldc = W; m.ntn = (W + GD_BN - 1) / GD_BN;
    m.z_only = p.bn_batch;
    ng_gemm(NG_FWD, m, 1, st);
    if (p.bn_batch) bn_forward(i, t, m, p.p_lat[i] + (int64_t)W * K + W);
  }
  hipLaunchKernelGGL(ng_pool_fwd_kernel, dim3(gd_blocks((int64_t)p.R[3] * W)), dim3(GD_THREADS), 0, st, B, p.s[2], W, (const float*)(ws + p.o_ly[3]), ws + p.o_p6, ng_bytes(ws, p.o_am6));
  hipLaunchKernelGGL(ng_pool_fwd_kernel, dim3(gd_blocks((int64_t)p.R[4] * W)), dim3(GD_THREADS), 0, st, B, p.s[3], W, (const float*)(ws + p.o_p6), ws + p.o_p7, ng_bytes(ws, p.o_am7));
  for (int r = 0; r < p.cells; r++)
    for (int j = 0; j < NG_NODES; j++) {
      const int l = kNodeLevel[j], R = p.R[l];
      const float* np = ng_node_params(p, ws, r, j);
      NGFuseArgs f{}; f.B = B; f.s = p.s[l]; f.W = W; f.n = kNodeNsrc[j];
      ng_node_sources(p, ws, r, j, f.src);
      f.am_out = j >= 4 ? ng_bytes(ws, p.o_am[r][j]) : nullptr;
      f.fw = ws + p.o_pp[r] + kNodeFw[j]; f.S = ws + p.o_s[r][j]; f.X = ws + p.o_x;
      hipLaunchKernelGGL(ng_fuse_fwd_kernel, dim3(gd_blocks((int64_t)R * W)), dim3(GD_THREADS), 0, st, f);
      hipLaunchKernelGGL(ng_dw_fwd_kernel, dim3(gd_blocks((int64_t)((R + GD_DW_ROWS - 1) / GD_DW_ROWS) * W)), dim3(GD_THREADS), 0, st, R, p.s[l], W,
                         (const float*)(ws + p.o_x), np, ws + p.o_u[r][j]);
      NGGemmArgs m{}; m.A = ws + p.o_u[r][j]; m.Bm = np + 9 * W; m.bias = np + 9 * W + (int64_t)W * W; m.bn = m.bias + W;
      m.C = ws + p.o_z[r][j]; m.C2 = ws + p.o_y[r][j]; m.I = R; m.J = W; m.K = W; m.lda = W; m.ldb = W; m.ldc = W; m.ntn = (W + GD_BN - 1) / GD_BN;
      m.z_only = p.bn_batch;
      ng_gemm(NG_FWD, m, 1, st);
      if (p.bn_batch) bn_forward(NG_LATERALS + r * NG_NODES + j, l, m, p.p_cell[r] + NG_FUSION_FLOATS + j * ng_node_stride(W) + 9 * W + (int64_t)W * W + W);
    }
  for (int l = 0; l < 5; l++) {
    NGRows3 rows{}; rows.p[0] = ws + p.o_y[p.cells - 1][kOutNode[l]]; rows.n = 1;
    hipLaunchKernelGGL(ng_nchw_from_rows_kernel, dim3(gd_blocks((int64_t)p.R[l] * W)), dim3(GD_THREADS), 0, st, B, W, p.s[l] * p.s[l], rows, feats[l]);
  }
}

void launch_neck_backward(const NGPlan& p, const float* const grad_feats[5], float* grad_params, float* const grad_taps[3], float* ws, hipStream_t st,
                          const hep_sync* sync) {
  const int W = p.W, B = p.B, ntn = (W + GD_BN - 1) / GD_BN;
  GDSync sy{};
  if (p.bn_sync) sy = ng_sync(p, ws, sync);
  const GDSync* const syp = p.bn_sync ? &sy : nullptr;
  auto gather = [&](NGGatherArgs& ga, int l) {
    ga.B = B; ga.s = p.s[l]; ga.W = W; ga.R = p.R[l];
    ga.pgamma = ws + p.o_pb[0]; ga.pbeta = ws + p.o_pb[1]; ga.pbias = ws + p.o_pb[2];
    hipLaunchKernelGGL(ng_gather_kernel, dim3(gd_blocks((int64_t)p.ntiles[l] * W)), dim3(GD_THREADS), 0, st, ga);
  };
  for (int r = p.cells - 1; r >= 0; r--) {
    float* gcell = grad_params + p.p_cell[r];
    for (int j = NG_NODES - 1; j >= 0; j--) {               // 7d 6d 5d 4d 3u 4u 5u 6u: every consumer of a map before the map
      const int l = kNodeLevel[j], R = p.R[l], T = p.ntiles[l];
      const float* np = ng_node_params(p, ws, r, j);
      float* gn = gcell + NG_FUSION_FLOATS + j * ng_node_stride(W);
      // the node's output map: its consumers in this cell, then in the next one (or the cotangent)
      NGGatherArgs ga{};
      int out_level = -1;
      for (int k = 0; k < 5; k++) if (kOutNode[k] == j) out_level = k;
      if (out_level >= 0 && r == p.cells - 1) ga.cot = grad_feats[out_level];
      ng_collect(p, ws, r, 8 + j, &ga);
      if (out_level >= 0 && r + 1 < p.cells) ng_collect(p, ws, r + 1, out_level, &ga);
      const int bk = NG_LATERALS + r * NG_NODES + j;
      ga.Z = ws + p.o_z[r][j]; ga.bn = p.bn_batch ? ng_bn_eff(p, ws, bk) : np + 9 * W + (int64_t)W * W + W; ga.out = ws + p.o_dz;
      gather(ga, l);
      if (p.bn_batch) ng_bn_backward(p, ws, bk, l, ga.Z, gn + 9 * W + (int64_t)W * W, gn + 9 * W + (int64_t)W * W + W, st, syp);
      NGGemmArgs md{}; md.A = ws + p.o_dz; md.Bm = np + 9 * W; md.C = ws + p.o_du; md.I = R; md.J = W; md.K = W; md.lda = W; md.ldb = W; md.ldc = W; md.ntn = ntn;
      ng_gemm(NG_DATA, md, 1, st);
      NGGemmArgs mw{}; mw.A = ws + p.o_dz; mw.Bm = ws + p.o_u[r][j]; mw.C = ws + p.o_pw; mw.I = W; mw.J = W; mw.K = R; mw.lda = W; mw.ldb = W; mw.ntn = ntn;
      mw.slab_rows = p.slab_rows[l];
      ng_gemm(NG_WGRAD, mw, p.nslab[l], st);
      NGDwBwdArgs db{}; db.B = B; db.s = p.s[l]; db.W = W; db.R = R; db.n = kNodeNsrc[j];
      db.G = ws + p.o_du; db.S = ws + p.o_s[r][j]; db.w = np; db.DS = ws + p.o_ds[r & 1][j]; db.pdw = ws + p.o_pdw;
      ng_node_sources(p, ws, r, j, db.src);
      for (int i = 0; i < 3; i++) db.pf[i] = reinterpret_cast<double*>(ws + p.o_pf[i]);
      hipLaunchKernelGGL(ng_dw_bwd_kernel, dim3(gd_blocks((int64_t)T * W)), dim3(GD_THREADS), 0, st, db);
      GDReduceArgs<NG_RED_JOBS> rd{};
      rd.j[0] = GDRedJob{ws + p.o_pw, gn + 9 * W, (int64_t)W * W, (int64_t)W * W, p.nslab[l]};
      rd.j[1] = GDRedJob{ws + p.o_pdw, gn, (int64_t)W * 9, (int64_t)W * 9, T};
      if (!p.bn_batch) ng_bn_jobs(p, ws, l, gn + 9 * W + (int64_t)W * W, gn + 9 * W + (int64_t)W * W + W, &rd, 2);
      hipLaunchKernelGGL(gd_reduce_kernel<NG_RED_JOBS>, dim3((unsigned)(((int64_t)W * W + GD_RED_E - 1) / GD_RED_E), NG_RED_JOBS), dim3(GD_THREADS), 0, st, rd);
      NGFusionArgs fa{}; fa.n = kNodeNsrc[j]; fa.count = gd_blocks((int64_t)T * W); fa.p = ws + p.o_pp[r] + kNodeFw[j]; fa.dp = gcell + kNodeFw[j];
      for (int i = 0; i < 3; i++) fa.pf[i] = reinterpret_cast<const double*>(ws + p.o_pf[i]);
      hipLaunchKernelGGL(ng_fusion_kernel, dim3(1), dim3(GD_THREADS), 0, st, fa);
    }
  }
  // cell 0's own inputs.  p7_in and p6_in are pooled maps (no parameters): their gradients feed the pool below them.
  {
    NGGatherArgs g7{}; ng_collect(p, ws, 0, 4, &g7); g7.out = ws + p.o_g7; gather(g7, 4);
    NGGatherArgs g6{}; ng_collect(p, ws, 0, 3, &g6); ng_collect_pool(ws + p.o_g7, ng_bytes(ws, p.o_am7), &g6); g6.out = ws + p.o_g6; gather(g6, 3);
  }
  for (int i = 0; i < NG_LATERALS; i++) {
    const int t = kLatTap[i], K = p.tapc[t], R = p.R[t];
    const float* lp = ng_lat_params(p, ws, i);
    float* gl = grad_params + p.p_lat[i];
    NGGatherArgs ga{};
    if (kLatCode[i] >= 0) ng_collect(p, ws, 0, kLatCode[i], &ga);
    else ng_collect_pool(ws + p.o_g6, ng_bytes(ws, p.o_am6), &ga);
    ga.Z = ws + p.o_lz[i]; ga.bn = p.bn_batch ? ng_bn_eff(p, ws, i) : lp + (int64_t)W * K + W; ga.out = ws + p.o_dz;
    gather(ga, t);
    if (p.bn_batch) ng_bn_backward(p, ws, i, t, ga.Z, gl + (int64_t)W * K, gl + (int64_t)W * K + W, st, syp);
    NGGemmArgs mw{}; mw.A = ws + p.o_dz; mw.Bm = ws + p.o_tap[t]; mw.C = ws + p.o_pw; mw.I = W; mw.J = K; mw.K = R; mw.lda = W; mw.ldb = K;
    mw.ntn = (K + GD_BN - 1) / GD_BN; mw.slab_rows = p.slab_rows[t];
    ng_gemm(NG_WGRAD, mw, p.nslab[t], st);
    if (grad_taps) {
      NGGemmArgs md{}; md.A = ws + p.o_dz; md.Bm = lp; md.C = ws + p.o_dtap[i]; md.I = R; md.J = K; md.K = W; md.lda = W; md.ldb = K; md.ldc = K;
      md.ntn = (K + GD_BN - 1) / GD_BN;
      ng_gemm(NG_DATA, md, 1, st);
    }
    GDReduceArgs<NG_RED_JOBS> rd{};
    rd.j[0] = GDRedJob{ws + p.o_pw, gl, (int64_t)W * K, (int64_t)W * K, p.nslab[t]};
    rd.j[1] = GDRedJob{nullptr, nullptr, 0, 0, 0};
    if (!p.bn_batch) ng_bn_jobs(p, ws, t, gl + (int64_t)W * K, gl + (int64_t)W * K + W, &rd, 2);
    hipLaunchKernelGGL(gd_reduce_kernel<NG_RED_JOBS>, dim3((unsigned)(((int64_t)W * K + GD_RED_E - 1) / GD_RED_E), NG_RED_JOBS), dim3(GD_THREADS), 0, st, rd);
  }
  if (grad_taps)
    for (int t = 0; t < 3; t++) {
      NGRows3 rows{};
      for (int i = 0; i < NG_LATERALS; i++) if (kLatTap[i] == t) rows.p[rows.n++] = ws + p.o_dtap[i];
      hipLaunchKernelGGL(ng_nchw_from_rows_kernel, dim3(gd_blocks((int64_t)p.R[t] * p.tapc[t])), dim3(GD_THREADS), 0, st, B, p.tapc[t], p.s[t] * p.s[t], rows, grad_taps[t]);
    }
}
