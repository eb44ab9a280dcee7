// k_head_grad.hip - training forward and backward of the five head nets (regressor, classifier, rotation_net,
// translation_net, hand_net; reference efficientdet/model.py:361-417, hmdegopose/model.py:55-228 with
// num_iteration_steps == 0) on gfx950, fp32.  By default the function is the inference function: BatchNorm uses the RUNNING
// statistics in forward and backward (frozen-statistics fine-tuning); gamma and beta get gradients.  HEP_BN_BATCH: every
// bn_list.{level}.{i} normalises with the statistics of its level's rows (the shared passes of grad_dev.h): LAYER stores z only,
// then statistics / finish / apply per layer; in the backward the gamma / beta reduce of a layer and the d z correction run
// right behind the dw_bwd that produced them, ahead of the products that read d z.
//
// Plain layouts, none of the inference plan's (the GEMM tile, the 3 x 3 window and the reduce core are grad_dev.h's, shared
// with the neck and the backbone): the parameters are one flat buffer in the reference's shapes and state_dict order,
// activations are rows [R][W] (pixels of level 0 for every image, then level 1, ...; W channels contiguous), so one
// launch covers the five levels, and blockIdx.y covers the five nets (or the six header convs).
// Per layer   x -> u = depthwise3x3(x) -> z = u . Wp^T + b -> a = bn_level(z) -> x' = swish(a).
//
//   forward   rows_from_nchw; per layer dw_fwd + gemm<LAYER> (stores z and x'); headers dw_fwd + gemm<HEADER>
//             (stores into the [B][N][K] outputs, classifier through a sigmoid, its logits kept)
//   backward  hdr_gather (cotangents -> rows, header-bias partials); gemm<DATA> (d u = d z . Wp); gemm<WGRAD>
//             (d Wp = d z^T . u, pixels as K, split into slabs); dw_bwd (depthwise weight partials, depthwise data
//             gradient = the 3x3 with mirrored taps, then swish' and BatchNorm of the layer below: d z, gamma / beta /
//             bias partials); reduce (second pass over slabs and tiles); per layer the same four; feats_grad at the end.
// The pointwise products are v_mfma_f32_16x16x4_f32, four independent accumulators per wave.  Every reduction over
// pixels, images and levels is partial sums in a fixed order (a thread walks the rows of its tile; a slab is one MFMA
// chain) plus a second pass that adds the partials in a fixed order in double: bit-reproducible, no float atomics.
#include "hep.h"
#include "grad_dev.h"
#include "hep_train.h"

static const int kFpnWidth[8] = {64, 88, 112, 160, 224, 288, 384, 384};
static const int kHeadDepth[8] = {3, 3, 3, 4, 4, 4, 5, 5};

__device__ __forceinline__ int hg_level(const HGGeom& g, int r) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < 5; i++) l += (r >= g.rowoff[i]);
  return l;
}

// ------------------------------------------------------------------------------------------------------------------
struct HGPtr5 { const float* in[5]; float* out[5]; };

// feats[l] NCHW [B][W][s][s] -> rows [R][W]
__global__ __launch_bounds__(GD_THREADS) void hg_rows_from_nchw_kernel(HGGeom g, HGPtr5 f, float* __restrict__ x0) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (idx >= (int64_t)g.R * g.W) return;
  const int r = (int)(idx / g.W), c = (int)(idx % g.W);
  const int l = hg_level(g, r), ss = g.s[l] * g.s[l], q = r - g.rowoff[l], b = q / ss, pix = q % ss;
  x0[idx] = f.in[l][((int64_t)b * g.W + c) * ss + pix];
}

// grad_feats[l] NCHW = sum over the five nets (in net order) of the rows d x_0[net]
__global__ __launch_bounds__(GD_THREADS) void hg_feats_grad_kernel(HGGeom g, HGPtr5 f, const float* __restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x, rw = (int64_t)g.R * g.W;
  if (idx >= rw) return;
  const int r = (int)(idx / g.W), c = (int)(idx % g.W);
  const int l = hg_level(g, r), ss = g.s[l] * g.s[l], q = r - g.rowoff[l], b = q / ss, pix = q % ss;
  float v = dx[idx];
#pragma unroll
  for (int n = 1; n < HG_NETS; n++) v += dx[n * rw + idx];
  f.out[l][((int64_t)b * g.W + c) * ss + pix] = v;
}

// ------------------------------------------------------------------------------------------------------------------
struct HGDwArgs {
  HGGeom g;
  const float* src[HG_SLOTS]; const float* w[HG_SLOTS]; float* dst[HG_SLOTS];     // rows, [W][1][3][3], rows
};

// depthwise 3x3 SAME (zero padding 1) on rows; blockIdx.y = slot; a thread = (GD_DW_ROWS consecutive rows, channel)
__global__ __launch_bounds__(GD_THREADS) void hg_dw_fwd_kernel(HGDwArgs a) {
  const HGGeom& g = a.g;
  const int slot = blockIdx.y, W = g.W;
  const int64_t idx = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  const int ra = (int)(idx / W) * GD_DW_ROWS, c = (int)(idx % W);
  if (ra >= g.R) return;
  const int rb = min(g.R, ra + GD_DW_ROWS);
  const float* __restrict__ src = a.src[slot];
  float w[9], v[3][3];
  gd_dw_taps(w, a.w[slot], c);
  for (int r = ra; r < rb; r++) {
    const int l = hg_level(g, r), s = g.s[l], pix = (r - g.rowoff[l]) % (s * s), y = pix / s, x = pix % s;
    gd_win_step<false>(v, r == ra || x == 0, src, r, y, x, s, W, c);
    a.dst[slot][(int64_t)r * W + c] = gd_dw_dot(w, v);
  }
}

// ------------------------------------------------------------------------------------------------------------------
enum { HG_LAYER = 0, HG_HEADER = 1, HG_DATA = 2, HG_WGRAD = 3 };
struct HGGemmArgs {
  HGGeom g;
  int ntmax, bn_lstride, z_only;       // z_only (batch statistics): LAYER stores z, the BatchNorm passes of grad_dev.h make x'
  const float* A[HG_SLOTS]; const float* Bm[HG_SLOTS]; float* C[HG_SLOTS]; float* C2[HG_SLOTS];
  const float* bias[HG_SLOTS]; const float* bn[HG_SLOTS];
  int I[HG_SLOTS], J[HG_SLOTS], K[HG_SLOTS], Kb[HG_SLOTS], lda[HG_SLOTS], ldb[HG_SLOTS], ldc[HG_SLOTS];
  int hK[HG_SLOTS], hkh[HG_SLOTS], hoff[HG_SLOTS], sigmoid[HG_SLOTS];
};

// C[i][j] = sum_k A(i,k) B(k,j), 64 x 64 per workgroup, wave w owns rows 16w..16w+15 and four 16-column accumulators.
//   LAYER   A = u rows (k contiguous), B = Wp [J][K] (k contiguous); z = C + bias -> C, swish(bn_level(z)) -> C2
//   HEADER  the same product; C + bias (sigmoid for the classifier) -> the [B][N][K] output C2, the logits -> C (nullable)
//   DATA    A = d z rows (k contiguous, pitch lda = K, padding columns zero), B = Wp [Kb][J] (j contiguous) -> C rows
//   WGRAD   A = d z rows read as (k = row, i = column), B = u rows (k = row); rows [z * slab_rows, ...) -> C[z][I][J]
template <int MODE> __global__ __launch_bounds__(GD_THREADS) void hg_gemm_kernel(HGGemmArgs a) {
  __shared__ __attribute__((aligned(16))) float As[GD_BK][GD_LDS_PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[GD_BK][GD_LDS_PITCH];
  const HGGeom& g = a.g;
  const int slot = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int I = a.I[slot], J = a.J[slot];
  const int i0 = (int)(blockIdx.x / a.ntmax) * GD_BM, j0 = (int)(blockIdx.x % a.ntmax) * GD_BN;
  if (i0 >= I || j0 >= J) return;                          // uniform over the workgroup
  int k_begin = 0, k_end = a.K[slot];
  if (MODE == HG_WGRAD) { k_begin = blockIdx.z * g.slab_rows; k_end = min(g.R, k_begin + g.slab_rows); }
  const int kb_end = MODE == HG_DATA ? a.Kb[slot] : k_end;
  f32x4 acc[4];
  gd_gemm_tile<MODE == HG_WGRAD ? GD_ROW_CONTIG : GD_K_CONTIG, MODE == HG_LAYER || MODE == HG_HEADER ? GD_K_CONTIG : GD_ROW_CONTIG>(
      As, Bs, acc, a.A[slot], a.lda[slot], a.Bm[slot], a.ldb[slot], i0, I, j0, J, k_begin, k_end, kb_end, t, lane, wv);
  // the slot's arguments by value: an epilogue that captured the whole argument struct would keep a private copy of it
  float* const C = a.C[slot];
  float* const C2 = a.C2[slot];
  const float* const bias = a.bias[slot];
  const float* const bn = a.bn[slot];
  const int ldc = a.ldc[slot], bn_lstride = a.bn_lstride, z_only = a.z_only, K = a.hK[slot], kh = a.hkh[slot], hoff = a.hoff[slot], sig = a.sigmoid[slot];
  gd_acc_visit(acc, i0, I, j0, J, lane, wv, [=, &g](int m, int n, float v) {
    if (MODE == HG_LAYER) {
      const float z = v + bias[n];
      C[(int64_t)m * g.W + n] = z;
      if (!z_only) {
        const int l = hg_level(g, m);
        const GDBn q = gd_bn_load(bn + (int64_t)l * bn_lstride, g.W, n);
        const float act = gd_bn_apply(q, z);
        C2[(int64_t)m * g.W + n] = act * gd_sigmoid(act);
      }
    } else if (MODE == HG_HEADER) {
      const int l = hg_level(g, m), ss = g.s[l] * g.s[l], q = m - g.rowoff[l], b = q / ss, pix = q % ss;
      const int an = n / kh, jj = n % kh;
      const float z = v + bias[n];
      if (C) C[(int64_t)m * ldc + n] = z;
      C2[((int64_t)b * g.S * 9 + (int64_t)(g.pixoff[l] + pix) * 9 + an) * K + hoff + jj] = sig ? gd_sigmoid(z) : z;
    } else if (MODE == HG_DATA) {
      C[(int64_t)m * ldc + n] = v;
    } else {
      C[((int64_t)blockIdx.z * I + m) * J + n] = v;
    }
  });
}

// ------------------------------------------------------------------------------------------------------------------
struct HGGatherArgs {
  HGGeom g;
  const float* gout[HG_SLOTS]; const float* logits[HG_SLOTS];   // [B][N][K] cotangent of the net's output; classifier logits rows (else NULL)
  float* dz[HG_SLOTS]; float* pbias[HG_SLOTS];                   // rows [R][ld] (padding columns zero); [tile][ld]
  int C[HG_SLOTS], ld[HG_SLOTS], hK[HG_SLOTS], hkh[HG_SLOTS], hoff[HG_SLOTS];
};

// header cotangents as rows + the per-tile partial sums of the header bias gradient; thread = (tile, column), blockIdx.y = slot
__global__ __launch_bounds__(GD_THREADS) void hg_hdr_gather_kernel(HGGatherArgs a) {
  const HGGeom& g = a.g;
  const int slot = blockIdx.y, ld = a.ld[slot];
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (gid >= (int64_t)g.ntiles * ld) return;
  const int tile = (int)(gid / ld), c = (int)(gid % ld);
  int l = 0;
#pragma unroll
  for (int i = 1; i < 5; i++) l += (tile >= g.tileoff[i]);
  const int r0 = g.rowoff[l] + (tile - g.tileoff[l]) * HG_TILE_ROWS, r1 = min(g.rowoff[l + 1], r0 + HG_TILE_ROWS);
  const int ss = g.s[l] * g.s[l], K = a.hK[slot], kh = a.hkh[slot], an = c / kh, jj = c % kh;
  const bool real = c < a.C[slot];
  float sum = 0.0f;
  for (int r = r0; r < r1; r++) {
    float v = 0.0f;
    if (real) {
      const int q = r - g.rowoff[l], b = q / ss, pix = q % ss;
      v = a.gout[slot][((int64_t)b * g.S * 9 + (int64_t)(g.pixoff[l] + pix) * 9 + an) * K + a.hoff[slot] + jj];
      if (a.logits[slot]) { const float y = gd_sigmoid(a.logits[slot][(int64_t)r * ld + c]); v *= y * (1.0f - y); }
    }
    a.dz[slot][(int64_t)r * ld + c] = v;
    sum += v;
  }
  a.pbias[slot][(int64_t)tile * ld + c] = sum;
}

// ------------------------------------------------------------------------------------------------------------------
struct HGDwBwdArgs {
  HGGeom g;
  int bn_lstride;
  int nsrc[HG_NETS];
  const float* G[HG_NETS][2]; const float* w[HG_NETS][2]; float* pdw[HG_NETS][2];   // d u rows, depthwise weights, [tile][W * 9] partials
  const float* X[HG_NETS];                        // the depthwise convs' input rows
  const float* Zprev[HG_NETS]; const float* bnprev[HG_NETS];   // pre-BatchNorm rows and BatchNorm (level 0) of the layer below; NULL at layer 0
  float* out[HG_NETS];                            // d z of the layer below, or d x_0 at layer 0
  float* pgamma[HG_NETS]; float* pbeta[HG_NETS]; float* pbias[HG_NETS];   // [tile][W]
};

// One thread = (tile, channel), blockIdx.y = net; it walks the rows of its tile in order:
//   depthwise weight gradient  pdw[tap] += d u[r] * x[neighbour(r, tap)]
//   depthwise data gradient    d x[r]    = sum_tap w[8 - tap] * d u[neighbour(r, tap)]   (summed over the net's headers)
//   below                      d a = d x * swish'(a), a = bn(z);  d gamma += d a * zhat;  d beta += d a;  d z = d a * gamma * rstd;  d bias += d z
__global__ __launch_bounds__(GD_THREADS) void hg_dw_bwd_kernel(HGDwBwdArgs a) {
  const HGGeom& g = a.g;
  const int net = blockIdx.y, W = g.W;
  const int64_t gid = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x;
  if (gid >= (int64_t)g.ntiles * W) return;
  const int tile = (int)(gid / W), c = (int)(gid % W);
  int l = 0;
#pragma unroll
  for (int i = 1; i < 5; i++) l += (tile >= g.tileoff[i]);
  const int r0 = g.rowoff[l] + (tile - g.tileoff[l]) * HG_TILE_ROWS, r1 = min(g.rowoff[l + 1], r0 + HG_TILE_ROWS);
  const int s = g.s[l], ss = s * s, nsrc = a.nsrc[net];
  const float* __restrict__ X = a.X[net];
  float wt[2][9], aw[2][9];
#pragma unroll
  for (int k = 0; k < 2; k++)
#pragma unroll
    for (int tp = 0; tp < 9; tp++) { wt[k][tp] = k < nsrc ? a.w[net][k][c * 9 + tp] : 0.0f; aw[k][tp] = 0.0f; }
  const float* __restrict__ Z = a.Zprev[net];
  GDBn q{};
  if (Z) q = gd_bn_load(a.bnprev[net] + (int64_t)l * a.bn_lstride, W, c);
  float ag = 0.0f, ab = 0.0f, abias = 0.0f;
  float xw[3][3], gw[2][3][3];
  for (int r = r0; r < r1; r++) {
    const int pix = (r - g.rowoff[l]) % ss, y = pix / s, x = pix % s;
    const bool fresh = r == r0 || x == 0;
    gd_win_step<false>(xw, fresh, X, r, y, x, s, W, c);
#pragma unroll
    for (int k = 0; k < 2; k++)
      if (k < nsrc) gd_win_step<false>(gw[k], fresh, a.G[net][k], r, y, x, s, W, c);
    float dx = 0.0f;
#pragma unroll
    for (int k = 0; k < 2; k++)
      if (k < nsrc) {
        const float gk = gw[k][1][1];
#pragma unroll
        for (int tp = 0; tp < 9; tp++) {
          aw[k][tp] = fmaf(gk, xw[tp / 3][tp % 3], aw[k][tp]);
          dx = fmaf(wt[k][8 - tp], gw[k][tp / 3][tp % 3], dx);
        }
      }
    if (Z) {
      const float zh = (Z[(int64_t)r * W + c] - q.mean) * q.rstd, act = zh * q.gamma + q.beta;
      const float da = dx * gd_swish_grad(act);
      const float dz = da * q.gamma * q.rstd;
      ag = fmaf(da, zh, ag); ab += da; abias += dz;
      a.out[net][(int64_t)r * W + c] = dz;
    } else if (a.out[net]) {
      a.out[net][(int64_t)r * W + c] = dx;
    }
  }
#pragma unroll
  for (int k = 0; k < 2; k++)
    if (k < nsrc)
#pragma unroll
      for (int tp = 0; tp < 9; tp++) a.pdw[net][k][((int64_t)tile * W + c) * 9 + tp] = aw[k][tp];
  if (Z) {
    a.pgamma[net][(int64_t)tile * W + c] = ag; a.pbeta[net][(int64_t)tile * W + c] = ab; a.pbias[net][(int64_t)tile * W + c] = abias;
  }
}

// ------------------------------------------------------------------------------------------------------------------
struct HGReduceArgs {
  HGGeom g;
  int bn_lstride, kind0;                                                                  // kind0: the first kind of this launch
  const float* pw[HG_SLOTS]; float* dW[HG_SLOTS]; int Cout[HG_SLOTS], I[HG_SLOTS];        // [slab][I][W] -> [Cout][W]
  const float* pdw[HG_SLOTS]; float* ddw[HG_SLOTS];                                       // [tile][W * 9] -> [W * 9]
  const float* pbias[HG_SLOTS]; float* dbias[HG_SLOTS]; int ldb[HG_SLOTS];                // [tile][ldb] -> [Cout]
  const float* pgamma[HG_SLOTS]; const float* pbeta[HG_SLOTS]; float* dbn[HG_SLOTS];      // [tile][W] -> per level gamma, beta, 0, 0 (NULL: none)
};

// second pass (gd_reduce_core): a workgroup = 16 consecutive elements, 64-byte reads of a partial row.
// blockIdx.y = slot, kind0 + blockIdx.z = kind (0 pointwise weight, 1 depthwise weight, 2 bias - no partials: zero, the bias
// in front of a batch-statistics BatchNorm - 3 BatchNorm of the five levels)
__global__ __launch_bounds__(GD_THREADS) void hg_reduce_kernel(HGReduceArgs a) {
  const HGGeom& g = a.g;
  const int slot = blockIdx.y, kind = a.kind0 + blockIdx.z, W = g.W, el = threadIdx.x % GD_RED_E, kl = threadIdx.x / GD_RED_E;
  const int64_t e = (int64_t)blockIdx.x * GD_RED_E + el;
  const float* __restrict__ src = nullptr;      // partial k of this element: src[k * stride]
  float* dst = nullptr;
  int64_t stride = 0;
  int k0 = 0, k1 = 0;
  if (kind == 0) {
    if (a.dW[slot] && e < (int64_t)a.Cout[slot] * W) { src = a.pw[slot] + e; stride = (int64_t)a.I[slot] * W; k1 = g.nslab; dst = a.dW[slot] + e; }
  } else if (kind == 1) {
    if (a.ddw[slot] && e < (int64_t)W * 9) { src = a.pdw[slot] + e; stride = (int64_t)W * 9; k1 = g.ntiles; dst = a.ddw[slot] + e; }
  } else if (kind == 2) {
    if (a.dbias[slot] && e < a.Cout[slot]) { src = a.pbias[slot] ? a.pbias[slot] + e : nullptr; stride = a.ldb[slot]; k1 = g.ntiles; dst = a.dbias[slot] + e; }
  } else if (a.dbn[slot] && e < (int64_t)5 * 4 * W) {
    const int l = (int)(e / (4 * W)), which = (int)(e / W) % 4, c = (int)(e % W);
    dst = a.dbn[slot] + (int64_t)l * a.bn_lstride + which * W + c;
    if (which < 2) { src = (which == 0 ? a.pgamma[slot] : a.pbeta[slot]) + c; stride = W; k0 = g.tileoff[l]; k1 = g.tileoff[l + 1]; }
  }
  const float v = gd_reduce_core(src, stride, k0, k1, el, kl);
  if (kl == 0 && dst) *dst = v;                    // (running statistics: no partials, zero)
}

// ------------------------------------------------------------------------------------------------------------------
// host side
int heads_plan(int phi, int num_classes, int size, int batch, HGPlan* p, const char** why, int bn_mode, int sync) {
  if (phi < 0 || phi > 7) { *why = "heads: phi must be in 0..7 (phi 8 needs a P8 level)"; return HEP_ERR_UNSUPPORTED; }
  if (num_classes < 1 || num_classes > 63) { *why = "heads: num_classes must be in 1..63"; return HEP_ERR_UNSUPPORTED; }
  HGGeom& g = p->g;
  g.W = kFpnWidth[phi]; g.D = kHeadDepth[phi];
  p->num_classes = num_classes;
  p->bn_batch = bn_mode == HEP_BN_BATCH; p->bn_sync = p->bn_batch && sync;
  if (bn_mode != HEP_BN_RUNNING && bn_mode != HEP_BN_BATCH) { *why = "heads: the BatchNorm mode must be HEP_BN_RUNNING or HEP_BN_BATCH"; return HEP_ERR_INVALID; }
  const int W = g.W, D = g.D;
  const int vals[HG_SLOTS] = {4, num_classes, 3, 2, 1, 63};
  const int nets[HG_SLOTS] = {0, 1, 2, 3, 3, 4}, Ks[HG_SLOTS] = {4, num_classes, 3, 3, 3, 63}, offs[HG_SLOTS] = {0, 0, 0, 0, 2, 0};
  for (int h = 0; h < HG_SLOTS; h++) {
    p->C[h] = 9 * vals[h]; p->ld[h] = (p->C[h] + 3) / 4 * 4; p->net[h] = nets[h]; p->K[h] = Ks[h]; p->kh[h] = vals[h]; p->koff[h] = offs[h];
  }
  // flat parameters: the reference's state_dict order restricted to the heads (regressor, classifier, rotation_net,
  // translation_net, hand_net), num_batches_tracked left out
  int64_t o = 0;
  for (int n = 0; n < HG_NETS; n++) {
    p->p_conv[n] = o; o += (int64_t)D * (9 * W + W * W + W);
    p->p_bn[n] = o; o += (int64_t)5 * D * 4 * W;
    for (int h = 0; h < HG_SLOTS; h++)
      if (nets[h] == n) { p->p_hdr[h] = o; o += 9 * W + (int64_t)p->C[h] * W + p->C[h]; }
  }
  p->nparams = o;
  if (size == 0 && batch == 0) return 0;                   // layout only
  if (size < 128 || size > 2048 || size % 128 != 0) { *why = "heads: size must be a multiple of 128 in [128, 2048]"; return HEP_ERR_UNSUPPORTED; }
  if (batch < 1) { *why = "heads: batch must be at least 1"; return HEP_ERR_UNSUPPORTED; }
  g.B = batch;
  int S = 0, tiles = 0;
  for (int l = 0; l < 5; l++) {
    g.s[l] = (size + (8 << l) - 1) / (8 << l);
    g.pixoff[l] = S; S += g.s[l] * g.s[l];
  }
  g.pixoff[5] = S; g.S = S;
  if ((int64_t)batch * S > (1 << 22)) { *why = "heads: batch * pixels exceeds 4 Mi rows"; return HEP_ERR_UNSUPPORTED; }
  g.R = batch * S;
  if (p->bn_batch && !p->bn_sync && batch * g.s[4] * g.s[4] < 2) { *why = "heads: batch statistics need at least 2 rows per BatchNorm (batch * top-level pixels)"; return HEP_ERR_UNSUPPORTED; }
  for (int l = 0; l < 6; l++) g.rowoff[l] = batch * g.pixoff[l];
  for (int l = 0; l < 5; l++) { g.tileoff[l] = tiles; tiles += (batch * g.s[l] * g.s[l] + HG_TILE_ROWS - 1) / HG_TILE_ROWS; }
  g.tileoff[5] = tiles; g.ntiles = tiles;
  gd_slabs(g.R, HG_MAX_SLABS, &g.slab_rows, &g.nslab);
  const int64_t RW = (int64_t)g.R * W;
  int64_t w = 0;
  auto take = [&](int64_t n) { const int64_t at = w; w += (n + 3) / 4 * 4; return at; };
  p->o_x0 = take(RW); p->o_x = take(D * HG_NETS * RW); p->o_u = take(D * HG_NETS * RW); p->o_z = take(D * HG_NETS * RW);
  p->o_uh = take(HG_SLOTS * RW); p->o_cl = take((int64_t)g.R * p->ld[1]);
  for (int h = 0; h < HG_SLOTS; h++) p->o_do[h] = take((int64_t)g.R * p->ld[h]);
  p->o_g1 = take(HG_SLOTS * RW); p->o_g2 = take(HG_NETS * RW);
  for (int h = 0; h < HG_SLOTS; h++) p->o_pw[h] = take((int64_t)g.nslab * (p->ld[h] > W ? p->ld[h] : W) * W);
  for (int h = 0; h < HG_SLOTS; h++) p->o_pdw[h] = take((int64_t)tiles * W * 9);
  for (int h = 0; h < HG_SLOTS; h++) p->o_pbh[h] = take((int64_t)tiles * p->ld[h]);
  for (int k = 0; k < 2; k++) { p->o_pg[k] = take((int64_t)HG_NETS * tiles * W); p->o_pb[k] = take((int64_t)HG_NETS * tiles * W); p->o_pbi[k] = take((int64_t)HG_NETS * tiles * W); }
  p->o_bne = p->o_bnp = 0;
  if (p->bn_batch) {                                       // the effective tables in the layout of p_bn; [net][tile][W][2] doubles
    p->o_bne = take((int64_t)HG_NETS * 5 * D * 4 * W);
    p->o_bnp = take((int64_t)HG_NETS * tiles * W * 4);
  }
  p->o_xch = p->bn_sync ? take(2 * gd_sync_doubles(HG_NETS * 5, W)) : 0;
  p->ws_floats = w;
  return 0;
}

static inline int64_t hg_conv_stride(const HGGeom& g) { return (int64_t)9 * g.W + (int64_t)g.W * g.W + g.W; }

// the tensors of the flat buffer in state_dict order: per net depth x (depthwise, pointwise, bias), 5 levels x depth BatchNorms of 4 vectors, a header's three
int heads_tensor_count(const HGPlan& p) { return HG_NETS * (3 * p.g.D + 5 * p.g.D * 4) + HG_SLOTS * 3; }
void heads_tensor_offsets(const HGPlan& p, int64_t* out) {
  const int W = p.g.W, D = p.g.D;
  int k = 0;
  for (int n = 0; n < HG_NETS; n++) {
    for (int i = 0; i < D; i++) {
      const int64_t c = p.p_conv[n] + i * hg_conv_stride(p.g);
      out[k++] = c; out[k++] = c + 9 * W; out[k++] = c + 9 * W + (int64_t)W * W;
    }
    for (int j = 0; j < 5 * D * 4; j++) out[k++] = p.p_bn[n] + (int64_t)j * W;
    for (int h = 0; h < HG_SLOTS; h++)
      if (p.net[h] == n) { out[k++] = p.p_hdr[h]; out[k++] = p.p_hdr[h] + 9 * W; out[k++] = p.p_hdr[h] + 9 * W + (int64_t)p.C[h] * W; }
  }
}

// the effective table of (net, layer) at level 0 (batch statistics), laid out as the parameters' bn_list of the net
static inline float* hg_bn_eff(const HGPlan& p, float* ws, int n, int i) { return ws + p.o_bne + ((int64_t)n * 5 * p.g.D + i) * 4 * p.g.W; }
// the 25 BatchNorms (net, level) of layer i as jobs of grad_dev.h's batch-statistics kernels; a job's rows are one level's
static inline GDSync hg_sync(const HGPlan& p, float* ws, const hep_sync* sync) { return GDSync{sync->sum, sync->ctx, reinterpret_cast<double*>(ws + p.o_xch)}; }
static void hg_bn_jobs(const HGPlan& p, const float* params, float* ws, int i, GDBnArgs<HG_NETS * 5>* a) {
  const HGGeom& g = p.g;
  const int W = g.W, bn_lstride = g.D * 4 * W;
  const int64_t RW = (int64_t)g.R * W;
  a->tile_rows = HG_TILE_ROWS;
  for (int n = 0; n < HG_NETS; n++)
    for (int l = 0; l < 5; l++) {
      GDBnJob& j = a->j[n * 5 + l];
      j.z = ws + p.o_z + ((int64_t)i * HG_NETS + n) * RW + (int64_t)g.rowoff[l] * W;
      j.bn = params + p.p_bn[n] + (int64_t)l * bn_lstride + (int64_t)i * 4 * W;
      j.eff = hg_bn_eff(p, ws, n, i) + (int64_t)l * bn_lstride;
      j.part = reinterpret_cast<double*>(ws + p.o_bnp) + ((int64_t)n * g.ntiles + g.tileoff[l]) * W * 2;
      j.R = g.rowoff[l + 1] - g.rowoff[l]; j.C = W;
    }
}

void launch_heads_forward(const HGPlan& p, const float* params, const float* const feats[5], float* const outs[5], float* ws, hipStream_t st,
                          float momentum, float* stats_out, const hep_sync* sync) {
  const HGGeom& g = p.g;
  const int W = g.W, D = g.D;
  GDSync sy{};
  if (p.bn_sync) sy = hg_sync(p, ws, sync);
  const int64_t RW = (int64_t)g.R * W;
  HGPtr5 f{};
  for (int l = 0; l < 5; l++) f.in[l] = feats[l];
  hipLaunchKernelGGL(hg_rows_from_nchw_kernel, dim3(gd_blocks(RW)), dim3(GD_THREADS), 0, st, g, f, ws + p.o_x0);
  const int mt = (g.R + GD_BM - 1) / GD_BM;
  const int64_t dw_threads = (int64_t)((g.R + GD_DW_ROWS - 1) / GD_DW_ROWS) * W;
  for (int i = 0; i < D; i++) {
    HGDwArgs d{}; d.g = g;
    HGGemmArgs m{}; m.g = g; m.ntmax = (W + GD_BN - 1) / GD_BN; m.bn_lstride = D * 4 * W; m.z_only = p.bn_batch;
    for (int n = 0; n < HG_NETS; n++) {
      const float* conv = params + p.p_conv[n] + i * hg_conv_stride(g);
      d.src[n] = i == 0 ? ws + p.o_x0 : ws + p.o_x + ((int64_t)(i - 1) * HG_NETS + n) * RW;
      d.w[n] = conv;
      d.dst[n] = ws + p.o_u + ((int64_t)i * HG_NETS + n) * RW;
      m.A[n] = d.dst[n]; m.Bm[n] = conv + 9 * W; m.bias[n] = conv + 9 * W + (int64_t)W * W;
      m.bn[n] = params + p.p_bn[n] + (int64_t)i * 4 * W;
      m.C[n] = ws + p.o_z + ((int64_t)i * HG_NETS + n) * RW;
      m.C2[n] = ws + p.o_x + ((int64_t)i * HG_NETS + n) * RW;
      m.I[n] = g.R; m.J[n] = W; m.K[n] = W; m.lda[n] = W; m.ldb[n] = W; m.ldc[n] = W;
    }
    hipLaunchKernelGGL(hg_dw_fwd_kernel, dim3(gd_blocks(dw_threads), HG_NETS), dim3(GD_THREADS), 0, st, d);
    hipLaunchKernelGGL(hg_gemm_kernel<HG_LAYER>, dim3(mt * m.ntmax, HG_NETS), dim3(GD_THREADS), 0, st, m);
    if (p.bn_batch) {                                      // z -> batch statistics -> x' = swish(bn(z)), per (net, level)
      GDBnArgs<HG_NETS * 5> bj{};
      hg_bn_jobs(p, params, ws, i, &bj);
      bj.momentum = momentum;
      for (int n = 0; n < HG_NETS; n++)
        for (int l = 0; l < 5; l++) {
          GDBnJob& j = bj.j[n * 5 + l];
          j.io = ws + p.o_x + ((int64_t)i * HG_NETS + n) * RW + (int64_t)g.rowoff[l] * W;
          j.stats = stats_out ? stats_out + (j.bn - params) : nullptr;
        }
      gd_bn_forward(bj, g.rowoff[1], W, GD_BN_SWISH, st, p.bn_sync ? &sy : nullptr);
    }
  }
  HGDwArgs d{}; d.g = g;
  HGGemmArgs m{}; m.g = g; m.ntmax = 1;
  for (int h = 0; h < HG_SLOTS; h++) {
    const float* hdr = params + p.p_hdr[h];
    d.src[h] = ws + p.o_x + ((int64_t)(D - 1) * HG_NETS + p.net[h]) * RW;
    d.w[h] = hdr;
    d.dst[h] = ws + p.o_uh + (int64_t)h * RW;
    m.A[h] = d.dst[h]; m.Bm[h] = hdr + 9 * W; m.bias[h] = hdr + 9 * W + (int64_t)p.C[h] * W;
    m.C[h] = h == 1 ? ws + p.o_cl : nullptr; m.C2[h] = outs[p.net[h]];
    m.I[h] = g.R; m.J[h] = p.C[h]; m.K[h] = W; m.lda[h] = W; m.ldb[h] = W; m.ldc[h] = p.ld[h];
    m.hK[h] = p.K[h]; m.hkh[h] = p.kh[h]; m.hoff[h] = p.koff[h]; m.sigmoid[h] = h == 1;
    const int nt = (p.C[h] + GD_BN - 1) / GD_BN;
    if (nt > m.ntmax) m.ntmax = nt;
  }
  hipLaunchKernelGGL(hg_dw_fwd_kernel, dim3(gd_blocks(dw_threads), HG_SLOTS), dim3(GD_THREADS), 0, st, d);
  hipLaunchKernelGGL(hg_gemm_kernel<HG_HEADER>, dim3(mt * m.ntmax, HG_SLOTS), dim3(GD_THREADS), 0, st, m);
}

void launch_heads_backward(const HGPlan& p, const float* params, const float* const grad_outs[5], float* grad_params, float* const grad_feats[5],
                           float* ws, hipStream_t st, const hep_sync* sync) {
  const HGGeom& g = p.g;
  const int W = g.W, D = g.D, T = g.ntiles;
  GDSync sy{};
  if (p.bn_sync) sy = hg_sync(p, ws, sync);
  const int64_t RW = (int64_t)g.R * W, TW = (int64_t)T * W;
  const int mt = (g.R + GD_BM - 1) / GD_BM, bn_lstride = D * 4 * W;
  const unsigned col_blocks = gd_blocks(TW);
  // batch statistics: the BatchNorm tables are the forward's effective ones, and a layer's d z is complete only after its
  // gamma / beta reduce: reduce them right behind the dw_bwd that made their partials, correct d z in place, then the products
  auto bn_table = [&](int n, int i) { return p.bn_batch ? (const float*)hg_bn_eff(p, ws, n, i) : params + p.p_bn[n] + (int64_t)i * 4 * W; };
  auto bn_below = [&](int i) {
    HGReduceArgs rb{}; rb.g = g; rb.bn_lstride = bn_lstride; rb.kind0 = 3;
    GDBnArgs<HG_NETS * 5> bj{};
    hg_bn_jobs(p, params, ws, i, &bj);
    for (int n = 0; n < HG_NETS; n++) {
      rb.pgamma[n] = ws + p.o_pg[i & 1] + n * TW; rb.pbeta[n] = ws + p.o_pb[i & 1] + n * TW;
      rb.dbn[n] = grad_params + p.p_bn[n] + (int64_t)i * 4 * W;
      for (int l = 0; l < 5; l++) {
        GDBnJob& j = bj.j[n * 5 + l];
        j.io = ws + p.o_g2 + (int64_t)n * RW + (int64_t)g.rowoff[l] * W;
        j.dbn = rb.dbn[n] + (int64_t)l * bn_lstride;
        j.pg = rb.pgamma[n] + (int64_t)g.tileoff[l] * W; j.pb = rb.pbeta[n] + (int64_t)g.tileoff[l] * W;
        j.pn = g.tileoff[l + 1] - g.tileoff[l]; j.pstride = W;
      }
    }
    hipLaunchKernelGGL(hg_reduce_kernel, dim3((unsigned)(((int64_t)5 * 4 * W + GD_RED_E - 1) / GD_RED_E), HG_NETS, 1), dim3(GD_THREADS), 0, st, rb);
    gd_bn_dz(bj, g.rowoff[1], W, st, p.bn_sync ? &sy : nullptr);
  };
  // ---- header stage ----
  {
    HGGatherArgs ga{}; ga.g = g;
    HGGemmArgs md{}; md.g = g; md.ntmax = (W + GD_BN - 1) / GD_BN;
    HGGemmArgs mw{}; mw.g = g; mw.ntmax = md.ntmax;
    HGDwBwdArgs db{}; db.g = g; db.bn_lstride = bn_lstride;
    HGReduceArgs rd{}; rd.g = g; rd.bn_lstride = bn_lstride;
    int ldmax = 0, itmax = 1;
    int64_t emax = (int64_t)W * 9;
    for (int h = 0; h < HG_SLOTS; h++) {
      const float* hdr = params + p.p_hdr[h];
      float* ghdr = grad_params + p.p_hdr[h];
      const int n = p.net[h];
      ga.gout[h] = grad_outs[n]; ga.logits[h] = h == 1 ? ws + p.o_cl : nullptr;
      ga.dz[h] = ws + p.o_do[h]; ga.pbias[h] = ws + p.o_pbh[h];
      ga.C[h] = p.C[h]; ga.ld[h] = p.ld[h]; ga.hK[h] = p.K[h]; ga.hkh[h] = p.kh[h]; ga.hoff[h] = p.koff[h];
      if (p.ld[h] > ldmax) ldmax = p.ld[h];
      md.A[h] = ga.dz[h]; md.Bm[h] = hdr + 9 * W; md.C[h] = ws + p.o_g1 + (int64_t)h * RW;
      md.I[h] = g.R; md.J[h] = W; md.K[h] = p.ld[h]; md.Kb[h] = p.C[h]; md.lda[h] = p.ld[h]; md.ldb[h] = W; md.ldc[h] = W;
      mw.A[h] = ga.dz[h]; mw.Bm[h] = ws + p.o_uh + (int64_t)h * RW; mw.C[h] = ws + p.o_pw[h];
      mw.I[h] = p.ld[h]; mw.J[h] = W; mw.lda[h] = p.ld[h]; mw.ldb[h] = W;
      const int it = (p.ld[h] + GD_BM - 1) / GD_BM;
      if (it > itmax) itmax = it;
      const int k = db.nsrc[n]++;
      db.G[n][k] = md.C[h]; db.w[n][k] = hdr; db.pdw[n][k] = ws + p.o_pdw[h];
      rd.pw[h] = mw.C[h]; rd.dW[h] = ghdr + 9 * W; rd.Cout[h] = p.C[h]; rd.I[h] = p.ld[h];
      rd.pdw[h] = ws + p.o_pdw[h]; rd.ddw[h] = ghdr;
      rd.pbias[h] = ga.pbias[h]; rd.dbias[h] = ghdr + 9 * W + (int64_t)p.C[h] * W; rd.ldb[h] = p.ld[h];
      if ((int64_t)p.C[h] * W > emax) emax = (int64_t)p.C[h] * W;
    }
    for (int n = 0; n < HG_NETS; n++) {
      db.X[n] = ws + p.o_x + ((int64_t)(D - 1) * HG_NETS + n) * RW;
      db.Zprev[n] = ws + p.o_z + ((int64_t)(D - 1) * HG_NETS + n) * RW;
      db.bnprev[n] = bn_table(n, D - 1);
      db.out[n] = ws + p.o_g2 + (int64_t)n * RW;
      const int par = (D - 1) & 1;
      db.pgamma[n] = ws + p.o_pg[par] + n * TW; db.pbeta[n] = ws + p.o_pb[par] + n * TW; db.pbias[n] = ws + p.o_pbi[par] + n * TW;
    }
    hipLaunchKernelGGL(hg_hdr_gather_kernel, dim3(gd_blocks((int64_t)T * ldmax), HG_SLOTS), dim3(GD_THREADS), 0, st, ga);
    hipLaunchKernelGGL(hg_gemm_kernel<HG_DATA>, dim3(mt * md.ntmax, HG_SLOTS), dim3(GD_THREADS), 0, st, md);
    hipLaunchKernelGGL(hg_gemm_kernel<HG_WGRAD>, dim3(itmax * mw.ntmax, HG_SLOTS, g.nslab), dim3(GD_THREADS), 0, st, mw);
    hipLaunchKernelGGL(hg_dw_bwd_kernel, dim3(col_blocks, HG_NETS), dim3(GD_THREADS), 0, st, db);
    hipLaunchKernelGGL(hg_reduce_kernel, dim3((unsigned)((emax + GD_RED_E - 1) / GD_RED_E), HG_SLOTS, 3), dim3(GD_THREADS), 0, st, rd);
    if (p.bn_batch) bn_below(D - 1);
  }
  // ---- the layers, top down ----
  for (int i = D - 1; i >= 0; i--) {
    HGGemmArgs md{}; md.g = g; md.ntmax = (W + GD_BN - 1) / GD_BN;
    HGGemmArgs mw{}; mw.g = g; mw.ntmax = md.ntmax;
    HGDwBwdArgs db{}; db.g = g; db.bn_lstride = bn_lstride;
    HGReduceArgs rd{}; rd.g = g; rd.bn_lstride = bn_lstride;
    for (int n = 0; n < HG_NETS; n++) {
      const float* conv = params + p.p_conv[n] + i * hg_conv_stride(g);
      float* gconv = grad_params + p.p_conv[n] + i * hg_conv_stride(g);
      const float* dz = ws + p.o_g2 + (int64_t)n * RW;
      md.A[n] = dz; md.Bm[n] = conv + 9 * W; md.C[n] = ws + p.o_g1 + (int64_t)n * RW;
      md.I[n] = g.R; md.J[n] = W; md.K[n] = W; md.Kb[n] = W; md.lda[n] = W; md.ldb[n] = W; md.ldc[n] = W;
      mw.A[n] = dz; mw.Bm[n] = ws + p.o_u + ((int64_t)i * HG_NETS + n) * RW; mw.C[n] = ws + p.o_pw[n];
      mw.I[n] = W; mw.J[n] = W; mw.lda[n] = W; mw.ldb[n] = W;
      db.nsrc[n] = 1; db.G[n][0] = md.C[n]; db.w[n][0] = conv; db.pdw[n][0] = ws + p.o_pdw[n];
      db.X[n] = i == 0 ? ws + p.o_x0 : ws + p.o_x + ((int64_t)(i - 1) * HG_NETS + n) * RW;
      const int par = i & 1, below = (i - 1) & 1;
      if (i > 0) {
        db.Zprev[n] = ws + p.o_z + ((int64_t)(i - 1) * HG_NETS + n) * RW;
        db.bnprev[n] = bn_table(n, i - 1);
        db.out[n] = ws + p.o_g2 + (int64_t)n * RW;
        db.pgamma[n] = ws + p.o_pg[below] + n * TW; db.pbeta[n] = ws + p.o_pb[below] + n * TW; db.pbias[n] = ws + p.o_pbi[below] + n * TW;
      } else {
        db.out[n] = grad_feats ? ws + p.o_g2 + (int64_t)n * RW : nullptr;
      }
      rd.pw[n] = mw.C[n]; rd.dW[n] = gconv + 9 * W; rd.Cout[n] = W; rd.I[n] = W;
      rd.pdw[n] = ws + p.o_pdw[n]; rd.ddw[n] = gconv;
      rd.pbias[n] = p.bn_batch ? nullptr : ws + p.o_pbi[par] + n * TW; rd.dbias[n] = gconv + 9 * W + (int64_t)W * W; rd.ldb[n] = W;
      rd.pgamma[n] = ws + p.o_pg[par] + n * TW; rd.pbeta[n] = ws + p.o_pb[par] + n * TW;
      rd.dbn[n] = grad_params + p.p_bn[n] + (int64_t)i * 4 * W;
    }
    hipLaunchKernelGGL(hg_gemm_kernel<HG_DATA>, dim3(mt * md.ntmax, HG_NETS), dim3(GD_THREADS), 0, st, md);
    hipLaunchKernelGGL(hg_gemm_kernel<HG_WGRAD>, dim3(md.ntmax * mw.ntmax, HG_NETS, g.nslab), dim3(GD_THREADS), 0, st, mw);
    hipLaunchKernelGGL(hg_dw_bwd_kernel, dim3(col_blocks, HG_NETS), dim3(GD_THREADS), 0, st, db);
    hipLaunchKernelGGL(hg_reduce_kernel, dim3((unsigned)(((int64_t)W * W + GD_RED_E - 1) / GD_RED_E), HG_NETS, p.bn_batch ? 3 : 4), dim3(GD_THREADS), 0, st, rd);
    if (p.bn_batch && i > 0) bn_below(i - 1);
  }
  if (grad_feats) {
    HGPtr5 f{};
    for (int l = 0; l < 5; l++) f.out[l] = grad_feats[l];
    hipLaunchKernelGGL(hg_feats_grad_kernel, dim3(gd_blocks(RW)), dim3(GD_THREADS), 0, st, g, f, ws + p.o_g2);
  }
}
