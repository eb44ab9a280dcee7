// k_sbf.hip - the first two convolutions of the EfficientNet backbone as ONE gfx950 kernel:
//
//   _conv_stem,_bn0,_swish                     3x3 stride 2, 3 -> C, TF-SAME (reference efficientdet/model.py:437-439)
//   block 0: _depthwise_conv,_bn1,_swish       3x3 stride 1 on the stem's output (block 0 has no expand conv:
//   adaptive_avg_pool2d (spatial half)         efficientnet/model.py:76-89 with expand_ratio 1)
//
// As two launches the stem wrote its output (16.8 MB at phi 0, b16, bf16) and the depthwise kernel read it back; each ran
// at ~2 TB/s on a chain of strided global loads.  Here a workgroup owns a 14x14 tile of the depthwise output: the fp32
// input pixels it needs (33x33x3, read through the caller's strides: the NHWC-memory view of eval/common.py:397 needs no
// copy) go to LDS once, every lane computes ONE of the 16x16 stem pixels of the tile + halo for all channels (27 inputs in
// registers, 8 output channels at a time, weights as scalar operands - the arithmetic of stem_kernel), the activated stem
// tile stays in LDS (zero outside the image: it is the depthwise conv's padding) and the depthwise taps read it from there.
// HBM sees the input once and the depthwise output once; the stem's output is stored only for the stage tests.
#include <algorithm>

#include "hep_dev.h"
#include "hep_internal.h"

#ifdef HEP_XBF_TRACE
__device__ unsigned long long* g_sbf_trace = nullptr;
#define SSTAMP(i) do { stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define SSTAMP(i)
#endif

namespace {
constexpr int ST = 256, SWV = ST / 64;          // threads, waves
constexpr int TO = 14;                            // depthwise output tile side
constexpr int TS_ = TO + 2;                       // stem tile side (16): 256 stem pixels = one per lane
constexpr int TI = 2 * TS_ + 1;                   // input tile side (33)
}

template <bool BF16>
__global__ __launch_bounds__(ST, 4) void sbf_kernel(SbfArgs a) {   // (four workgroups per CU)
  typedef Vec8<BF16> V;
  typedef typename V::elem T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#ifdef HEP_XBF_TRACE
  unsigned long long stamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  SSTAMP(0);
  float* in_s = reinterpret_cast<float*>(smem);                         // [TI][TI][3] input tile, channels interleaved (zero outside the image)
  T* s_s = reinterpret_cast<T*>(smem + a.off_s);                        // [TS_*TS_][C + PAD] activated stem tile (zero outside the map)
  float* wdw_s = reinterpret_cast<float*>(smem + a.off_w);              // [9][C] depthwise weights, then [C] bias
  float* ws_s = wdw_s + 10 * a.C;                                       // [27][C] stem weights, then [C] bias
  float (*red9)[9] = reinterpret_cast<float (*)[9]>(smem);               // [ST][9] channel-sum staging (the input tile is dead by then)
  float* csum_s = reinterpret_cast<float*>(smem) + ST * 9;              // [C]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, CP = C + (BF16 ? 8 : 4), cgs = C >> 3;
  const int logical = xcd_remap(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
  const int b = udiv_rcp(logical, a.tiles_rcp), tile = logical - b * a.tiles;
  const int tyi = udiv_rcp(tile, a.tiles_x_rcp), txi = tile - tyi * a.tiles_x;
  const int oy0 = tyi * TO, ox0 = txi * TO;                             // depthwise output (= stem map) coordinates of the tile
  const int sy0 = oy0 - 1, sx0 = ox0 - 1;                               // stem pixel of tile position (0, 0)
  const int iy0 = sy0 * 2 - a.pad_t, ix0 = sx0 * 2 - a.pad_l;           // input pixel of input-tile position (0, 0)

  // ---- P0: input tile + depthwise weights -> LDS (loads first, stores behind them); the stem's MFMA weight fragments and
  //      biases are requested here as well, so that their round trip is hidden behind the input tile's ----
  const int r = lane & 15, g = lane >> 4;
  const int ntl = (C + 15) >> 4;                                       // n-tiles of 16 output channels (<= 4)
  {
    const float* img = a.in + (int64_t)b * a.sn;
    constexpr int NIN = 3 * TI * TI, NL = (NIN + ST - 1) / ST;          // 3267 floats, 13 per lane
    float v[NL]; bool ok[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) {
      const int i = min(tid + j * ST, NIN - 1);
      const int ci = i / (TI * TI), rem = i - ci * (TI * TI), ty = rem / TI, tx = rem - ty * TI;
      const int gy = iy0 + ty, gx = ix0 + tx;
      ok[j] = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      v[j] = img[(int64_t)ci * a.sc + (int64_t)min(max(gy, 0), a.H - 1) * a.sh + (int64_t)min(max(gx, 0), a.W - 1) * a.sw];
    }
    // stem weights [27][C] + bias [C] -> LDS as 16-byte vectors (the MFMA fragments are read from there: as 28 four-byte
    // global loads per lane they cost more vector-memory issue time than the whole input tile)
    const int nsv = (28 * C) >> 2;                                       // (27 C weights, then C biases)
    const int isv = min(tid, nsv - 1);
    const f32x4 sv = isv < ((27 * C) >> 2) ? reinterpret_cast<const f32x4*>(a.w_stem)[isv] : reinterpret_cast<const f32x4*>(a.b_stem)[isv - ((27 * C) >> 2)];
    const int nw = 10 * C;
    float wv[3];
#pragma unroll
    for (int j = 0; j < 3; j++) { const int i = min(tid + j * ST, nw - 1); const float* src = i < 9 * C ? a.wdw + i : a.bdw + (i - 9 * C); wv[j] = *src; }
#pragma unroll
    for (int j = 0; j < NL; j++) {
      const int i = tid + j * ST;
      if (i < NIN) { const int ci = i / (TI * TI), rem = i - ci * (TI * TI); in_s[rem * 3 + ci] = ok[j] ? v[j] : 0.f; }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) if (tid + j * ST < nw) wdw_s[tid + j * ST] = wv[j];
    if (tid < nsv) reinterpret_cast<f32x4*>(ws_s)[tid] = sv;
    for (int i = tid + ST; i < nsv; i += ST)                             // (C > 36)
      reinterpret_cast<f32x4*>(ws_s)[i] = i < ((27 * C) >> 2) ? reinterpret_cast<const f32x4*>(a.w_stem)[i] : reinterpret_cast<const f32x4*>(a.b_stem)[i - ((27 * C) >> 2)];
  }
  SSTAMP(1);
  __syncthreads();
  SSTAMP(2);

  // ---- P1: stem conv on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32: an fp32 fma chain in k order, the arithmetic of the
  //      VALU stem kernel).  As VALU code with scalar weight operands the phase ran at 30 % of the fp32 rate: every 8 FMAs
  //      waited for their s_load.  Here an m-tile is one row of the 16x16 stem tile (16 pixels), k = (ky, kx, ci) padded
  //      27 -> 28, the B operand is the im2col gather from the input tile in LDS (one ds_read_b32 per k-step and lane), the
  //      A operand the weights (loaded once per wave), and a lane ends with 4 consecutive channels of one pixel. ----
  // k = (ky, kx, ci) = 9 ky + (3 kx + ci): with the channels interleaved the 9 taps of one ky are 9 consecutive floats
  auto tap_off = [](int k) { const int ky = k / 9; return ky * TI * 3 + (k - ky * 9); };
  if constexpr (BF16) {
    // bf16 sessions: split-bf16 operands (x = xh + xl, w = wh + wl; wh xh + wh xl + wl xh: 2^-16 relative, far below the bf16
    // rounding of the result) on v_mfma_f32_16x16x32_bf16: ONE k-step holds all 27 taps and three MFMAs per n-tile replace
    // seven exact-fp32 ones at 1/16 of the matrix-pipe time (the fp32 form made the phase MFMA-bound: 4.7 us chip-wide)
    int koff[8];
#pragma unroll
    for (int j = 0; j < 8; j++) koff[j] = tap_off(min(8 * g + j, 26));
    bf16x8 wh[4], wl[4];
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
      u32x4 h, l;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        float w2[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int k = 8 * g + 2 * q + e, n = nt * 16 + r;
          const float wv_ = ws_s[min(k, 26) * C + min(n, C - 1)];
          w2[e] = (nt < ntl && k < 27 && n < C) ? wv_ : 0.f;
        }
        h[q] = pack_bf16x2(w2[0], w2[1]);
        l[q] = pack_bf16x2(w2[0] - __uint_as_float(h[q] << 16), w2[1] - __uint_as_float(h[q] & 0xffff0000u));
      }
      wh[nt] = __builtin_bit_cast(bf16x8, h); wl[nt] = __builtin_bit_cast(bf16x8, l);
    }
    f32x4 bias[4];
#pragma unroll
    for (int nt = 0; nt < 4; nt++) bias[nt] = *reinterpret_cast<const f32x4*>(ws_s + 27 * C + min(nt * 16 + 4 * g, C - 4));
#pragma unroll 1
    for (int mt = wave; mt < TS_; mt += SWV) {                           // stem tile row mt, pixel (mt, r)
      const int sy = sy0 + mt, sx = sx0 + r;
      const bool live = sy >= 0 && sy < a.Hs;                            // (uniform) rows outside the map are the depthwise zero padding
      const bool inside = live && sx >= 0 && sx < a.Ws;
      f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; nt++) acc[nt] = bias[nt];
      if (live) {
        const float* xrow = in_s + ((2 * mt) * TI + 2 * r) * 3;
        u32x4 xh_, xl_;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          float x0_ = xrow[koff[2 * q]], x1_ = xrow[koff[2 * q + 1]];
          if (8 * g + 2 * q >= 27) x0_ = 0.f;
          if (8 * g + 2 * q + 1 >= 27) x1_ = 0.f;
          xh_[q] = pack_bf16x2(x0_, x1_);
          xl_[q] = pack_bf16x2(x0_ - __uint_as_float(xh_[q] << 16), x1_ - __uint_as_float(xh_[q] & 0xffff0000u));
        }
        const bf16x8 xh = __builtin_bit_cast(bf16x8, xh_), xl = __builtin_bit_cast(bf16x8, xl_);
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {
          if (nt < ntl) {
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[nt], xh, acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[nt], xl, acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[nt], xh, acc[nt], 0, 0, 0);
          }
        }
      }
      const bool owned = inside && mt >= 1 && mt <= TO && r >= 1 && r <= TO;
      const int64_t spix = ((int64_t)b * a.Hs + min(max(sy, 0), a.Hs - 1)) * a.Ws + min(max(sx, 0), a.Ws - 1);
#pragma unroll
      for (int nt = 0; nt < 4; nt++) {
        const int n = nt * 16 + 4 * g;
        if (nt < ntl && n < C) {
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; q++) v[q] = inside ? swish_t<BF16>(acc[nt][q]) : 0.f;
          V::store4(s_s, (mt * TS_ + r) * CP + n, v);
          if (a.stem_out && owned) V::store4(a.stem_out, spix * C + n, v);
        }
      }
    }
  } else {
    // fp32 sessions: exact-fp32 MFMA (v_mfma_f32_16x16x4_f32: an fp32 fma chain in k order, the arithmetic of stem_kernel)
    int koff[7];
#pragma unroll
    for (int s_ = 0; s_ < 7; s_++) koff[s_] = tap_off(min(4 * s_ + g, 26));
    float wf[4][7];                                                      // A operand: W[n = 16 nt + r][k = 4 s + g]
#pragma unroll
    for (int nt = 0; nt < 4; nt++)
#pragma unroll
      for (int s_ = 0; s_ < 7; s_++) {
        const int k = 4 * s_ + g, n = nt * 16 + r;
        const float wv_ = ws_s[min(k, 26) * C + min(n, C - 1)];
        wf[nt][s_] = (nt < ntl && k < 27 && n < C) ? wv_ : 0.f;
      }
    f32x4 bias[4];
#pragma unroll
    for (int nt = 0; nt < 4; nt++) bias[nt] = *reinterpret_cast<const f32x4*>(ws_s + 27 * C + min(nt * 16 + 4 * g, C - 4));
#pragma unroll 1
    for (int mt = wave; mt < TS_; mt += SWV) {
      const int sy = sy0 + mt, sx = sx0 + r;
      const bool live = sy >= 0 && sy < a.Hs;
      const bool inside = live && sx >= 0 && sx < a.Ws;
      f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; nt++) acc[nt] = bias[nt];
      if (live) {
        const float* xrow = in_s + ((2 * mt) * TI + 2 * r) * 3;
        float xb[7];
#pragma unroll
        for (int s_ = 0; s_ < 7; s_++) { xb[s_] = xrow[koff[s_]]; if (4 * s_ + g >= 27) xb[s_] = 0.f; }
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {
          if (nt < ntl) {
#pragma unroll
            for (int s_ = 0; s_ < 7; s_++) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[nt][s_], xb[s_], acc[nt], 0, 0, 0);
          }
        }
      }
      const bool owned = inside && mt >= 1 && mt <= TO && r >= 1 && r <= TO;
      const int64_t spix = ((int64_t)b * a.Hs + min(max(sy, 0), a.Hs - 1)) * a.Ws + min(max(sx, 0), a.Ws - 1);
#pragma unroll
      for (int nt = 0; nt < 4; nt++) {
        const int n = nt * 16 + 4 * g;
        if (nt < ntl && n < C) {
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; q++) v[q] = inside ? swish_t<BF16>(acc[nt][q]) : 0.f;
          V::store4(s_s, (mt * TS_ + r) * CP + n, v);
          if (a.stem_out && owned) V::store4(a.stem_out, spix * C + n, v);
        }
      }
    }
  }
  SSTAMP(3);
  __syncthreads();
  SSTAMP(4);

  // ---- P2: depthwise 3x3 from LDS; thread -> (pixel-pair group, 8-channel group), channel group fixed per thread ----
  float sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const float cgs_inv = __builtin_amdgcn_rcpf((float)cgs);
  const int npg = udiv_f(ST, cgs, cgs_inv);
  const int pg = udiv_f(tid, cgs, cgs_inv), cg = tid - pg * cgs;
  constexpr int NPP = TO * TO / 2;
  if (pg < npg) {
    float bias[8];
    {
      const f32x4* bp = reinterpret_cast<const f32x4*>(wdw_s + 9 * C + cg * 8);
      const f32x4 q0 = bp[0], q1 = bp[1];
#pragma unroll
      for (int c = 0; c < 4; c++) { bias[c] = q0[c]; bias[4 + c] = q1[c]; }
    }
    T* out_b = reinterpret_cast<T*>(a.out) + (int64_t)b * a.Hs * a.Ws * C + cg * 8;
    for (int pp = pg; pp < NPP; pp += npg) {
      const int py = pp / (TO / 2), px = (pp - py * (TO / 2)) * 2;
      float acc0[8], acc1[8];
#pragma unroll
      for (int c = 0; c < 8; c++) { acc0[c] = bias[c]; acc1[c] = bias[c]; }
#pragma unroll 1
      for (int ky = 0; ky < 3; ky++) {
        float ev[4][8];
#pragma unroll
        for (int j = 0; j < 4; j++) V::load(s_s, ((py + ky) * TS_ + px + j) * CP + cg * 8, ev[j]);
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
          const f32x4* wp = reinterpret_cast<const f32x4*>(wdw_s + (ky * 3 + kx) * C + cg * 8);
          const f32x4 w0 = wp[0], w1 = wp[1];
#pragma unroll
          for (int c = 0; c < 4; c++) {
            acc0[c] = fmaf(ev[kx][c], w0[c], acc0[c]); acc0[4 + c] = fmaf(ev[kx][4 + c], w1[c], acc0[4 + c]);
            acc1[c] = fmaf(ev[kx + 1][c], w0[c], acc1[c]); acc1[4 + c] = fmaf(ev[kx + 1][4 + c], w1[c], acc1[4 + c]);
          }
        }
      }
      const int oy = oy0 + py, ox = ox0 + px;
      if (oy < a.Hs && ox < a.Ws) {
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; c++) { v[c] = swish_t<BF16>(acc0[c]); sum[c] += v[c]; }
        V::store(out_b, (int64_t)((oy * a.Ws + ox) * C), v);
        if (ox + 1 < a.Ws) {
#pragma unroll
          for (int c = 0; c < 8; c++) { v[c] = swish_t<BF16>(acc1[c]); sum[c] += v[c]; }
          V::store(out_b, (int64_t)((oy * a.Ws + ox + 1) * C), v);
        }
      }
    }
  }
  SSTAMP(5);
  // ---- P3: channel sums in a fixed order -> partial reduce-FC products of block 0 -> hpart[b][tile][j] ----
#pragma unroll
  for (int c = 0; c < 8; c++) red9[tid][c] = sum[c];
  __syncthreads();
  for (int c = tid; c < C; c += ST) {
    const int cg_ = c >> 3, cl = c & 7;
    float s_ = 0.f;
    for (int q = 0; q < npg; q++) s_ += red9[cg_ + q * cgs][cl];
    csum_s[c] = s_;
  }
  __syncthreads();
  {
    const int lp = tid & 31;
    float* hrow = a.hpart + ((int64_t)b * a.tiles + tile) * a.sqp;
    for (int j = tid >> 5; j < ((a.sq + 7) & ~7); j += ST / 32) {
      float dot = 0.f;
      if (j < a.sq)
        for (int c = lp; c < C; c += 32) dot = fmaf(a.se_wr[(uint32_t)(j * C + c)], csum_s[c], dot);
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) dot += __shfl_xor(dot, off, 64);
      if (lp == 0 && j < a.sq) hrow[j] = dot;
    }
  }
#ifdef HEP_XBF_TRACE
  SSTAMP(6);
  if (g_sbf_trace && lane == 0) {
    unsigned long long* o = g_sbf_trace + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * SWV + wave) * 8;
    for (int i = 0; i < 7; i++) o[i] = stamps[i];
  }
#endif
}

#ifdef HEP_XBF_TRACE
extern "C" int hep_dbg_sbf_trace(unsigned long long* host, int max_waves, int enable) {
  static unsigned long long* buf = nullptr;
  const size_t cap = (size_t)1 << 20;
  if (!buf) { if (hipMalloc((void**)&buf, cap * 8) != hipSuccess) return -1; hipMemset(buf, 0, cap * 8); }
  unsigned long long* p = enable ? buf : nullptr;
  hipMemcpyToSymbol(HIP_SYMBOL(g_sbf_trace), &p, sizeof p);
  if (host) { hipDeviceSynchronize(); hipMemcpy(host, buf, (size_t)max_waves * 64, hipMemcpyDeviceToHost); }
  return 0;
}
#endif

void sbf_layout(SbfArgs* a) {
  const size_t es = a->bf16 ? 2 : 4, pad = a->bf16 ? 8 : 4;
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t in_bytes = al((size_t)3 * TI * TI * 4), s_bytes = al((size_t)TS_ * TS_ * (a->C + pad) * es), w_bytes = al((size_t)(10 + 28) * a->C * 4);
  const size_t uni = std::max(in_bytes, al(((size_t)ST * 9 + a->C) * 4));     // input tile, later the channel-sum staging
  a->off_s = (int)uni; a->off_w = a->off_s + (int)s_bytes; a->off_red = 0;
  a->lds_bytes = (size_t)a->off_w + w_bytes;
  a->tiles_x = (a->Ws + TO - 1) / TO; a->tiles = a->tiles_x * ((a->Hs + TO - 1) / TO);
}

Pick sbf_pick(const SbfArgs& a) { return a.bf16 ? HEP_PICK(ST, a.lds_bytes, 0, sbf_kernel, true) : HEP_PICK(ST, a.lds_bytes, 0, sbf_kernel, false); }

void launch_sbf(const SbfArgs& a_, hipStream_t s) {
  SbfArgs a = a_;
  a.tiles_rcp = rcp_u32((uint32_t)a.tiles); a.tiles_x_rcp = rcp_u32((uint32_t)a.tiles_x);
  dim3 grid(a.tiles, a.B);
  sbf_pick(a).launch(grid, s, a);
}
