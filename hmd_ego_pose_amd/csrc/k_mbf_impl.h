// k_mbf_impl.h - the fused-front kernel (see k_mbf.hip for what it computes) as a template, shared by the translation units that
// instantiate it: k_mbf.hip (the generic kernels, every shape) and k_mbf_s16.hip / k_mbf_s8.hip (the shape-specialised ones).
#pragma once
#include "hep_dev.h"
#include "hep_internal.h"
#include "se_finish.h"

// Layer shapes as compile-time constants ("shapes as template parameters on hot launches", as K1C / NT2C of
// xbf_kernel).  The prologue and the index arithmetic of every phase are issue-bound (below); with the layer's dimensions known every
// index split, loop bound, LDS pitch and reciprocal folds and the branches on has_expand / out_frag / se_tail disappear.  Descriptor
// D = 0 takes everything from MbfArgs - mbf_kernel, the path of every other width, map size and phi; D > 0 is row D of MBF_SHAPES and
// runs as mbf_shape_kernel<..., D>.  One row per (layer shape, tile, dtype) the benchmarked session launches (phi 0 @ 256 in bf16,
// blocks 4-15; 6|7, 9|10 and 12|13|14 share a row) - no cross product.  launch_mbf selects a row only when EVERY folded field of the
// launch equals it (mbf_shape_id), so a row that no longer matches the planner falls back to D = 0 instead of computing with stale
// constants.  Only where the numbers come from changes: no arithmetic, accumulation order, LDS layout or reduction tree does.
//        id bf16 KS S  TS MP   Cin  Cexp CC   H   W  Ho  Wo pt pl  sq sqp expand out_frag
#define MBF_SHAPES_16(X) \
  X(1, true, 5, 1, 16, 0,   40,  240, 64, 32, 32, 32, 32, 2, 2, 10, 16, 1, 0) \
  X(3, true, 3, 1, 16, 0,   80,  480, 64, 16, 16, 16, 16, 1, 1, 20, 24, 1, 1) \
  X(4, true, 5, 1, 16, 0,   80,  480, 64, 16, 16, 16, 16, 2, 2, 20, 24, 1, 1) \
  X(5, true, 5, 1, 16, 0,  112,  672, 64, 16, 16, 16, 16, 2, 2, 28, 32, 1, 1)
#define MBF_SHAPES_8(X) \
  X(2, true, 3, 2,  8, 0,   40,  240, 64, 32, 32, 16, 16, 0, 0, 10, 16, 1, 1) \
  X(6, true, 5, 2,  8, 0,  112,  672, 64, 16, 16,  8,  8, 1, 1, 28, 32, 1, 1) \
  X(7, true, 5, 1,  8, 0,  192, 1152, 64,  8,  8,  8,  8, 2, 2, 48, 48, 1, 1) \
  X(8, true, 3, 1,  8, 0,  192, 1152, 64,  8,  8,  8,  8, 1, 1, 48, 48, 1, 1)
#define MBF_SHAPES(X) MBF_SHAPES_16(X) MBF_SHAPES_8(X)

struct MbfShape { int Cin, Cexp, CC, H, W, Ho, Wo, pad_t, pad_l, sq, sqp, has_expand, out_frag; };
constexpr MbfShape mbf_shape(int d) {
  switch (d) {
#define X(id, bf, ks, s, ts, mp, cin, cexp, cc, h, w, ho, wo, pt, pl, sq, sqp, he, of) case id: return MbfShape{cin, cexp, cc, h, w, ho, wo, pt, pl, sq, sqp, he, of};
    MBF_SHAPES(X)
#undef X
    default: return MbfShape{};
  }
}

// Tile side TS: 8 (512 threads, two workgroups per CU) for the stride-2 layers and the 8x8 maps, 16 (1024
// threads) for the stride-1 layers on 16x16 / 32x32 maps: there an 8x8 tile re-expands its k x k halo (2.25x the
// pixels for k = 5) and every one of the 4x more workgroups pays the fixed staging / drain latency - the 16x16
// tile is the whole 16x16 map (no halo work at all) and a quarter of the 32x32 one.

// Optional per-wave timeline (make EXTRA=-DHEP_MBF_TRACE): s_memrealtime (100 MHz) stamps at the phase
// boundaries of the LAST mbf launch, read back with hep_dbg_mbf_trace() - profiling builds only.
#ifdef HEP_MBF_TRACE
static __device__ unsigned long long* g_mbf_trace = nullptr;      // one per translation unit: hep_dbg_mbf_trace binds them all (mbf_trace_bind*)
static inline void mbf_trace_bind_tu(unsigned long long* p) { hipMemcpyToSymbol(HIP_SYMBOL(g_mbf_trace), &p, sizeof p); }
#ifdef HEP_MBF_TRACE_A      // sub-steps of phase A instead of the phase boundaries: 1 kernargs in, 2 loads issued, 3 first data, 4 all parked, 5 barrier
#define MSTAMP(i) do { if ((i) == 0 || (i) == 6) stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define XSTAMP(i) do { stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define MSTAMP(i) do { stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define XSTAMP(i)
#endif
#else
#define MSTAMP(i)
#define XSTAMP(i)
#endif


// F8: e4m3 operands in the expand MFMA (fp8 sessions).  A template parameter: as a run-time flag both operand paths sat in
// the expand loop of every bf16 session and kept it from unrolling (340 instructions per 32-pixel x 16-channel item).
// MP: the expand conv runs in several passes over slices of its K input channels (a.kp channels per pass): per pass the slice of
// the input tile and of the weight chunk is staged in LDS and every wave adds its products to accumulators that stay in
// registers.  fp32 sessions: a whole-K input tile next to the expanded tile does not fit LDS for the 16x16 tile (blocks 9, 10
// fell back to 8x8 tiles = 704 workgroups = three rounds) or leaves one workgroup per CU where 288 want to be resident (the 8x8
// maps: two rounds).  With K in slices the fp32 fronts get the workgroup counts of the bf16 plan.
// MP = 1: the slices are fetched pass by pass (the next one under the running pass's MFMAs: a pass is then about one memory round
// trip, ~2 us); MP = 2: the WHOLE input tile and weight chunk are requested at kernel start into registers (up to six 8-channel
// vectors per lane: one round trip for the launch, as in the single-pass form) and only parked slice by slice - chosen whenever
// the vectors fit (mbf_mp_fits).
// D: the layer descriptor (above); 0 = every shape from the arguments.
template <bool BF16, int KS, int S, int TS, bool F8, int MP, int D>
__device__ __forceinline__ void mbf_body(const MbfArgs& a) {
  constexpr int MBF_THREADS = TS == 16 ? 1024 : 512, MBF_WAVES = MBF_THREADS / 64;
  constexpr MbfShape SH = mbf_shape(D);
  const int Cexp = D ? SH.Cexp : a.Cexp, CC = D ? SH.CC : a.CC, H = D ? SH.H : a.H, W = D ? SH.W : a.W, Ho = D ? SH.Ho : a.Ho, Wo = D ? SH.Wo : a.Wo;
  const int pad_t = D ? SH.pad_t : a.pad_t, pad_l = D ? SH.pad_l : a.pad_l, sq = D ? SH.sq : a.sq, sqp = D ? SH.sqp : a.sqp;
  const int has_expand = D ? SH.has_expand : a.has_expand, out_frag = D ? SH.out_frag : a.out_frag;
  [[maybe_unused]] const int se_tail = D ? 0 : a.se_tail;                       // (a specialised launch never finishes the squeeze-excite in its tail)
  // what launch_mbf derives from the shape: tiles per row, workgroups per image (= gridDim.x) and their reciprocals
  constexpr int TX_C = (SH.Wo + TS - 1) / TS, CH_C = SH.CC ? (SH.Cexp + SH.CC - 1) / SH.CC : 0, GX_C = TX_C * ((SH.Ho + TS - 1) / TS) * CH_C;
  const int tiles_x = D ? TX_C : a.tiles_x;
  const unsigned ngx = D ? (unsigned)GX_C : gridDim.x;
  const uint32_t chunks_rcp = D ? rcp_u32(CH_C) : a.chunks_rcp, tiles_x_rcp = D ? rcp_u32(TX_C) : a.tiles_x_rcp, gx_rcp = D ? rcp_u32(GX_C) : a.gx_rcp;
  typedef Vec8<BF16> V;
  typedef typename V::elem T;
  typedef Frag<BF16> F;
  typedef typename F::raw raw_t;
  constexpr int KSTEP = F::KSTEP, KLANE = F::KLANE, PAD = BF16 ? 8 : 4;
  constexpr int PW = (TS - 1) * S + KS;              // input tile side
  constexpr int PIN = PW * PW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  HEP_POISON(smem, a.lds_bytes);
#ifdef HEP_MBF_TRACE
  unsigned long long stamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  MSTAMP(0);
#endif
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (uniform: whatever is derived from it alone runs on the scalar unit)
  const int r = lane & 15, g = lane >> 4;
  // The prologue below runs in every wave of a latency-bound workgroup: its instruction count is kernel time
  // (measured with the phase-A stamps: 1250 instructions = 2.6 us before the last staging load was issued).  So every
  // uniform quotient arrives as a host-made reciprocal, the shifts come from clz, addresses are 32-bit offsets from a
  // uniform base and the staging loads are unconditional on a clamped address.
  const int chunks = D ? CH_C : a.chunks;
  // XCD-aware order: the workgroups of one tile (its channel chunks) all stage the same input pixels; as consecutive
  // LOGICAL blocks they share an XCD and its L2 instead of fetching the tile into up to eight of them
  const int logical = xcd_remap(blockIdx.x + blockIdx.y * ngx, ngx * gridDim.y);
  const int b = udiv_rcp(logical, gx_rcp), bxl = logical - b * (int)ngx;
  const int tile = udiv_rcp(bxl, chunks_rcp), chunk = bxl - tile * chunks;
  const int tile_y = udiv_rcp(tile, tiles_x_rcp);
  const int oy0 = tile_y * TS, ox0 = (tile - tile_y * tiles_x) * TS;
  const int iy0 = oy0 * S - pad_t, ix0 = ox0 * S - pad_l;         // input coords of tile pixel (0,0)
  const int c0 = chunk * CC;                                       // first expanded channel of this block
  const int cc = min(CC, Cexp - c0);                               // channels of this block (multiple of 8)
  const int K = D ? SH.Cin : a.Cin;
  const int KP = (MP ? a.kp : K) + PAD, EP = CC + PAD;             // LDS row pitches (elements)
  T* a_s = reinterpret_cast<T*>(smem);                             // [PIN][KP]   input tile
  T* e_s = reinterpret_cast<T*>(smem + a.off_e);                   // [PIN][EP]   expanded (activated) tile
  T* w_s = reinterpret_cast<T*>(smem + a.off_we);                  // [CC][KP]    expand-weight chunk
  float* wdw_s = reinterpret_cast<float*>(smem + a.off_w);         // [KS*KS][CC]
  float* be_s = wdw_s + KS * KS * CC;                              // [CC] expand bias
  float* bdw_s = be_s + CC;                                        // [CC] depthwise bias
  const int K16 = (K + 15) & ~15, KP8 = K16 + 16;                  // fp8 weight rows: bytes in memory / in LDS
  unsigned char* w8_s = smem + a.off_we;

  // ---- phase A: everything this workgroup needs, global -> LDS, all loads issued in batches of 8
  //      before the first LDS store (one memory round trip per batch): depthwise weights + biases,
  //      the expand-weight chunk [cc][K], and the input tile (zero outside the image) ----
  const int ntiles = (cc + 15) / 16;
  const int ksteps = (K + KSTEP - 1) / KSTEP;
  const int r0 = max(0, -iy0), r1 = min(PW, H - iy0), q0 = max(0, -ix0), q1 = min(PW, W - ix0);       // inside rectangle
  const int wi = q1 - q0, n_in = wi * (r1 - r0);
  // inside pixel m -> (row, column) of the rectangle: m < 2^10 and wi <= 20, so (m + 0.5) / wi stays 0.5 / wi away from
  // an integer and the 1-ulp reciprocal cannot move the truncation
  const float wi_inv = __builtin_amdgcn_rcpf((float)wi);
  auto row_of = [&](int m) { return (int)(((float)m + 0.5f) * wi_inv); };
  // depthwise weights + biases: 16-byte vectors; their loads are issued here, the input-tile / expand-weight
  // loads right behind them, and only then are they parked in LDS - one memory round trip for all of
  // phase A (cc and c0 are multiples of 8)
  constexpr int NDW = (KS * KS * 128 / 4 + MBF_THREADS - 1) / MBF_THREADS;       // CC <= 128
  const int cv = cc >> 2;                                                        // float4 vectors per tap
  const int cvsh = cv <= 2 ? 1 : 32 - __builtin_clz(cv - 1);
  f32x4 wv[NDW];
#ifdef HEP_MBF_TRACE_A
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
  XSTAMP(1);
  const float* wdw_g = a.wdw + c0;
#pragma unroll
  for (int j = 0; j < NDW; j++) {
    const int i = threadIdx.x + j * MBF_THREADS, tap = i >> cvsh, c4 = i & ((1 << cvsh) - 1);
    const bool ok = tap < KS * KS && c4 < cv;
    wv[j] = *reinterpret_cast<const f32x4*>(wdw_g + (ok ? (uint32_t)(tap * Cexp + c4 * 4) : 0u));
  }
  const int bi = threadIdx.x;                        // threads [0, cv): depthwise bias, [64, 64 + cv): expand bias
  const bool b_dw = bi < cv, b_ex = has_expand && bi >= 64 && bi - 64 < cv;
  const f32x4 bv = *reinterpret_cast<const f32x4*>((b_ex ? a.be : a.bdw) + c0 + (b_dw || b_ex ? (uint32_t)(bi & 63) * 4 : 0u));
  auto park_weights = [&]() {
#pragma unroll
    for (int j = 0; j < NDW; j++) {
      const int i = threadIdx.x + j * MBF_THREADS, tap = i >> cvsh, c4 = i & ((1 << cvsh) - 1);
      if (tap < KS * KS && c4 < cv) *reinterpret_cast<f32x4*>(wdw_s + tap * CC + c4 * 4) = wv[j];
    }
    if (b_dw) *reinterpret_cast<f32x4*>(bdw_s + bi * 4) = bv;
    else if (b_ex) *reinterpret_cast<f32x4*>(be_s + (bi - 64) * 4) = bv;
  };
  {
    constexpr int NB = BF16 ? 8 : 4;                               // 16-byte vectors (bf16) / 32-byte pairs (fp32) in flight per lane
    constexpr int VB = 8 * (int)sizeof(T);                         // bytes of one 8-channel vector
    const int vecs = has_expand ? K >> 3 : cc >> 3;                // 8-channel vectors per staged pixel
    const unsigned char* in_b = reinterpret_cast<const unsigned char*>(a.in) + (int64_t)b * H * W * K * (int)sizeof(T);
    // thread -> (row, vector): vectors rounded up to a power of two so the split is a shift and a mask
    const int vsh = vecs <= 1 ? 0 : 32 - __builtin_clz(vecs - 1);
    const int v = threadIdx.x & ((1 << vsh) - 1), row0 = threadIdx.x >> vsh, rstride = MBF_THREADS >> vsh;
    if constexpr (MP != 0) {
      // ---- multi-pass expand (see the template comment): pass p = input channels [p * kp, (p + 1) * kp) ----
      const int Kp = a.kp, npass = a.npass, n_wrows = ntiles * 16;
      const int pvecs = Kp >> 3;                                     // 8-channel vectors per row and pass
      const int pvsh = pvecs <= 1 ? 0 : 32 - __builtin_clz(pvecs - 1);
      const int pv = threadIdx.x & ((1 << pvsh) - 1), prow0 = threadIdx.x >> pvsh, prs = MBF_THREADS >> pvsh;
      constexpr int NIW = TS == 16 ? 1 : 2, NIP = TS == 16 ? 2 : 3;   // row batches per lane and pass (host-checked: mbf_mp_fits)
      const unsigned char* w_b = reinterpret_cast<const unsigned char*>(a.we) + (int64_t)c0 * K * (int)sizeof(T);
      const int pix0 = (iy0 + r0) * W + ix0 + q0;
      constexpr bool RES = MP == 2;
      // RES: item i = tid + j * threads of the (weight rows + inside pixels) x (K / 8 vectors) grid; everything in flight at once
      constexpr int NJ = RES ? 6 : 1;
      raw_t rq0[NJ], rq1[NJ]; int qdst[NJ], qsl[NJ];                   // vectors, LDS element offset (>= 0: in a_s, < 0: -(1 + offset) in w_s), slice
      if constexpr (RES) {
        const int vk_ = K >> 3;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
          const int i = threadIdx.x + j * MBF_THREADS, row = udiv_rcp(i, a.vk_rcp), vec = i - row * vk_;
          const bool ok = row < n_wrows + n_in, is_w = row < n_wrows;
          const int m = min(max(row - n_wrows, 0), n_in - 1), ri = row_of(m);
          const uint32_t off_w = (uint32_t)(min(row, n_wrows - 1) * K + vec * 8) * (uint32_t)sizeof(T);
          const uint32_t off_p = (uint32_t)((pix0 + ri * W + (m - ri * wi)) * K + vec * 8) * (uint32_t)sizeof(T);
          const unsigned char* src = (is_w ? w_b : in_b) + (ok ? (is_w ? off_w : off_p) : 0u);
          rq0[j] = *reinterpret_cast<const raw_t*>(src); if (!BF16) rq1[j] = *reinterpret_cast<const raw_t*>(src + 16);
          const int sl = udiv_rcp(vec, a.kpv_rcp), col = vec * 8 - sl * Kp;
          qsl[j] = ok ? sl : -1;
          qdst[j] = is_w ? -(1 + row * KP + col) : m * KP + col;
        }
      }
      raw_t w0[NIW], w1[NIW], p0[NIP], p1[NIP];
      auto issue = [&](int p) {
        if constexpr (RES) return;
        const int kb = p * Kp + pv * 8;
        const bool vk = pv < pvecs && kb < K;                       // (K is a multiple of 8: a vector is inside or outside)
#pragma unroll
        for (int j = 0; j < NIW; j++) {
          const int row = j * prs + prow0;
          const unsigned char* src = w_b + (vk && row < n_wrows ? (uint32_t)(row * K + kb) * (uint32_t)sizeof(T) : 0u);
          w0[j] = *reinterpret_cast<const raw_t*>(src); if (!BF16) w1[j] = *reinterpret_cast<const raw_t*>(src + 16);
        }
#pragma unroll
        for (int j = 0; j < NIP; j++) {
          const int mm = j * prs + prow0, m = min(mm, n_in - 1), ri = row_of(m);
          const uint32_t off = (uint32_t)((pix0 + ri * W + (m - ri * wi)) * K + kb) * (uint32_t)sizeof(T);
          const unsigned char* src = in_b + (vk && mm < n_in ? off : 0u);
          p0[j] = *reinterpret_cast<const raw_t*>(src); if (!BF16) p1[j] = *reinterpret_cast<const raw_t*>(src + 16);
        }
      };
      auto park = [&](int p) {
        if constexpr (RES) {
#pragma unroll
          for (int j = 0; j < NJ; j++)
            if (qsl[j] == p) {
              raw_t* d = qdst[j] < 0 ? reinterpret_cast<raw_t*>(w_s + (-1 - qdst[j])) : reinterpret_cast<raw_t*>(a_s + qdst[j]);
              d[0] = rq0[j]; if (!BF16) d[1] = rq1[j];
            }
          return;
        }
        const bool vk = pv < pvecs && p * Kp + pv * 8 < K;          // weights beyond K are parked as ZEROS (the activation columns there
#pragma unroll                                                        //  keep the previous pass's finite values: finite x 0)
        for (int j = 0; j < NIW; j++) {
          const int row = j * prs + prow0;
          if (pv < pvecs && row < n_wrows) {
            raw_t* d = reinterpret_cast<raw_t*>(w_s + row * KP + pv * 8);
            d[0] = vk ? w0[j] : raw_t{}; if (!BF16) d[1] = vk ? w1[j] : raw_t{};
          }
        }
#pragma unroll
        for (int j = 0; j < NIP; j++) {
          const int m = j * prs + prow0;
          if (vk && m < n_in) {
            raw_t* d = reinterpret_cast<raw_t*>(a_s + m * KP + pv * 8);
            d[0] = p0[j]; if (!BF16) d[1] = p1[j];
          }
        }
      };
      issue(0);
      {
        const int nv = PIN * EP * (int)sizeof(T) / 16;               // the whole [PIN][EP] tile: zeros = the depthwise conv's padding
        for (int i = threadIdx.x; i < nv; i += MBF_THREADS) reinterpret_cast<u32x4*>(e_s)[i] = (u32x4){0, 0, 0, 0};
      }
      XSTAMP(2); park_weights(); XSTAMP(3);
      park(0);
      MSTAMP(1); XSTAMP(4);
      __syncthreads();
      MSTAMP(2); XSTAMP(5);
      const int ntsh = ntiles <= 1 ? 0 : 32 - __builtin_clz(ntiles - 1);
      const int nt = wave & ((1 << ntsh) - 1), grp = wave >> ntsh, ngrp = MBF_WAVES >> ntsh;
      const int mtiles = (n_in + 15) >> 4, kspp = Kp / KSTEP;
      constexpr int MAXMT = TS == 16 ? 7 : 5, KSPMAX = 3;            // m-tiles per wave, k-steps per pass (host-checked)
      f32x4 acc[MAXMT];
#pragma unroll
      for (int i = 0; i < MAXMT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int p = 0; p < npass; p++) {
        if (p + 1 < npass) issue(p + 1);                             // the next slice travels under this pass's MFMAs
        if (nt < ntiles) {
          raw_t wfr[KSPMAX];
          const T* wrow = w_s + (nt * 16 + r) * KP + KLANE * g;
#pragma unroll
          for (int ks = 0; ks < KSPMAX; ks++) {
            wfr[ks] = *reinterpret_cast<const raw_t*>(wrow + (ks < kspp ? ks * KSTEP : 0));
            if (p * Kp + ks * KSTEP + KLANE * g >= K) wfr[ks] = raw_t{};     // k >= K (last slice): the weight is the zero, the activation column holds finite leftovers
          }
#pragma unroll
          for (int i = 0; i < MAXMT; i++) {
            const int mt = grp + i * ngrp;
            if (mt < mtiles) {                                       // (wave-uniform)
              const T* arow = a_s + min(mt * 16 + r, n_in - 1) * KP + KLANE * g;
#pragma unroll
              for (int ks = 0; ks < KSPMAX; ks++) {
                if (ks < kspp) {                                     // (uniform)
                  const raw_t xa = *reinterpret_cast<const raw_t*>(arow + ks * KSTEP);
                  acc[i] = F::mma(wfr[ks], xa, acc[i]);
                }
              }
            }
          }
        }
        __syncthreads();                                             // every wave has read this slice
        if (p + 1 < npass) { park(p + 1); __syncthreads(); }
      }
      // bias + swish -> the expanded tile (only pixels inside the image; the rest stays zero)
      {
        const int n = nt * 16 + 4 * g;
        if (nt < ntiles && n < cc) {
          const f32x4 bias = *reinterpret_cast<const f32x4*>(be_s + n);
#pragma unroll
          for (int i = 0; i < MAXMT; i++) {
            const int m = (grp + i * ngrp) * 16 + r;
            if (m < n_in) {
              const int ri = row_of(m), pp_ = (r0 + ri) * PW + q0 + (m - ri * wi);
              float vv[4];
#pragma unroll
              for (int q = 0; q < 4; q++) vv[q] = acc[i][q] + bias[q];
              swish_n<BF16, 4>(vv);
              V::store4(e_s, (int64_t)pp_ * EP + n, vv);
            }
          }
        }
      }
      MSTAMP(3);
      __syncthreads();
      MSTAMP(4);
    } else if (has_expand) {
      // rows = the expand-weight rows c0 .. c0 + 16*ntiles, then the tile pixels INSIDE the image (compact rows
      // m = ri * wi + ci of the rectangle [r0,r1) x [q0,q1) of the PW x PW tile): only those are staged and expanded;
      // the rest of the expanded tile is the zero padding of the depthwise conv and is written as zeros right here
      const int n_wrows = ntiles * 16;
      // fp8 sessions: the expand weights are e4m3, rows padded to K16 = ceil16(K) bytes in memory and K16 + 16 in LDS
      const int wrow_b = F8 ? K16 : K * (int)sizeof(T), vecs_w = F8 ? K16 >> 4 : vecs, wv_b = F8 ? 16 : VB;
      const unsigned char* w_b = reinterpret_cast<const unsigned char*>(a.we) + (int64_t)c0 * wrow_b;
      const int pix0 = (iy0 + r0) * W + ix0 + q0;                  // first inside pixel of the tile in the image
      const int nv = PIN * EP * (int)sizeof(T) / 16;               // the whole [PIN][EP] tile in 16-byte vectors
      for (int i = threadIdx.x; i < nv; i += MBF_THREADS) reinterpret_cast<u32x4*>(e_s)[i] = (u32x4){0, 0, 0, 0};
      // weight rows and pixel rows are separate batches (a per-row select between the two address forms compiled to
      // two branches per load); the first batch of each is in flight before anything is parked
      constexpr int NH = NB / 2;
      const bool vok_w = v < vecs_w, vok = v < vecs;
      const int wstep = rstride * wrow_b;
      raw_t w0[NH], w1[NH], p0[NH], p1[NH];
      auto issue_w = [&](int base) {
        uint32_t off = (uint32_t)((base + row0) * wrow_b + v * wv_b);
#pragma unroll
        for (int j = 0; j < NH; j++, off += wstep) {
          const unsigned char* src = w_b + (vok_w && base + j * rstride + row0 < n_wrows ? off : 0u);
          w0[j] = *reinterpret_cast<const raw_t*>(src); if (!BF16) w1[j] = *reinterpret_cast<const raw_t*>(src + 16);
        }
      };
      auto store_w = [&](int base) {
#pragma unroll
        for (int j = 0; j < NH; j++) {
          const int row = base + j * rstride + row0;
          if (vok_w && row < n_wrows) {
            raw_t* d = F8 ? reinterpret_cast<raw_t*>(w8_s + row * KP8 + v * 16) : reinterpret_cast<raw_t*>(w_s + row * KP + v * 8);
            d[0] = w0[j]; if (!BF16) d[1] = w1[j];
          }
        }
      };
      auto issue_p = [&](int base) {
#pragma unroll
        for (int j = 0; j < NH; j++) {
          const int mm = base + j * rstride + row0, m = min(mm, n_in - 1), ri = row_of(m);
          const uint32_t off = (uint32_t)((pix0 + ri * W + (m - ri * wi)) * K) * (uint32_t)sizeof(T) + (uint32_t)(v * VB);
          const unsigned char* src = in_b + (vok && mm < n_in ? off : 0u);
          p0[j] = *reinterpret_cast<const raw_t*>(src); if (!BF16) p1[j] = *reinterpret_cast<const raw_t*>(src + 16);
        }
      };
      auto store_p = [&](int base) {
#pragma unroll
        for (int j = 0; j < NH; j++) {
          const int m = base + j * rstride + row0;
          if (vok && m < n_in) {
            raw_t* d = reinterpret_cast<raw_t*>(a_s + m * KP + v * 8);
            d[0] = p0[j]; if (!BF16) d[1] = p1[j];
          }
        }
      };
      issue_w(0); issue_p(0);
      XSTAMP(2); park_weights(); XSTAMP(3);                       // their loads were issued first: this waits for them only
      store_w(0); store_p(0);
      for (int base = rstride * NH; base < n_wrows; base += rstride * NH) { issue_w(base); store_w(base); }
      for (int base = rstride * NH; base < n_in; base += rstride * NH) { issue_p(base); store_p(base); }
    } else {
      // depthwise alone: the PIN tile pixels of this block's channels, zero outside the image
      for (int base = 0; base < PIN; base += rstride * NB) {
        raw_t x0[NB], x1[NB];
        bool inside[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) {
          const int p = base + j * rstride + row0, ty = p / PW, gy = iy0 + ty, gx = ix0 + p - ty * PW;
          inside[j] = p < PIN && v < vecs && gy >= 0 && gy < H && gx >= 0 && gx < W;
          const uint32_t off = (uint32_t)((gy * W + gx) * K + c0) * (uint32_t)sizeof(T) + (uint32_t)(v * VB);
          const unsigned char* src = in_b + (inside[j] ? off : 0u);
          x0[j] = *reinterpret_cast<const raw_t*>(src); if (!BF16) x1[j] = *reinterpret_cast<const raw_t*>(src + 16);
        }
        if (base == 0) { XSTAMP(2); park_weights(); XSTAMP(3); }
#pragma unroll
        for (int j = 0; j < NB; j++) {
          const int p = base + j * rstride + row0;
          if (p < PIN && v < vecs) {
            raw_t* d = reinterpret_cast<raw_t*>(e_s + p * EP + v * 8);
            d[0] = inside[j] ? x0[j] : raw_t{}; if (!BF16) d[1] = inside[j] ? x1[j] : raw_t{};
          }
        }
      }
    }
  }
  if constexpr (MP == 0) {
  MSTAMP(1); XSTAMP(4);
  __syncthreads();
  MSTAMP(2); XSTAMP(5);
  }

  // ---- phase B: expand 1x1 + bias + swish -> e_s ----
  if (MP == 0 && has_expand) {
    // a wave takes TWO m-tiles per weight fragment (one LDS weight read feeds two MFMAs) and keeps
    // three k-steps of fragments in flight
    const int mpairs = (n_in + 31) >> 5;                           // pairs of 16-pixel m-tiles over the inside pixels
    const int ntsh = ntiles <= 1 ? 0 : 32 - __builtin_clz(ntiles - 1);   // pp -> (mp, nt): a shift and a mask
    constexpr int KSMAX = BF16 ? 6 : 12;                           // k-steps of weight fragments a wave keeps in registers (K <= 192)
    if (!F8 && ksteps <= KSMAX && (1 << ntsh) <= MBF_WAVES) {
      // A wave owns ONE n-tile for the whole phase: its weight fragments are read once into registers and every m-tile costs
      // ksteps activation reads + MFMAs + the epilogue.  As (m-pair, n-tile) items dealt round-robin each item re-read its
      // weights and ran ~260 instructions for 8 outputs per lane: the phase was issue-bound at 32 instructions per output.
      const int nt = wave & ((1 << ntsh) - 1), grp = wave >> ntsh, ngrp = MBF_WAVES >> ntsh;
      const int n = nt * 16 + 4 * g;
      if (nt < ntiles) {
        // (k >= K: the fragment is read from the START of the row - staged, finite data - and replaced by zeros.  The row's
        //  pad columns are never written: read as an operand they multiply the other side's zero by whatever an earlier
        //  launch left in LDS, and 0 x NaN is NaN - phi 0 @ 128 produced NaNs that way, K = 24.)
        raw_t wfr[KSMAX];
        const T* wrow = w_s + (nt * 16 + r) * KP;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ks++) {
          const bool kok = ks < ksteps && ks * KSTEP + KLANE * g < K;
          wfr[ks] = *reinterpret_cast<const raw_t*>(wrow + (kok ? ks * KSTEP + KLANE * g : 0));
          if (!kok) wfr[ks] = raw_t{};                              // k >= K: the weight is the zero (the activation read is clamped, finite)
        }
        const f32x4 bias = *reinterpret_cast<const f32x4*>(be_s + min(n, cc - 4));
        const int mtiles = (n_in + 15) >> 4;
        for (int mt = grp; mt < mtiles; mt += 2 * ngrp) {           // two m-tiles at a time: independent MFMA chains
          const int m0 = mt * 16 + r, m1 = m0 + 16 * ngrp;
          const T* arow0 = a_s + min(m0, n_in - 1) * KP;
          const T* arow1 = a_s + min(m1, n_in - 1) * KP;
          f32x4 acc0 = bias, acc1 = bias;
#pragma unroll
          for (int ks = 0; ks < KSMAX; ks++) {
            if (ks < ksteps) {                                      // (uniform)
              const int ko = ks * KSTEP + KLANE * g < K ? ks * KSTEP + KLANE * g : 0;
              const raw_t xa0 = *reinterpret_cast<const raw_t*>(arow0 + ko), xa1 = *reinterpret_cast<const raw_t*>(arow1 + ko);
              acc0 = F::mma(wfr[ks], xa0, acc0);
              acc1 = F::mma(wfr[ks], xa1, acc1);
            }
          }
          if (n < cc) {
#pragma unroll
            for (int half = 0; half < 2; half++) {
              const int m = half ? m1 : m0;
              if (m < n_in) {
                const f32x4 acc = half ? acc1 : acc0;
                const int ri = row_of(m), p = (r0 + ri) * PW + q0 + (m - ri * wi);   // tile position of inside pixel m
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = acc[q];
                swish_n<BF16, 4>(v);
                V::store4(e_s, (int64_t)p * EP + n, v);
              }
            }
          }
        }
      }
    } else
    for (int pp = wave; pp < (mpairs << ntsh); pp += MBF_WAVES) {
      const int nt = pp & ((1 << ntsh) - 1), mp = pp >> ntsh;
      if (nt >= ntiles) continue;
      const int m0 = mp * 32 + r, m1 = m0 + 16;
      const T* wrow = w_s + (int64_t)(nt * 16 + r) * KP;
      const T* arow0 = a_s + (int64_t)m0 * KP;
      const T* arow1 = a_s + (int64_t)m1 * KP;
      f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
      const unsigned char* w8row = w8_s + (int64_t)(nt * 16 + r) * KP8;
      const float inv_as = F8 ? 1.0f / a.a_scale : 1.0f;
      // (LDS reads are unconditional on clamped offsets - rows past the staged pixels and k past K read staged data and the
      //  activation fragment is zeroed by a select, so W needs none; a read under a branch costs a full wait per k-step)
      const int mc0 = min(m0, n_in - 1) - m0, mc1 = min(m1, n_in - 1) - m1;      // row clamps as element offsets below
      const bool mok0 = m0 < n_in, mok1 = m1 < n_in;
#pragma unroll 2
      for (int ks = 0; ks < ksteps; ks++) {
        const int k = ks * KSTEP + KLANE * g;
        const bool kok = k < K;
        const int ko = kok ? k : 0;                 // (k >= K: the start of the row, never its unwritten pad columns - 0 x NaN is NaN)
        raw_t xa0 = *reinterpret_cast<const raw_t*>(arow0 + mc0 * KP + ko), xa1 = *reinterpret_cast<const raw_t*>(arow1 + mc1 * KP + ko);
        if (!(kok && mok0)) xa0 = raw_t{};
        if (!(kok && mok1)) xa1 = raw_t{};
        if constexpr (F8) {
          const u32x2 wf8 = *reinterpret_cast<const u32x2*>(w8row + (kok ? ks * 32 + 8 * g : 0));
          const long wl = __builtin_bit_cast(long, wf8);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wl, cvt_fp8x8(xa0, nullptr, inv_as), acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wl, cvt_fp8x8(xa1, nullptr, inv_as), acc1, 0, 0, 0);
        } else {
          const raw_t wf = *reinterpret_cast<const raw_t*>(wrow + ko);
          acc0 = F::mma(wf, xa0, acc0);
          acc1 = F::mma(wf, xa1, acc1);
        }
      }
      const int n = nt * 16 + 4 * g;          // lane: 4 consecutive expanded channels of tile pixels m0, m1
      if (n < cc) {
        const f32x4 bias = *reinterpret_cast<const f32x4*>(be_s + n);
        f32x4 ws = (f32x4){1.f, 1.f, 1.f, 1.f};
        if constexpr (F8) ws = *reinterpret_cast<const f32x4*>(a.we_scale + c0 + n) * a.a_scale;       // dequantisation: a_scale * w_scale[n]
#pragma unroll
        for (int half = 0; half < 2; half++) {
          const int m = half ? m1 : m0;
          if (m < n_in) {
            const f32x4 acc = half ? acc1 : acc0;
            const int ri = row_of(m), p = (r0 + ri) * PW + q0 + (m - ri * wi);   // tile position of inside pixel m
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = F8 ? fmaf(acc[q], ws[q], bias[q]) : acc[q] + bias[q];
            swish_n<BF16, 4>(v);
            V::store4(e_s, (int64_t)p * EP + n, v);
          }
        }
      }
    }
    MSTAMP(3);
    __syncthreads();
  }
  if constexpr (MP == 0) { MSTAMP(4); }

  // ---- phase C: depthwise taps from LDS -> global, SE sums ----
  // A lane owns FOUR horizontally adjacent output pixels x FOUR channels (round 6; before: two pixels x eight channels): the 3 S + KS
  // input columns of a tap row are read (8 bytes in bf16) and unpacked once for all four pixels and the row's KS weight vectors are read
  // once - per tap row of a 5x5 stride-1 layer 8 + 5 LDS reads of 144 bytes and 32 unpack instructions instead of 6 + 10 reads of 256
  // bytes and 48.  Every output still accumulates its taps in the order (ky, kx) ascending, and the squeeze-excite sums keep their
  // tree (pixel pairs first, then pairs of pairs = this lane's four pixels, then the lanes): bit-identical to the two-pixel form.
  // The (pixel quad, channel quad) items are split over BOTH halves of the workgroup by tap row on the 8x8 tiles: waves 0-3 take the
  // first (KS+1)/2 rows of taps, waves 4-7 the rest and hand their partial sums over through LDS (the dead input tile) - the phase is a
  // chain of dependent LDS reads per tap row, so halving the rows per lane shortens it.
  const int cqs = cc >> 2;                                                 // channel quads of this chunk (cc is a multiple of 8)
  const int cqsh = cqs <= 1 ? 0 : 32 - __builtin_clz(cqs - 1), cqp = 1 << cqsh;
  // (TS 16: 64 pixel quads x 16 channel quads = one item per lane, all tap rows, no hand-over)
  constexpr bool SPLIT = TS == 8;
  constexpr int HALF = SPLIT ? MBF_THREADS / 2 : MBF_THREADS;
  const int half = SPLIT ? threadIdx.x / HALF : 0, tl = SPLIT ? threadIdx.x % HALF : threadIdx.x;
  const int cq = tl & (cqp - 1), qd = tl >> cqsh;                          // pixel quad 0 .. TS*TS/4 - 1
  f32x4* xch = reinterpret_cast<f32x4*>(smem);                             // [4][HALF] float4: partial sums of the second half (SPLIT)
  float sum[4] = {0, 0, 0, 0};
  const bool item = cq < cqs && qd < TS * TS / 4;
  constexpr int KH = SPLIT ? (KS + 1) / 2 : KS;
  constexpr int NX = 3 * S + KS;                                           // input columns under four adjacent outputs
  const int py = qd / (TS / 4), px = (qd % (TS / 4)) * 4;
  float acc[4][4];                                                         // [pixel][channel]
  if (item) {
    {
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(bdw_s + cq * 4);
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[j][c] = half ? 0.f : b0[c];
    }
#pragma unroll 1      // a real loop: unrolled, the compiler hoists all KS*KS weight reads and spills
    for (int ky = half ? KH : 0; ky < (half ? KS : KH); ky++) {
      f32x4 wr[KS];
#pragma unroll
      for (int kx = 0; kx < KS; kx++) wr[kx] = *reinterpret_cast<const f32x4*>(wdw_s + (ky * KS + kx) * CC + cq * 4);
      const int64_t erow = (int64_t)((py * S + ky) * PW + px * S) * EP + cq * 4;
#pragma unroll
      for (int hx = 0; hx < NX; hx++) {
        float ev[4];
        V::load4(e_s, erow + (int64_t)hx * EP, ev);
        // column hx is tap kx = hx - j S of output j: ascending hx = ascending kx for every output
#pragma unroll
        for (int j = 3; j >= 0; j--) {
          const int kx = hx - j * S;
          if (kx >= 0 && kx < KS) {
#pragma unroll
            for (int c = 0; c < 4; c++) acc[j][c] = fmaf(ev[c], wr[kx][c], acc[j][c]);
          }
        }
      }
    }
    if (SPLIT && half) {
#pragma unroll
      for (int j = 0; j < 4; j++) xch[j * HALF + tl] = (f32x4){acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
    }
  }
  __syncthreads();
  if (item && !half) {
    if constexpr (SPLIT) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const f32x4 pj = xch[j * HALF + tl];
#pragma unroll
        for (int c = 0; c < 4; c++) acc[j][c] += pj[c];
      }
    }
    const int oy = oy0 + py, ox = ox0 + px;
    // (out_frag: the project GEMM's fragment order - row m = (image, pixel); a 16-byte unit holds KLANE channels from k:
    //  unit ((m / 16) * ksteps + k / KSTEP) * 64 + (k % KSTEP) / KLANE * 16 + m % 16; bf16: a lane's four channels are half a unit)
    auto ostore = [&](int ox_, const float* vv) {
      const int m = (b * Ho + oy) * Wo + ox_, k = c0 + cq * 4;
      if (!out_frag) { V::store4(a.out, (int64_t)m * Cexp + k, vv); return; }
      constexpr int KST = BF16 ? 32 : 16, KLN = BF16 ? 8 : 4;
      const int kst = (Cexp + KST - 1) / KST;
      const int64_t unit = (int64_t)((m >> 4) * kst + k / KST) * 64 + ((k % KST) / KLN) * 16 + (m & 15);
      V::store4(a.out, unit * KLN + (k & (KLN - 1)), vv);
    };
    if (oy < Ho) {
      // channel sums in the order of the two-pixel form: (0 + v0) + v1 per pixel pair, then the two pairs
      float sp[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        // (the second pixel of a pair is only inside when the first one is: ox + j < Wo is the two-pixel form's nesting)
        if (ox + j < Wo) {
          float v[4];
#pragma unroll
          for (int c = 0; c < 4; c++) v[c] = acc[j][c];
          swish_n<BF16, 4>(v);
#pragma unroll
          for (int c = 0; c < 4; c++) sp[j >> 1][c] += v[c];
          ostore(ox + j, v);
        }
      }
#pragma unroll
      for (int c = 0; c < 4; c++) sum[c] = sp[0][c] + sp[1][c];
    }
  }
  MSTAMP(5);

  // ---- phase D: squeeze-excite.  The mean over the image and the reduce FC are linear in the channel
  //      sums, so every workgroup contributes the partial products of ITS channels and pixels:
  //        hpart[b][workgroup][j] = sum_{c in chunk} wr[j][c0 + c] * (sum of this tile's outputs of channel c)
  //      and the project GEMM (k_pw.hip) adds the rows up, applies 1/HW, bias and swish and runs the
  //      expand FC in its prologue - no squeeze-excite launch.  Fixed order everywhere (wave butterfly,
  //      the depthwise waves added in order, lane butterfly): bit-reproducible, no atomics. ----
  if (a.hpart) {
    constexpr int NWC = HALF / 64;                                        // waves that produced outputs
    float* ssum = reinterpret_cast<float*>(smem + a.off_e);               // [NWC][CC]: the expanded tile is dead
    // The reduce-FC weights of this thread's hidden unit (8 lanes share unit j = thread / 8; sq <= 64: one unit per thread
    // group) are requested HERE: their address depends on nothing computed below, the depthwise registers are dead, and the
    // L2 round trip (~1 us behind the output stores) then runs under the butterfly, the barrier and the channel sums instead of
    // after them.  (Requested at kernel start they cost eight live registers through every phase and lost, round 4.)
    const int part = threadIdx.x & 7, ch = part * 8;                      // 8 lanes share one hidden unit j
    const int jp = threadIdx.x >> 3;
    f32x4 wp0, wp1;
    {
      const f32x4* wp = reinterpret_cast<const f32x4*>(a.se_wr + (int64_t)min(jp, sq - 1) * Cexp + c0 + min(ch, max(cc - 8, 0)));
      wp0 = wp[0]; wp1 = wp[1];
    }
    if (wave < NWC) {
      for (int off = cqp; off < 64; off <<= 1) {                           // (the lane already holds a pair of pixel pairs: the first level of the old tree)
#pragma unroll
        for (int c = 0; c < 4; c++) sum[c] += __shfl_xor(sum[c], off, 64);
      }
      if (lane < cqs) *reinterpret_cast<f32x4*>(ssum + wave * CC + lane * 4) = (f32x4){sum[0], sum[1], sum[2], sum[3]};
    }
    __syncthreads();
    float cs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ch < cc) {
#pragma unroll
      for (int w4 = 0; w4 < NWC; w4++) {
        const f32x4* sp = reinterpret_cast<const f32x4*>(ssum + w4 * CC + ch);
        const f32x4 s0 = sp[0], s1 = sp[1];
#pragma unroll
        for (int c = 0; c < 4; c++) { cs[c] += s0[c]; cs[4 + c] += s1[c]; }
      }
    }
    // (round 4: requesting the reduce weights at kernel start - their addresses depend on nothing the kernel computes, at the end
    //  they are a dependent L2 round trip - measured SLOWER: 48.7k against 49.6k frames/s in bf16, 24.75k against 24.94k in fp32,
    //  three interleaved runs each; eight more live registers through every phase cost more than the round trip)
    float* hrow = a.hpart + ((int64_t)b * ngx + bxl) * sqp;         // ngx = tiles * chunks
    for (int j = threadIdx.x >> 3; j < ((sq + 63) & ~63); j += MBF_THREADS / 8) {
      float dot = 0.f;
      if (j < sq && ch < cc) {
        f32x4 w0 = wp0, w1 = wp1;
        if (j != jp) {                                                    // (more than MBF_THREADS / 8 hidden units: never at the reference's widths)
          const f32x4* wp = reinterpret_cast<const f32x4*>(a.se_wr + (int64_t)j * Cexp + c0 + ch);
          w0 = wp[0]; w1 = wp[1];
        }
        dot = ((w0[0] * cs[0] + w0[1] * cs[1]) + (w0[2] * cs[2] + w0[3] * cs[3])) + ((w1[0] * cs[4] + w1[1] * cs[5]) + (w1[2] * cs[6] + w1[3] * cs[7]));
      }
      dot += __shfl_xor(dot, 1, 64); dot += __shfl_xor(dot, 2, 64); dot += __shfl_xor(dot, 4, 64);
      if (part == 0 && j < sq) {
#ifdef HEP_ALT
        if (se_tail) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dot), __builtin_amdgcn_make_buffer_rsrc(hrow, 0, 0x7fffffff, 0x00020000), j * 4, 0, 17);     // sc0 sc1: written through
        else
#endif
        hrow[j] = dot;
      }
    }
#ifdef HEP_ALT      // (alternative library only: HEP_SE_TAIL=1, a measured loss against se_finish_kernel - NOTEBOOK.md)
    // ---- tail: the image's LAST workgroup finishes the squeeze-excite (hidden vector, expand FC, sigmoid -> scale[b][Cexp]) ----
    // No workgroup waits for another one: a ticket per image, and whoever draws the last one has every row in memory (each
    // workgroup's stores are acknowledged - vmcnt(0) - and its lanes met at a barrier before its ticket is drawn) and reads the
    // rows past its XCD's L2.  The counter is zero again when the launch ends.  (The memory-model-correct release / acquire pair at
    // agent scope writes back and invalidates the whole L2: 2-6 us per workgroup, MI355X_MICROARCH price list; this costs one
    // atomic round trip per workgroup and ~3 us in the one workgroup that runs the finish, against a ~4 us launch + its boundary.)
    if (se_tail) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      unsigned* flag = reinterpret_cast<unsigned*>(smem);                 // (everything in LDS is dead)
      if (threadIdx.x == 0) {
        unsigned* cnt = a.tail_counter + b * 32;
        const bool last = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == ngx;
        if (last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = last;
      }
      __syncthreads();
      if (*flag) se_finish_body<BF16, MBF_THREADS, true>(a.tail, b, 0, a.tail.C, threadIdx.x, reinterpret_cast<float*>(smem) + 32);
    }
#endif
  }
#ifdef HEP_MBF_TRACE
  MSTAMP(6);
  if (g_mbf_trace && a.trace && lane == 0) {
    unsigned long long* o = g_mbf_trace + ((size_t)(b * ngx + bxl) * MBF_WAVES + wave) * 8;
    for (int i = 0; i < 7; i++) o[i] = stamps[i];
    o[7] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));
  }
#endif
}

// the generic kernel: every shape from the arguments
template <bool BF16, int KS, int S, int TS, bool F8, int MP>
__global__ __launch_bounds__(TS == 16 ? 1024 : 512) void mbf_kernel(MbfArgs a) { mbf_body<BF16, KS, S, TS, F8, MP, 0>(a); }
// row D of MBF_SHAPES: the layer's shape folded in
template <bool BF16, int KS, int S, int TS, int MP, int D>
__global__ __launch_bounds__(TS == 16 ? 1024 : 512) void mbf_shape_kernel(MbfArgs a) { mbf_body<BF16, KS, S, TS, false, MP, D>(a); }

// the pick (hep_pick.h) of the rows a translation unit instantiates (k_mbf_s16.hip, k_mbf_s8.hip): empty when the row is not theirs
#define MBF_SHAPE_TU(ROWS, PICK, BIND) \
  Pick PICK(int id, const MbfArgs& a) { \
    switch (id) { \
      ROWS(MBF_SHAPE_PICK_ROW) \
      default: return Pick(); \
    } \
  } \
  void BIND(unsigned long long* p) { MBF_TRACE_BIND_TU(p); }
#define MBF_SHAPE_PICK_ROW(id, bf, ks, s_, ts, mp, ...) \
  case id: return HEP_PICK(ts == 16 ? 1024 : 512, a.lds_bytes, 159 * 1024, mbf_shape_kernel, bf, ks, s_, ts, mp, id);
#ifdef HEP_MBF_TRACE
#define MBF_TRACE_BIND_TU(p) mbf_trace_bind_tu(p)
#else
#define MBF_TRACE_BIND_TU(p) (void)(p)
#endif
