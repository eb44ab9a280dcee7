// k_sep_impl.h - the fused SeparableConvBlock kernel (see k_sep.hip for what it computes) as a template, shared by the translation
// units that instantiate it: k_sep.hip (the generic kernels, every shape) and k_sep_shape.hip (the shape-specialised single nodes).
#pragma once
#include <type_traits>

#include "hep_dev.h"
#include "hep_internal.h"

// Node shapes as compile-time constants (as MBF_SHAPES of k_mbf_impl.h).  A single-node workgroup lives 5.4-6.3 us
// and spends 2.1-2.8 us of them between "kernel arguments arrived" and "halo stored": descriptor loads, address arithmetic and one
// memory round trip.  Descriptor D = 0 takes everything from SepArgs - sep_kernel, the path of every other width, map size, phi and
// dtype; D > 0 is row D of SEP_SHAPES and runs as sep_shape_kernel<true, D>.  One row per single-node shape of the benchmarked session
// (phi 0 @ 256 in bf16; every row serves BiFPN cells 0, 1 and 2).  Every row is bf16, width SEP_SHAPE_C, 8x8 tiles, eight waves, no
// staged weights, swish in front of the depthwise conv, no activation behind the pointwise one, map output.  launch_sep selects a row
// only when EVERY folded field of the launch equals it (sep_shape_id), so a row that no longer matches the planner falls back to
// D = 0 instead of computing with stale constants.  Only where the numbers come from changes: taps, order of the weighted sum and of
// the depthwise accumulation, rounding points, (m-tile, n-tile) dealing and LDS layout are those of D = 0.  With the sources known the
// "same" loads of unused source slots and the (y, x) read of a pooled source - issued and ignored by D = 0 - are not issued.
//   id   h   w nsrc  kind[3]                         sh[3]         sw[3]         pool_pad[3]
#define SEP_SHAPES(X) \
  X(1, 16, 16, 2, SRC_SAME, SRC_UP,   SRC_SAME,  16,  8,  0,   16,  8,  0,   0, 0, 0)   /* conv4_up */ \
  X(2, 32, 32, 2, SRC_SAME, SRC_UP,   SRC_SAME,  32, 16,  0,   32, 16,  0,   0, 0, 0)   /* conv3_up */ \
  X(3, 16, 16, 3, SRC_SAME, SRC_SAME, SRC_DOWN,  16, 16, 32,   16, 16, 32,   0, 0, 0)   /* conv4_down */
#define SEP_SHAPE_C 64
#define SEP_SHAPE_TS 8

struct SepShape { int h, w, nsrc, kind[HEP_MAX_SRC], sh[HEP_MAX_SRC], sw[HEP_MAX_SRC], pool_pad[HEP_MAX_SRC]; };
constexpr SepShape sep_shape(int d) {
  switch (d) {
#define X(id, h, w, ns, k0, k1, k2, sh0, sh1, sh2, sw0, sw1, sw2, p0, p1, p2) case id: return SepShape{h, w, ns, {k0, k1, k2}, {sh0, sh1, sh2}, {sw0, sw1, sw2}, {p0, p1, p2}};
    SEP_SHAPES(X)
#undef X
    default: return SepShape{};
  }
}

// the LDS layout of a launch (sep_lds_layout fills SepArgs with it; the shape rows fold it)
struct SepLds { size_t off_atile, off_wdw, off_bias, lds_bytes; };
constexpr SepLds sep_lds_of(int C, int bf16, int ts, int max_cols_f32, int max_cols_map) {
  const size_t es = bf16 ? 2 : 4, pad = bf16 ? 8 : 4;
  const size_t hs = ts + 2, px = (size_t)ts * ts;
  size_t region = hs * hs * (C + pad) * es;                                                       // halo ...
  if (px * (size_t)max_cols_f32 * 4 > region) region = px * (size_t)max_cols_f32 * 4;             // ... or the fp32 output tile
  if (px * (size_t)max_cols_map * es > region) region = px * (size_t)max_cols_map * es;           // ... or the dtype output tile
  region = (region + 15) & ~(size_t)15;
  SepLds l{};
  l.off_atile = region;
  l.off_wdw = l.off_atile + px * (C + pad) * es;
  l.off_bias = l.off_wdw + (size_t)9 * C * 4;
  l.lds_bytes = l.off_bias + (size_t)SEP_MAX_TILES_MAP * 16 * 4;
  return l;
}
constexpr SepLds SEP_SHAPE_LDS = sep_lds_of(SEP_SHAPE_C, 1, SEP_SHAPE_TS, 0, SEP_SHAPE_C);

// profiling build (make trace): per-wave s_memrealtime stamps at the phase boundaries of the single-node launches on maps of side
// g_sep_trace_hw, read back with hep_dbg_sep_trace() (tools/trace_sep.py); compiled out of the product library
#ifdef HEP_TOWER_TRACE
static __device__ unsigned long long* g_sep_trace = nullptr;      // one per translation unit: hep_dbg_sep_trace binds them all
static __device__ int g_sep_trace_hw = 0;
static inline void sep_trace_bind_tu(unsigned long long* p, int hw) {
  hipMemcpyToSymbol(HIP_SYMBOL(g_sep_trace), &p, sizeof p);
  hipMemcpyToSymbol(HIP_SYMBOL(g_sep_trace_hw), &hw, sizeof hw);
}
#define SSTAMP(i) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); sstamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define SSTAMP_NOWAIT(i) do { sstamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define SSTAMP(i)
#define SSTAMP_NOWAIT(i)
#endif

// Launch modes:
//   0  one segment, descriptor in the kernel arguments            (BiFPN node on a 16x16 / 32x32 level)
//   1  many independent segments, tile -> segment table            (a tower layer / the headers of all heads)
//   2  a CHAIN of dependent single-tile segments run back to back by one workgroup per image
//      (consecutive BiFPN nodes on levels <= 8x8: p5_out -> p6_out -> p7_out -> p6_up' -> p5_up'):
//      the dependency is carried by a workgroup barrier instead of 4 kernel boundaries
// Modes 0/2 (<= 256 workgroups, pure latency): 16 waves per workgroup.  Mode 1 (~2000 workgroups,
// throughput): 8 waves so two workgroups share a CU.
// fp32 sessions: 8 waves in every mode - with 16 the 128-register budget spilled (20-100 bytes of scratch per lane, and scratch memory
// that the runtime keeps per queue: 2 MB per session created and destroyed)
#define SEP_THREADS_OF(mode, bf16) ((mode) != 1 && (bf16) ? 1024 : 512)
#ifndef SEP_M1_WAVES
#define SEP_M1_WAVES 4
#endif

// fused value of 8 channels at (y, x): sum_i fw_i * gather_i, optional swish.  Every load of the
// item is issued before the first one is consumed (one memory round trip per item in bf16; the
// fp32 parity mode walks the max-pool window row by row to stay inside the register budget).
// All loads are UNCONDITIONAL on in-range addresses (a load under a branch costs its own round trip): SAME and UP
// sources differ by a shift, a DOWN source is also read at (y, x) (in range: it is the larger map) and ignored,
// window taps outside the map read a clamped address and are replaced by the zero padding.  Offsets inside an image
// are 32-bit; the per-image base is uniform.
// D > 0 (row D of SEP_SHAPES): number, kind and size of the sources are constants; the loads D = 0 issues for nothing - unused
// source slots, a pooled source at (y, x) - are left out.
template <bool BF16, int D = 0>
__device__ __forceinline__ void gather_fuse(const SepSeg& sg, int b, int y, int x, int c0, float v[8]) {
  constexpr SepShape SH = sep_shape(D);
  const int C = D ? SEP_SHAPE_C : sg.C, nsrc = D ? SH.nsrc : sg.nsrc;
  constexpr int ROWS = BF16 ? 3 : 1;        // window rows in flight at once
  typedef typename std::conditional<BF16, bf16_t, float>::type T;
  Raw8<BF16> same[HEP_MAX_SRC];
  Raw8<BF16> win[ROWS * 3];
  // (the descriptor's arrays are only ever indexed by unrolled constants: a run-time index would
  //  push the whole by-value struct out of scalar registers into scratch memory)
  int down = -1, dsh = 1, dsw = 1, dpad = 0; const T* dsrc = reinterpret_cast<const T*>(sg.src[0]);
#pragma unroll
  for (int i = 0; i < HEP_MAX_SRC; i++) {
    const bool used = i < nsrc;                                      // (uniform)
    if (D && !used) continue;
    const int sh = D ? SH.sh[i] : (used ? sg.sh[i] : sg.sh[0]), sw = D ? SH.sw[i] : (used ? sg.sw[i] : sg.sw[0]);
    const T* src = reinterpret_cast<const T*>(used ? sg.src[i] : sg.src[0]) + (int64_t)b * sh * sw * C;
    const int kind = D ? SH.kind[i] : (used ? sg.kind[i] : SRC_SAME), sft = kind == SRC_UP ? 1 : 0;
    if (!D || kind != SRC_DOWN) same[i].load(src, (uint32_t)(((y >> sft) * sw + (x >> sft)) * C + c0));
    if (used && kind == SRC_DOWN) { down = i; dsh = sh; dsw = sw; dpad = D ? SH.pool_pad[i] : sg.pool_pad[i]; dsrc = src; }   // (at most one per node)
  }
  float pooled[8];
  if (down >= 0) {                                                  // (uniform)
#pragma unroll
    for (int r0 = 0; r0 < 3; r0 += ROWS) {
      bool in[ROWS * 3];
#pragma unroll
      for (int q = 0; q < ROWS * 3; q++) {
        const int iy = 2 * y - dpad + r0 + q / 3, ix = 2 * x - dpad + q % 3;
        in[q] = iy >= 0 && iy < dsh && ix >= 0 && ix < dsw;
        win[q].load(dsrc, (uint32_t)((min(max(iy, 0), dsh - 1) * dsw + min(max(ix, 0), dsw - 1)) * C + c0));
      }
#pragma unroll
      for (int c = 0; c < 8; c++) {
        float m = in[0] ? win[0].get(c) : 0.f;
#pragma unroll
        for (int q = 1; q < ROWS * 3; q++) m = fmaxf(m, in[q] ? win[q].get(c) : 0.f);
        pooled[c] = r0 == 0 ? m : fmaxf(pooled[c], m);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 8; c++) v[c] = 0.f;
#pragma unroll
  for (int i = 0; i < HEP_MAX_SRC; i++) {
    if (i >= nsrc) break;
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] = fmaf(sg.fw[i], i == down ? pooled[c] : same[i].get(c), v[c]);
  }
  if (D ? 1 : sg.pre_act) {
    swish_n<BF16, 8>(v);
  }
}

// WL: the node's pointwise weights are staged in LDS (a.off_wpw; bf16 nodes wider than 64 channels, modes 0 / 2)
// W8: eight waves instead of sixteen for a single bf16 node of width <= 64 (round 6).  A 1024-thread workgroup at 112 VGPRs is alone on
// its CU and spends 2.9 of its 5.4 us waiting for the fused gather; two 512-thread workgroups - of this launch or of another stream's -
// share the CU.  Alone the launches get 0.3-1.0 us slower (6.1 / 6.8 / 7.4 -> 6.4 / 7.3 / 8.4 us), with four batches in flight
// 53.66k -> 55.60k frames/s (+3.6 %), one batch -0.8 %, bit-identical.  (Width 160 with staged weights: 5598 -> 5376 at phi 3: stays at sixteen.)
// D: the node descriptor (above); 0 = every shape from the arguments.  D > 0 is the W8 form of mode 0.
template <bool BF16, int MODE, bool WL = false, bool W8 = false>
__global__ __launch_bounds__(W8 ? 512 : SEP_THREADS_OF(MODE, BF16), MODE == 1 ? SEP_M1_WAVES : (BF16 ? 4 : 2)) void sep_kernel(SepArgs a) {
  constexpr int D = 0;      // the generic kernel: every shape from the arguments
#include "k_sep_body.h"
}
// row D of SEP_SHAPES: the node's shape folded in (the eight-wave single-node form)
template <bool BF16, int D>
__global__ __launch_bounds__(512, 4) void sep_shape_kernel(SepArgs a) {
  constexpr int MODE = 0; constexpr bool WL = false, W8 = true;
#include "k_sep_body.h"
}
