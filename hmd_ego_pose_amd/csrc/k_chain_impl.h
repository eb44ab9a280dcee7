// k_chain_impl.h - the LDS-resident BiFPN chain kernel (see k_chain.hip for what it computes) as a template, shared by the translation
// units that instantiate it: k_chain.hip (the generic kernels, every shape) and k_chain_shape.hip (the shape-specialised chains).
#pragma once
#include <type_traits>

#include "hep_dev.h"
#include "hep_internal.h"

// Chain shapes as compile-time constants (as MBF_SHAPES of k_mbf_impl.h).  A chain spends 3.96 of its 15.7 us in
// the prologue: the eight-entry external-map table is walked with the copy path AND the nine-tap pool path for every slot, every
// bound and offset a scalar load.  Descriptor D = 0 takes everything from ChainArgs - chain_kernel, the path of every other width,
// map size, phi and dtype; D > 0 is row D of chain_shape() and runs as chain_shape_kernel<true, D>.  One row per chain of the
// benchmarked session (phi 0 @ 256 in bf16) as Planner::add_chain builds them:
//   1  cell 0's first chain: p6_in = pool(p6_pre) while it is loaded (also stored), p7_in = pool(p6_in), conv6_up, conv5_up
//   2  the five-node chain between two cells (conv5_down, conv6_down, conv7_down, the next cell's conv6_up, conv5_up)
//   3  the three-node chain behind the last cell (conv5_down, conv6_down, conv7_down)
// What folds: the width (channel groups, pitches, thread split, k-steps), the whole external-map table (count, sizes, kind, pool pad,
// LDS slot, whether the pooled map is also stored), node counts, bytes of a node's weights and the four LDS offsets.  What stays: the
// per-node loop is a rolled loop over the ChainNode table (unrolled it is fetched cold: +20 %), the scalar-cache warm-up of the
// descriptor lines and kernarg_warm.  launch_chain selects a row only when EVERY folded field of the launch equals it
// (chain_shape_id), so a row that no longer matches the planner falls back to D = 0 instead of computing with stale constants.
#define CHAIN_SHAPE_C 64
#define CHAIN_SHAPE_ROWS 3
#define CHAIN_SHAPE_WNODE_BYTES 12288        // 10 * C floats + C rows of C + 8 bf16, in whole KB (Planner::add_chain)
struct ChainExtShape { int sh, sw, kind, h, w, pool_pad, off, store; };
struct ChainShape { int next, nnodes, nconv; size_t off_w, off_halo, off_atile, lds_bytes; ChainExtShape ext[CH_MAX_EXT]; };
constexpr ChainShape chain_shape(int d) {
  switch (d) {
    //                 next nodes conv  off_w  off_halo off_atile lds_bytes    sh  sw  kind      h  w pad   off store
    case 1: return ChainShape{2, 3, 2, 10752,  35328,  49728,  58944, {{ 8,  8, SRC_DOWN, 4, 4, 0,     0, 1},      // p6_pre -> p6_in
                                                                          { 8,  8, SRC_SAME, 8, 8, 0,  1024, 0}}};    // p5_in
    case 2: return ChainShape{6, 5, 5, 29184,  90624, 105024, 114240, {{ 8,  8, SRC_SAME, 8, 8, 0,     0, 0},      // p5_in2 / the last cell's p5_out
                                                                          { 8,  8, SRC_SAME, 8, 8, 0,  4096, 0},      // p5_up
                                                                          {16, 16, SRC_DOWN, 8, 8, 0,  8192, 0},      // p4_out, pooled
                                                                          { 4,  4, SRC_SAME, 4, 4, 0, 12288, 0},      // p6_in / p6_out
                                                                          { 4,  4, SRC_SAME, 4, 4, 0, 13312, 0},      // p6_up
                                                                          { 2,  2, SRC_SAME, 2, 2, 0, 14336, 0}}};    // p7_in / p7_out
    case 3: return ChainShape{6, 3, 3, 29184,  66048,  80448,  89664, {{ 8,  8, SRC_SAME, 8, 8, 0,     0, 0},
                                                                          { 8,  8, SRC_SAME, 8, 8, 0,  4096, 0},
                                                                          {16, 16, SRC_DOWN, 8, 8, 0,  8192, 0},
                                                                          { 4,  4, SRC_SAME, 4, 4, 0, 12288, 0},
                                                                          { 4,  4, SRC_SAME, 4, 4, 0, 13312, 0},
                                                                          { 2,  2, SRC_SAME, 2, 2, 0, 14336, 0}}};
    default: return ChainShape{};
  }
}

#ifndef CHAIN_THREADS
#define CHAIN_THREADS 1024
#endif
#define CHAIN_WAVES (CHAIN_THREADS / 64)

// profiling build (make trace): wave 0 of every workgroup stamps s_memrealtime (100 MHz) at the phase boundaries
#ifdef HEP_MBF_TRACE
static __device__ unsigned long long* g_chain_trace = nullptr;      // one per translation unit: hep_dbg_chain_trace binds them all
static inline void chain_trace_bind_tu(unsigned long long* p) { hipMemcpyToSymbol(HIP_SYMBOL(g_chain_trace), &p, sizeof p); }
#define CSTAMP() do { if (g_chain_trace && lane == 0 && nst < 60) st_buf[nst++] = __builtin_amdgcn_s_memrealtime(); } while (0)   // (every wave stamps)
#else
#define CSTAMP()
#endif

namespace {

// 8 channels of a map slot at pixel (y, x) as floats; zero outside the map (SAME padding of the pool / the depthwise halo).
// The load is unconditional (clamped address) and the zero is a select: conditional loads would each sit in a basic
// block of their own and serialise into one memory round trip per tap.
template <bool BF16, typename T> __device__ __forceinline__ Raw8<BF16> slot_raw(const T* slot, int h, int w, int C, int y, int x, int c0) {
  const bool ok = y >= 0 && y < h && x >= 0 && x < w;
  const int yc = min(max(y, 0), h - 1), xc = min(max(x, 0), w - 1);
  Raw8<BF16> r = Raw8<BF16>::load(slot + (int64_t)(yc * w + xc) * C + c0);
  if (!ok) r.zero();
  return r;
}
template <bool BF16, typename T> __device__ __forceinline__ void slot_load(const T* slot, int h, int w, int C, int y, int x, int c0, float v[8]) {
  slot_raw<BF16>(slot, h, w, C, y, x, c0).unpack(v);
}

// zero-padded 3x3 stride-2 max-pool of a slot at output pixel (y, x) (utils_extra.py:72-86: the pad value takes part);
// all nine loads are in flight before the first is consumed
// (fp32: two passes of four channels - nine 32-byte vectors in flight per lane spilled)
__device__ __forceinline__ void slot_pool4(const float* slot, int h, int w, int C, int pad, int y, int x, int c0, float* m) {
  f32x4 raw[9];
#pragma unroll
  for (int q = 0; q < 9; q++) {
    const int yy = 2 * y - pad + q / 3, xx = 2 * x - pad + q % 3;
    const bool ok = yy >= 0 && yy < h && xx >= 0 && xx < w;
    raw[q] = *reinterpret_cast<const f32x4*>(slot + (int64_t)(min(max(yy, 0), h - 1) * w + min(max(xx, 0), w - 1)) * C + c0);
    if (!ok) raw[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int q = 0; q < 9; q++)
#pragma unroll
    for (int c = 0; c < 4; c++) m[c] = q == 0 ? raw[q][c] : fmaxf(m[c], raw[q][c]);
}
template <bool BF16, typename T> __device__ __forceinline__ void slot_pool(const T* slot, int h, int w, int C, int pad, int y, int x, int c0, float m[8]) {
  if constexpr (!BF16) { slot_pool4(slot, h, w, C, pad, y, x, c0, m); slot_pool4(slot, h, w, C, pad, y, x, c0 + 4, m + 4); return; }
  Raw8<BF16> raw[9];
#pragma unroll
  for (int q = 0; q < 9; q++) raw[q] = slot_raw<BF16>(slot, h, w, C, 2 * y - pad + q / 3, 2 * x - pad + q % 3, c0);
#pragma unroll
  for (int q = 0; q < 9; q++) {
    float v[8];
    raw[q].unpack(v);
#pragma unroll
    for (int c = 0; c < 8; c++) m[c] = q == 0 ? v[c] : fmaxf(m[c], v[c]);
  }
}

}  // namespace

// WMODE: where a node's weights live.  0: all nodes' weights resident in LDS (bf16, width 64); 1: two nodes' weights in LDS, the next
// node's streamed in by LDS-DMA under the running node (fp32, width 64); 2: only the depthwise weights and biases in LDS, the pointwise
// weight fragments of an (m-tile, n-tile) pair requested together straight from global memory (L2) in front of its MFMAs (width 160:
// one node's pointwise weights are 60 KB and do not fit next to three 8x8x160 maps).
// D: the chain descriptor (above); 0 = every shape from the arguments.  D > 0 is the resident-weights form (WMODE 0) in bf16.
// the generic kernel: every shape from the arguments
template <bool BF16, int WMODE>
__global__ __launch_bounds__(CHAIN_THREADS) void chain_kernel(ChainArgs a) {
  constexpr int D = 0;
#include "k_chain_body.h"
}
// row D of chain_shape(): the chain's shape folded in
template <bool BF16, int D>
__global__ __launch_bounds__(CHAIN_THREADS) void chain_shape_kernel(ChainArgs a) {
  constexpr int WMODE = 0;
#include "k_chain_body.h"
}
