// k_xbf_impl.h - the MBConv block BOUNDARY kernel (see k_xbf.hip for what it computes) as a template, shared by the translation units
// that instantiate it: k_xbf.hip (xbf_kernel: every shape from XbfArgs, the widths K1C / NT2C optionally folded) and k_xbf_shape.hip
// (xbf_kernel_shape: the whole layer shape folded).  The kernel text itself is k_xbf_body.h, included by both __global__ templates.
#pragma once
#include <algorithm>
#include <type_traits>

#include "hep_dev.h"
#include "hep_internal.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;

constexpr int XT = 512, XW = XT / 64;      // threads, waves per workgroup
constexpr int XCH = 2;                      // LDS chunks of expanded channels (<=)

// Boundary shapes as compile-time constants (as MBF_SHAPES of k_mbf_impl.h and SEP_SHAPES of k_sep_impl.h).
// xbf_kernel folds the two widths (K1C, NT2C); map size, output size, pads, tile counts, the chunking, the LDS offsets, the
// squeeze-excite widths and the residual still arrive in XbfArgs, so no e_s address of P2 / P3 folds into an immediate offset (the
// pitch EP is chunk_tiles * 16 + PAD) and every instantiation carries a second channel chunk that the rows below never run.
// Descriptor D = 0 takes everything from XbfArgs - xbf_kernel, the path of every other width, map size, phi and dtype; D > 0 is row D
// of XBF_SHAPES and runs as xbf_kernel_shape<true, D>.  One row per boundary launch of the benchmarked session (phi 0 @ 256 in bf16:
// blocks 0|1, 1|2, 2|3; phi 1 @ 256 repeats them).  launch_xbf selects a row only when EVERY folded field of the launch equals it
// (xbf_shape_id), so a row that no longer matches the planner falls back to D = 0 instead of computing with stale constants.  Only
// where the numbers come from changes: arithmetic, tap and accumulation order, rounding points, LDS layout, reduction tree and
// launch bounds are those of D = 0.  What depends on the batch or on the session flags stays an argument: every pointer (mid: stored
// or not), B, tpw, se_rows, the workgroups per image and their reciprocal.
//   id  k  s toh tow NT1  K1 NT2    H    W   Ho   Wo  N1 pad_t pad_l  sq sqp sq2 sqp2 res
#define XBF_SHAPES(X) \
  X(1,  3, 2,  8,  8,  1,  32,  6,  128, 128,  64,  64, 16,   0,    0,   8,  8,  4,   8,  0)   /* b0.project+b1.front */ \
  X(2,  3, 1,  8, 16,  2,  96,  9,   64,  64,  64,  64, 24,   1,    1,   4,  8,  6,   8,  0)   /* b1.project+b2.front */ \
  X(3,  5, 2,  8,  8,  2, 144,  9,   64,  64,  32,  32, 24,   1,    1,   6,  8,  6,   8,  1)   /* b2.project+b3.front */

struct XbfShape { int k, s, toh, tow, NT1, K1, NT2, H, W, Ho, Wo, N1, pad_t, pad_l, sq, sqp, sq2, sqp2, res; };
constexpr XbfShape xbf_shape(int d) {
  switch (d) {
#define X(id, k, s, th, tw, n1, k1, n2, H, W, Ho, Wo, N1, pt, pl, sq, sqp, sq2, sqp2, res) case id: return XbfShape{k, s, th, tw, n1, k1, n2, H, W, Ho, Wo, N1, pt, pl, sq, sqp, sq2, sqp2, res};
    XBF_SHAPES(X)
#undef X
    default: return XbfShape{};
  }
}

// the LDS layout and the channel chunking of a launch (xbf_layout fills XbfArgs with it; the shape rows fold it): lds_bytes 0 = does not fit
struct XbfLds { int chunk_tiles, nchunks, off_w1, off_w2, off_f, off_misc, blob_bytes; size_t lds_bytes; };
constexpr size_t xbf_al16(size_t v) { return (v + 15) & ~(size_t)15; }
// union region: the input tile (P0/P1), then the expanded chunk (P2/P3), then the channel-sum staging (P4)
constexpr size_t xbf_union_of(size_t pin, int K1, int NT2, int nch, size_t es, size_t pad) {
  const int ct = (NT2 + nch - 1) / nch;
  const size_t a_bytes = pin * K1 * es, red_bytes = (size_t)XT * 9 * 4, e_bytes = xbf_al16(pin * ((size_t)ct * 16 + pad) * es);
  return xbf_al16(std::max(std::max(a_bytes, e_bytes), red_bytes));
}
constexpr XbfLds xbf_lds_of(int bf16, int k, int s, int toh, int tow, int K1, int NT1, int NT2, int Cexp) {
  const size_t es = bf16 ? 2 : 4, pad = bf16 ? 8 : 4;
  const size_t ph = (size_t)(toh - 1) * s + k, pw = (size_t)(tow - 1) * s + k, pin = ph * pw;
  const size_t w1_bytes = xbf_al16((size_t)NT1 * 16 * (K1 + pad) * es), w2_bytes = xbf_al16((size_t)NT2 * 16 * (NT1 * 16 + pad) * es);
  const size_t f_bytes = xbf_al16(((size_t)(k * k + 1) * Cexp + (size_t)NT2 * 16 + (size_t)NT1 * 16) * 4);
  const size_t misc = ((size_t)((K1 + 15) & ~15) + 16 + XW * 16 + Cexp) * 4;
  size_t best = 0; int best_nch = 0;
  for (int nch = 1; nch <= XCH; nch++) {
    const size_t total = xbf_union_of(pin, K1, NT2, nch, es, pad) + w1_bytes + w2_bytes + f_bytes + misc;
    if (total > 160 * 1024) continue;
    // the fewest chunks that let two workgroups share a CU; otherwise the fewest chunks that fit at all
    if (!best || (best > 80 * 1024 && total <= 80 * 1024)) { best = total; best_nch = nch; }
  }
  XbfLds l{};
  if (!best) return l;
  const int ct = (NT2 + best_nch - 1) / best_nch;
  l.chunk_tiles = ct; l.nchunks = (NT2 + ct - 1) / ct;
  l.off_w1 = (int)xbf_union_of(pin, K1, NT2, best_nch, es, pad); l.off_w2 = l.off_w1 + (int)w1_bytes;
  l.off_f = l.off_w2 + (int)w2_bytes; l.off_misc = l.off_f + (int)f_bytes;
  l.blob_bytes = l.off_misc - l.off_w1;
  l.lds_bytes = best;
  return l;
}
constexpr XbfLds xbf_shape_lds(int d) {
  const XbfShape sh = xbf_shape(d);
  return d ? xbf_lds_of(1, sh.k, sh.s, sh.toh, sh.tow, sh.K1, sh.NT1, sh.NT2, sh.NT2 * 16) : XbfLds{};
}

// Optional per-wave timeline (make trace: -DHEP_XBF_TRACE): s_memrealtime (100 MHz) stamps at the phase boundaries of
// the launches selected by HEP_XBF_TRACE_SEL="Cexp", read back with hep_dbg_xbf_trace() - profiling builds only.
#ifdef HEP_XBF_TRACE
static __device__ unsigned long long* g_xbf_trace = nullptr;      // one per translation unit: hep_dbg_xbf_trace binds them all
static inline void xbf_trace_bind_tu(unsigned long long* p) { hipMemcpyToSymbol(HIP_SYMBOL(g_xbf_trace), &p, sizeof p); }
#define XSTAMP(i) do { stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define XSTAMP(i)
#endif

// K1C / NT2C: the depthwise width of block i-1 and the expanded n-tiles of block i as compile-time constants (the BASELINE
// networks' boundaries: every index split, loop bound and LDS pitch folds), or 0 = taken from the arguments (any width).
template <bool BF16, int KS, int S, int TOH, int TOW, int NT1, int K1C, int NT2C>
__global__ __launch_bounds__(XT, KS == 3 ? 4 : 2) void xbf_kernel(XbfArgs a) {   // (3x3 layers: two workgroups per CU, at most 128 VGPRs)
  constexpr int D = 0;      // every shape from the arguments
#include "k_xbf_body.h"
}
// row D of XBF_SHAPES: the whole boundary folded in
template <bool BF16, int D>
__global__ __launch_bounds__(XT, xbf_shape(D).k == 3 ? 4 : 2) void xbf_kernel_shape(XbfArgs a) {
  constexpr int KS = xbf_shape(D).k, S = xbf_shape(D).s, TOH = xbf_shape(D).toh, TOW = xbf_shape(D).tow, NT1 = xbf_shape(D).NT1, K1C = xbf_shape(D).K1, NT2C = xbf_shape(D).NT2;
#include "k_xbf_body.h"
}
