// k_mbf.hip - the front half of an MBConv block as ONE gfx950 kernel:
//
//   expand 1x1 (+BN0, swish)  ->  depthwise k x k stride s, TF-SAME (+BN1, swish)  ->  SE partial sums
//
// replaces `_expand_conv,_bn0,_swish,_depthwise_conv,_bn1,_swish` and the spatial half of
// `adaptive_avg_pool2d` (reference efficientnet/model.py:76-89).  The 6x expanded tensor - the
// largest activation of every block - never exists in HBM: it is produced by MFMA straight into
// LDS for one (8x8 output tile + halo) x (chunk of CC expanded channels) and consumed from LDS by
// the depthwise taps ("depthwise staged in LDS").  Every input element is fetched from global
// memory once per channel chunk, with 16-byte loads of contiguous channel runs.
//
//   phase A  input tile (with halo, zero outside the image) -> LDS [PIN pixels][K]
//   phase B  expand: D[n, pixel] = We[n,:] . tile[pixel,:] (the transposed MFMA product of
//            k_pw.hip; weight fragments run 4 deep ahead in a register ring) -> +bias, swish ->
//            LDS [PIN][CC]; only the tile pixels inside the image are expanded, the others are the
//            depthwise conv's padding of the *activated* map (reference utils_extra.py:33-44): zeros
//   phase C  depthwise taps from LDS (weights in LDS) -> +bias, swish -> global, 16 bytes per lane;
//            per-lane channel sums for squeeze-excite
//   phase D  channel sums of the tile (fixed order) -> their partial products with the squeeze-excite
//            reduce weights -> hpart[b][workgroup][j]   (no atomics; the project GEMM finishes the SE)
// Blocks without an expand conv (first block of the net) skip phase B: the input tile IS the
// depthwise input.
//
// The kernel text is k_mbf_impl.h.  This file holds the generic kernels (mbf_kernel: every shape arrives in MbfArgs), the LDS
// layout, and launch_mbf, which runs a launch on its shape-specialised form (mbf_shape_kernel, instantiated in k_mbf_s16.hip /
// k_mbf_s8.hip) when one exists for exactly these arguments - mbf_shape_id - and on the generic kernel otherwise.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include <type_traits>

#include "k_mbf_impl.h"

// k_mbf_s16.hip, k_mbf_s8.hip
Pick mbf_shape_pick_16(int id, const MbfArgs&); Pick mbf_shape_pick_8(int id, const MbfArgs&);
void mbf_trace_bind_16(unsigned long long*); void mbf_trace_bind_8(unsigned long long*);

#ifdef HEP_MBF_TRACE
extern "C" int hep_dbg_mbf_trace(unsigned long long* host, int max_waves, int enable) {
  static unsigned long long* buf = nullptr;
  const size_t cap = (size_t)1 << 21;
  if (!buf) { if (hipMalloc((void**)&buf, cap * 8) != hipSuccess) return -1; hipMemset(buf, 0, cap * 8); }
  unsigned long long* p = enable ? buf : nullptr;
  mbf_trace_bind_tu(p); mbf_trace_bind_16(p); mbf_trace_bind_8(p);
  if (host) { hipDeviceSynchronize(); hipMemcpy(host, buf, (size_t)max_waves * 64, hipMemcpyDeviceToHost); }
  return (int)(cap / 8);
}
#endif

// rows of the compact input tile: the most in-image pixels any ts x ts-output tile of an H x W map covers
int mbf_max_inside(int H, int W, int k, int s, int pad_t, int pad_l, int ts) {
  const int pw = (ts - 1) * s + k;
  auto span = [&](int n, int pad) {
    const int no = (n + s - 1) / s;                        // output size along this axis (SAME)
    int best = 0;
    for (int t0 = 0; t0 < no; t0 += ts) {
      const int i0 = t0 * s - pad, lo = std::max(0, -i0), hi = std::min(pw, n - i0);
      best = std::max(best, hi - lo);
    }
    return best;
  };
  return span(H, pad_t) * span(W, pad_l);
}

int mbf_threads(int ts) { return ts == 16 ? 1024 : 512; }

// kp: input channels per pass of the multi-pass expand (0 or >= Cin: one pass, the whole K in LDS)
size_t mbf_lds_layout(int Cin, int CC, int k, int s, int bf16, int has_expand, int max_inside, int ts, MbfArgs* a, int kp) {
  const size_t es = bf16 ? 2 : 4, pad = bf16 ? 8 : 4;
  const size_t pw = (size_t)(ts - 1) * s + k, pin = pw * pw;
  const size_t arows = (((size_t)std::min<int>(max_inside, (int)pin) + 31) / 32) * 32;   // phase B reads whole pairs of 16-row m-tiles
  const bool mp = has_expand && kp > 0 && kp < Cin;
  const size_t kcols = mp ? (size_t)kp : (size_t)Cin;
  size_t in_bytes = has_expand ? arows * (kcols + pad) * es : 0;
  // the tap-row hand-over of phase C lives there too (8x8 tiles: two halves of the workgroup; the multi-pass 16x16 form has none)
  in_bytes = std::max(in_bytes, mp && ts == 16 ? (size_t)0 : (size_t)mbf_threads(ts) * 9 * 4);
  in_bytes = (in_bytes + 15) & ~(size_t)15;
  const size_t e_bytes = (std::max(pin * (CC + pad) * es, (size_t)16 * CC * 4) + 15) & ~(size_t)15;   // (phase D: [<= 16][CC] channel sums)
  const size_t w_bytes = (size_t)(k * k + 2) * CC * 4;                    // depthwise weights + the two bias vectors
  const size_t we_bytes = has_expand ? (((size_t)CC * (kcols + pad) * es + 15) & ~(size_t)15) : 0;   // expand-weight chunk (one K slice of it)
  if (a) { a->off_e = in_bytes; a->off_we = in_bytes + e_bytes; a->off_w = a->off_we + we_bytes; a->lds_bytes = a->off_w + w_bytes; }
  return in_bytes + e_bytes + we_bytes + w_bytes;
}

// does a multi-pass plan fit the kernel's compile-time budgets (row batches per lane and pass, k-steps per pass, m-tiles per wave)?
int mbf_mp_fits(int CC, int kp, int bf16, int max_inside, int ts) {
  const int threads = mbf_threads(ts), waves = threads / 64, kstep = bf16 ? 32 : 16;
  if (kp <= 0 || kp % kstep != 0 || kp / kstep > 3) return 0;
  int vp = 1; while (vp < kp / 8) vp <<= 1;
  const int prs = threads / vp, niw = ts == 16 ? 1 : 2, nip = ts == 16 ? 2 : 3;
  const int ntiles = (CC + 15) / 16; int np2 = 1; while (np2 < ntiles) np2 <<= 1;
  if (np2 > waves) return 0;
  const int ngrp = waves / np2, mtiles = (max_inside + 15) / 16, maxmt = ts == 16 ? 7 : 5;
  return ntiles * 16 <= niw * prs && max_inside <= nip * prs && (mtiles + ngrp - 1) / ngrp <= maxmt;
}
// ... and can the whole tile (weight rows + inside pixels, K / 8 vectors each) be held in six vectors per lane (MP = 2)?
int mbf_mp_resident(int Cin, int CC, int max_inside, int ts) {
  const long items = (long)(((CC + 15) / 16) * 16 + max_inside) * (Cin / 8);
  return Cin % 8 == 0 && items <= 6L * mbf_threads(ts);
}

static int mbf_mp(const MbfArgs& a) { return a.has_expand && a.npass > 1 ? (a.mp_resident ? 2 : 1) : 0; }      // template parameter MP: 1 / 2 = multi-pass expand

// the row of MBF_SHAPES (k_mbf_impl.h) whose kernel runs this launch: every field the kernel folds must equal the row; 0 = the
// generic kernel (no such row, or the plan asked for it: HEP_MBF_GENERIC)
int mbf_shape_id(const MbfArgs& a) {
  if (a.generic || a.fp8 || a.se_tail) return 0;
  const int mp = mbf_mp(a);
#define X(id, bf, ks, s_, ts_, mp_, cin, cexp, cc, h, w, ho, wo, pt, pl, sq_, sqp_, he, of) \
  if ((a.bf16 != 0) == bf && a.k == ks && a.s == s_ && a.ts == ts_ && mp == mp_ && a.Cin == cin && a.Cexp == cexp && a.CC == cc && a.H == h && a.W == w && \
      a.Ho == ho && a.Wo == wo && a.pad_t == pt && a.pad_l == pl && a.sq == sq_ && a.sqp == sqp_ && (a.has_expand != 0) == (he != 0) && (a.out_frag != 0) == (of != 0)) return id;
  MBF_SHAPES(X)
#undef X
  return 0;
}

#define MBF_PICK(ks, s_, ts_) HEP_PICK(ts_ == 16 ? 1024 : 512, a.lds_bytes, 159 * 1024, mbf_kernel, BF16, ks, s_, ts_, F8, MP)
template <bool BF16, bool F8, int MP>
static Pick mbf_pick_t(const MbfArgs& a) {
  if (a.ts == 16) return a.k == 3 ? MBF_PICK(3, 1, 16) : MBF_PICK(5, 1, 16);       // stride 1 only (the planner never asks for 16x16 tiles on a stride-2 layer)
  if (a.k == 3 && a.s == 1) return MBF_PICK(3, 1, 8);
  if (a.k == 3 && a.s == 2) return MBF_PICK(3, 2, 8);
  if (a.k == 5 && a.s == 1) return MBF_PICK(5, 1, 8);
  return MBF_PICK(5, 2, 8);
}
#undef MBF_PICK
// the instantiation a launch runs (hep_pick.h): the fp8 fronts are single-pass, a launch whose every folded field equals a row of
// MBF_SHAPES runs that row, everything else the generic kernel of its tap size, stride, tile and expand form
Pick mbf_pick(const MbfArgs& a) {
#ifdef HEP_WITH_FP8
  if (a.bf16 && a.fp8) return mbf_pick_t<true, true, 0>(a);
#endif
  if (const int id = mbf_shape_id(a)) { const Pick p = mbf_shape_pick_16(id, a); return p.fn ? p : mbf_shape_pick_8(id, a); }
  const int mp = mbf_mp(a);
  if (a.bf16) return mp == 2 ? mbf_pick_t<true, false, 2>(a) : (mp == 1 ? mbf_pick_t<true, false, 1>(a) : mbf_pick_t<true, false, 0>(a));
  return mp == 2 ? mbf_pick_t<false, false, 2>(a) : (mp == 1 ? mbf_pick_t<false, false, 1>(a) : mbf_pick_t<false, false, 0>(a));
}
void launch_mbf(const MbfArgs& a_, hipStream_t s) {
  MbfArgs a = a_;
#ifdef HEP_MBF_TRACE
  {   // profiling build: HEP_MBF_TRACE_SEL="Cexp,H" keeps the stamps of that layer only (default: every launch, last wins)
    static const char* sel = getenv("HEP_MBF_TRACE_SEL");
    int c = 0, h = 0;
    if (sel) sscanf(sel, "%d,%d", &c, &h);
    a.trace = !sel || (a.Cexp == c && a.H == h);
  }
#endif
  const int tiles = ((a.Wo + a.ts - 1) / a.ts) * ((a.Ho + a.ts - 1) / a.ts), chunks = (a.Cexp + a.CC - 1) / a.CC;
  dim3 grid(tiles * chunks, a.B);
  a.chunks = chunks; a.tiles_x = (a.Wo + a.ts - 1) / a.ts;
  a.chunks_rcp = rcp_u32(chunks); a.tiles_x_rcp = rcp_u32(a.tiles_x); a.gx_rcp = rcp_u32(grid.x);
  a.vk_rcp = rcp_u32((uint32_t)std::max(1, a.Cin >> 3)); a.kpv_rcp = rcp_u32((uint32_t)std::max(1, a.kp >> 3));      // (read by the resident multi-pass form only)
  mbf_pick(a).launch(grid, s, a);
}
