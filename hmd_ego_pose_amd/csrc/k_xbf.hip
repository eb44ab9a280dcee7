// k_xbf.hip - one MBConv block BOUNDARY of the EfficientNet backbone on the big maps (128x128, 64x64) as ONE
// gfx950 kernel.  The reference runs, between the depthwise conv of block i-1 and the depthwise conv of block i
// (efficientnet/model.py:86-104 of block i-1, :76-89 of block i):
//
//   _se_reduce,_swish,_se_expand,sigmoid,*   (squeeze-excite of block i-1; its means arrive as partial reduce-FC rows)
//   _project_conv,_bn2 (+ inputs)            1x1, K1 -> N1
//   _expand_conv,_bn0,_swish                 1x1, N1 -> Cexp = 6 N1
//   _depthwise_conv,_bn1,_swish              k x k, stride s, TF-SAME
//   adaptive_avg_pool2d (spatial half)       squeeze-excite of block i
//
// As separate launches that is three kernels and ~10x the unavoidable HBM traffic on the early blocks: the project
// writes the block output, the expand reads it and writes the 6x expanded tensor, the depthwise reads that back.
// Here a workgroup owns one output tile of one image: it stages the (halo'd) tile of block i-1's depthwise output in
// LDS, finishes the squeeze-excite scale, runs both 1x1 convs on MFMA with the project result handed to the expand
// conv IN REGISTERS (the transposed product D[n, pixel] = W . A^T leaves a lane with 4 consecutive channels of one
// pixel, which is exactly the k-fragment of v_mfma_f32_16x16x16_bf16 / v_mfma_f32_16x16x4_f32), writes the activated
// expanded tile to LDS and takes the depthwise taps from there.  HBM sees the input tile once (plus halo) and the
// depthwise output once.  Stored only when somebody needs it: the block output (a later residual / BiFPN tap).
//
//   P0  blob of all weights (host-packed in LDS layout) + input tile -> LDS; squeeze-excite prologue -> scale[K1]
//   P1  project: A frags (LDS) * scale -> MFMA -> + bias (+ residual) -> rounded to the session dtype -> x frags (registers)
//   P2  expand (per chunk of expanded channels): x frags . W2 -> + bias, swish -> LDS (zero outside the image)
//   P3  depthwise taps from LDS -> + bias, swish -> global; per-lane channel sums
//   P4  channel sums (fixed order) -> partial reduce-FC products of block i -> hpart_out[b][tile][j]
//
// The kernel itself is k_xbf_impl.h / k_xbf_body.h.  This translation unit instantiates xbf_kernel (every shape from XbfArgs, the widths
// optionally folded) and holds the LDS layout and launch_xbf, which runs a boundary on its shape row (xbf_kernel_shape, instantiated
// in k_xbf_shape.hip) when one exists for exactly these arguments - xbf_shape_id - and on xbf_kernel otherwise.
#include <stdlib.h>

#include "k_xbf_impl.h"

// k_xbf_shape.hip
Pick xbf_shape_pick(int id, const XbfArgs&);
void xbf_shape_trace_bind(unsigned long long* p);

#ifdef HEP_XBF_TRACE
extern "C" int hep_dbg_xbf_trace(unsigned long long* host, int max_waves, int enable) {
  static unsigned long long* buf = nullptr;
  const size_t cap = (size_t)1 << 21;
  if (!buf) { if (hipMalloc((void**)&buf, cap * 8) != hipSuccess) return -1; hipMemset(buf, 0, cap * 8); }
  unsigned long long* p = enable ? buf : nullptr;
  xbf_trace_bind_tu(p); xbf_shape_trace_bind(p);
  if (host) { hipDeviceSynchronize(); hipMemcpy(host, buf, (size_t)max_waves * 96, hipMemcpyDeviceToHost); }
  return (int)(cap / 12);
}
#endif

// ---- host side ----
void xbf_tile(int k, int s, int* toh, int* tow) { (void)k; *toh = 8; *tow = s == 2 ? 8 : 16; }
int xbf_supports(int k, int s) { return (k == 3 || k == 5) && (s == 1 || s == 2); }

size_t xbf_layout(XbfArgs* a) {
  xbf_tile(a->k, a->s, &a->toh, &a->tow);
  const XbfLds l = xbf_lds_of(a->bf16, a->k, a->s, a->toh, a->tow, a->K1, a->NT1, a->NT2, a->Cexp);      // (k_xbf_impl.h: the rows fold the same formula)
  if (!l.lds_bytes) return 0;
  a->chunk_tiles = l.chunk_tiles; a->nchunks = l.nchunks;
  a->off_w1 = l.off_w1; a->off_w2 = l.off_w2; a->off_f = l.off_f; a->off_misc = l.off_misc;
  a->blob_bytes = l.blob_bytes;
  a->lds_bytes = l.lds_bytes;
  return l.lds_bytes;
}

// specialised boundaries: (k, s, NT1, K1, NT2) of phi 0 (blocks 0|1, 1|2, 2|3) and phi 3 (1|2 .. 7|8); anything else runs
// the generic instantiation (K1C = NT2C = 0)
#define XBF_SPECS(X) \
  X(3, 2, 8, 8, 1, 32, 6) X(3, 1, 8, 16, 2, 96, 9) X(5, 2, 8, 8, 2, 144, 9) \
  X(3, 2, 8, 8, 2, 24, 9) X(3, 1, 8, 16, 2, 144, 12) X(3, 1, 8, 16, 2, 192, 12) X(5, 2, 8, 8, 2, 192, 12) X(5, 1, 8, 16, 3, 288, 18) X(3, 2, 8, 8, 3, 288, 18)

#define XBF_PICK(...) HEP_PICK(XT, a.lds_bytes, 160 * 1024, xbf_kernel, BF16, __VA_ARGS__)
template <bool BF16, int KS, int S, int TOH, int TOW>
static Pick xbf_pick_n(const XbfArgs& a) {
  if (a.NT1 == 1) return XBF_PICK(KS, S, TOH, TOW, 1, 0, 0);
  if (a.NT1 == 2) return XBF_PICK(KS, S, TOH, TOW, 2, 0, 0);
  return XBF_PICK(KS, S, TOH, TOW, 3, 0, 0);
}
template <bool BF16>
static Pick xbf_pick_t(const XbfArgs& a) {
  const bool generic = a.generic == 1;           // A/B switch, parity test of the generic path (decided when the plan is built)
#define X(k_, s_, th, tw, n1, k1, n2) \
  if (!generic && a.k == k_ && a.s == s_ && a.NT1 == n1 && a.K1 == k1 && a.NT2 == n2) return XBF_PICK(k_, s_, th, tw, n1, k1, n2);
  XBF_SPECS(X)
#undef X
  if (a.k == 3 && a.s == 1) return xbf_pick_n<BF16, 3, 1, 8, 16>(a);
  if (a.k == 3 && a.s == 2) return xbf_pick_n<BF16, 3, 2, 8, 8>(a);
  if (a.k == 5 && a.s == 1) return xbf_pick_n<BF16, 5, 1, 8, 16>(a);
  return xbf_pick_n<BF16, 5, 2, 8, 8>(a);
}
#undef XBF_PICK
// the row of XBF_SHAPES (k_xbf_impl.h) whose kernel runs this launch: every field the kernel folds must equal the row; 0 = xbf_kernel
// (no such row, or the plan asked for it: HEP_XBF_GENERIC=1 the generic instantiation, =2 the width-specialised one).  Only fields the
// planner sets are compared (xbf_pick is asked before launch_xbf has filled the reciprocals, which follow from the compared ones).
int xbf_shape_id(const XbfArgs& a) {
  if (a.generic || !a.bf16) return 0;
#define X(id, k_, s_, th, tw, n1, k1, n2, H_, W_, Ho_, Wo_, N1_, pt, pl, sq_, sqp_, sq2_, sqp2_, res_) { \
    constexpr XbfLds L = xbf_shape_lds(id); \
    constexpr int tx = (Wo_ + tw - 1) / tw, ty = (Ho_ + th - 1) / th; \
    if (a.k == k_ && a.s == s_ && a.toh == th && a.tow == tw && a.NT1 == n1 && a.K1 == k1 && a.NT2 == n2 && a.Cexp == n2 * 16 && a.H == H_ && a.W == W_ && \
        a.Ho == Ho_ && a.Wo == Wo_ && a.N1 == N1_ && a.pad_t == pt && a.pad_l == pl && a.sq == sq_ && a.sqp == sqp_ && a.sq2 == sq2_ && a.sqp2 == sqp2_ && \
        (a.has_res != 0) == (res_ != 0) && a.inv_hw == 1.0f / (float)(H_ * W_) && a.tiles_x == tx && a.tiles == tx * ty && \
        a.chunk_tiles == L.chunk_tiles && a.nchunks == L.nchunks && a.off_w1 == L.off_w1 && a.off_w2 == L.off_w2 && a.off_f == L.off_f && \
        a.off_misc == L.off_misc && a.blob_bytes == L.blob_bytes && a.lds_bytes == L.lds_bytes) return id; }
  XBF_SHAPES(X)
#undef X
  return 0;
}
// the instantiation a launch runs (hep_pick.h): its shape row, else the width-specialised xbf_kernel, else the generic one
Pick xbf_pick(const XbfArgs& a) {
  if (const int id = xbf_shape_id(a)) return xbf_shape_pick(id, a);
  return a.bf16 ? xbf_pick_t<true>(a) : xbf_pick_t<false>(a);
}
void launch_xbf(const XbfArgs& a_, hipStream_t s) {
  XbfArgs a = a_;
#ifdef HEP_XBF_TRACE
  { static const char* sel = getenv("HEP_XBF_TRACE_SEL"); a.trace = !sel || a.Cexp == atoi(sel); }
#endif
  const int wgs = (a.tiles + a.tpw - 1) / a.tpw;                        // workgroups per image
  a.tiles_rcp = rcp_u32((uint32_t)wgs); a.tiles_x_rcp = rcp_u32((uint32_t)a.tiles_x);
  {
    const int es = a.bf16 ? 2 : 4, pw = (a.tow - 1) * a.s + a.k, rv = (pw * a.K1 * es) >> 4;
    a.sw_rcp = rcp_u32((uint32_t)((rv + 63) >> 6));
  }
  dim3 grid(wgs, a.B);
  xbf_pick(a).launch(grid, s, a);
}
