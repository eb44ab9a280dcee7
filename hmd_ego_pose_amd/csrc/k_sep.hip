// k_sep.hip - fused SeparableConvBlock of the BiFPN nodes on gfx950 (and, with HEP_TOWER=0, of the head
// layers - by default those run on k_tower.hip):
//
//   [ weighted fusion of 2-3 maps (nearest x2 up / zero-padded 3x3/2 max-pool gathers) + swish ]
//     -> depthwise 3x3 SAME (no bias) -> pointwise 1x1 (+bias, BN folded) -> [swish | sigmoid]
//
// replaces, per BiFPN node, `swish(w0*a + w1*up(b) [+ w2*pool(c)])` + `SeparableConvBlock`
// (reference efficientdet/model.py:212-264, 42-52) and, per head layer,
// `conv(feat); bn(feat); swish(feat)` / the header conv + permute/view/cat
// (efficientdet/model.py:361-417; hmdegopose/model.py:55-90,127-156,191-228).
//
// One workgroup = one 8x8 output tile (4x4 where the fp32 tile of a wide layer would not fit in LDS) of one image of one "segment" (a node, or one (head, level,
// column-chunk) triple).  These maps are tiny (32x32 .. 2x2 per image), so the kernel is latency-bound:
// the design goal is the shortest dependent chain per workgroup and full-line stores.
//   phase 0  depthwise weights + bias -> LDS
//   phase 1  fused (+swish) 10x10 halo of the depthwise input -> LDS (dtype), zero outside the
//            map; all gather loads of an item are issued before the first is consumed
//   phase 2  depthwise 3x3 from LDS -> MFMA operand tile [64 pixels][C] in LDS
//   phase 3  1x1 conv as the transposed MFMA product of k_pw.hip (W fragment = A operand,
//            pixels = B operand); (m-tile, n-tile) pairs are dealt round-robin to the waves;
//            results go to an LDS output tile (over the dead halo)
//   phase 4  the output tile leaves as full coalesced rows.  Head outputs land directly at their
//            anchor offset in the [B, N_anchors, K] result (no permute / cat pass).
// All index arithmetic is shifts, masks and compile-time divisors (see the note in the kernel).
//
// The kernel itself is k_sep_impl.h.  This translation unit instantiates the generic kernels (sep_kernel: every shape from SepArgs)
// and holds the LDS layout and launch_sep, which runs a single node on its shape-specialised form (sep_shape_kernel, instantiated in
// k_sep_shape.hip) when one exists for exactly these arguments - sep_shape_id - and on the generic kernel otherwise.
#include <stdlib.h>

#include "k_sep_impl.h"

// k_sep_shape.hip
Pick sep_shape_pick(int id, const SepArgs&);
void sep_shape_trace_bind(unsigned long long* p, int hw);

#ifdef HEP_TOWER_TRACE
// profiling build: stamps of the LAST single-node launch on a map of side `hw`, [workgroups * waves][8]; hw = 0 turns the stamps off
extern "C" int hep_dbg_sep_trace(unsigned long long* host, int max_waves, int hw) {
  static unsigned long long* buf = nullptr;
  const size_t cap = (size_t)1 << 20;
  if (!buf) { if (hipMalloc((void**)&buf, cap * 8) != hipSuccess) return -1; }
  if (!host) hipMemset(buf, 0, cap * 8);
  unsigned long long* p = hw ? buf : nullptr;
  sep_trace_bind_tu(p, hw); sep_shape_trace_bind(p, hw);
  if (host) { hipDeviceSynchronize(); hipMemcpy(host, buf, (size_t)max_waves * 64, hipMemcpyDeviceToHost); }
  return (int)(cap / 8);
}
#endif

void sep_lds_layout(int C, int bf16, int ts, int max_cols_f32, int max_cols_map, SepArgs* a, int stage_w) {
  const size_t es = bf16 ? 2 : 4, pad = bf16 ? 8 : 4;
  const SepLds l = sep_lds_of(C, bf16, ts, max_cols_f32, max_cols_map);      // halo | fp32 / dtype output tile, operand tile, depthwise weights, bias
  a->off_atile = l.off_atile; a->off_wdw = l.off_wdw; a->off_bias = l.off_bias; a->lds_bytes = l.lds_bytes;
  // BiFPN nodes wider than 64 channels (bf16, 8x8 tiles): the pointwise weights [C][C + pad] next to the tiles when they fit -
  // requested behind the gather barrier, parked before the MFMA phase.  (At width 64 every wave's only (m-tile, n-tile)
  // pair has its fragments prefetched at kernel start; at width 160 a wave runs 2.5 pairs, each one a round trip to L2
  // that nothing overlapped: 15-28 us per node at phi 3 @ 512 for 1.5-24 MB.)
  a->off_wpw = 0;
  const size_t wrows = (size_t)((C + 15) / 16) * 16, wbytes = wrows * (C + pad) * es;      // whole n-tiles: widths like 88 end in a half-used one
  if (stage_w && bf16 && C > 64 && (ts == 8 || ts == 4) && wrows * (C / 8) <= 4 * 1024 && a->lds_bytes + wbytes <= 159 * 1024) { a->off_wpw = (a->lds_bytes + 15) & ~(size_t)15; a->lds_bytes = a->off_wpw + wbytes; }
}

// single bf16 node of width <= 64 without staged weights: the eight-wave instantiation (sep_pick; the shape rows are all of this kind)
static int sep_w8(const SepArgs& a) { return a.bf16 && !a.chain && a.nseg == 1 && !a.off_wpw && a.C <= 64; }

// the row of SEP_SHAPES (k_sep_impl.h) whose kernel runs this launch: every field the kernel folds must equal the row; 0 = the
// generic kernel (no such row, or the plan asked for it: HEP_NECK_GENERIC)
int sep_shape_id(const SepArgs& a) {
  if (a.generic || a.direct || !sep_w8(a)) return 0;
  const SepSeg& g = a.seg0;
  constexpr SepLds L = SEP_SHAPE_LDS;
  constexpr int C = SEP_SHAPE_C, TS = SEP_SHAPE_TS;
  if (a.C != C || g.C != C || g.N != C || g.tilesN != C / 16 || g.ts != TS || g.pre_act != 1 || g.act != ACT_NONE || g.out_f32 || g.out_off != 0 ||
      g.out_rowstride != C || g.tile_begin != 0 || a.off_atile != L.off_atile || a.off_wdw != L.off_wdw || a.off_bias != L.off_bias || a.lds_bytes != L.lds_bytes) return 0;
#define X(id, h_, w_, ns, k0, k1, k2, sh0, sh1, sh2, sw0, sw1, sw2, p0, p1, p2) { \
    const int kind[HEP_MAX_SRC] = {k0, k1, k2}, sh[HEP_MAX_SRC] = {sh0, sh1, sh2}, sw[HEP_MAX_SRC] = {sw0, sw1, sw2}, pp[HEP_MAX_SRC] = {p0, p1, p2}; \
    bool same = g.h == h_ && g.w == w_ && g.nsrc == ns && g.tiles_x == w_ / TS && g.tiles_y == h_ / TS && g.tiles_x_rcp == rcp_u32(w_ / TS) && \
                a.total_tiles == (w_ / TS) * (h_ / TS) && g.out_bstride == (int64_t)h_ * w_ * C; \
    for (int i = 0; i < ns; i++) same = same && g.kind[i] == kind[i] && g.sh[i] == sh[i] && g.sw[i] == sw[i] && g.pool_pad[i] == pp[i]; \
    if (same) return id; }
  SEP_SHAPES(X)
#undef X
  return 0;
}

static int sep_mode(const SepArgs& a) { return a.chain ? 2 : (a.nseg == 1 ? 0 : 1); }      // 0 one node, 1 independent segments, 2 a chain

// the instantiation a launch runs (hep_pick.h): a single node on its shape row when it has one, else a generic sep_kernel
Pick sep_pick(const SepArgs& a) {
  const int mode = sep_mode(a);
  const unsigned block = SEP_THREADS_OF(mode, a.bf16);
  if (mode == 0)
    if (const int id = sep_shape_id(a)) return sep_shape_pick(id, a);
#define SEP_PICK(blk, ...) HEP_PICK(blk, a.lds_bytes, 159 * 1024, sep_kernel, __VA_ARGS__)
  if (a.bf16) {
    // (staged weights: every segment of the launch is a map-to-map node of the full width - the planner only sets off_wpw then)
    if (mode == 0 && a.off_wpw) return SEP_PICK(block, true, 0, true, false);
    if (mode == 2 && a.off_wpw) return SEP_PICK(block, true, 2, true, false);
    if (mode == 0 && sep_w8(a)) return SEP_PICK(512, true, 0, false, true);
    if (mode == 0) return SEP_PICK(block, true, 0, false, false);
    if (mode == 1) return SEP_PICK(block, true, 1, false, false);
    return SEP_PICK(block, true, 2, false, false);
  }
  if (mode == 0) return SEP_PICK(block, false, 0, false, false);
  if (mode == 1) return SEP_PICK(block, false, 1, false, false);
  return SEP_PICK(block, false, 2, false, false);
#undef SEP_PICK
}

void launch_sep(const SepArgs& a, hipStream_t s) {
  dim3 grid(sep_mode(a) == 2 ? 1 : a.total_tiles, a.B);
  sep_pick(a).launch(grid, s, a);
}
