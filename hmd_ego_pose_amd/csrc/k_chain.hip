// k_chain.hip - the small pyramid levels of a BiFPN cell boundary as ONE LDS-resident chain per image (bf16 and fp32 sessions).
//
// Between two visits of the 16x16 / 32x32 levels a BiFPN walks up to five nodes on maps of 8x8, 4x4 and 2x2 pixels
// (reference efficientdet/model.py:212-264: p5_out -> p6_out -> p7_out -> next cell's p6_up -> p5_up; in cell 0
// also the two zero-padded max-pools that make p6_in / p7_in, model.py:198-203).  Each node is
//   swish(sum_i w_i * gather_i)  ->  depthwise 3x3 SAME  ->  pointwise 1x1 (+bias, BN folded)
// on at most 64 pixels x 64 channels: microseconds of arithmetic.  As a chain inside k_sep.hip (mode 2) every node
// still paid three to four dependent global round trips (descriptor, gather, weights, store drain): 4.6 us per node,
// 23 us per chain, 16 workgroups busy - the worst line of the round-1 roofline table (0.0065 of HBM peak).
//
// Here one workgroup per image
//   1. fetches EVERYTHING the chain will need in one burst: the depthwise / pointwise weights and biases of all its
//      nodes and every external input map (a map that needs the 3x3/2 max-pool is pooled while it is loaded), all into
//      LDS - one memory round trip for the whole chain;
//   2. runs the nodes out of LDS: gathers read LDS map slots (external inputs or earlier nodes' outputs), results are
//      written to their slot and streamed to global memory without waiting (later launches read them from there);
//   3. three workgroup barriers per node, no global round trip until the kernel ends.
// Arithmetic, rounding points and operation order are those of sep_kernel (k_sep.hip), so the stage-parity tests
// gate it like every other BiFPN node.  Widths other than what fits in LDS keep the k_sep.hip path.
//
// fp32 sessions (round 4): maps and weights are twice the bytes, so (a) the map slots are shared by liveness (host:
// Planner::add_chain - a node's output takes the slot of a map nobody reads any more) and (b) the node weights are STREAMED
// (template parameter): LDS holds two nodes' weights; the next node's are requested at the head of a node by LDS-DMA
// (global_load_lds_dwordx4, 1 KB per wave instruction, no registers) into the buffer the previous node has left.  The chains of
// an fp32 session ran as sep_kernel<false, 2> before: 35 us per five-node chain against 20 us here in bf16.
//
// The kernel itself is k_chain_impl.h.  This translation unit instantiates the generic kernels (chain_kernel: every shape from
// ChainArgs) and holds launch_chain, which runs a chain on its shape-specialised form (chain_shape_kernel, instantiated in
// k_chain_shape.hip) when one exists for exactly these arguments - chain_shape_id - and on the generic kernel otherwise.
#include "k_chain_impl.h"

// k_chain_shape.hip
Pick chain_shape_pick(int id, const ChainArgs&);
void chain_shape_trace_bind(unsigned long long* p);

#ifdef HEP_MBF_TRACE
extern "C" int hep_dbg_chain_trace(unsigned long long* host, int nblocks, int enable) {
  static unsigned long long* buf = nullptr;
  if (!buf) { if (hipMalloc((void**)&buf, (size_t)4096 * CHAIN_WAVES * 64 * 8) != hipSuccess) return -1; hipMemset(buf, 0, (size_t)4096 * CHAIN_WAVES * 64 * 8); }
  unsigned long long* p = enable ? buf : nullptr;
  chain_trace_bind_tu(p); chain_shape_trace_bind(p);
  if (host) { hipDeviceSynchronize(); hipMemcpy(host, buf, (size_t)nblocks * CHAIN_WAVES * 64 * 8, hipMemcpyDeviceToHost); }
  return 0;
}
#endif

// the row of chain_shape() (k_chain_impl.h) whose kernel runs this launch: every field the kernel folds must equal the row, the
// external-map table included; 0 = the generic kernel (no such row, or the plan asked for it: HEP_NECK_GENERIC)
int chain_shape_id(const ChainArgs& a) {
  if (a.generic || !a.bf16 || a.stream_w != 0 || a.C != CHAIN_SHAPE_C || a.wnode_bytes != CHAIN_SHAPE_WNODE_BYTES) return 0;
  for (int id = 1; id <= CHAIN_SHAPE_ROWS; id++) {
    const ChainShape sh = chain_shape(id);
    bool same = a.next == sh.next && a.nnodes == sh.nnodes && a.nconv == sh.nconv && a.off_w == sh.off_w && a.off_halo == sh.off_halo && a.off_atile == sh.off_atile &&
                a.lds_bytes == sh.lds_bytes;
    for (int e = 0; same && e < sh.next; e++) {
      const ChainExt& x = a.ext[e]; const ChainExtShape& r = sh.ext[e];
      same = x.sh == r.sh && x.sw == r.sw && x.kind == r.kind && x.h == r.h && x.w == r.w && x.pool_pad == r.pool_pad && x.off == r.off && x.has_store == r.store;
    }
    if (same) return id;
  }
  return 0;
}

// the instantiation a launch runs (hep_pick.h): its shape row when it has one, else the generic kernel of its dtype and weight mode
Pick chain_pick(const ChainArgs& a) {
  if (const int id = chain_shape_id(a)) return chain_shape_pick(id, a);
#define CHAIN_PICK(...) HEP_PICK(CHAIN_THREADS, a.lds_bytes, 159 * 1024, chain_kernel, __VA_ARGS__)
  if (a.bf16) return a.stream_w == 2 ? CHAIN_PICK(true, 2) : (a.stream_w == 1 ? CHAIN_PICK(true, 1) : CHAIN_PICK(true, 0));
  return a.stream_w == 2 ? CHAIN_PICK(false, 2) : (a.stream_w == 1 ? CHAIN_PICK(false, 1) : CHAIN_PICK(false, 0));
#undef CHAIN_PICK
}

void launch_chain(const ChainArgs& a_, hipStream_t s) {
  ChainArgs a = a_;
  a.nt_rcp = rcp_u32((uint32_t)((a.C + 15) >> 4));
  chain_pick(a).launch(dim3(a.B), s, a);
}
