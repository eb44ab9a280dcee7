// k_chain_shape.hip - the shape-specialised BiFPN chains (k_chain_impl.h chain_shape(): chain_shape_kernel<true, D>): a translation
// unit of its own so that the build stays parallel; k_chain.hip selects a row (chain_shape_id) and takes its pick from
// chain_shape_pick.
#include "k_chain_impl.h"

// empty when `id` is no row of the table
Pick chain_shape_pick(int id, const ChainArgs& a) {
  static_assert(CHAIN_SHAPE_ROWS == 3, "one line per row below");
  switch (id) {
    case 1: return HEP_PICK(CHAIN_THREADS, a.lds_bytes, 159 * 1024, chain_shape_kernel, true, 1);
    case 2: return HEP_PICK(CHAIN_THREADS, a.lds_bytes, 159 * 1024, chain_shape_kernel, true, 2);
    case 3: return HEP_PICK(CHAIN_THREADS, a.lds_bytes, 159 * 1024, chain_shape_kernel, true, 3);
    default: return Pick();
  }
}

void chain_shape_trace_bind(unsigned long long* p) {
#ifdef HEP_MBF_TRACE
  chain_trace_bind_tu(p);
#else
  (void)p;
#endif
}
