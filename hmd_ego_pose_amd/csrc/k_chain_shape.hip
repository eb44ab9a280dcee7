// k_chain_shape.hip - the shape-specialised BiFPN chains (k_chain_impl.h chain_shape(): chain_shape_kernel<true, D>): a translation
// unit of its own so that the build stays parallel; k_chain.hip selects a row (chain_shape_id) and launches it through
// launch_chain_shape.
#include "k_chain_impl.h"

template <int D> static int chain_shape_prep_one() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(chain_shape_kernel<true, D>), hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024) == hipSuccess ? 0 : -1;
}
int chain_shape_prepare(void) {
  static_assert(CHAIN_SHAPE_ROWS == 3, "one line per row below");
  return chain_shape_prep_one<1>() | chain_shape_prep_one<2>() | chain_shape_prep_one<3>();
}

// false when `id` is no row of the table
bool launch_chain_shape(int id, const ChainArgs& a, dim3 grid, hipStream_t s) {
  switch (id) {
    case 1: hipLaunchKernelGGL((chain_shape_kernel<true, 1>), grid, dim3(CHAIN_THREADS), a.lds_bytes, s, a); return true;
    case 2: hipLaunchKernelGGL((chain_shape_kernel<true, 2>), grid, dim3(CHAIN_THREADS), a.lds_bytes, s, a); return true;
    case 3: hipLaunchKernelGGL((chain_shape_kernel<true, 3>), grid, dim3(CHAIN_THREADS), a.lds_bytes, s, a); return true;
    default: return false;
  }
}

void chain_shape_trace_bind(unsigned long long* p) {
#ifdef HEP_MBF_TRACE
  chain_trace_bind_tu(p);
#else
  (void)p;
#endif
}
