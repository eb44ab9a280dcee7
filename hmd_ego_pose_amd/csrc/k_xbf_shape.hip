// k_xbf_shape.hip - the shape-specialised block boundaries (k_xbf_impl.h XBF_SHAPES: xbf_kernel_shape<true, D>): a translation unit of
// its own so that the build stays parallel; k_xbf.hip selects a row (xbf_shape_id) and launches it through launch_xbf_shape.
#include "k_xbf_impl.h"

#define XBF_SHAPE_PREP_ROW(id, ...) \
  rc |= hipFuncSetAttribute(reinterpret_cast<const void*>(xbf_kernel_shape<true, id>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess ? 0 : -1;
#define XBF_SHAPE_LAUNCH_ROW(id, ...) \
  case id: hipLaunchKernelGGL((xbf_kernel_shape<true, id>), grid, dim3(XT), a.lds_bytes, s, a); return true;

int xbf_shape_prepare(void) {
  int rc = 0;
  XBF_SHAPES(XBF_SHAPE_PREP_ROW)
  return rc;
}

// false when `id` is no row of the table
bool launch_xbf_shape(int id, const XbfArgs& a, dim3 grid, hipStream_t s) {
  switch (id) {
    XBF_SHAPES(XBF_SHAPE_LAUNCH_ROW)
    default: return false;
  }
}

void xbf_shape_trace_bind(unsigned long long* p) {
#ifdef HEP_XBF_TRACE
  xbf_trace_bind_tu(p);
#else
  (void)p;
#endif
}
