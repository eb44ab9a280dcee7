// k_xbf_shape.hip - the shape-specialised block boundaries (k_xbf_impl.h XBF_SHAPES: xbf_kernel_shape<true, D>): a translation unit of
// its own so that the build stays parallel; k_xbf.hip selects a row (xbf_shape_id) and takes its pick from xbf_shape_pick.
#include "k_xbf_impl.h"

#define XBF_SHAPE_PICK_ROW(id, ...) \
  case id: return HEP_PICK(XT, a.lds_bytes, 160 * 1024, xbf_kernel_shape, true, id);

// empty when `id` is no row of the table
Pick xbf_shape_pick(int id, const XbfArgs& a) {
  switch (id) {
    XBF_SHAPES(XBF_SHAPE_PICK_ROW)
    default: return Pick();
  }
}

void xbf_shape_trace_bind(unsigned long long* p) {
#ifdef HEP_XBF_TRACE
  xbf_trace_bind_tu(p);
#else
  (void)p;
#endif
}
