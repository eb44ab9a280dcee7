// k_sep_shape.hip - the shape-specialised single BiFPN nodes (k_sep_impl.h SEP_SHAPES: sep_shape_kernel<true, D>): a translation unit
// of its own so that the build stays parallel; k_sep.hip selects a row (sep_shape_id) and takes its pick from sep_shape_pick.
#include <algorithm>

#include "k_sep_impl.h"

// A/B hook (NOTEBOOK.md section 31): the dynamic LDS a row asks for at least.  The rows need 76-78 VGPRs and 25.6 KB of LDS, so three
// 512-thread workgroups fit on a CU where the generic kernel (112 VGPRs) has two; -DSEP_SHAPE_MIN_LDS=55296 keeps two.
#ifndef SEP_SHAPE_MIN_LDS
#define SEP_SHAPE_MIN_LDS 0
#endif

#define SEP_SHAPE_PICK_ROW(id, ...) \
  case id: return HEP_PICK(512, std::max<size_t>(a.lds_bytes, SEP_SHAPE_MIN_LDS), 159 * 1024, sep_shape_kernel, true, id);

// empty when `id` is no row of the table
Pick sep_shape_pick(int id, const SepArgs& a) {
  switch (id) {
    SEP_SHAPES(SEP_SHAPE_PICK_ROW)
    default: return Pick();
  }
}

void sep_shape_trace_bind(unsigned long long* p, int hw) {
#ifdef HEP_TOWER_TRACE
  sep_trace_bind_tu(p, hw);
#else
  (void)p; (void)hw;
#endif
}
