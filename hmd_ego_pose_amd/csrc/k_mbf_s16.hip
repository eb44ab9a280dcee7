// k_mbf_s16.hip - the shape-specialised fused fronts on 16x16 output tiles (k_mbf_impl.h MBF_SHAPES_16): a translation unit of its
// own so that the library builds in the wall time it had (as k_pw_{bf16,f32}.hip).
#include "k_mbf_impl.h"

MBF_SHAPE_TU(MBF_SHAPES_16, mbf_shape_pick_16, mbf_trace_bind_16)
