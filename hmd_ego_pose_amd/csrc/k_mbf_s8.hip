// k_mbf_s8.hip - the shape-specialised fused fronts on 8x8 output tiles (k_mbf_impl.h MBF_SHAPES_8); see k_mbf_s16.hip.
#include "k_mbf_impl.h"

MBF_SHAPE_TU(MBF_SHAPES_8, mbf_shape_pick_8, mbf_trace_bind_8)
