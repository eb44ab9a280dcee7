// hep_session.cpp - realisation of a launch plan (hep_plan.cpp) on a device: kernel attributes, streams and events, the
// weight blob, the activation arena, the head outputs, one patched copy of the plan per lane, segment and node tables.
#include <string.h>

#include <algorithm>

#include "hep.h"
#include "hep_plan.h"

namespace hep {

// everything build_session and the entry points (hep_api.cpp, hep_api_pose.cpp) allocated for the handle, at first use or before
Session::~Session() {
  if (!realised) return;            // planned on the host only (hep_plan_launch_list): no device object exists and no HIP call is made
  for (auto& g : graphs) for (hipGraphExec_t ge : g.second) hipGraphExecDestroy(ge);
  for (auto& lo : lane_ops) for (Op& o : lo) {
    if (o.kind == OP_SEP) { hipFree((void*)o.sep.segs); hipFree((void*)o.sep.tile_seg); }
    if (o.kind == OP_CHAIN) hipFree((void*)o.chain.nodes);
  }
  for (hipStream_t st : lane_streams) hipStreamDestroy(st);
  for (hipEvent_t ev : lane_events) hipEventDestroy(ev);
  if (fork_event) hipEventDestroy(fork_event);
  if (pre_event) hipEventDestroy(pre_event);
  hipFree(d_sync); hipFree(d_weights); hipFree(d_arena); hipFree(d_pre[0]); hipFree(d_pre[1]);
  for (int i = 0; i < 5; i++) { hipFree(d_out[i]); hipFree(d_feat_nchw[i]); }
  hipFree(d_in); hipFree(d_anchors); hipFree(d_tanchors); hipFree(d_boxes); hipFree(d_trans); hipFree(d_cam);
  hipFree(d_keys); hipFree(d_det); hipFree(d_part);
  for (int i = 0; i < 5; i++) hipFree(d_stage[i]);
  hipFree(d_pose_in); hipFree(d_rec); hipHostFree(h_pose_in); hipHostFree(h_rec); hipFree(d_recs); hipHostFree(h_recs);
  hipFree(d_best); hipHostFree(h_best);
  if (stream) hipStreamDestroy(stream);
}

size_t sync_lane_words(const Session& s, const Plan& plan) {
  // per lane: 16 words per image for the grouped late kernel, then ntails blocks of one 128-byte line per image (arrival tickets of the fronts' tails)
  return (size_t)s.lane_batch * 16 + (size_t)plan.ntails * s.lane_batch * 32;
}

void patch_lane(const Session& s, const Plan& plan, int lane, std::vector<Op>* ops) {
  for (const Ref& r : plan.refs) {
    void* ptr = nullptr;
    switch (r.kind) {
      case TO_TENSOR: ptr = s.tptr((int)r.at, lane); break;
      case TO_WEIGHT: ptr = s.d_weights + r.at; break;
      case TO_HEAD_OUT: ptr = s.d_out[r.at] + (size_t)lane * s.lane_batch * s.num_anchors * s.out_k((int)r.at); break;
    }
    r.set((*ops)[r.op], r.seg, r.idx, ptr);
  }
  unsigned* sync = s.d_sync + (size_t)lane * sync_lane_words(s, plan);
  for (Op& o : *ops) {
#ifdef HEP_ALT
    if (o.kind == OP_LATE) o.late.counters = sync;
#endif
    if (o.kind == OP_MBF && o.mbf.se_tail) o.mbf.tail_counter = sync + (size_t)s.lane_batch * 16 + (size_t)(o.mbf.se_tail - 1) * s.lane_batch * 32;
  }
}

int build_session(Session* s, const Pack& pack, std::string* err) {
  s->realised = true;
  if (hipDeviceGetAttribute(&s->cu_count, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || s->cu_count <= 0) s->cu_count = 256;
  Plan plan;
  if (int rc = plan_session(s, pack, &plan, err)) return rc;

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { *err = std::string(#x) + ": " + hipGetErrorString(e_); return HEP_ERR_DEVICE; } } while (0)
  HIPCHK(hipSetDevice(s->device));
  // dynamic LDS beyond the default limit: raised for the device functions this plan launches (their picks say how far), and for the detection filter
  for (const Op& o : s->ops) {
    const Pick p = op_pick(o);
    if (p.max_lds && hipFuncSetAttribute(p.fn, hipFuncAttributeMaxDynamicSharedMemorySize, p.max_lds) != hipSuccess) {
      *err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for " + p.name() + " (" + o.name + ")"; return HEP_ERR_DEVICE;
    }
  }
  if (filter_prepare() != 0) { *err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for filter_kernel"; return HEP_ERR_DEVICE; }
  HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  s->weights_bytes = plan.weights.size();
  HIPCHK(hipMalloc((void**)&s->d_weights, s->weights_bytes));
  HIPCHK(hipMemcpy(s->d_weights, plan.weights.data(), s->weights_bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMalloc((void**)&s->d_arena, std::max<size_t>(s->arena_bytes * s->lanes, 256)));
#ifdef HEP_POISON_LDS     // sanitizer build: activation cells nobody has written yet read as NaN (0xFFFF / 0xFFFFFFFF)
  HIPCHK(hipMemset(s->d_arena, 0xFF, std::max<size_t>(s->arena_bytes * s->lanes, 256)));
#endif
  for (int i = 0; i < 5; i++) HIPCHK(hipMalloc((void**)&s->d_out[i], (size_t)s->max_batch * s->num_anchors * s->out_k(i) * 4));
  {
    std::vector<float> a, t; host_anchors(s->size, &a, &t);
    HIPCHK(hipMalloc((void**)&s->d_anchors, a.size() * 4)); HIPCHK(hipMemcpy(s->d_anchors, a.data(), a.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&s->d_tanchors, t.size() * 4)); HIPCHK(hipMemcpy(s->d_tanchors, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  }
  HIPCHK(hipEventCreateWithFlags(&s->fork_event, hipEventDisableTiming));
  const size_t sync_bytes = s->lanes * sync_lane_words(*s, plan) * 4 + 64;
  HIPCHK(hipMalloc((void**)&s->d_sync, sync_bytes));
  HIPCHK(hipMemset(s->d_sync, 0, sync_bytes));
  // ---- one patched copy of the plan per lane: own arena slice, own slice of the head outputs ----
  s->lane_ops.assign(s->lanes, s->ops);
  for (int lane = 0; lane < s->lanes; lane++) {
    hipStream_t st; HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); s->lane_streams.push_back(st);
    hipEvent_t ev; HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); s->lane_events.push_back(ev);
    std::vector<Op>& ops = s->lane_ops[lane];
    patch_lane(*s, plan, lane, &ops);
    // segment tables to device
    for (Op& o : ops)
      if (o.kind == OP_SEP) {
        SepSeg* d; HIPCHK(hipMalloc((void**)&d, o.segs.size() * sizeof(SepSeg)));
        HIPCHK(hipMemcpy(d, o.segs.data(), o.segs.size() * sizeof(SepSeg), hipMemcpyHostToDevice));
        o.sep.segs = d;
        std::vector<int> tile_seg(o.sep.total_tiles);
        for (size_t si = 0; si < o.segs.size(); si++)
          for (int t = 0; t < o.segs[si].tiles_x * o.segs[si].tiles_y; t++) tile_seg[o.segs[si].tile_begin + t] = (int)si;
        int* dt; HIPCHK(hipMalloc((void**)&dt, tile_seg.size() * sizeof(int)));
        HIPCHK(hipMemcpy(dt, tile_seg.data(), tile_seg.size() * sizeof(int), hipMemcpyHostToDevice));
        o.sep.tile_seg = dt;
        o.sep.seg0 = o.segs[0];
      } else if (o.kind == OP_CHAIN) {
        // (whole 256-byte chunks: chain_kernel warms the scalar cache with one s_load_dword per 64-byte line of every chunk it touches)
        ChainNode* d; HIPCHK(hipMalloc((void**)&d, (o.cnodes.size() * sizeof(ChainNode) + 255) & ~(size_t)255));
        HIPCHK(hipMemcpy(d, o.cnodes.data(), o.cnodes.size() * sizeof(ChainNode), hipMemcpyHostToDevice));
        o.chain.nodes = d;
      }
  }
#undef HIPCHK
  return 0;
}

}  // namespace hep
