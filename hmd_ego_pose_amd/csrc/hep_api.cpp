// hep_api.cpp - the session side of the C ABI of libhep.so (include/hep.h) and the forward executor:
// eager stem launch (it reads the caller's input pointer) + one captured hipGraph for
// everything behind it, replayed on the caller's stream.  The entry points that take no handle are in files of their
// own: the evaluation and visualisation toolkit in hep_api_eval.cpp, the training side in hep_api_train.cpp.
#include <float.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <math.h>

#include <chrono>
#include <fstream>
#include <memory>

#include "hep_api_util.h"
#include "hep_plan.h"

using namespace hep;

thread_local std::string hep::g_err;      // the message behind hep_last_error(): the one definition (hep_api_util.h)

struct hep_handle { Session s; };

namespace hep {

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

void launch_op(const Session& s, const Op& op, int batch, hipStream_t st, const float* in, const int64_t* strides) {
  switch (op.kind) {
    case OP_STEM: {
      StemArgs a = op.stem; a.B = batch; a.in = in;
      a.sn = strides[0]; a.sc = strides[1]; a.sh = strides[2]; a.sw = strides[3];
      launch_stem(a, st); break;
    }
    case OP_PW: { PwArgs a = op.pw; a.M = batch * a.HW; launch_pw(a, st); break; }
    case OP_DW: { DwArgs a = op.dw; a.B = batch; launch_dw(a, st); break; }
    case OP_POOL: { PoolArgs a = op.pool; a.B = batch; launch_pool(a, st); break; }
    case OP_PWG: { PwgArgs a = op.pwg; a.B = batch; launch_pwg(a, st); break; }
    case OP_MBF: { MbfArgs a = op.mbf; a.B = batch; launch_mbf(a, st); break; }
    case OP_CHAIN: { ChainArgs a = op.chain; a.B = batch; launch_chain(a, st); break; }
    case OP_SE: { SeFinishArgs a = op.se; a.B = batch; launch_se_finish(a, st); break; }
    case OP_XBF: { XbfArgs a = op.xbf; a.B = batch; launch_xbf(a, st); break; }
#ifdef HEP_ALT
    case OP_LATE: { LateArgs a = op.late; a.B = batch; launch_late(a, st); break; }
    case OP_HEADS: { HeadsArgs a = op.heads; a.B = batch; launch_heads(a, st); break; }
    case OP_SBF: {
      SbfArgs a = op.sbf; a.B = batch; a.in = in;
      a.sn = strides[0]; a.sc = strides[1]; a.sh = strides[2]; a.sw = strides[3];
      launch_sbf(a, st); break;
    }
#endif
    case OP_SEP: {
      SepArgs a = op.sep; a.B = batch;
      if (a.direct) launch_tower(a, st);
      else launch_sep(a, st);
      break;
    }
  }
}

// the device function launch_op runs for `op` and how (hep_pick.h): the family's own pick, which reads what the planner set
Pick op_pick(const Op& op) {
  switch (op.kind) {
    case OP_STEM: return stem_pick(op.stem);
    case OP_PW: return pw_pick(op.pw);
    case OP_DW: return dw_pick(op.dw);
    case OP_POOL: return pool_pick(op.pool);
    case OP_PWG: return pwg_pick(op.pwg);
    case OP_MBF: return mbf_pick(op.mbf);
    case OP_CHAIN: return chain_pick(op.chain);
    case OP_SE: return se_finish_pick(op.se);
    case OP_XBF: return xbf_pick(op.xbf);
#ifdef HEP_ALT
    case OP_LATE: return late_pick(op.late);
    case OP_HEADS: return heads_pick(op.heads);
    case OP_SBF: return sbf_pick(op.sbf);
#endif
    case OP_SEP: return op.sep.direct ? tower_pick(op.sep) : sep_pick(op.sep);
    default: return Pick();
  }
}

// forward = per lane: ops[0] (stem, eager: its input pointer belongs to the caller) + the rest inside
// ONE hipGraph whose lanes are parallel branches (fork/join captured through events)
int run_forward(Session* s, const float* in_dev, const int64_t* strides, int batch, hipStream_t st, std::string* err) {
  const int64_t S = s->size;
  const int64_t contiguous[4] = {3 * S * S, S * S, S, 1};
  if (!strides) strides = contiguous;
  const int nl = s->lanes_for(batch);
  for (int l = 0; l < nl; l++)
    launch_op(*s, s->lane_ops[l][0], s->lane_count(batch, l), st, in_dev + (int64_t)l * s->lane_batch * strides[0], strides);
  if (s->flags & HEP_FLAG_NO_GRAPH) {
    for (int l = 0; l < nl; l++)
      for (size_t i = 1; i < s->ops.size(); i++) launch_op(*s, s->lane_ops[l][i], s->lane_count(batch, l), st, nullptr, nullptr);
  } else {
    // one captured graph per lane, replayed on the lane's own stream so that the lanes' kernel
    // chains overlap on the device; the caller's stream forks into the lane streams and joins them
    auto it = s->graphs.find(batch);
    if (it == s->graphs.end()) {
      std::vector<hipGraphExec_t> execs;
      for (int l = 0; l < nl; l++) {
        hipGraph_t g; hipGraphExec_t ge;
        hipError_t e = hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) { *err = std::string("hipStreamBeginCapture: ") + hipGetErrorString(e); return HEP_ERR_DEVICE; }
        for (size_t i = 1; i < s->ops.size(); i++) launch_op(*s, s->lane_ops[l][i], s->lane_count(batch, l), s->stream, nullptr, nullptr);
        e = hipStreamEndCapture(s->stream, &g);
        if (e != hipSuccess) { *err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e); return HEP_ERR_DEVICE; }
        e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (e != hipSuccess) { *err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e); return HEP_ERR_DEVICE; }
        execs.push_back(ge);
      }
      it = s->graphs.emplace(batch, execs).first;
    }
    hipError_t e = hipSuccess;
    if (nl == 1) e = hipGraphLaunch(it->second[0], st);
    else {
      e = hipEventRecord(s->fork_event, st);
      for (int l = 0; l < nl && e == hipSuccess; l++) {
        hipStream_t ls = s->lane_streams[l];
        e = hipStreamWaitEvent(ls, s->fork_event, 0);
        if (e == hipSuccess) e = hipGraphLaunch(it->second[l], ls);
        if (e == hipSuccess) e = hipEventRecord(s->lane_events[l], ls);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, s->lane_events[l], 0);
      }
    }
    if (e != hipSuccess) { *err = std::string("hipGraphLaunch: ") + hipGetErrorString(e); return HEP_ERR_DEVICE; }
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *err = std::string("kernel launch: ") + hipGetErrorString(e); return HEP_ERR_DEVICE; }
  s->last_batch = batch;
  return 0;
}

}  // namespace hep

// fp8 sessions: one power-of-two scale per quantised GEMM input, from the amax of that tensor on a deterministic
// calibration batch (pseudo-normal frames) run eagerly through the session's own kernels: the scale of a launch is set
// before the launch runs, so every later tensor already sees the quantised arithmetic in front of it.  The e4m3
// conversion saturates at +-448 * scale, and the scale carries 2x headroom over the calibration amax.
static int calibrate_fp8(Session& s, const float* frames_dev = nullptr, int nframes = 0) {
  HIPRET(hipSetDevice(s.device));
  const int nb = frames_dev ? std::min(s.lane_batch, nframes) : std::min(s.lane_batch, 2);
  const size_t in_floats = (size_t)3 * s.size * s.size;
  if (!s.d_in) HIPRET(hipMalloc((void**)&s.d_in, in_floats * s.max_batch * 4));
  if (frames_dev) HIPRET(hipMemcpy(s.d_in, frames_dev, in_floats * nb * 4, hipMemcpyDeviceToDevice));
  else {
    std::vector<float> x(in_floats * nb);
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto u01 = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return ((st >> 11) + 0.5) * (1.0 / 9007199254740992.0); };
    for (size_t i = 0; i + 1 < x.size(); i += 2) {          // Box-Muller
      const double r = sqrt(-2.0 * log(u01())), t = 6.283185307179586 * u01();
      x[i] = (float)(r * cos(t)); x[i + 1] = (float)(r * sin(t));
    }
    HIPRET(hipMemcpy(s.d_in, x.data(), x.size() * 4, hipMemcpyHostToDevice));
  }
  unsigned* d_m = nullptr;
  HIPRET(hipMalloc((void**)&d_m, 4));
  const int64_t S = s.size; const int64_t strides[4] = {3 * S * S, S * S, S, 1};
  for (size_t i = 0; i < s.ops.size(); i++) {
    Op& o = s.ops[i];
    const bool q = (o.kind == OP_PW && o.pw.fp8) || (o.kind == OP_MBF && o.mbf.fp8);
    if (q) {
      const TensorDesc& t = s.tensors[o.reads[0]];
      hipMemsetAsync(d_m, 0, 4, s.stream);
      launch_amax_bf16(s.tptr(o.reads[0], 0), (int64_t)nb * t.H * t.W * t.C, d_m, s.stream);
      unsigned bits = 0;
      if (hipMemcpyAsync(&bits, d_m, 4, hipMemcpyDeviceToHost, s.stream) != hipSuccess || hipStreamSynchronize(s.stream) != hipSuccess) {
        hipFree(d_m); return fail(HEP_ERR_DEVICE, "fp8 calibration failed");
      }
      float amax; memcpy(&amax, &bits, 4);
      float sc = 1.f;
      if (amax > 0.f && amax < 3e38f) sc = exp2f(ceilf(log2f(2.f * amax / 448.f)));
      for (auto& lo : s.lane_ops) { if (o.kind == OP_PW) lo[i].pw.a_scale = sc; else lo[i].mbf.a_scale = sc; }
      if (o.kind == OP_PW) o.pw.a_scale = sc; else o.mbf.a_scale = sc;
    }
    launch_op(s, s.lane_ops[0][i], nb, s.stream, s.d_in, strides);
  }
  hipError_t e = hipStreamSynchronize(s.stream);
  hipFree(d_m);
  if (e != hipSuccess || (e = hipGetLastError()) != hipSuccess) return fail(HEP_ERR_DEVICE, std::string("fp8 calibration: ") + hipGetErrorString(e));
  // the scales travel by value in the launch arguments: graphs captured with the old ones are dropped
  for (auto& g : s.graphs) for (hipGraphExec_t ge : g.second) hipGraphExecDestroy(ge);
  s.graphs.clear();
  return 0;
}

extern "C" {

int hep_abi_version(void) { return HEP_ABI_VERSION; }
const char* hep_build_info(void) {
  return "libhep gfx950"
#ifdef HEP_ALT
         " alt"
#endif
#ifdef HEP_WITH_FP8
         " fp8"
#endif
#ifdef HEP_POISON_LDS
         " poison"
#endif
#if defined(HEP_MBF_TRACE) || defined(HEP_TOWER_TRACE) || defined(HEP_PW_TRACE) || defined(HEP_XBF_TRACE)
         " trace"
#endif
      ;
}
const char* hep_last_error(void) { return g_err.c_str(); }

int hep_device_count(void) try {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
} HEP_CATCH_INT

// knobs of the environment and the lanes they ask for: slices of the batch that run as parallel graph branches (HEP_LANES overrides)
static void session_lanes(Session* s) {
  s->knobs = read_knobs();
  int lanes = s->knobs.lanes;   // 1: measured on MI355X at bs16, 2/4/8 lanes are 4 % / 75 % / 150 % SLOWER (kernels contend instead of overlapping)
  lanes = std::max(1, std::min(lanes, std::min(s->max_batch, 16)));
  s->lane_batch = (s->max_batch + lanes - 1) / lanes;
  s->lanes = (s->max_batch + s->lane_batch - 1) / s->lane_batch;
}

int hep_create_from_memory(const void* pack, size_t pack_bytes, int phi, int size, int max_batch, int dtype, int device,
                           unsigned flags, hep_handle** out) try {
  if (!out) return fail(HEP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!pack || pack_bytes < 12) return fail(HEP_ERR_PACK, "weight pack: empty");
  if (dtype != HEP_F32 && dtype != HEP_BF16 && dtype != HEP_FP8) return fail(HEP_ERR_INVALID, "dtype must be HEP_F32, HEP_BF16 or HEP_FP8");
#ifndef HEP_WITH_FP8
  if (dtype == HEP_FP8) return fail(HEP_ERR_UNSUPPORTED, "this libhep.so was built without the fp8 path (make -C hmd_ego_pose_amd/csrc FP8=1): it measured slower than bf16");
#endif
  if (max_batch < 1 || max_batch > 4096) return fail(HEP_ERR_INVALID, "max_batch out of range (1..4096)");
  if (size < 128 || size > 2048 || size % 128 != 0)
    return fail(HEP_ERR_UNSUPPORTED, "size must be a multiple of 128 in [128, 2048] (P7 has stride 128)");
  std::unique_ptr<hep_handle> h(new hep_handle);
  Session& s = h->s;
  if (!make_arch(phi, &s.arch)) return fail(HEP_ERR_UNSUPPORTED, "phi must be in 0..7 (phi 8 needs a P8 level)");
  Pack pk; std::string err;                       // host-only: a malformed pack is reported before any device is touched
  if (!pk.parse(pack, pack_bytes, &err)) return fail(HEP_ERR_PACK, err);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(HEP_ERR_DEVICE, "no HIP device visible: libhep has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(HEP_ERR_INVALID, "device index out of range");
  hipDeviceProp_t prop;
  HIPRET(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(HEP_ERR_DEVICE, std::string("device is ") + prop.gcnArchName + ", libhep is built for gfx950 (MI355X) only");
  s.size = size; s.max_batch = max_batch; s.dtype = dtype; s.device = device; s.flags = flags;
  session_lanes(&s);
  int rc = build_session(&s, pk, &err);
  if (rc != 0) return fail(rc, err);
  if (dtype == HEP_FP8) if (int rc2 = calibrate_fp8(s)) return rc2;
  *out = h.release();
  return 0;
} HEP_CATCH_INT

int hep_create(const char* pack_path, int phi, int size, int max_batch, int dtype, int device, unsigned flags, hep_handle** out) try {
  if (out) *out = nullptr;
  if (!pack_path) return fail(HEP_ERR_INVALID, "pack_path is NULL");
  std::ifstream f(pack_path, std::ios::binary | std::ios::ate);
  if (!f) return fail(HEP_ERR_PACK, std::string("cannot open weight pack '") + pack_path + "'");
  const std::streamsize n = f.tellg();
  f.seekg(0);
  std::vector<char> buf((size_t)n);
  if (!f.read(buf.data(), n)) return fail(HEP_ERR_PACK, "cannot read weight pack");
  return hep_create_from_memory(buf.data(), buf.size(), phi, size, max_batch, dtype, device, flags, out);
} HEP_CATCH_INT

void hep_destroy(hep_handle* h) try {
  if (!h) return;
  hipSetDevice(h->s.device);
  hipDeviceSynchronize();
#ifdef HEP_POISON_LDS
  {   // sanitizer build: the bytes between the end of every activation tensor and the next one still hold the 0xFF the arena was
      // created with - a kernel that stored past the end of its output is named here and the process stops
    const Session& s = h->s;
    std::vector<unsigned char> host(s.arena_bytes * s.lanes);
    if (!host.empty() && hipMemcpy(host.data(), s.d_arena, host.size(), hipMemcpyDeviceToHost) == hipSuccess)
      for (int lane = 0; lane < s.lanes; lane++)
        for (const TensorDesc& t : s.tensors) {
          if (t.external || t.first_op < 0) continue;
          const size_t used = t.bytes_per_image * s.lane_batch, end = ((used + 255) & ~(size_t)255) + 256;
          for (size_t i = used; i < end; i++)
            if (host[(size_t)lane * s.arena_bytes + t.offset + i] != 0xFF) {
              fprintf(stderr, "libhep sanitizer: tensor '%s' (lane %d) was written %zu byte(s) past its end\n", t.name.c_str(), lane, i - used + 1);
              abort();
            }
        }
  }
#endif
  delete h;
} HEP_CATCH_VOID

int hep_num_anchors(const hep_handle* h) try { return h ? h->s.num_anchors : fail(HEP_ERR_INVALID, "handle is NULL"); } HEP_CATCH_INT
int hep_num_classes(const hep_handle* h) try { return h ? h->s.num_classes : fail(HEP_ERR_INVALID, "handle is NULL"); } HEP_CATCH_INT

int hep_output_shape(const hep_handle* h, int index, int batch, int64_t dims[4], int* ndim) try {
  if (!h || !dims || index < 0 || index >= HEP_NUM_OUTPUTS) return fail(HEP_ERR_INVALID, "bad argument");
  const Session& s = h->s;
  if (index < 5) { dims[0] = batch; dims[1] = s.arch.fpn_w; dims[2] = s.levels[index]; dims[3] = s.levels[index]; if (ndim) *ndim = 4; }
  else { dims[0] = batch; dims[1] = s.num_anchors; dims[2] = s.out_k(index - 5); dims[3] = 1; if (ndim) *ndim = 3; }
  return 0;
} HEP_CATCH_INT

int hep_output_device(const hep_handle* h, int index, float** ptr) try {
  if (!h || !ptr || index < 5 || index >= HEP_NUM_OUTPUTS) return fail(HEP_ERR_INVALID, "hep_output_device: index must be one of the five head outputs");
  *ptr = h->s.d_out[index - 5];
  return 0;
} HEP_CATCH_INT

static int check_run(hep_handle* h, const void* input, int batch) {
  if (!h) return fail(HEP_ERR_INVALID, "handle is NULL");
  if (!input) return fail(HEP_ERR_INVALID, "input is NULL");
  if (batch < 1 || batch > h->s.max_batch) return fail(HEP_ERR_UNSUPPORTED, "batch outside 1..max_batch given to hep_create");
  return 0;
}

static int export_feats(Session& s, int batch, float* const feats[5], bool device_dst, hipStream_t st) {
  if (!feats) return 0;
  for (int l = 0; l < 5; l++) {
    if (!feats[l]) continue;
    const TensorDesc& t = s.tensors[s.feat_ids[l]];
    const size_t n = (size_t)batch * t.H * t.W * t.C;
    float* dst = feats[l];
    if (!device_dst) {
      if (!s.d_feat_nchw[l]) HIPRET(hipMalloc((void**)&s.d_feat_nchw[l], (size_t)s.max_batch * t.H * t.W * t.C * 4));
      dst = s.d_feat_nchw[l];
    }
    for (int ln = 0; ln < s.lanes_for(batch); ln++) {
      ExportArgs a; a.in = s.tptr(s.feat_ids[l], ln); a.out = dst + (size_t)ln * s.lane_batch * t.H * t.W * t.C;
      a.B = s.lane_count(batch, ln); a.H = t.H; a.W = t.W; a.C = t.C; a.bf16 = s.dtype;
      launch_export(a, st);
    }
    if (!device_dst) HIPRET(hipMemcpyAsync(feats[l], dst, n * 4, hipMemcpyDeviceToHost, st));
  }
  return 0;
}

int hep_run_device(hep_handle* h, const float* input, const int64_t in_strides[4], int batch, float* const outs[5],
                   float* const feats[5], void* stream) try {
  if (int rc = check_run(h, input, batch)) return rc;
  Session& s = h->s;
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  hipStream_t st = (hipStream_t)stream;
  std::string err;
  if (int rc = run_forward(&s, input, in_strides, batch, st, &err)) return fail(rc, err);
  if (outs)
    for (int i = 0; i < 5; i++)
      if (outs[i] && outs[i] != s.d_out[i])
        HIPRET(hipMemcpyAsync(outs[i], s.d_out[i], (size_t)batch * s.num_anchors * s.out_k(i) * 4, hipMemcpyDeviceToDevice, st));
  return export_feats(s, batch, feats, true, st);
} HEP_CATCH_INT

int hep_run(hep_handle* h, const float* input_nchw, int batch, float* const feats[5], float* regression, float* classification,
            float* rotation, float* translation_raw, float* hand) try {
  if (int rc = check_run(h, input_nchw, batch)) return rc;
  Session& s = h->s;
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  const size_t in_floats = (size_t)3 * s.size * s.size;
  if (!s.d_in) HIPRET(hipMalloc((void**)&s.d_in, in_floats * s.max_batch * 4));
  HIPRET(hipMemcpyAsync(s.d_in, input_nchw, in_floats * batch * 4, hipMemcpyHostToDevice, s.stream));
  std::string err;
  if (int rc = run_forward(&s, s.d_in, nullptr, batch, s.stream, &err)) return fail(rc, err);
  float* outs[5] = {regression, classification, rotation, translation_raw, hand};
  for (int i = 0; i < 5; i++)
    if (outs[i]) HIPRET(hipMemcpyAsync(outs[i], s.d_out[i], (size_t)batch * s.num_anchors * s.out_k(i) * 4, hipMemcpyDeviceToHost, s.stream));
  if (int rc = export_feats(s, batch, feats, false, s.stream)) return rc;
  HIPRET(hipStreamSynchronize(s.stream));
  return 0;
} HEP_CATCH_INT

int hep_anchors(int size, float* anchors, float* translation_anchors) try {
  if (size < 128 || size % 128 != 0) return fail(HEP_ERR_UNSUPPORTED, "size must be a positive multiple of 128");
  std::vector<float> a, t;
  const int n = host_anchors(size, anchors ? &a : nullptr, translation_anchors ? &t : nullptr);
  if (anchors) memcpy(anchors, a.data(), a.size() * 4);
  if (translation_anchors) memcpy(translation_anchors, t.data(), t.size() * 4);
  return n;
} HEP_CATCH_INT

int hep_preprocess_u8_device(hep_handle* h, const uint8_t* rgb_hwc, int batch, int height, int width, float* out_hwc, void* stream) try {
  if (!h || !rgb_hwc || !out_hwc || batch < 1 || height < 1 || width < 1) return fail(HEP_ERR_INVALID, "bad argument");
  Session& s = h->s;
  HIPRET(hipSetDevice(s.device));
  ResizeGeom g;
  if (!resize_geometry(height, width, s.size, &g)) return fail(HEP_ERR_UNSUPPORTED, "preprocess: resized frame does not fit the network size");
  PreprocArgs a; a.in = rgb_hwc; a.out = out_hwc; a.B = batch; a.H = height; a.W = width; a.S = s.size;
  a.resize = g.resize; a.nh = g.nh; a.nw = g.nw; a.inv_scale_x = g.inv_scale_x; a.inv_scale_y = g.inv_scale_y;
  launch_preprocess(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

// the frame geometry both I420 entry points refuse (host arithmetic only)
static int check_i420(int height, int width, int crop, int resized) {
  if (height < 2 || width < 2 || (height & 1) || (width & 1)) return fail(HEP_ERR_INVALID, "4:2:0 frames have even sides");
  if (crop < 1 || crop > height || crop > width || resized < 1) return fail(HEP_ERR_INVALID, "crop must fit the frame, resized must be positive");
  return 0;
}

// the launches of the frame path on `st`; s.mu is held (the two scratch buffers belong to the handle)
// windows (hep_preprocess_i420_windows_device): a device table [batch][3] {frame, ox, oy} - output image i is that window of the frames at `yuv`
// in place of the centre crop of frame i; everything behind the first launch is the same
// rect (hep_preprocess_i420_rectified_device): a device table [batch][HEP_RECTIFY_ROW_DOUBLES] next to `windows` - image i is the rectified window
static int preprocess_i420_locked(Session& s, const uint8_t* yuv, int batch, int height, int width, int crop, int resized,
                                  float* out_hwc, hipStream_t st, const int32_t* windows = nullptr, const double* rect = nullptr) {
  // The scratch frames are used ASYNCHRONOUSLY on the caller's stream and the mutex only covers the enqueue: a second call on
  // another stream (an in-flight pool) must not overwrite them while the first call's kernels still read them.  An event is
  // recorded behind the last launch of every call and the next call's stream waits for it first (device-side, no host stall).
  if (!s.pre_event) HIPRET(hipEventCreateWithFlags(&s.pre_event, hipEventDisableTiming));
  // sized once for the handle's max_batch frames of this geometry; growing them (a larger geometry later) waits for the
  // last user first - hipFree would stall every stream of the device anyway, so it is kept off the steady state
  const int cap = batch > s.max_batch ? batch : s.max_batch;
  const size_t need[2] = {(size_t)batch * crop * crop * 3, (size_t)batch * resized * resized * 3};
  const size_t want[2] = {(size_t)cap * crop * crop * 3, (size_t)cap * resized * resized * 3};
  for (int i = 0; i < 2; i++)
    if (s.pre_bytes[i] < need[i]) {
      if (s.pre_pending) { HIPRET(hipEventSynchronize(s.pre_event)); s.pre_pending = false; }
      hipFree(s.d_pre[i]); s.d_pre[i] = nullptr; s.pre_bytes[i] = 0;
      HIPRET(hipMalloc((void**)&s.d_pre[i], want[i])); s.pre_bytes[i] = want[i];
    }
  // (the handle-owned event would become a captured event: a later wait outside the capture may fail - this entry point is
  //  not for stream capture)
  {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return fail(HEP_ERR_UNSUPPORTED, std::string(rect ? "hep_preprocess_i420_rectified_device" : windows ? "hep_preprocess_i420_windows_device" : "hep_preprocess_i420_device") + " must not be called under stream capture");
  }
  if (s.pre_pending) HIPRET(hipStreamWaitEvent(st, s.pre_event, 0));
  // from the first launch on, EVERY return path leaves the event behind the scratch frames' last user
  struct Guard { Session& s; hipStream_t st; ~Guard() { if (hipEventRecord(s.pre_event, st) == hipSuccess) s.pre_pending = true; } } guard{s, st};
  // Program.cs:161 cvtColor + 383-397 CenterCropAndRescaleMat
  if (rect) {
    Yv12RectArgs ra; ra.in = yuv; ra.bgr = s.d_pre[0]; ra.windows = windows; ra.table = rect; ra.n = batch; ra.H = height; ra.W = width; ra.crop = crop; ra.resized = resized;
    launch_yv12_rectified_windows(ra, st);
  } else if (windows) {
    Yv12WinArgs wa; wa.in = yuv; wa.bgr = s.d_pre[0]; wa.windows = windows; wa.n = batch; wa.H = height; wa.W = width; wa.crop = crop;
    launch_yv12_windows(wa, st);
  } else {
    Yv12Args ya; ya.in = yuv; ya.bgr = s.d_pre[0]; ya.B = batch; ya.H = height; ya.W = width; ya.crop = crop;
    ya.ow = (width - crop) / 2; ya.oh = (height - crop) / 2;
    launch_yv12_crop(ya, st);
  }
  ResizeArgs r1; r1.in = s.d_pre[0]; r1.out = s.d_pre[1]; r1.B = batch; r1.H = crop; r1.W = crop; r1.nh = resized; r1.nw = resized; r1.S = resized; r1.norm = 0;
  r1.inv_scale_x = (double)crop / resized; r1.inv_scale_y = r1.inv_scale_x;
  launch_resize_u8(r1, st);
  // Program.cs:399-445 ResizeAndNormalizeMat on the square resized x resized frame: scale = (float)img_size / image_width
  const float scale = (float)s.size / (float)resized;
  ResizeArgs r2; r2.in = s.d_pre[1]; r2.out = out_hwc; r2.B = batch; r2.H = resized; r2.W = resized; r2.S = s.size; r2.norm = 1;
  r2.nw = s.size; r2.nh = (int)((float)resized * scale);
  if (r2.nh < 1 || r2.nh > s.size) return fail(HEP_ERR_UNSUPPORTED, "preprocess: resized frame does not fit the network size");
  r2.inv_scale_x = (double)resized / r2.nw; r2.inv_scale_y = (double)resized / r2.nh;
  launch_resize_u8(r2, st);
  HIPRET(hipGetLastError());
  return 0;
}

int hep_preprocess_i420_device(hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop, int resized,
                               float* out_hwc, void* stream) try {
  if (!h || !yuv || !out_hwc || batch < 1) return fail(HEP_ERR_INVALID, "bad argument");
  if (int rc = check_i420(height, width, crop, resized)) return rc;
  Session& s = h->s;
  HIPRET(hipSetDevice(s.device));
  std::lock_guard<std::mutex> lk(s.mu);
  return preprocess_i420_locked(s, yuv, batch, height, width, crop, resized, out_hwc, (hipStream_t)stream);
} HEP_CATCH_INT

int hep_preprocess_i420_windows_device(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n,
                                       int crop, int resized, float* out_hwc, void* stream) try {
  const Check c{"hep_preprocess_i420_windows_device: "};
  CHECKED(c.ptrs({{h, "handle"}, {yuv, "yuv"}, {windows, "windows"}, {out_hwc, "out_hwc"}}));
  CHECKED(c.at_least("frames", frames, 1)); CHECKED(check_i420(height, width, crop, resized));
  Session& s = h->s;      // (the handle is read from here on)
  CHECKED(c.range("n", n, 1, s.max_batch, HEP_ERR_INVALID, "max_batch given to hep_create"));
  HIPRET(hipSetDevice(s.device));
  std::lock_guard<std::mutex> lk(s.mu);
  return preprocess_i420_locked(s, yuv, n, height, width, crop, resized, out_hwc, (hipStream_t)stream, windows);
} HEP_CATCH_INT

int hep_preprocess_i420_rectified_device(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows,
                                         const double* table, int n, int crop, int resized, float* out_hwc, void* stream) try {
  const Check c{"hep_preprocess_i420_rectified_device: "};
  CHECKED(c.ptrs({{h, "handle"}, {yuv, "yuv"}, {windows, "windows"}, {table, "table"}, {out_hwc, "out_hwc"}}));
  CHECKED(c.at_least("frames", frames, 1)); CHECKED(check_i420(height, width, crop, resized));
  Session& s = h->s;      // (the handle is read from here on)
  CHECKED(c.range("n", n, 1, s.max_batch, HEP_ERR_INVALID, "max_batch given to hep_create"));
  HIPRET(hipSetDevice(s.device));
  std::lock_guard<std::mutex> lk(s.mu);
  return preprocess_i420_locked(s, yuv, n, height, width, crop, resized, out_hwc, (hipStream_t)stream, windows, table);
} HEP_CATCH_INT

// ---- decode / filter ----
// The *_locked helpers expect s.mu to be held; the device entry points take it around the launch, the host
// entry points around staging + launch + copy-back + synchronise, so that a concurrent call on the same handle
// (the C# frame callbacks re-enter from WebRTC worker threads) can never see another caller's staged tensors.
// Host inputs are staged in buffers of their own (d_stage), never in the forward's output buffers.
static int decode_locked(Session& s, const float* regression, const float* translation_raw, const float* camera, int batch,
                         float* boxes, float* translation, hipStream_t st) {
  DecodeArgs a;
  a.regression = regression ? regression : s.d_out[0];         // NULL = the handle's own last outputs
  a.translation_raw = translation_raw ? translation_raw : s.d_out[3];
  a.camera = camera; a.anchors = s.d_anchors; a.t_anchors = s.d_tanchors; a.boxes = boxes; a.translation = translation;
  a.B = batch; a.N = s.num_anchors; a.clip_max = (float)(s.size - 1);
  launch_decode(a, st);
  HIPRET(hipGetLastError());
  return 0;
}

int hep_decode_device(hep_handle* h, const float* regression, const float* translation_raw, const float* camera, int batch,
                      float* boxes, float* translation, void* stream) try {
  if (!h || !camera || !boxes || !translation) return fail(HEP_ERR_INVALID, "bad argument");
  Session& s = h->s;
  if (batch < 1 || batch > s.max_batch) return fail(HEP_ERR_UNSUPPORTED, "batch outside 1..max_batch");
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  return decode_locked(s, regression, translation_raw, camera, batch, boxes, translation, (hipStream_t)stream);
} HEP_CATCH_INT

static int ensure_post(Session& s) {
  const size_t n = (size_t)s.max_batch * s.num_anchors;
  if (!s.d_boxes) HIPRET(hipMalloc((void**)&s.d_boxes, n * 4 * 4));
  if (!s.d_trans) HIPRET(hipMalloc((void**)&s.d_trans, n * 3 * 4));
  if (!s.d_cam) HIPRET(hipMalloc((void**)&s.d_cam, (size_t)s.max_batch * 6 * 4));
  if (!s.d_keys) {
    s.npow2 = 1; while (s.npow2 < s.num_anchors) s.npow2 <<= 1;
    HIPRET(hipMalloc((void**)&s.d_keys, (size_t)s.max_batch * s.num_classes * s.npow2 * 8));
  }
  if (s.num_classes > 1 && !s.d_part) HIPRET(hipMalloc((void**)&s.d_part, (size_t)s.max_batch * s.num_classes * (FILTER_MAX_DET + 1) * 4));
  return 0;
}
// staging buffer i (0 regression .. 4 hand, same widths as the outputs) for host-side inputs
static int ensure_stage(Session& s, int i) {
  if (!s.d_stage[i]) HIPRET(hipMalloc((void**)&s.d_stage[i], (size_t)s.max_batch * s.num_anchors * s.out_k(i) * 4));
  return 0;
}

int hep_decode(hep_handle* h, const float* regression, const float* translation_raw, const float* camera, int batch,
               float* boxes, float* translation) try {
  if (!h || !camera || !boxes || !translation) return fail(HEP_ERR_INVALID, "bad argument");
  Session& s = h->s;
  if (batch < 1 || batch > s.max_batch) return fail(HEP_ERR_UNSUPPORTED, "batch outside 1..max_batch");
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  if (int rc = ensure_post(s)) return rc;
  const size_t n = (size_t)batch * s.num_anchors;
  const float *dreg = nullptr, *dtrn = nullptr;
  if (regression) {
    if (int rc = ensure_stage(s, 0)) return rc;
    HIPRET(hipMemcpyAsync(s.d_stage[0], regression, n * 16, hipMemcpyHostToDevice, s.stream)); dreg = s.d_stage[0];
  }
  if (translation_raw) {
    if (int rc = ensure_stage(s, 3)) return rc;
    HIPRET(hipMemcpyAsync(s.d_stage[3], translation_raw, n * 12, hipMemcpyHostToDevice, s.stream)); dtrn = s.d_stage[3];
  }
  HIPRET(hipMemcpyAsync(s.d_cam, camera, (size_t)batch * 24, hipMemcpyHostToDevice, s.stream));
  if (int rc = decode_locked(s, dreg, dtrn, s.d_cam, batch, s.d_boxes, s.d_trans, s.stream)) return rc;
  HIPRET(hipMemcpyAsync(boxes, s.d_boxes, n * 16, hipMemcpyDeviceToHost, s.stream));
  HIPRET(hipMemcpyAsync(translation, s.d_trans, n * 12, hipMemcpyDeviceToHost, s.stream));
  HIPRET(hipStreamSynchronize(s.stream));
  return 0;
} HEP_CATCH_INT

static int filter_locked(Session& s, const float* boxes, const float* classification, const float* rotation,
                         const float* translation, const float* hand, int batch, float score_threshold, float nms_threshold,
                         int max_detections, float* det_boxes, float* det_scores, int32_t* det_labels, float* det_rotation,
                         float* det_translation, float* det_hand, int32_t* det_index, int32_t* det_count, hipStream_t st) {
  if (int rc = ensure_post(s)) return rc;
  FilterArgs a;
  a.boxes = boxes; a.scores = classification ? classification : s.d_out[1];
  a.rotation = rotation ? rotation : s.d_out[2]; a.translation = translation ? translation : s.d_trans;
  a.hand = hand ? hand : s.d_out[4];
  a.B = batch; a.N = s.num_anchors; a.max_det = max_detections; a.score_thr = score_threshold; a.nms_thr = nms_threshold;
  a.keys = s.d_keys; a.npow2 = s.npow2;
  a.K = s.num_classes; a.any_class = s.class_specific_filter ? 0 : 1; a.part_idx = s.d_part; a.part_cnt = s.d_part ? s.d_part + (size_t)s.max_batch * s.num_classes * FILTER_MAX_DET : nullptr;
  a.det_boxes = det_boxes; a.det_scores = det_scores; a.det_labels = det_labels; a.det_rotation = det_rotation;
  a.det_translation = det_translation; a.det_hand = det_hand; a.det_index = det_index; a.det_count = det_count;
  launch_filter(a, st);
  HIPRET(hipGetLastError());
  return 0;
}

int hep_set_class_specific_filter(hep_handle* h, int on) try {
  if (!h) return fail(HEP_ERR_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(h->s.mu);
  h->s.class_specific_filter = on ? 1 : 0;
  return 0;
} HEP_CATCH_INT

int hep_filter_device(hep_handle* h, const float* boxes, const float* classification, const float* rotation,
                      const float* translation, const float* hand, int batch, float score_threshold, float nms_threshold,
                      int max_detections, float* det_boxes, float* det_scores, int32_t* det_labels, float* det_rotation,
                      float* det_translation, float* det_hand, int32_t* det_index, int32_t* det_count, void* stream) try {
  if (!h || !boxes || !det_count) return fail(HEP_ERR_INVALID, "bad argument");
  Session& s = h->s;
  if (batch < 1 || batch > s.max_batch) return fail(HEP_ERR_UNSUPPORTED, "batch outside 1..max_batch");
  if (max_detections < 1 || max_detections > 256) return fail(HEP_ERR_UNSUPPORTED, "max_detections must be in 1..256");
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  return filter_locked(s, boxes, classification, rotation, translation, hand, batch, score_threshold, nms_threshold, max_detections,
                       det_boxes, det_scores, det_labels, det_rotation, det_translation, det_hand, det_index, det_count, (hipStream_t)stream);
} HEP_CATCH_INT

int hep_filter(hep_handle* h, const float* boxes, const float* classification, const float* rotation, const float* translation,
               const float* hand, int batch, float score_threshold, float nms_threshold, int max_detections, float* det_boxes,
               float* det_scores, int32_t* det_labels, float* det_rotation, float* det_translation, float* det_hand,
               int32_t* det_index, int32_t* det_count) try {
  if (!h || !boxes || !classification || !rotation || !translation || !hand || !det_count) return fail(HEP_ERR_INVALID, "bad argument");
  Session& s = h->s;
  if (batch < 1 || batch > s.max_batch) return fail(HEP_ERR_UNSUPPORTED, "batch outside 1..max_batch");
  if (max_detections < 1 || max_detections > 256) return fail(HEP_ERR_UNSUPPORTED, "max_detections must be in 1..256");
  const size_t n = (size_t)batch * s.num_anchors, M = (size_t)batch * max_detections;
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  if (int rc = ensure_post(s)) return rc;
  for (int i = 0; i < 5; i++) if (int rc = ensure_stage(s, i)) return rc;
  const size_t need = (size_t)s.max_batch * 256 * (4 + 1 + 1 + 3 + 3 + 63 + 1) + s.max_batch;
  if (!s.d_det) { HIPRET(hipMalloc((void**)&s.d_det, need * 4)); s.det_floats = need; }
  float* d = s.d_det;
  // staged inputs: boxes -> stage 0 (same width as regression), scores 1, rotation 2, translation 3, hand 4
  HIPRET(hipMemcpyAsync(s.d_stage[0], boxes, n * 16, hipMemcpyHostToDevice, s.stream));
  HIPRET(hipMemcpyAsync(s.d_stage[1], classification, n * s.num_classes * 4, hipMemcpyHostToDevice, s.stream));
  HIPRET(hipMemcpyAsync(s.d_stage[2], rotation, n * 12, hipMemcpyHostToDevice, s.stream));
  HIPRET(hipMemcpyAsync(s.d_stage[3], translation, n * 12, hipMemcpyHostToDevice, s.stream));
  HIPRET(hipMemcpyAsync(s.d_stage[4], hand, n * 63 * 4, hipMemcpyHostToDevice, s.stream));
  float* b_ = d; float* sc_ = b_ + M * 4; int32_t* lb_ = (int32_t*)(sc_ + M); float* ro_ = (float*)(lb_ + M);
  float* tr_ = ro_ + M * 3; float* hd_ = tr_ + M * 3; int32_t* ix_ = (int32_t*)(hd_ + M * 63); int32_t* ct_ = ix_ + M;
  if (int rc = filter_locked(s, s.d_stage[0], s.d_stage[1], s.d_stage[2], s.d_stage[3], s.d_stage[4], batch, score_threshold, nms_threshold,
                             max_detections, b_, sc_, lb_, ro_, tr_, hd_, ix_, ct_, s.stream)) return rc;
  if (det_boxes) HIPRET(hipMemcpyAsync(det_boxes, b_, M * 16, hipMemcpyDeviceToHost, s.stream));
  if (det_scores) HIPRET(hipMemcpyAsync(det_scores, sc_, M * 4, hipMemcpyDeviceToHost, s.stream));
  if (det_labels) HIPRET(hipMemcpyAsync(det_labels, lb_, M * 4, hipMemcpyDeviceToHost, s.stream));
  if (det_rotation) HIPRET(hipMemcpyAsync(det_rotation, ro_, M * 12, hipMemcpyDeviceToHost, s.stream));
  if (det_translation) HIPRET(hipMemcpyAsync(det_translation, tr_, M * 12, hipMemcpyDeviceToHost, s.stream));
  if (det_hand) HIPRET(hipMemcpyAsync(det_hand, hd_, M * 63 * 4, hipMemcpyDeviceToHost, s.stream));
  if (det_index) HIPRET(hipMemcpyAsync(det_index, ix_, M * 4, hipMemcpyDeviceToHost, s.stream));
  HIPRET(hipMemcpyAsync(det_count, ct_, (size_t)batch * 4, hipMemcpyDeviceToHost, s.stream));
  HIPRET(hipStreamSynchronize(s.stream));
  return 0;
} HEP_CATCH_INT

// ---- top detection / frame to pose ----
static int top1_locked(Session& s, const float* regression, const float* classification, const float* rotation,
                       const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                       uint32_t* records, hipStream_t st, bool per_label = false) {
  Top1Args a;
  a.regression = regression ? regression : s.d_out[0];         // NULL = the handle's own last outputs
  a.scores = classification ? classification : s.d_out[1];
  a.rotation = rotation ? rotation : s.d_out[2];
  a.translation_raw = translation_raw ? translation_raw : s.d_out[3];
  a.hand = hand ? hand : s.d_out[4];
  a.camera = camera; a.anchors = s.d_anchors; a.t_anchors = s.d_tanchors;
  a.B = batch; a.N = s.num_anchors; a.K = s.num_classes; a.any_class = s.class_specific_filter ? 0 : 1;
  a.score_thr = score_threshold; a.clip_max = (float)(s.size - 1);
  a.records = records;                                         // per_label: [batch][num_classes] records, class-specific whatever the handle's mode
  if (per_label) launch_toplabel(a, st); else launch_top1(a, st);
  HIPRET(hipGetLastError());
  return 0;
}

// the body of hep_top1_device and hep_top_labels_device: `who` is the prefix of the entry point's messages
static int top_device(const char* who, bool per_label, hep_handle* h, const float* regression, const float* classification, const float* rotation,
                      const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                      uint32_t* records, void* stream) {
  const Check c{who};
  CHECKED(c.ptrs({{h, "handle"}, {camera, "camera"}, {records, "records"}}));      // (the handle is not read before the pointers are checked)
  Session& s = h->s; CHECKED(c.range("batch", batch, 1, s.max_batch, HEP_ERR_INVALID, "max_batch"));
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  return top1_locked(s, regression, classification, rotation, translation_raw, hand, camera, batch, score_threshold, records, (hipStream_t)stream, per_label);
}

int hep_top1_device(hep_handle* h, const float* regression, const float* classification, const float* rotation,
                    const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                    uint32_t* records, void* stream) try {
  return top_device("hep_top1_device: ", false, h, regression, classification, rotation, translation_raw, hand, camera, batch, score_threshold, records, stream);
} HEP_CATCH_INT

int hep_top_labels_device(hep_handle* h, const float* regression, const float* classification, const float* rotation,
                          const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                          uint32_t* records, void* stream) try {
  return top_device("hep_top_labels_device: ", true, h, regression, classification, rotation, translation_raw, hand, camera, batch, score_threshold, records, stream);
} HEP_CATCH_INT

namespace {
struct PoseOut { int32_t* found; float* scores; int32_t* labels; int32_t* index; float* boxes; float* rotation; float* translation; float* hand; };
constexpr size_t kRecBytes = (size_t)HEP_POSE_RECORD_WORDS * 4;
static_assert(HEP_POSE_RECORD_WORDS == POSE_RECORD_WORDS, "the record of include/hep.h is the kernel's");
}  // namespace

// what the host entry points refuse first, without reading the handle: NULL pointers and a batch below 1 (check_pose); then, behind the frame
// geometry where there is one, the batch against the handle's max_batch (check_pose_batch)
static int check_pose_batch(const Check& c, int batch, int most) { return c.range("batch", batch, 1, most, HEP_ERR_INVALID, "max_batch given to hep_create"); }
static int check_pose(const Check& c, const hep_handle* h, const void* input, const char* input_name, int batch, const float* camera, const int32_t* found) {
  CHECKED(c.ptrs({{h, "handle"}, {input, input_name}, {camera, "camera"}, {found, "found"}}));
  return check_pose_batch(c, batch, INT_MAX);
}

// Staging of one call: [camera rows, padded to cam_pad bytes | payload] on the device.  Direct (the default): two hipMemcpyAsync from
// the caller's pageable memory.  Pinned (HEP_POSE_UPLOAD=pinned, kept for the A/B of tools/pose_call_time.py): camera and payload are
// copied into a pinned buffer of the handle and go up as ONE hipMemcpyAsync.  Measured twice (NOTEBOOK.md section 24): the 3 MB float
// blob is 0.05 ms faster direct (the host copy into the pinned buffer costs more than the runtime's own staging), the 1.4 MB frame
// 0.02 ms faster back to back and level at 60 Hz.  Buffers are sized for max_batch payloads of this call's per-image size and only
// ever grown: a repeated shape allocates nothing.
static size_t pose_cam_pad(const Session& s) { return ((size_t)s.max_batch * 24 + 255) & ~(size_t)255; }
// the buffers of a call that stages `need` bytes
static int pose_reserve(Session& s, size_t need) {
  if (!s.d_rec) {
    const char* e = getenv("HEP_POSE_UPLOAD");
    s.pose_upload_pinned = e && !strcmp(e, "pinned");
    HIPRET(hipMalloc((void**)&s.d_rec, kRecBytes * s.max_batch));
  }
  const bool direct = !s.pose_upload_pinned;
  if (!s.h_rec) HIPRET(hipHostMalloc((void**)&s.h_rec, kRecBytes * s.max_batch, hipHostMallocDefault));
  if (s.pose_in_bytes < need) {
    HIPRET(hipStreamSynchronize(s.stream));
    hipFree(s.d_pose_in); s.d_pose_in = nullptr; s.pose_in_bytes = 0;
    HIPRET(hipMalloc((void**)&s.d_pose_in, need)); s.pose_in_bytes = need;
  }
  if (!direct && s.pose_pin_bytes < need) {
    HIPRET(hipStreamSynchronize(s.stream));
    hipHostFree(s.h_pose_in); s.h_pose_in = nullptr; s.pose_pin_bytes = 0;
    HIPRET(hipHostMalloc((void**)&s.h_pose_in, need, hipHostMallocDefault)); s.pose_pin_bytes = need;
  }
  return 0;
}
static int pose_stage(Session& s, const void* payload, size_t per_image, int batch, const float* camera) {
  const size_t pad = pose_cam_pad(s);
  if (int rc = pose_reserve(s, pad + per_image * (size_t)s.max_batch)) return rc;
  const bool direct = !s.pose_upload_pinned;
  const size_t bytes = per_image * (size_t)batch;
  if (direct) {
    HIPRET(hipMemcpyAsync(s.d_pose_in, camera, (size_t)batch * 24, hipMemcpyHostToDevice, s.stream));
    HIPRET(hipMemcpyAsync(s.d_pose_in + pad, payload, bytes, hipMemcpyHostToDevice, s.stream));
  } else {
    memcpy(s.h_pose_in, camera, (size_t)batch * 24);
    memcpy(s.h_pose_in + pad, payload, bytes);
    HIPRET(hipMemcpyAsync(s.d_pose_in, s.h_pose_in, pad + bytes, hipMemcpyHostToDevice, s.stream));
  }
  return 0;
}

// the handle's buffers for num_classes records per image (hep_poses_from_*): allocated at the first such call for max_batch images - the
// size never changes for a handle, so nothing is allocated or freed afterwards
static int poses_buffers(Session& s) {
  const size_t need = kRecBytes * s.max_batch * s.num_classes;
  if (!s.d_recs) HIPRET(hipMalloc((void**)&s.d_recs, need));
  if (!s.h_recs) HIPRET(hipHostMalloc((void**)&s.h_recs, need, hipHostMallocDefault));
  return 0;
}

// the records of a download -> the caller's arrays, row by row
static void pose_scatter(const uint32_t* hr, int rows, const PoseOut& o) {
  for (int b = 0; b < rows; b++) {
    const uint32_t* r = hr + (size_t)b * HEP_POSE_RECORD_WORDS;
    memcpy(&o.found[b], r + 0, 4);
    if (o.labels) memcpy(&o.labels[b], r + 1, 4);
    if (o.index) memcpy(&o.index[b], r + 2, 4);
    if (o.scores) memcpy(&o.scores[b], r + 4, 4);
    if (o.boxes) memcpy(o.boxes + (size_t)b * 4, r + 5, 16);
    if (o.rotation) memcpy(o.rotation + (size_t)b * 3, r + 9, 12);
    if (o.translation) memcpy(o.translation + (size_t)b * 3, r + 12, 12);
    if (o.hand) memcpy(o.hand + (size_t)b * 63, r + 15, 63 * 4);
  }
}

// top-detection launch on the handle's own head outputs, the records back through the pinned buffer, synchronise, scatter.
// per_label (hep_poses_from_*): the launch of hep_top_labels_device, num_classes records per image, output row b * num_classes + c
static int pose_finish(Session& s, int batch, float score_threshold, const PoseOut& o, bool per_label) {
  uint32_t* d = per_label ? s.d_recs : s.d_rec;
  uint32_t* hr = per_label ? s.h_recs : s.h_rec;
  const int rows = per_label ? batch * s.num_classes : batch;
  if (int rc = top1_locked(s, nullptr, nullptr, nullptr, nullptr, nullptr, (const float*)s.d_pose_in, batch, score_threshold, d, s.stream, per_label)) return rc;
  HIPRET(hipMemcpyAsync(hr, d, kRecBytes * rows, hipMemcpyDeviceToHost, s.stream));
  HIPRET(hipStreamSynchronize(s.stream));
  pose_scatter(hr, rows, o);
  return 0;
}

// the bodies of hep_pose_from_input / hep_poses_from_input and of hep_pose_from_i420 / hep_poses_from_i420: `who` is the prefix of the entry point's messages
static int pose_from_input(const char* who, bool per_label, hep_handle* h, const float* input_nchw, int batch, const float* camera,
                           float score_threshold, const PoseOut& o) {
  const Check c{who};
  CHECKED(check_pose(c, h, input_nchw, "input_nchw", batch, camera, o.found)); CHECKED(check_pose_batch(c, batch, h->s.max_batch));
  Session& s = h->s;
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  if (per_label) if (int rc = poses_buffers(s)) return rc;
  if (int rc = pose_stage(s, input_nchw, (size_t)3 * s.size * s.size * 4, batch, camera)) return rc;
  std::string err;
  if (int rc = run_forward(&s, (const float*)(s.d_pose_in + pose_cam_pad(s)), nullptr, batch, s.stream, &err)) return fail(rc, err);
  return pose_finish(s, batch, score_threshold, o, per_label);
}
static int pose_from_i420(const char* who, bool per_label, hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop,
                          int resized, const float* camera, float score_threshold, const PoseOut& o) {
  const Check c{who};
  CHECKED(check_pose(c, h, yuv, "yuv", batch, camera, o.found)); CHECKED(check_i420(height, width, crop, resized)); CHECKED(check_pose_batch(c, batch, h->s.max_batch));
  Session& s = h->s;
  {   // ResizeAndNormalizeMat's row count (preprocess_i420_locked computes the same): refused here, before any HIP call
    const int nh = (int)((float)resized * ((float)s.size / (float)resized));
    if (nh < 1 || nh > s.size) return fail(HEP_ERR_UNSUPPORTED, "preprocess: resized frame does not fit the network size");
  }
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  const size_t in_floats = (size_t)3 * s.size * s.size;
  if (!s.d_in) HIPRET(hipMalloc((void**)&s.d_in, in_floats * s.max_batch * 4));
  if (per_label) if (int rc = poses_buffers(s)) return rc;
  if (int rc = pose_stage(s, yuv, (size_t)height * width * 3 / 2, batch, camera)) return rc;
  if (int rc = preprocess_i420_locked(s, s.d_pose_in + pose_cam_pad(s), batch, height, width, crop, resized, s.d_in, s.stream)) return rc;
  const int64_t S = s.size; const int64_t nhwc[4] = {3 * S * S, 1, 3 * S, 3};      // the NCHW view of the [batch,S,S,3] frames
  std::string err;
  if (int rc = run_forward(&s, s.d_in, nhwc, batch, s.stream, &err)) return fail(rc, err);
  return pose_finish(s, batch, score_threshold, o, per_label);
}

int hep_pose_from_input(hep_handle* h, const float* input_nchw, int batch, const float* camera, float score_threshold,
                        int32_t* found, float* scores, int32_t* labels, int32_t* index, float* boxes, float* rotation,
                        float* translation, float* hand) try {
  return pose_from_input("hep_pose_from_input: ", false, h, input_nchw, batch, camera, score_threshold,
                         PoseOut{found, scores, labels, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

int hep_pose_from_i420(hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop, int resized,
                       const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels,
                       int32_t* index, float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420("hep_pose_from_i420: ", false, h, yuv, batch, height, width, crop, resized, camera, score_threshold,
                        PoseOut{found, scores, labels, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

// several objects: [batch][num_classes] rows per output, slot c = label c (no labels array)
int hep_poses_from_input(hep_handle* h, const float* input_nchw, int batch, const float* camera, float score_threshold,
                         int32_t* found, float* scores, int32_t* index, float* boxes, float* rotation, float* translation,
                         float* hand) try {
  return pose_from_input("hep_poses_from_input: ", true, h, input_nchw, batch, camera, score_threshold,
                         PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

int hep_poses_from_i420(hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop, int resized,
                        const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index, float* boxes,
                        float* rotation, float* translation, float* hand) try {
  return pose_from_i420("hep_poses_from_i420: ", true, h, yuv, batch, height, width, crop, resized, camera, score_threshold,
                        PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

// ---- whole-frame search: windows of a frame, best of the windows (include/hep.h) ----
// a grid offset along one axis: span = side - crop; one cell sits at the centre (the frame path's crop), several reach both borders
static int tile_offset(int i, int cells, int span) { return cells == 1 ? span / 2 : (int)(((int64_t)i * span) / (cells - 1)); }
static void tile_windows(int height, int width, int crop, int nx, int ny, int frames, int32_t* w) {
  for (int f = 0; f < frames; f++)
    for (int r = 0; r < ny; r++)
      for (int i = 0; i < nx; i++, w += 3) { w[0] = f; w[1] = tile_offset(i, nx, width - crop); w[2] = tile_offset(r, ny, height - crop); }
}
// camera row of window {frame, ox, oy}: the frame's row with the principal point moved by the window's offset from the centre crop, in pixels
// of the resized image; every rounding stated (tests/_windows.py restates it)
static void window_camera(const float* camera, const int32_t* w, int height, int width, int crop, int resized, float* out) {
  const float* row = camera + (size_t)w[0] * 6;
  memcpy(out, row, 24);
  out[2] = (float)((double)row[2] - (double)(w[1] - (width - crop) / 2) * (double)resized / (double)crop);
  out[3] = (float)((double)row[3] - (double)(w[2] - (height - crop) / 2) * (double)resized / (double)crop);
}
// a host table: every window inside its frame; frames < 0: the frame index has no upper limit to hold (hep_window_cameras)
static int check_windows(const Check& c, const int32_t* windows, int n, int frames, int height, int width, int crop) {
  for (int i = 0; i < n; i++) {
    const int32_t* w = windows + (size_t)i * 3;
    if (w[0] < 0 || (frames >= 0 && w[0] >= frames) || w[1] < 0 || w[1] > width - crop || w[2] < 0 || w[2] > height - crop)
      return c.fail(HEP_ERR_INVALID, "window " + std::to_string(i) + " {" + std::to_string(w[0]) + ", " + std::to_string(w[1]) + ", " + std::to_string(w[2]) +
                                     "} lies outside the frame (frame index or offsets)");
  }
  return 0;
}

int hep_tile_windows(int height, int width, int crop, int nx, int ny, int frames, int32_t* windows_out) try {
  const Check c{"hep_tile_windows: "};
  CHECKED(c.ptrs({{windows_out, "windows_out"}}));
  CHECKED(c.at_least("nx", nx, 1)); CHECKED(c.at_least("ny", ny, 1)); CHECKED(c.at_least("frames", frames, 1));
  CHECKED(check_i420(height, width, crop, 1));
  tile_windows(height, width, crop, nx, ny, frames, windows_out);
  return 0;
} HEP_CATCH_INT

int hep_window_cameras(const float* camera, const int32_t* windows, int n, int height, int width, int crop, int resized, float* camera_out) try {
  const Check c{"hep_window_cameras: "};
  CHECKED(c.ptrs({{camera, "camera"}, {windows, "windows"}, {camera_out, "camera_out"}}));
  CHECKED(c.at_least("n", n, 1)); CHECKED(check_i420(height, width, crop, resized)); CHECKED(check_windows(c, windows, n, -1, height, width, crop));
  for (int i = 0; i < n; i++) window_camera(camera, windows + (size_t)i * 3, height, width, crop, resized, camera_out + (size_t)i * 6);
  return 0;
} HEP_CATCH_INT

int hep_window_from_box(const float* box, int ox, int oy, int height, int width, int crop, int size, int32_t* ox_out, int32_t* oy_out) try {
  const Check c{"hep_window_from_box: "};
  CHECKED(c.ptrs({{box, "box"}, {ox_out, "ox_out"}, {oy_out, "oy_out"}}));
  CHECKED(check_i420(height, width, crop, 1)); CHECKED(c.at_least("size", size, 1));
  const int32_t w[3] = {0, ox, oy};
  CHECKED(check_windows(c, w, 1, 1, height, width, crop));
  // the centre of the box in frame pixels, then the window around it, kept inside the frame (compared in double: no cast of a value an int cannot hold)
  auto around = [&](int o, float lo, float hi, int side) {
    const double centre = (double)o + 0.5 * ((double)lo + (double)hi) * (double)crop / (double)size;
    const double v = floor(centre - 0.5 * (double)crop + 0.5);
    return !(v > 0.0) ? 0 : (v > (double)(side - crop) ? side - crop : (int)v);
  };
  *ox_out = around(ox, box[0], box[2], width); *oy_out = around(oy, box[1], box[3], height);
  return 0;
} HEP_CATCH_INT

int hep_best_window_device(const uint32_t* records, int slots, const int32_t* windows, int n, int frames, uint32_t* out_records,
                           int32_t* out_window, void* stream) try {
  const Check c{"hep_best_window_device: "};
  CHECKED(c.ptrs({{records, "records"}, {windows, "windows"}, {out_records, "out_records"}, {out_window, "out_window"}}));
  CHECKED(c.range("slots", slots, 1, 63)); CHECKED(c.at_least("n", n, 1)); CHECKED(c.range("frames", frames, 1, INT_MAX / 64));
  BestWindowArgs a; a.records = records; a.windows = windows; a.out_records = out_records; a.out_window = out_window; a.n = n; a.slots = slots; a.frames = frames;
  launch_best_window(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

// rectified windows: the host arithmetic is hep_rectify.cpp's (built without contraction), the checks are here
static_assert(HEP_RECTIFY_ROW_DOUBLES == RECTIFY_ROW_DOUBLES, "the table row of include/hep.h and of the kernels");
// every window's frame has a camera row whose focal lengths are finite and positive
static int check_rectify_camera(const Check& c, const float* camera, const int32_t* windows, int n) {
  for (int i = 0; i < n; i++) {
    const float* row = camera + (size_t)windows[(size_t)i * 3] * 6;
    if (!(row[0] > 0.f && row[0] <= FLT_MAX && row[1] > 0.f && row[1] <= FLT_MAX))
      return c.fail(HEP_ERR_INVALID, "camera row " + std::to_string(windows[(size_t)i * 3]) + ": fx and fy must be finite and positive");
  }
  return 0;
}
static int check_rectify_row(const Check& c, const double* row) {
  return row[9] > 0.0 && row[9] <= DBL_MAX && row[10] > 0.0 && row[10] <= DBL_MAX ? 0 : c.fail(HEP_ERR_INVALID, "row: fx and fy must be finite and positive");
}

int hep_rectify_windows(const float* camera, int frames, const int32_t* windows, int n, int height, int width, int crop, int resized,
                        double* table_out) try {
  const Check c{"hep_rectify_windows: "};
  CHECKED(c.ptrs({{camera, "camera"}, {windows, "windows"}, {table_out, "table_out"}}));
  CHECKED(c.at_least("frames", frames, 1)); CHECKED(c.at_least("n", n, 1)); CHECKED(check_i420(height, width, crop, resized));
  CHECKED(check_windows(c, windows, n, frames, height, width, crop)); CHECKED(check_rectify_camera(c, camera, windows, n));
  for (int i = 0; i < n; i++)
    rectify_row(camera + (size_t)windows[(size_t)i * 3] * 6, windows + (size_t)i * 3, height, width, crop, resized, table_out + (size_t)i * HEP_RECTIFY_ROW_DOUBLES);
  return 0;
} HEP_CATCH_INT

int hep_rectified_point_to_frame(const double* row, double x, double y, int height, int width, int crop, int resized, int size, double* xy_out) try {
  const Check c{"hep_rectified_point_to_frame: "};
  CHECKED(c.ptrs({{row, "row"}, {xy_out, "xy_out"}}));
  CHECKED(check_i420(height, width, crop, resized)); CHECKED(c.at_least("size", size, 1)); CHECKED(check_rectify_row(c, row));
  rectified_point(row, x, y, height, width, crop, resized, size, xy_out);
  return 0;
} HEP_CATCH_INT

int hep_window_from_box_rectified(const double* row, const float* box, int height, int width, int crop, int resized, int size, int32_t* ox_out,
                                  int32_t* oy_out) try {
  const Check c{"hep_window_from_box_rectified: "};
  CHECKED(c.ptrs({{row, "row"}, {box, "box"}, {ox_out, "ox_out"}, {oy_out, "oy_out"}}));
  CHECKED(check_i420(height, width, crop, resized)); CHECKED(c.at_least("size", size, 1)); CHECKED(check_rectify_row(c, row));
  double xy[2];
  rectified_point(row, 0.5 * ((double)box[0] + (double)box[2]), 0.5 * ((double)box[1] + (double)box[3]), height, width, crop, resized, size, xy);
  // the window around that frame position, kept inside the frame as hep_window_from_box keeps it (a NaN - a ray that points backwards - gives 0)
  auto around = [&](double centre, int side) {
    const double v = floor(centre - 0.5 * (double)crop + 0.5);
    return !(v > 0.0) ? 0 : (v > (double)(side - crop) ? side - crop : (int)v);
  };
  *ox_out = around(xy[0], width); *oy_out = around(xy[1], height);
  return 0;
} HEP_CATCH_INT

int hep_derotate_records_device(uint32_t* records, int slots, const double* table, int n, void* stream) try {
  const Check c{"hep_derotate_records_device: "};
  CHECKED(c.ptrs({{records, "records"}, {table, "table"}}));
  CHECKED(c.range("slots", slots, 1, 63)); CHECKED(c.range("n", n, 1, INT_MAX / 64));
  DerotateArgs a; a.records = records; a.table = table; a.n = n; a.slots = slots;
  launch_derotate_records(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

// the handle's buffers for the winners of hep_pose(s)_from_i420_tiled: records and window indices of max_batch x num_classes rows, one size for both calls
static int best_buffers(Session& s) {
  const size_t need = (kRecBytes + 4) * s.max_batch * s.num_classes;
  if (!s.d_best) HIPRET(hipMalloc((void**)&s.d_best, need));
  if (!s.h_best) HIPRET(hipHostMalloc((void**)&s.h_best, need, hipHostMallocDefault));
  return 0;
}

// The body of the windowed host calls; every argument has been checked and s.mu is held.  Staging: [camera rows of the windows, padded | table,
// padded | frames] in the buffer hep_pose_from_i420 stages in, sized for max_batch frames of this geometry and only ever grown; then the
// windowed preprocess, one forward at batch n and the top-detection launch.  window_out == NULL: the n (x num_classes) records come back as
// they are.  Otherwise the best-of-windows launch follows and `frames` (x num_classes) winners with their window indices come back in one copy.
// rect != NULL (the *_rectified calls): the host table [n][HEP_RECTIFY_ROW_DOUBLES] goes up between the window table and the frames, the
// rectified preprocess takes the place of the windowed one, `camera` holds every window's frame's CENTRE row and the back-rotation launch
// follows the top-detection launch.
static int pose_from_windows_locked(Session& s, bool per_label, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n,
                                    int crop, int resized, const float* camera, float score_threshold, const PoseOut& o, int32_t* window_out,
                                    const double* rect = nullptr) {
  HIPRET(hipSetDevice(s.device));
  const size_t in_floats = (size_t)3 * s.size * s.size;
  if (!s.d_in) HIPRET(hipMalloc((void**)&s.d_in, in_floats * s.max_batch * 4));
  if (per_label) if (int rc = poses_buffers(s)) return rc;
  if (window_out) if (int rc = best_buffers(s)) return rc;
  const size_t pad = pose_cam_pad(s), tpad = ((size_t)s.max_batch * 12 + 255) & ~(size_t)255, per_frame = (size_t)height * width * 3 / 2;
  const size_t row_bytes = HEP_RECTIFY_ROW_DOUBLES * sizeof(double), rpad = rect ? ((size_t)s.max_batch * row_bytes + 255) & ~(size_t)255 : 0;
  if (int rc = pose_reserve(s, pad + tpad + rpad + per_frame * (size_t)s.max_batch)) return rc;
  if (!s.pose_upload_pinned) {
    HIPRET(hipMemcpyAsync(s.d_pose_in, camera, (size_t)n * 24, hipMemcpyHostToDevice, s.stream));
    HIPRET(hipMemcpyAsync(s.d_pose_in + pad, windows, (size_t)n * 12, hipMemcpyHostToDevice, s.stream));
    if (rect) HIPRET(hipMemcpyAsync(s.d_pose_in + pad + tpad, rect, (size_t)n * row_bytes, hipMemcpyHostToDevice, s.stream));
    HIPRET(hipMemcpyAsync(s.d_pose_in + pad + tpad + rpad, yuv, per_frame * frames, hipMemcpyHostToDevice, s.stream));
  } else {
    memcpy(s.h_pose_in, camera, (size_t)n * 24);
    memcpy(s.h_pose_in + pad, windows, (size_t)n * 12);
    if (rect) memcpy(s.h_pose_in + pad + tpad, rect, (size_t)n * row_bytes);
    memcpy(s.h_pose_in + pad + tpad + rpad, yuv, per_frame * frames);
    HIPRET(hipMemcpyAsync(s.d_pose_in, s.h_pose_in, pad + tpad + rpad + per_frame * frames, hipMemcpyHostToDevice, s.stream));
  }
  const int32_t* d_table = (const int32_t*)(s.d_pose_in + pad);
  const double* d_rect = rect ? (const double*)(s.d_pose_in + pad + tpad) : nullptr;      // (256-byte aligned)
  if (int rc = preprocess_i420_locked(s, s.d_pose_in + pad + tpad + rpad, n, height, width, crop, resized, s.d_in, s.stream, d_table, d_rect)) return rc;
  const int64_t S = s.size; const int64_t nhwc[4] = {3 * S * S, 1, 3 * S, 3};      // the NCHW view of the [n,S,S,3] windows
  std::string err;
  if (int rc = run_forward(&s, s.d_in, nhwc, n, s.stream, &err)) return fail(rc, err);
  if (!window_out && !rect) return pose_finish(s, n, score_threshold, o, per_label);
  uint32_t* d = per_label ? s.d_recs : s.d_rec;
  if (int rc = top1_locked(s, nullptr, nullptr, nullptr, nullptr, nullptr, (const float*)s.d_pose_in, n, score_threshold, d, s.stream, per_label)) return rc;
  const int slots = per_label ? s.num_classes : 1, rows = frames * slots;
  if (rect) {
    DerotateArgs da; da.records = d; da.table = d_rect; da.n = n; da.slots = slots;
    launch_derotate_records(da, s.stream);
    HIPRET(hipGetLastError());
  }
  if (!window_out) {                                  // the rectified windows call: the n (x num_classes) back-rotated records as they are
    uint32_t* hr = per_label ? s.h_recs : s.h_rec;
    HIPRET(hipMemcpyAsync(hr, d, kRecBytes * n * slots, hipMemcpyDeviceToHost, s.stream));
    HIPRET(hipStreamSynchronize(s.stream));
    pose_scatter(hr, n * slots, o);
    return 0;
  }
  BestWindowArgs a; a.records = d; a.windows = d_table; a.out_records = s.d_best; a.out_window = (int32_t*)(s.d_best + (size_t)rows * HEP_POSE_RECORD_WORDS);
  a.n = n; a.slots = slots; a.frames = frames;
  launch_best_window(a, s.stream);
  HIPRET(hipGetLastError());
  HIPRET(hipMemcpyAsync(s.h_best, s.d_best, (kRecBytes + 4) * rows, hipMemcpyDeviceToHost, s.stream));
  HIPRET(hipStreamSynchronize(s.stream));
  pose_scatter(s.h_best, rows, o);
  memcpy(window_out, s.h_best + (size_t)rows * HEP_POSE_RECORD_WORDS, (size_t)rows * 4);
  return 0;
}
// ResizeAndNormalizeMat's row count (preprocess_i420_locked computes the same): refused before any HIP call
static int check_fits(const Session& s, int resized) {
  const int nh = (int)((float)resized * ((float)s.size / (float)resized));
  return nh < 1 || nh > s.size ? fail(HEP_ERR_UNSUPPORTED, "preprocess: resized frame does not fit the network size") : 0;
}

// the host tables of the tiled and of the rectified calls, built under the mutex: sized once, max_batch rows
static void win_buffers(Session& s) {
  if (s.win_table.empty()) { s.win_table.resize((size_t)s.max_batch * 3); s.win_cam.resize((size_t)s.max_batch * 6); s.win_rect.resize((size_t)s.max_batch * HEP_RECTIFY_ROW_DOUBLES); }
}
// the rectified calls' host side: s.win_cam = every window's frame's centre row as it is, s.win_rect = the table of hep_rectify_windows
static void rectify_tables(Session& s, const float* camera, const int32_t* windows, int n, int height, int width, int crop, int resized) {
  for (int i = 0; i < n; i++) {
    const float* row = camera + (size_t)windows[(size_t)i * 3] * 6;
    memcpy(s.win_cam.data() + (size_t)i * 6, row, 24);
    rectify_row(row, windows + (size_t)i * 3, height, width, crop, resized, s.win_rect.data() + (size_t)i * HEP_RECTIFY_ROW_DOUBLES);
  }
}

// rectified: camera is [frames,6], the centre rows
static int pose_from_i420_windows(const char* who, bool per_label, hep_handle* h, const uint8_t* yuv, int frames, int height, int width,
                                  const int32_t* windows, int n, int crop, int resized, const float* camera, float score_threshold, const PoseOut& o,
                                  bool rectified = false) {
  const Check c{who};
  CHECKED(c.ptrs({{h, "handle"}, {yuv, "yuv"}, {windows, "windows"}, {camera, "camera"}, {o.found, "found"}}));
  CHECKED(c.range("n", n, 1, INT_MAX, HEP_ERR_INVALID, "max_batch given to hep_create")); CHECKED(c.at_least("frames", frames, 1));
  CHECKED(check_i420(height, width, crop, resized)); CHECKED(check_windows(c, windows, n, frames, height, width, crop));
  if (rectified) CHECKED(check_rectify_camera(c, camera, windows, n));
  Session& s = h->s;      // (the handle is read from here on)
  CHECKED(c.range("n", n, 1, s.max_batch, HEP_ERR_INVALID, "max_batch given to hep_create"));
  CHECKED(c.range("frames", frames, 1, s.max_batch, HEP_ERR_INVALID, "max_batch given to hep_create")); CHECKED(check_fits(s, resized));
  std::lock_guard<std::mutex> lk(s.mu);
  if (rectified) {
    win_buffers(s);
    rectify_tables(s, camera, windows, n, height, width, crop, resized);
    return pose_from_windows_locked(s, per_label, yuv, frames, height, width, windows, n, crop, resized, s.win_cam.data(), score_threshold, o, nullptr, s.win_rect.data());
  }
  return pose_from_windows_locked(s, per_label, yuv, frames, height, width, windows, n, crop, resized, camera, score_threshold, o, nullptr);
}

static int pose_from_i420_tiled(const char* who, bool per_label, hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop,
                                int resized, int nx, int ny, const float* camera, float score_threshold, const PoseOut& o, int32_t* window,
                                bool rectified = false) {
  const Check c{who};
  CHECKED(c.ptrs({{h, "handle"}, {yuv, "yuv"}, {camera, "camera"}, {o.found, "found"}, {window, "window"}}));
  CHECKED(c.at_least("nx", nx, 1)); CHECKED(c.at_least("ny", ny, 1)); CHECKED(c.at_least("frames", frames, 1));
  CHECKED(check_i420(height, width, crop, resized));
  Session& s = h->s;      // (the handle is read from here on)
  int64_t n = (int64_t)nx * ny;                     // (two factors at a time: neither product can pass int64)
  if (n <= s.max_batch) n *= frames;
  if (n > s.max_batch) return c.fail(HEP_ERR_INVALID, "frames * nx * ny outside 1..max_batch given to hep_create");
  CHECKED(check_fits(s, resized));
  if (rectified)
    for (int f = 0; f < frames; f++) { const int32_t w[3] = {f, 0, 0}; CHECKED(check_rectify_camera(c, camera, w, 1)); }
  std::lock_guard<std::mutex> lk(s.mu);
  win_buffers(s);
  tile_windows(height, width, crop, nx, ny, frames, s.win_table.data());
  if (rectified) {
    rectify_tables(s, camera, s.win_table.data(), (int)n, height, width, crop, resized);
    return pose_from_windows_locked(s, per_label, yuv, frames, height, width, s.win_table.data(), (int)n, crop, resized, s.win_cam.data(), score_threshold, o, window,
                                    s.win_rect.data());
  }
  for (int i = 0; i < (int)n; i++) window_camera(camera, s.win_table.data() + (size_t)i * 3, height, width, crop, resized, s.win_cam.data() + (size_t)i * 6);
  return pose_from_windows_locked(s, per_label, yuv, frames, height, width, s.win_table.data(), (int)n, crop, resized, s.win_cam.data(), score_threshold, o, window);
}

int hep_pose_from_i420_windows(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                               int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels,
                               int32_t* index, float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420_windows("hep_pose_from_i420_windows: ", false, h, yuv, frames, height, width, windows, n, crop, resized, camera, score_threshold,
                                PoseOut{found, scores, labels, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

int hep_poses_from_i420_windows(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                                int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index,
                                float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420_windows("hep_poses_from_i420_windows: ", true, h, yuv, frames, height, width, windows, n, crop, resized, camera, score_threshold,
                                PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand});
} HEP_CATCH_INT

int hep_pose_from_i420_tiled(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                             const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels, int32_t* index,
                             float* boxes, float* rotation, float* translation, float* hand, int32_t* window) try {
  return pose_from_i420_tiled("hep_pose_from_i420_tiled: ", false, h, yuv, frames, height, width, crop, resized, nx, ny, camera, score_threshold,
                              PoseOut{found, scores, labels, index, boxes, rotation, translation, hand}, window);
} HEP_CATCH_INT

int hep_poses_from_i420_tiled(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                              const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index, float* boxes,
                              float* rotation, float* translation, float* hand, int32_t* window) try {
  return pose_from_i420_tiled("hep_poses_from_i420_tiled: ", true, h, yuv, frames, height, width, crop, resized, nx, ny, camera, score_threshold,
                              PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand}, window);
} HEP_CATCH_INT

// the rectified forms of the four calls above (include/hep.h): camera is [frames,6], the centre rows, for all four
int hep_pose_from_i420_windows_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                                         int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels,
                                         int32_t* index, float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420_windows("hep_pose_from_i420_windows_rectified: ", false, h, yuv, frames, height, width, windows, n, crop, resized, camera, score_threshold,
                                PoseOut{found, scores, labels, index, boxes, rotation, translation, hand}, true);
} HEP_CATCH_INT

int hep_poses_from_i420_windows_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                                          int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index,
                                          float* boxes, float* rotation, float* translation, float* hand) try {
  return pose_from_i420_windows("hep_poses_from_i420_windows_rectified: ", true, h, yuv, frames, height, width, windows, n, crop, resized, camera, score_threshold,
                                PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand}, true);
} HEP_CATCH_INT

int hep_pose_from_i420_tiled_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                                       const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels, int32_t* index,
                                       float* boxes, float* rotation, float* translation, float* hand, int32_t* window) try {
  return pose_from_i420_tiled("hep_pose_from_i420_tiled_rectified: ", false, h, yuv, frames, height, width, crop, resized, nx, ny, camera, score_threshold,
                              PoseOut{found, scores, labels, index, boxes, rotation, translation, hand}, window, true);
} HEP_CATCH_INT

int hep_poses_from_i420_tiled_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                                        const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index, float* boxes,
                                        float* rotation, float* translation, float* hand, int32_t* window) try {
  return pose_from_i420_tiled("hep_poses_from_i420_tiled_rectified: ", true, h, yuv, frames, height, width, crop, resized, nx, ny, camera, score_threshold,
                              PoseOut{found, scores, nullptr, index, boxes, rotation, translation, hand}, window, true);
} HEP_CATCH_INT

// ---- introspection ----
int hep_debug_tensor_count(const hep_handle* h) try { return h ? (int)h->s.tensors.size() : 0; } HEP_CATCH_INT
int hep_debug_tensor_info(const hep_handle* h, int i, const char** name, int64_t dims[4]) try {
  if (!h || i < 0 || i >= (int)h->s.tensors.size()) return fail(HEP_ERR_INVALID, "bad tensor index");
  const TensorDesc& t = h->s.tensors[i];
  if (name) *name = t.name.c_str();
  if (dims) { dims[0] = h->s.max_batch; dims[1] = t.H; dims[2] = t.W; dims[3] = t.C_logical ? t.C_logical : t.C; }
  return 0;
} HEP_CATCH_INT
int hep_debug_tensor(hep_handle* h, const char* name, int batch, float* out, size_t capacity) try {
  if (!h || !name || !out) return fail(HEP_ERR_INVALID, "bad argument");
  Session& s = h->s;
  auto it = s.tensor_by_name.find(name);
  if (it == s.tensor_by_name.end()) return fail(HEP_ERR_INVALID, std::string("no stage tensor named '") + name + "'");
  if (batch < 1 || batch > s.max_batch) return fail(HEP_ERR_UNSUPPORTED, "batch outside 1..max_batch");
  const TensorDesc& t = s.tensors[it->second];
  const int C = t.C_logical ? t.C_logical : t.C;                     // (the allocation may be padded: NHWC rows are C apart all the same)
  const size_t n = (size_t)batch * t.H * t.W * C;
  if (n > capacity) return fail(HEP_ERR_INVALID, "output buffer too small");
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  HIPRET(hipDeviceSynchronize());
  const bool f32 = t.f32 || s.dtype == HEP_F32;
  const size_t per = (size_t)t.H * t.W * C, per_alloc = (size_t)t.H * t.W * t.C;
  for (int ln = 0; ln < s.lanes_for(batch); ln++) {
    const int nb = s.lane_count(batch, ln);
    float* dst = out + (size_t)ln * s.lane_batch * per;
    const size_t cnt = (size_t)nb * (t.frag ? per_alloc : per);      // elements to fetch
    std::vector<float> raw(cnt);
    if (f32) { HIPRET(hipMemcpy(raw.data(), s.tptr(it->second, ln), cnt * 4, hipMemcpyDeviceToHost)); }
    else {
      std::vector<uint16_t> tmp(cnt);
      HIPRET(hipMemcpy(tmp.data(), s.tptr(it->second, ln), cnt * 2, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < cnt; i++) { uint32_t u = (uint32_t)tmp[i] << 16; memcpy(&raw[i], &u, 4); }
    }
    if (!t.frag) { memcpy(dst, raw.data(), cnt * 4); continue; }
    // fragment order -> NHWC: row m = (image, pixel) of this lane, channel k lives in the 16-byte unit
    // ((m / 16) * ksteps + k / KSTEP) * 64 + (k % KSTEP) / KLANE * 16 + m % 16 at element k % KLANE (k_mbf.hip ostore)
    const int kstep = f32 ? 16 : 32, klane = f32 ? 4 : 8, kst = (C + kstep - 1) / kstep;
    const size_t rows = (size_t)nb * t.H * t.W;
    for (size_t m = 0; m < rows; m++)
      for (int k = 0; k < C; k++) {
        const size_t unit = ((m >> 4) * kst + k / kstep) * 64 + (size_t)((k % kstep) / klane) * 16 + (m & 15);
        dst[m * C + k] = raw[unit * klane + k % klane];
      }
  }
  return 0;
} HEP_CATCH_INT

int hep_kernel_count(const hep_handle* h, int) try { return h ? (int)h->s.ops.size() : 0; } HEP_CATCH_INT
int hep_kernel_info(const hep_handle* h, int batch, int i, const char** name, double* bytes, double* flops) try {
  if (!h || i < 0 || i >= (int)h->s.ops.size()) return fail(HEP_ERR_INVALID, "bad kernel index");
  const Op& o = h->s.ops[i];
  if (name) *name = o.name.c_str();
  const int per_launch = std::min(batch, h->s.lane_batch);      // frames one launch of this kernel sees
  if (bytes) *bytes = o.act_bytes_per_image * per_launch + o.weight_bytes;
  if (flops) *flops = o.flops_per_image * per_launch;
  return 0;
} HEP_CATCH_INT

int hep_fp8_scale(const hep_handle* h, int i, float* a_scale) try {
  if (!h || !a_scale || i < 0 || i >= (int)h->s.ops.size()) return fail(HEP_ERR_INVALID, "bad kernel index");
  const Op& o = h->s.ops[i];
  *a_scale = (o.kind == OP_PW && o.pw.fp8) ? o.pw.a_scale : ((o.kind == OP_MBF && o.mbf.fp8) ? o.mbf.a_scale : 0.f);
  return 0;
} HEP_CATCH_INT

int hep_calibrate_fp8(hep_handle* h, const float* frames_nchw_device, int batch) try {
  if (!h || !frames_nchw_device || batch < 1) return fail(HEP_ERR_INVALID, "bad argument");
  Session& s = h->s;
  if (s.dtype != HEP_FP8) return fail(HEP_ERR_UNSUPPORTED, "hep_calibrate_fp8 needs an HEP_FP8 session");
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipDeviceSynchronize());
  return calibrate_fp8(s, frames_nchw_device, batch);
} HEP_CATCH_INT

// the device function (as rocprofv3 --kernel-trace names it) that launch_op runs for launch i: the name of its pick, host arithmetic only
// (bench.py looks the PMC traffic of a device function up by this string)
int hep_kernel_symbol(const hep_handle* h, int i, const char** symbol) try {
  if (!h || !symbol || i < 0 || i >= (int)h->s.ops.size()) return fail(HEP_ERR_INVALID, "bad kernel index");
  static thread_local std::string buf;
  buf = op_pick(h->s.ops[i]).name(); *symbol = buf.c_str();
  return 0;
} HEP_CATCH_INT

int hep_plan_launch_list(const void* pack, size_t pack_bytes, int phi, int size, int max_batch, int dtype, unsigned flags,
                         char* out, size_t capacity, size_t* needed) try {
  if (!needed && !out) return fail(HEP_ERR_INVALID, "out and needed are both NULL");
  if (needed) *needed = 0;
  if (!pack || pack_bytes < 12) return fail(HEP_ERR_PACK, "weight pack: empty");
  if (dtype != HEP_F32 && dtype != HEP_BF16 && dtype != HEP_FP8) return fail(HEP_ERR_INVALID, "dtype must be HEP_F32, HEP_BF16 or HEP_FP8");
#ifndef HEP_WITH_FP8
  if (dtype == HEP_FP8) return fail(HEP_ERR_UNSUPPORTED, "this libhep.so was built without the fp8 path (make -C hmd_ego_pose_amd/csrc FP8=1): it measured slower than bf16");
#endif
  if (max_batch < 1 || max_batch > 4096) return fail(HEP_ERR_INVALID, "max_batch out of range (1..4096)");
  if (size < 128 || size > 2048 || size % 128 != 0)
    return fail(HEP_ERR_UNSUPPORTED, "size must be a multiple of 128 in [128, 2048] (P7 has stride 128)");
  Session s;                                        // never realised on a device: its destructor has nothing to release
  if (!make_arch(phi, &s.arch)) return fail(HEP_ERR_UNSUPPORTED, "phi must be in 0..7 (phi 8 needs a P8 level)");
  Pack pk; std::string err;
  if (!pk.parse(pack, pack_bytes, &err, /*borrow=*/true)) return fail(HEP_ERR_PACK, err);
  s.size = size; s.max_batch = max_batch; s.dtype = dtype; s.device = 0; s.flags = flags;
  session_lanes(&s);
  s.cu_count = 256;                                 // build_session's fallback when the device does not say
  Plan plan; plan.layout_only = true;               // the launch list needs the ops, not the weight blob they would point into
  if (int rc = plan_session(&s, pk, &plan, &err)) return fail(rc, err);
  std::string text;
  for (const Op& o : s.ops) { text += op_pick(o).name(); text += " | "; text += o.name; text += '\n'; }
  if (needed) *needed = text.size() + 1;
  if (out) {
    if (capacity < text.size() + 1) return fail(HEP_ERR_INVALID, "hep_plan_launch_list: the output buffer is smaller than *needed");
    memcpy(out, text.c_str(), text.size() + 1);
  }
  return 0;
} HEP_CATCH_INT

namespace {
struct EventSet {     // events and streams of the profilers, released on every return path
  std::vector<hipEvent_t> ev; std::vector<hipStream_t> st;
  ~EventSet() { for (hipEvent_t e : ev) hipEventDestroy(e); for (hipStream_t x : st) hipStreamDestroy(x); }
  int add_events(size_t n) { for (size_t i = 0; i < n; i++) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return -1; ev.push_back(e); } return 0; }
  int add_streams(size_t n) { for (size_t i = 0; i < n; i++) { hipStream_t x; if (hipStreamCreateWithFlags(&x, hipStreamNonBlocking) != hipSuccess) return -1; st.push_back(x); } return 0; }
};
}  // namespace

int hep_profile(hep_handle* h, int batch, int iters, float* total_ms_per_iter, float* per_kernel_ms) try {
  if (!h || iters < 1) return fail(HEP_ERR_INVALID, "bad argument");
  Session& s = h->s;
  if (batch < 1 || batch > s.max_batch) return fail(HEP_ERR_UNSUPPORTED, "batch outside 1..max_batch");
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  const size_t in_floats = (size_t)3 * s.size * s.size;
  if (!s.d_in) { HIPRET(hipMalloc((void**)&s.d_in, in_floats * s.max_batch * 4)); HIPRET(hipMemset(s.d_in, 0, in_floats * s.max_batch * 4)); }
  EventSet es;
  if (es.add_events(2)) return fail(HEP_ERR_DEVICE, "hipEventCreate failed");
  hipEvent_t e0 = es.ev[0], e1 = es.ev[1];
  std::string err;
  const int64_t S = s.size; const int64_t st[4] = {3 * S * S, S * S, S, 1};
  for (int w = 0; w < 3; w++) if (int rc = run_forward(&s, s.d_in, st, batch, s.stream, &err)) return fail(rc, err);
  HIPRET(hipEventRecord(e0, s.stream));
  for (int i = 0; i < iters; i++) if (int rc = run_forward(&s, s.d_in, st, batch, s.stream, &err)) return fail(rc, err);
  HIPRET(hipEventRecord(e1, s.stream));
  HIPRET(hipEventSynchronize(e1));
  float ms = 0; HIPRET(hipEventElapsedTime(&ms, e0, e1));
  if (total_ms_per_iter) *total_ms_per_iter = ms / iters;
  if (per_kernel_ms) {
    // in-sequence timing: the forward is launched eagerly with an event in front of every kernel,
    // so each duration is taken in its real context (cold caches, real predecessor), on the stream
    // the kernel runs on.  It includes the inter-kernel boundary, like a hipGraph replay does.
    const size_t n = s.ops.size();
    if (es.add_events(n + 1)) return fail(HEP_ERR_DEVICE, "hipEventCreate failed");
    hipEvent_t* ev = es.ev.data() + 2;
    std::vector<double> acc(n, 0.0);
    for (int i = 0; i < iters + 1; i++) {
      for (size_t k = 0; k < n; k++) {     // lane 0's launches (lane_batch frames each), one after the other
        HIPRET(hipEventRecord(ev[k], s.stream));
        launch_op(s, s.lane_ops[0][k], s.lane_count(batch, 0), s.stream, s.d_in, st);
      }
      HIPRET(hipEventRecord(ev[n], s.stream));
      HIPRET(hipEventSynchronize(ev[n]));
      if (i == 0) continue;     // first pass warms the instruction caches
      for (size_t k = 0; k < n; k++) { HIPRET(hipEventElapsedTime(&ms, ev[k], ev[k + 1])); acc[k] += ms; }
    }
    for (size_t k = 0; k < n; k++) per_kernel_ms[k] = (float)(acc[k] / iters);
  }
  return 0;
} HEP_CATCH_INT

int hep_profile_concurrent(hep_handle* h, int batch, int iters, int nstreams, float* per_kernel_ms) try {
  if (!h || iters < 1 || nstreams < 1 || nstreams > 16 || !per_kernel_ms) return fail(HEP_ERR_INVALID, "bad argument");
  Session& s = h->s;
  if (batch < 1 || batch > s.max_batch) return fail(HEP_ERR_UNSUPPORTED, "batch outside 1..max_batch");
  std::lock_guard<std::mutex> lk(s.mu);
  HIPRET(hipSetDevice(s.device));
  const size_t in_floats = (size_t)3 * s.size * s.size;
  if (!s.d_in) { HIPRET(hipMalloc((void**)&s.d_in, in_floats * s.max_batch * 4)); HIPRET(hipMemset(s.d_in, 0, in_floats * s.max_batch * 4)); }
  std::string err;
  const int64_t S = s.size; const int64_t st[4] = {3 * S * S, S * S, S, 1};
  if (int rc = run_forward(&s, s.d_in, st, batch, s.stream, &err)) return fail(rc, err);
  HIPRET(hipStreamSynchronize(s.stream));
  EventSet es;
  if (es.add_streams(nstreams)) return fail(HEP_ERR_DEVICE, "hipStreamCreate failed");
  std::vector<hipStream_t>& ss = es.st;
  const size_t n = s.ops.size();
  for (size_t k = 0; k < n; k++) {
    // the same launch repeated on every stream at once (identical inputs, identical outputs): its
    // time per launch with the chip shared is what the launch costs a pipeline of batches in flight
    for (int rep = 0; rep < 2; rep++) {
      auto t0 = std::chrono::steady_clock::now();
      long issued = 0;
      for (int i = 0; i < (rep ? iters : 2); i++)
        for (auto& x : ss) {
          launch_op(s, s.lane_ops[0][k], s.lane_count(batch, 0), x, s.d_in, st);
          issued++;
#ifdef HEP_ALT
          if (s.lane_ops[0][k].kind == OP_LATE && s.lane_ops[0][k].late.G > 1) break;      // (grouped launches of ONE session share its meeting counters: never two at once - that row is a SERIAL cost)
#endif
        }
      for (auto& x : ss) HIPRET(hipStreamSynchronize(x));
      if (rep) per_kernel_ms[k] = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (double)std::max(1L, issued));      // per launch ISSUED
    }
  }
  return 0;
} HEP_CATCH_INT

}  // extern "C"
