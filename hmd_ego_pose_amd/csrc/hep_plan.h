// hep_plan.h - the host-only half of session creation: weight folding and layout (hep_pack.cpp) and the launch plan
// (hep_plan.cpp).  Nothing declared here touches a device; hep_session.cpp turns a Plan into device memory and pointers.
#pragma once
#include <type_traits>

#include "hep_host.h"

namespace hep {

// ---- weight builder: lays weights out in the host copy of the weight blob, converts to the session dtype ----
uint16_t f32_to_bf16(float f);
struct WBuilder {
  std::vector<unsigned char> host;
  size_t size = 0;                                  // bytes laid out so far (host.size() unless layout_only)
  bool layout_only = false;                         // hand out offsets, write nothing: a plan that no device will run (Plan::layout_only)
  int dtype = 0;
  size_t alloc(size_t bytes);                       // 256-byte aligned, zero-filled
  size_t put_bytes(const std::vector<unsigned char>& v);
  size_t put_f32(const std::vector<float>& v);
  size_t put_f32(const PackTensor* t) { return put_f32(std::vector<float>(t->data, t->data + t->count)); }
  // e4m3 rows [rows][stride] of a [rows][K] matrix, one scale per row (amax / 448): w ~ e4m3 * scale
  size_t put_fp8(const std::vector<float>& v, int rows, int K, int stride, std::vector<float>* scales);
  size_t put_typed(const std::vector<float>& v);    // dtype elements (fp8 sessions store bf16 everywhere except the quantised weights)
};

struct BnFold { std::vector<float> scale, shift; };
bool fold_bn(const Pack& pk, const std::string& prefix, int c, BnFold* out, std::string* err);

// Pointwise conv [N][K] (+ optional conv bias) followed by an optional BatchNorm, rows n0 .. n0 + Nc - 1:
// w[row(n)][k] = W[n0 + n][k] * scale, b[n] = bias * scale + shift; `rows` >= Nc rows, the rest zero.
// row_of (optional) permutes the weight rows (k_tower.hip's map layers); the bias stays in channel order.
struct FoldedPw { std::vector<float> w, b; };
FoldedPw fold_pw(const PackTensor* w, int K, const PackTensor* conv_bias, const BnFold* bn, int n0, int Nc, int rows, const std::vector<int>* row_of = nullptr);
// Depthwise conv [C][taps] -> [taps][C], times an optional per-channel scale
std::vector<float> fold_dw(const PackTensor* wd, int C, int taps, const float* scale = nullptr);

// ---- pointer references ----
// Ops are stored by value in a vector that grows and every lane gets its own copy of the plan, so the planner records
// where each pointer goes and what it points at; hep_session.cpp resolves them per lane once the memory exists.
typedef void (*Slot)(Op& o, int seg, int idx, void* p);
// the setter of one pointer member of Op, e.g. SLOT(pw.A), SLOT(segs[seg].src[idx]): the member is named here and nowhere else
#define SLOT(member) (+[](::hep::Op& o, int seg, int idx, void* p) { (void)seg; (void)idx; o.member = static_cast<std::remove_reference_t<decltype(o.member)>>(p); })
enum RefKind { TO_TENSOR, TO_WEIGHT, TO_HEAD_OUT };   // arena tensor `at`, byte offset `at` of the weight blob, head output `at` (0..4)
struct Ref { int op; Slot set; int seg, idx; RefKind kind; size_t at; };

struct Plan {
  std::vector<unsigned char> weights;   // host copy of the weight blob
  std::vector<Ref> refs;
  int ntails = 0;                       // fused fronts that finish their squeeze-excite in their tail (one counter block each)
  bool layout_only = false;             // set by the caller: same ops, references and offsets, but `weights` stays empty (hep_plan_launch_list)
};
// Fills s->ops, tensors (offset, first_op, last_op), arena_bytes, num_classes, levels, level_off, num_anchors, feat_ids from
// arch / size / max_batch / dtype / flags / knobs / lanes / lane_batch (and cu_count).  0 or HEP_ERR_PACK.
int plan_session(Session* s, const Pack& pack, Plan* plan, std::string* err);
// words of s->d_sync one lane owns
size_t sync_lane_words(const Session& s, const Plan& plan);
// resolves every reference of the plan for one lane from s.d_weights / d_arena / d_out / d_sync (pure address arithmetic)
void patch_lane(const Session& s, const Plan& plan, int lane, std::vector<Op>* ops);

}  // namespace hep
