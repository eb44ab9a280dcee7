// hep_api_train.cpp - the training side of the C ABI of libhep.so (include/hep.h): every entry point that takes no hep_handle.
// Anchor targets, the losses and their backward, the three trainable parts (heads, neck, backbone), the augmentations, the
// optimiser and the translation glue.  All of it is stateless: arguments are checked on the host, then the kernels are launched
// on the caller's stream into the caller's buffers.  (Sessions and inference: hep_api.cpp; evaluation and visualisation: hep_api_eval.cpp.)
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "hep_api_util.h"
#include "hep_train.h"

using namespace hep;

extern "C" {

// ---- anchor targets, the five losses and their backward ----
int hep_anchor_targets_device(const float* anchors, int num_anchors, const double* gt_boxes, const int32_t* gt_labels,
                              const float* gt_transform, const float* gt_coords, const int32_t* num_gt, const int32_t* image_hw,
                              int batch, int kmax, int num_classes, int num_transform, double negative_overlap, double positive_overlap,
                              float* labels, float* regression, float* transformation, float* coords, void* stream) try {
  if (!anchors || !gt_boxes || !gt_labels || !gt_transform || !num_gt || !image_hw || !labels || !regression || !transformation)
    return fail(HEP_ERR_INVALID, "bad argument");
  if (num_anchors < 1 || batch < 1 || num_classes < 1 || num_transform < 0) return fail(HEP_ERR_INVALID, "bad size");
  if (kmax < 1 || kmax > AT_MAX_GT) return fail(HEP_ERR_UNSUPPORTED, "kmax must be in 1..64 ground-truth boxes per image");
  AnchorTargetArgs a; a.anchors = anchors; a.N = num_anchors; a.gt_boxes = gt_boxes; a.gt_labels = gt_labels; a.gt_transform = gt_transform;
  a.gt_coords = gt_coords; a.num_gt = num_gt; a.image_hw = image_hw; a.B = batch; a.kmax = kmax; a.num_classes = num_classes; a.rt = num_transform;
  a.negative_overlap = negative_overlap; a.positive_overlap = positive_overlap;
  a.labels = labels; a.regression = regression; a.transformation = transformation; a.coords = coords;
  launch_anchor_targets(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

int hep_losses_device(const float* gt_classification, const float* classification, const float* gt_regression, const float* regression,
                      const float* gt_transformation, const float* transformation, const float* gt_hand, const float* hand,
                      const float* model_points, int batch, int num_anchors, int num_classes, int num_rotation, int num_hand,
                      int num_model_classes, int num_points, float* per_image, float* losses, void* stream) try {
  if (!gt_classification || !classification || !gt_regression || !regression || !gt_transformation || !transformation || !model_points ||
      !per_image || !losses) return fail(HEP_ERR_INVALID, "bad argument");
  if ((gt_hand == nullptr) != (hand == nullptr)) return fail(HEP_ERR_INVALID, "gt_hand and hand go together");
  if (batch < 1 || num_anchors < 1 || num_classes < 1 || num_rotation != 3 || num_hand < 0 || num_model_classes < 1) return fail(HEP_ERR_INVALID, "bad size");
  if (num_points < 1 || num_points > LOSS_MAX_POINTS) return fail(HEP_ERR_UNSUPPORTED, "num_points must be in 1..2048 model points per class");
  LossArgs a; a.gt_cls = gt_classification; a.cls = classification; a.gt_reg = gt_regression; a.reg = regression; a.gt_tr = gt_transformation;
  a.tr = transformation; a.gt_hand = gt_hand; a.hand = hand; a.points = model_points; a.B = batch; a.N = num_anchors; a.K = num_classes;
  a.R = num_rotation; a.H = num_hand; a.classes = num_model_classes; a.P = num_points; a.per_image = per_image; a.losses = losses;
  launch_losses(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

int hep_losses_backward_device(const float* gt_classification, const float* classification, const float* gt_regression, const float* regression,
                               const float* gt_transformation, const float* transformation, const float* gt_hand, const float* hand,
                               const float* model_points, int batch, int num_anchors, int num_classes, int num_rotation, int num_hand,
                               int num_model_classes, int num_points, const float* grad_per_image, float* grad_classification,
                               float* grad_regression, float* grad_transformation, float* grad_hand, int32_t* workspace, void* stream) try {
  if (!gt_classification || !classification || !gt_regression || !regression || !gt_transformation || !transformation || !model_points ||
      !grad_per_image || !workspace) return fail(HEP_ERR_INVALID, "bad argument");
  if ((gt_hand == nullptr) != (hand == nullptr)) return fail(HEP_ERR_INVALID, "gt_hand and hand go together");
  if (grad_hand && !hand) return fail(HEP_ERR_INVALID, "grad_hand needs hand");
  if (batch < 1 || num_anchors < 1 || num_classes < 1 || num_rotation != 3 || num_hand < 0 || num_model_classes < 1) return fail(HEP_ERR_INVALID, "bad size");
  if (grad_hand && num_hand < 1) return fail(HEP_ERR_INVALID, "grad_hand needs num_hand >= 1");
  if (num_points < 1 || num_points > LOSS_MAX_POINTS) return fail(HEP_ERR_UNSUPPORTED, "num_points must be in 1..2048 model points per class");
  LossGradArgs g;
  LossArgs& a = g.f;
  a.gt_cls = gt_classification; a.cls = classification; a.gt_reg = gt_regression; a.reg = regression; a.gt_tr = gt_transformation;
  a.tr = transformation; a.gt_hand = gt_hand; a.hand = hand; a.points = model_points; a.B = batch; a.N = num_anchors; a.K = num_classes;
  a.R = num_rotation; a.H = num_hand; a.classes = num_model_classes; a.P = num_points; a.per_image = nullptr; a.losses = nullptr;
  g.u = grad_per_image; g.g_cls = grad_classification; g.g_reg = grad_regression; g.g_tr = grad_transformation; g.g_hand = grad_hand;
  g.ws = workspace;
  launch_losses_backward(g, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

}  // extern "C"

// ---- the three trainable parts: the five head nets (k_head_grad.hip), the BiFPN neck (k_neck_grad.hip), the EfficientNet trunk (k_backbone_grad.hip).
// A part is described once and everything in front of a launch is written once over that description; num_classes is the heads' alone.
namespace {
template <class Plan> struct Part {
  const char *name, *noun;
  int (*plan)(int phi, int num_classes, int size, int batch, Plan* p, const char** why, int bn_mode, int sync);
  int (*tensor_count)(const Plan&); void (*tensor_offsets)(const Plan&, int64_t* offsets);
  int (*stage_count)(const Plan&); int (*stage)(const Plan&, int i, char name[32], int64_t dims[4], int64_t* offset_floats);      // (NULL for the heads: no stage_* call is theirs)
};
const Part<HGPlan> kHeads = {"heads", "head", heads_plan, heads_tensor_count, heads_tensor_offsets, nullptr, nullptr};
const Part<NGPlan> kNeck = {"neck", "neck", neck_plan, neck_tensor_count, neck_tensor_offsets, neck_stage_count, neck_stage};
const Part<BGPlan> kBackbone = {"backbone", "backbone", backbone_plan, backbone_tensor_count, backbone_tensor_offsets, backbone_stage_count, backbone_stage};
// fills the part's plan.  size == batch == 0 is how the plan functions are asked for the parameter layout alone (layout_only): a run may not say it
template <class Plan> int plan_part(const Part<Plan>& part, int phi, int num_classes, int size, int batch, int bn_mode, Plan* p, bool layout_only = false,
                                    bool sync = false) {
  const char* why = "";
  if (!layout_only && size == 0 && batch == 0) return fail(HEP_ERR_UNSUPPORTED, std::string(part.name) + ": size must be a multiple of 128 in [128, 2048]");
  if (int rc = part.plan(phi, num_classes, size, batch, p, &why, bn_mode, sync)) return fail(rc, why);
  return 0;
}
template <class Plan> int64_t param_count(const Part<Plan>& part, int phi, int num_classes) {
  Plan p; const int rc = plan_part(part, phi, num_classes, 0, 0, HEP_BN_RUNNING, &p, true);
  return rc ? rc : p.nparams;
}
template <class Plan> int param_layout(const Part<Plan>& part, int phi, int num_classes, int64_t* offsets, int capacity) {      // offsets == NULL: the count alone
  Plan p; if (int rc = plan_part(part, phi, num_classes, 0, 0, HEP_BN_RUNNING, &p, true)) return rc;
  const int count = part.tensor_count(p);
  if (offsets && capacity < count) return fail(HEP_ERR_INVALID, std::string("hep_") + part.name + "_param_layout: capacity is smaller than the number of " + part.noun + " tensors");
  if (offsets) part.tensor_offsets(p, offsets);
  return count;
}
template <class Plan> int64_t workspace_bytes(const Part<Plan>& part, int phi, int num_classes, int size, int batch, int bn_mode, bool sync = false) {
  Plan p; const int rc = plan_part(part, phi, num_classes, size, batch, bn_mode, &p, false, sync);
  return rc ? rc : p.ws_floats * (int64_t)sizeof(float);
}
// a forward or backward behind the checks of its own pointers: the momentum (a backward passes 0), the plan, the workspace, `launch(plan, workspace)`, its status.
// sync (the *_sync group): batch statistics over all replicas through the caller's hook, checked first; a hook that fails ends the launch (GDSyncFailed)
template <class Plan, class Launch> int run(const Part<Plan>& part, int phi, int num_classes, int size, int batch, int bn_mode, float momentum, void* workspace,
                                            size_t workspace_bytes, Launch launch, const hep_sync* const* sync = nullptr) {
  const std::string name = part.name, prefix = name + ": "; const Check c{prefix.c_str()};
  if (sync && (!*sync || !(*sync)->sum)) return c.fail(HEP_ERR_INVALID, "sync and sync->sum must not be NULL");
  if (bn_mode == HEP_BN_BATCH && !(momentum >= 0.0f && momentum <= 1.0f)) return c.fail(HEP_ERR_INVALID, "the BatchNorm momentum must be in [0, 1]");
  Plan p; if (int rc = plan_part(part, phi, num_classes, size, batch, bn_mode, &p, false, sync != nullptr)) return rc;
  CHECKED(c.aligned(workspace, 16, "the workspace"));
  if (workspace_bytes < (size_t)p.ws_floats * sizeof(float)) return c.fail(HEP_ERR_INVALID, "the workspace is smaller than hep_" + name + "_workspace_bytes");
  try {
    launch(p, (float*)workspace);
  } catch (const GDSyncFailed& e) {
    return c.fail(HEP_ERR_DEVICE, "the sum hook (hep_sync.sum) returned " + std::to_string(e.rc) + ": nothing further was launched");
  }
  HIPRET(hipGetLastError());
  return 0;
}
template <class Plan> int stage_count(const Part<Plan>& part, int phi) {
  Plan p; const int rc = plan_part(part, phi, 0, 0, 0, HEP_BN_RUNNING, &p, true);
  return rc ? rc : part.stage_count(p);
}
template <class Plan> int stage_info(const Part<Plan>& part, int phi, int size, int batch, int i, const char** name, int64_t dims[4], int64_t* offset_bytes) {
  Plan p; if (int rc = plan_part(part, phi, 0, size, batch, HEP_BN_RUNNING, &p)) return rc;
  static thread_local char buf[32];                 // (per part: the name stays valid until the thread's next call for the same part)
  int64_t unasked[4], off = 0;
  if (part.stage(p, i, buf, dims ? dims : unasked, &off)) return fail(HEP_ERR_INVALID, "bad stage index");
  if (name) *name = buf;
  if (offset_bytes) *offset_bytes = off * (int64_t)sizeof(float);
  return 0;
}
template <class T> bool any_null(T* const* ptrs, int n) { return std::find(ptrs, ptrs + n, nullptr) != ptrs + n; }
}  // namespace
extern "C" {
// ---- the five head nets.  They read params in place, so it must be aligned; neck and backbone read an aligned copy ----
int64_t hep_heads_param_count(int phi, int num_classes) try { return param_count(kHeads, phi, num_classes); } HEP_CATCH_INT
int hep_heads_param_layout(int phi, int num_classes, int64_t* offsets, int capacity) try { return param_layout(kHeads, phi, num_classes, offsets, capacity); } HEP_CATCH_INT
int64_t hep_heads_workspace_bytes_bn(int phi, int num_classes, int size, int batch, int bn_mode) try { return workspace_bytes(kHeads, phi, num_classes, size, batch, bn_mode); } HEP_CATCH_INT
int64_t hep_heads_workspace_bytes(int phi, int num_classes, int size, int batch) try { return hep_heads_workspace_bytes_bn(phi, num_classes, size, batch, HEP_BN_RUNNING); } HEP_CATCH_INT
int hep_heads_forward_device_bn(const float* params, const float* const feats[5], int phi, int num_classes, int size, int batch, float* const outs[5],
                                void* workspace, size_t workspace_bytes, int bn_mode, float momentum, float* stats_out, void* stream) try {
  if (!params || !feats || !outs || !workspace || any_null(feats, 5) || any_null(outs, 5)) return fail(HEP_ERR_INVALID, "bad argument");
  CHECKED(Check{"heads: "}.aligned(params, 16, "params"));
  return run(kHeads, phi, num_classes, size, batch, bn_mode, momentum, workspace, workspace_bytes,
             [&](const HGPlan& p, float* ws) { launch_heads_forward(p, params, feats, outs, ws, (hipStream_t)stream, momentum, stats_out); });
} HEP_CATCH_INT
int hep_heads_forward_device(const float* params, const float* const feats[5], int phi, int num_classes, int size, int batch,
                             float* const outs[5], void* workspace, size_t workspace_bytes, void* stream) try {
  return hep_heads_forward_device_bn(params, feats, phi, num_classes, size, batch, outs, workspace, workspace_bytes, HEP_BN_RUNNING, 0.0f, nullptr, stream);
} HEP_CATCH_INT
int hep_heads_backward_device_bn(const float* params, const float* const grad_outs[5], int phi, int num_classes, int size, int batch, float* grad_params,
                                 float* const grad_feats[5], void* workspace, size_t workspace_bytes, int bn_mode, void* stream) try {
  if (!params || !grad_outs || !grad_params || !workspace || any_null(grad_outs, 5) || (grad_feats && any_null(grad_feats, 5))) return fail(HEP_ERR_INVALID, "bad argument");
  CHECKED(Check{"heads: "}.aligned(params, 16, "params"));
  return run(kHeads, phi, num_classes, size, batch, bn_mode, 0.0f, workspace, workspace_bytes,
             [&](const HGPlan& p, float* ws) { launch_heads_backward(p, params, grad_outs, grad_params, grad_feats, ws, (hipStream_t)stream); });
} HEP_CATCH_INT
int hep_heads_backward_device(const float* params, const float* const grad_outs[5], int phi, int num_classes, int size, int batch,
                              float* grad_params, float* const grad_feats[5], void* workspace, size_t workspace_bytes, void* stream) try {
  return hep_heads_backward_device_bn(params, grad_outs, phi, num_classes, size, batch, grad_params, grad_feats, workspace, workspace_bytes, HEP_BN_RUNNING, stream);
} HEP_CATCH_INT
// synchronised statistics: HEP_BN_BATCH over the rows of all replicas (all three parts alike)
int64_t hep_heads_workspace_bytes_sync(int phi, int num_classes, int size, int batch) try { return workspace_bytes(kHeads, phi, num_classes, size, batch, HEP_BN_BATCH, true); } HEP_CATCH_INT
int hep_heads_forward_device_sync(const float* params, const float* const feats[5], int phi, int num_classes, int size, int batch, float* const outs[5],
                                  void* workspace, size_t workspace_bytes, float momentum, float* stats_out, const hep_sync* sync, void* stream) try {
  if (!params || !feats || !outs || !workspace || any_null(feats, 5) || any_null(outs, 5)) return fail(HEP_ERR_INVALID, "bad argument");
  CHECKED(Check{"heads: "}.aligned(params, 16, "params"));
  return run(kHeads, phi, num_classes, size, batch, HEP_BN_BATCH, momentum, workspace, workspace_bytes,
             [&](const HGPlan& p, float* ws) { launch_heads_forward(p, params, feats, outs, ws, (hipStream_t)stream, momentum, stats_out, sync); }, &sync);
} HEP_CATCH_INT
int hep_heads_backward_device_sync(const float* params, const float* const grad_outs[5], int phi, int num_classes, int size, int batch, float* grad_params,
                                   float* const grad_feats[5], void* workspace, size_t workspace_bytes, const hep_sync* sync, void* stream) try {
  if (!params || !grad_outs || !grad_params || !workspace || any_null(grad_outs, 5) || (grad_feats && any_null(grad_feats, 5))) return fail(HEP_ERR_INVALID, "bad argument");
  CHECKED(Check{"heads: "}.aligned(params, 16, "params"));
  return run(kHeads, phi, num_classes, size, batch, HEP_BN_BATCH, 0.0f, workspace, workspace_bytes,
             [&](const HGPlan& p, float* ws) { launch_heads_backward(p, params, grad_outs, grad_params, grad_feats, ws, (hipStream_t)stream, sync); }, &sync);
} HEP_CATCH_INT

// ---- the BiFPN neck ----
int64_t hep_neck_param_count(int phi) try { return param_count(kNeck, phi, 0); } HEP_CATCH_INT
int hep_neck_param_layout(int phi, int64_t* offsets, int capacity) try { return param_layout(kNeck, phi, 0, offsets, capacity); } HEP_CATCH_INT
int64_t hep_neck_workspace_bytes_bn(int phi, int size, int batch, int bn_mode) try { return workspace_bytes(kNeck, phi, 0, size, batch, bn_mode); } HEP_CATCH_INT
int64_t hep_neck_workspace_bytes(int phi, int size, int batch) try { return hep_neck_workspace_bytes_bn(phi, size, batch, HEP_BN_RUNNING); } HEP_CATCH_INT
int hep_neck_stage_count(int phi) try { return stage_count(kNeck, phi); } HEP_CATCH_INT
int hep_neck_stage_info(int phi, int size, int batch, int i, const char** name, int64_t dims[4], int64_t* offset_bytes) try {
  return stage_info(kNeck, phi, size, batch, i, name, dims, offset_bytes);
} HEP_CATCH_INT
int hep_neck_forward_device_bn(const float* params, const float* const taps[3], int phi, int size, int batch, float* const feats[5],
                               void* workspace, size_t workspace_bytes, int bn_mode, float momentum, float* stats_out, void* stream) try {
  if (!params || !taps || !feats || !workspace || any_null(taps, 3) || any_null(feats, 5)) return fail(HEP_ERR_INVALID, "bad argument");
  return run(kNeck, phi, 0, size, batch, bn_mode, momentum, workspace, workspace_bytes,
             [&](const NGPlan& p, float* ws) { launch_neck_forward(p, params, taps, feats, ws, (hipStream_t)stream, momentum, stats_out); });
} HEP_CATCH_INT
int hep_neck_forward_device(const float* params, const float* const taps[3], int phi, int size, int batch, float* const feats[5],
                            void* workspace, size_t workspace_bytes, void* stream) try {
  return hep_neck_forward_device_bn(params, taps, phi, size, batch, feats, workspace, workspace_bytes, HEP_BN_RUNNING, 0.0f, nullptr, stream);
} HEP_CATCH_INT
int hep_neck_backward_device_bn(const float* params, const float* const grad_feats[5], int phi, int size, int batch, float* grad_params,
                                float* const grad_taps[3], void* workspace, size_t workspace_bytes, int bn_mode, void* stream) try {
  if (!params || !grad_feats || !grad_params || !workspace || any_null(grad_feats, 5) || (grad_taps && any_null(grad_taps, 3))) return fail(HEP_ERR_INVALID, "bad argument");
  return run(kNeck, phi, 0, size, batch, bn_mode, 0.0f, workspace, workspace_bytes,
             [&](const NGPlan& p, float* ws) { launch_neck_backward(p, grad_feats, grad_params, grad_taps, ws, (hipStream_t)stream); });
} HEP_CATCH_INT
int hep_neck_backward_device(const float* params, const float* const grad_feats[5], int phi, int size, int batch, float* grad_params,
                             float* const grad_taps[3], void* workspace, size_t workspace_bytes, void* stream) try {
  return hep_neck_backward_device_bn(params, grad_feats, phi, size, batch, grad_params, grad_taps, workspace, workspace_bytes, HEP_BN_RUNNING, stream);
} HEP_CATCH_INT
int64_t hep_neck_workspace_bytes_sync(int phi, int size, int batch) try { return workspace_bytes(kNeck, phi, 0, size, batch, HEP_BN_BATCH, true); } HEP_CATCH_INT
int hep_neck_forward_device_sync(const float* params, const float* const taps[3], int phi, int size, int batch, float* const feats[5],
                                 void* workspace, size_t workspace_bytes, float momentum, float* stats_out, const hep_sync* sync, void* stream) try {
  if (!params || !taps || !feats || !workspace || any_null(taps, 3) || any_null(feats, 5)) return fail(HEP_ERR_INVALID, "bad argument");
  return run(kNeck, phi, 0, size, batch, HEP_BN_BATCH, momentum, workspace, workspace_bytes,
             [&](const NGPlan& p, float* ws) { launch_neck_forward(p, params, taps, feats, ws, (hipStream_t)stream, momentum, stats_out, sync); }, &sync);
} HEP_CATCH_INT
int hep_neck_backward_device_sync(const float* params, const float* const grad_feats[5], int phi, int size, int batch, float* grad_params,
                                  float* const grad_taps[3], void* workspace, size_t workspace_bytes, const hep_sync* sync, void* stream) try {
  if (!params || !grad_feats || !grad_params || !workspace || any_null(grad_feats, 5) || (grad_taps && any_null(grad_taps, 3))) return fail(HEP_ERR_INVALID, "bad argument");
  return run(kNeck, phi, 0, size, batch, HEP_BN_BATCH, 0.0f, workspace, workspace_bytes,
             [&](const NGPlan& p, float* ws) { launch_neck_backward(p, grad_feats, grad_params, grad_taps, ws, (hipStream_t)stream, sync); }, &sync);
} HEP_CATCH_INT

// ---- the EfficientNet trunk ----
int64_t hep_backbone_param_count(int phi) try { return param_count(kBackbone, phi, 0); } HEP_CATCH_INT
int hep_backbone_param_layout(int phi, int64_t* offsets, int capacity) try { return param_layout(kBackbone, phi, 0, offsets, capacity); } HEP_CATCH_INT
int64_t hep_backbone_workspace_bytes_bn(int phi, int size, int batch, int bn_mode) try { return workspace_bytes(kBackbone, phi, 0, size, batch, bn_mode); } HEP_CATCH_INT
int64_t hep_backbone_workspace_bytes(int phi, int size, int batch) try { return hep_backbone_workspace_bytes_bn(phi, size, batch, HEP_BN_RUNNING); } HEP_CATCH_INT
int hep_backbone_stage_count(int phi) try { return stage_count(kBackbone, phi); } HEP_CATCH_INT
int hep_backbone_stage_info(int phi, int size, int batch, int i, const char** name, int64_t dims[4], int64_t* offset_bytes) try {
  return stage_info(kBackbone, phi, size, batch, i, name, dims, offset_bytes);
} HEP_CATCH_INT
int hep_backbone_forward_device_bn(const float* params, const float* image, const float* branch_scale, int phi, int size, int batch, float* const taps[3],
                                   void* workspace, size_t workspace_bytes, int bn_mode, float momentum, float* stats_out, void* stream) try {
  if (!params || !image || !taps || !workspace || any_null(taps, 3)) return fail(HEP_ERR_INVALID, "bad argument");
  return run(kBackbone, phi, 0, size, batch, bn_mode, momentum, workspace, workspace_bytes,
             [&](const BGPlan& p, float* ws) { launch_backbone_forward(p, params, image, branch_scale, taps, ws, (hipStream_t)stream, momentum, stats_out); });
} HEP_CATCH_INT
int hep_backbone_forward_device(const float* params, const float* image, const float* branch_scale, int phi, int size, int batch, float* const taps[3],
                                void* workspace, size_t workspace_bytes, void* stream) try {
  return hep_backbone_forward_device_bn(params, image, branch_scale, phi, size, batch, taps, workspace, workspace_bytes, HEP_BN_RUNNING, 0.0f, nullptr, stream);
} HEP_CATCH_INT
int hep_backbone_backward_device_bn(const float* params, const float* const grad_taps[3], const float* branch_scale, int phi, int size, int batch,
                                    float* grad_params, float* grad_image, void* workspace, size_t workspace_bytes, int bn_mode, void* stream) try {
  if (!params || !grad_taps || !grad_params || !workspace || any_null(grad_taps, 3)) return fail(HEP_ERR_INVALID, "bad argument");
  return run(kBackbone, phi, 0, size, batch, bn_mode, 0.0f, workspace, workspace_bytes,
             [&](const BGPlan& p, float* ws) { launch_backbone_backward(p, grad_taps, branch_scale, grad_params, grad_image, ws, (hipStream_t)stream); });
} HEP_CATCH_INT
int hep_backbone_backward_device(const float* params, const float* const grad_taps[3], const float* branch_scale, int phi, int size, int batch,
                                 float* grad_params, float* grad_image, void* workspace, size_t workspace_bytes, void* stream) try {
  return hep_backbone_backward_device_bn(params, grad_taps, branch_scale, phi, size, batch, grad_params, grad_image, workspace, workspace_bytes, HEP_BN_RUNNING, stream);
} HEP_CATCH_INT
int64_t hep_backbone_workspace_bytes_sync(int phi, int size, int batch) try { return workspace_bytes(kBackbone, phi, 0, size, batch, HEP_BN_BATCH, true); } HEP_CATCH_INT
int hep_backbone_forward_device_sync(const float* params, const float* image, const float* branch_scale, int phi, int size, int batch, float* const taps[3],
                                     void* workspace, size_t workspace_bytes, float momentum, float* stats_out, const hep_sync* sync, void* stream) try {
  if (!params || !image || !taps || !workspace || any_null(taps, 3)) return fail(HEP_ERR_INVALID, "bad argument");
  return run(kBackbone, phi, 0, size, batch, HEP_BN_BATCH, momentum, workspace, workspace_bytes,
             [&](const BGPlan& p, float* ws) { launch_backbone_forward(p, params, image, branch_scale, taps, ws, (hipStream_t)stream, momentum, stats_out, sync); }, &sync);
} HEP_CATCH_INT
int hep_backbone_backward_device_sync(const float* params, const float* const grad_taps[3], const float* branch_scale, int phi, int size, int batch,
                                      float* grad_params, float* grad_image, void* workspace, size_t workspace_bytes, const hep_sync* sync, void* stream) try {
  if (!params || !grad_taps || !grad_params || !workspace || any_null(grad_taps, 3)) return fail(HEP_ERR_INVALID, "bad argument");
  return run(kBackbone, phi, 0, size, batch, HEP_BN_BATCH, 0.0f, workspace, workspace_bytes,
             [&](const BGPlan& p, float* ws) { launch_backbone_backward(p, grad_taps, branch_scale, grad_params, grad_image, ws, (hipStream_t)stream, sync); }, &sync);
} HEP_CATCH_INT

// ---- training input: 6DoF augmentation + preprocess (k_augment.hip) ----
static int64_t augment_partial_bytes(int batch, int height, int kmax) {
  const int64_t tiles = (height + AUG_TILE_ROWS - 1) / AUG_TILE_ROWS;
  return ((int64_t)batch * tiles * (4 * kmax + 1) * 4 + 255) & ~(int64_t)255;
}

// the box partials and the uint8 frame of the resize launch (counted whether or not this size needs it: the figure never shrinks as an argument grows)
int64_t hep_augment_workspace_bytes(int batch, int height, int width, int size, int kmax) try {
  const Check c{"augment: "};      // (hep_augment_6dof_device takes these refusals from here, with the figure)
  CHECKED(c.at_least("batch", batch, 1)); CHECKED(c.frame(height, width, true));
  if (size < 16 || size > 4096 || size % 4 != 0) return c.fail(HEP_ERR_UNSUPPORTED, "size must be a multiple of 4 in [16, 4096]");
  if (kmax < 1 || kmax > AUG_MAX_K) return c.fail(HEP_ERR_UNSUPPORTED, "kmax must be in 1..16 annotations per image");
  return augment_partial_bytes(batch, height, kmax) + (((int64_t)batch * height * width * 3 + 255) & ~(int64_t)255);
} HEP_CATCH_INT

int hep_augment_6dof_device(const uint8_t* rgb_hwc, const uint8_t* mask, const double* xform, const float* camera_k, const double* boxes,
                            const int32_t* labels, const int32_t* mask_values, const float* rvec, const float* tvec, const float* extra,
                            const int32_t* num_gt, int batch, int height, int width, int size, int kmax, float translation_scale_norm,
                            float* image_nchw, uint8_t* mask_out, float* camera, double* gt_boxes, int32_t* gt_labels, float* gt_transform,
                            int32_t* gt_num, int32_t* applied, void* workspace, int64_t workspace_bytes, void* stream) try {
  const Check c{"augment: "};
  if (!rgb_hwc || !mask || !xform || !camera_k || !boxes || !labels || !mask_values || !rvec || !tvec || !extra || !num_gt)
    return c.fail(HEP_ERR_INVALID, "a required input pointer is NULL");
  if (!image_nchw || !camera || !gt_boxes || !gt_labels || !gt_transform || !gt_num || !applied)
    return c.fail(HEP_ERR_INVALID, "a required output pointer is NULL (only mask_out may be)");
  CHECKED(c.ptrs({{workspace, "workspace"}}));
  const int64_t need = hep_augment_workspace_bytes(batch, height, width, size, kmax); if (need < 0) return (int)need;
  if (((uintptr_t)image_nchw & 15) != 0 || ((uintptr_t)workspace & 15) != 0) return c.fail(HEP_ERR_INVALID, "image_nchw and workspace must be 16-byte aligned");
  CHECKED(c.workspace(workspace, workspace_bytes, need, "hep_augment_workspace_bytes"));
  AugmentArgs a;
  a.rgb = rgb_hwc; a.mask = mask; a.xform = xform; a.camera_k = camera_k; a.boxes = boxes; a.labels = labels; a.mask_values = mask_values;
  a.rvec = rvec; a.tvec = tvec; a.extra = extra; a.num_gt = num_gt;
  a.B = batch; a.H = height; a.W = width; a.S = size; a.kmax = kmax; a.tiles = (height + AUG_TILE_ROWS - 1) / AUG_TILE_ROWS;
  a.tsn = translation_scale_norm;
  ResizeGeom g;      // preprocess_image, as hep_preprocess_u8_device
  if (!resize_geometry(height, width, size, &g)) return c.fail(HEP_ERR_UNSUPPORTED, "resized frame does not fit the network size");
  a.resize = g.resize; a.image_scale = g.scale; a.nh = g.nh; a.nw = g.nw; a.inv_scale_x = g.inv_scale_x; a.inv_scale_y = g.inv_scale_y;
  a.image = image_nchw; a.mask_out = mask_out; a.camera = camera; a.gt_boxes = gt_boxes; a.gt_labels = gt_labels; a.gt_transform = gt_transform;
  a.gt_num = gt_num; a.applied = applied;
  a.partials = (int32_t*)workspace; a.frame_u8 = (uint8_t*)workspace + augment_partial_bytes(batch, height, kmax);
  launch_augment(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

// ---- training input: colour augmentation (k_colour.hip) ----
static int64_t colour_counter_bytes(int batch) { return ((int64_t)batch * 3 * COL_COUNTERS * 4 + 255) & ~(int64_t)255; }
static int64_t colour_frame_bytes(int batch, int height, int width) { return ((int64_t)batch * height * width * 3 + 255) & ~(int64_t)255; }

// the counters and the two frames the operations between an image's first and last go through
int64_t hep_colour_workspace_bytes(int batch, int height, int width) try {
  const Check c{"colour: "};      // (hep_colour_augment_device takes these refusals from here, with the figure)
  CHECKED(c.at_least("batch", batch, 1)); CHECKED(c.frame(height, width, true));
  if (batch > 65535) return c.fail(HEP_ERR_UNSUPPORTED, "batch must be at most 65535");
  return colour_counter_bytes(batch) + 2 * colour_frame_bytes(batch, height, width);
} HEP_CATCH_INT

int hep_colour_augment_device(const uint8_t* rgb_hwc, const int32_t* ops, const float* args, int batch, int height, int width,
                              uint8_t* out_hwc, void* workspace, int64_t workspace_bytes, void* stream) try {
  const Check c{"colour: "};
  if (!rgb_hwc || !ops || !args) return c.fail(HEP_ERR_INVALID, "a required input pointer is NULL");
  if (!out_hwc) return c.fail(HEP_ERR_INVALID, "the output pointer is NULL");
  CHECKED(c.ptrs({{workspace, "workspace"}}));
  if (out_hwc == rgb_hwc) return c.fail(HEP_ERR_INVALID, "out_hwc must not be rgb_hwc (the filters read neighbours)");
  const int64_t need = hep_colour_workspace_bytes(batch, height, width); if (need < 0) return (int)need;
  if (((uintptr_t)workspace & 15) != 0 || ((uintptr_t)ops & 3) != 0 || ((uintptr_t)args & 3) != 0)
    return c.fail(HEP_ERR_INVALID, "workspace must be 16-byte, ops and args 4-byte aligned");
  CHECKED(c.workspace(workspace, workspace_bytes, need, "hep_colour_workspace_bytes"));
  ColourArgs a;
  a.rgb = rgb_hwc; a.ops = ops; a.args = args; a.B = batch; a.H = height; a.W = width; a.out = out_hwc;
  a.counters = (uint32_t*)workspace;
  a.frame0 = (uint8_t*)workspace + colour_counter_bytes(batch);
  a.frame1 = a.frame0 + colour_frame_bytes(batch, height, width);
  HIPRET(hipMemsetAsync(a.counters, 0, (size_t)batch * 3 * COL_COUNTERS * 4, (hipStream_t)stream));
  launch_colour(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

// ---- the training step between the parts: optimiser, gradient norm, translation glue (k_train.hip) ----
static int optim_check(const Check& c, int64_t n, int optimizer, const void* const* ptrs, int count, const void* kind, const void* state) {
  if (n <= 0) return c.fail(HEP_ERR_INVALID, "n must be > 0");
  if (!kind || !state) return c.fail(HEP_ERR_INVALID, "kind or state is NULL");
  for (int i = 0; i < count; i++) {
    if (!ptrs[i]) return c.fail(HEP_ERR_INVALID, "a required pointer is NULL");
    CHECKED(c.aligned(ptrs[i], 16, "the float buffers"));
  }
  if (((uintptr_t)kind & 3) != 0 || ((uintptr_t)state & 15) != 0) return c.fail(HEP_ERR_INVALID, "kind must be 4-byte, state 16-byte aligned");
  if (optimizer != HEP_OPT_ADAM && optimizer != HEP_OPT_SGD_NESTEROV)
    return c.fail(HEP_ERR_UNSUPPORTED, "optimizer " + std::to_string(optimizer) + " is not built (HEP_OPT_ADAM = 0, HEP_OPT_SGD_NESTEROV = 1)");
  return 0;
}

int64_t hep_optim_workspace_bytes(int64_t n) try {
  if (n <= 0) return fail(HEP_ERR_INVALID, "optim: n must be > 0");
  return ((int64_t)optim_grid(n) * 8 + 15) & ~(int64_t)15;
} HEP_CATCH_INT

int hep_optim_grad_norm_device(const float* grad, const uint8_t* kind, int64_t n, int optimizer, float beta1, float beta2, float max_norm,
                               void* state, void* workspace, size_t workspace_bytes, void* stream) try {
  const void* ptrs[2] = {grad, workspace};
  const Check c{"optim_grad_norm: "};
  CHECKED(optim_check(c, n, optimizer, ptrs, 2, kind, state));
  CHECKED(c.workspace(workspace, (int64_t)workspace_bytes, hep_optim_workspace_bytes(n), "hep_optim_workspace_bytes"));
  OptimArgs a{};
  a.grad = grad; a.kind = kind; a.n = n; a.optimizer = optimizer; a.blocks = optim_grid(n); a.beta1 = beta1; a.beta2 = beta2; a.max_norm = max_norm;
  a.state = (OptimState*)state; a.partials = (double*)workspace;
  launch_optim_norm(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

int hep_optim_update_device(float* params, const float* grad, float* m, float* v, const float* stats, const uint8_t* kind, int64_t n,
                            int optimizer, float lr, float beta1, float beta2, float eps, const void* state, void* stream) try {
  const void* ptrs[4] = {params, grad, m, v};
  const Check c{"optim_update: "};
  CHECKED(optim_check(c, n, optimizer, ptrs, optimizer == HEP_OPT_SGD_NESTEROV && !v ? 3 : 4, kind, state));
  CHECKED(c.aligned(stats, 16, "the float buffers"));      // (stats may be NULL)
  OptimArgs a{};
  a.params = params; a.grad = grad; a.m = m; a.v = v; a.stats = stats; a.kind = kind; a.n = n; a.optimizer = optimizer; a.blocks = optim_grid(n);
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.state = (OptimState*)state;
  launch_optim_update(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

static int transform_check(const char* what, int batch, int num_anchors, int num_rotation) {
  if (batch < 1 || num_anchors < 1 || num_rotation < 1 || num_rotation > 8) return fail(HEP_ERR_INVALID, std::string(what) + ": bad size");
  return 0;
}

int hep_transformation_pack_device(const float* rotation, const float* translation_raw, const float* camera, const float* translation_anchors,
                                   int batch, int num_anchors, int num_rotation, float* transformation, void* stream) try {
  if (!rotation || !translation_raw || !camera || !translation_anchors || !transformation) return fail(HEP_ERR_INVALID, "transformation_pack: a pointer is NULL");
  if (int rc = transform_check("transformation_pack", batch, num_anchors, num_rotation)) return rc;
  TransformArgs a{};
  a.rotation = rotation; a.raw = translation_raw; a.camera = camera; a.anchors = translation_anchors; a.transformation = transformation;
  a.B = batch; a.N = num_anchors; a.R = num_rotation;
  launch_transformation_pack(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

int hep_transformation_unpack_grad_device(const float* grad_transformation, const float* translation_raw, const float* camera,
                                          const float* translation_anchors, int batch, int num_anchors, int num_rotation,
                                          float* grad_rotation, float* grad_translation_raw, void* stream) try {
  if (!grad_transformation || !translation_raw || !camera || !translation_anchors || !grad_rotation || !grad_translation_raw)
    return fail(HEP_ERR_INVALID, "transformation_unpack_grad: a pointer is NULL");
  if (int rc = transform_check("transformation_unpack_grad", batch, num_anchors, num_rotation)) return rc;
  TransformArgs a{};
  a.transformation = const_cast<float*>(grad_transformation); a.raw = translation_raw; a.camera = camera; a.anchors = translation_anchors;
  a.g_rotation = grad_rotation; a.g_raw = grad_translation_raw; a.B = batch; a.N = num_anchors; a.R = num_rotation;
  launch_transformation_unpack_grad(a, (hipStream_t)stream);
  HIPRET(hipGetLastError());
  return 0;
} HEP_CATCH_INT

}  // extern "C"
