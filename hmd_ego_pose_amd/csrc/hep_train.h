// hep_train.h - launch arguments, limits, plans and launch functions of the stateless training side (hep_api_train.cpp; k_eval.hip's anchor targets and
// losses, k_loss_grad.hip, the k_*_grad.hip files through grad_dev.h, k_augment.hip, k_colour.hip, k_train.hip).  Plan and session: hep_internal.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct hep_sync;      // include/hep.h: the sum hook of synchronised BatchNorm
struct GDSyncFailed { int rc; };      // thrown by a launch function whose hook returned rc != 0 (grad_dev.h); caught at the ABI

// ---- training side: anchor-target assignment (generators/utils/anchors.py:69-221) ----
#define AT_MAX_GT 64
struct AnchorTargetArgs {
  const float* anchors; int N;                                     // [N,4]
  const double* gt_boxes; const int32_t* gt_labels;                // [B][kmax][4] x1,y1,x2,y2 ; [B][kmax]
  const float* gt_transform; const float* gt_coords;               // [B][kmax][rt] ; [B][kmax][63] (nullable)
  const int32_t* num_gt; const int32_t* image_hw;                  // [B] ; [B][2] (height, width)
  int B, kmax, num_classes, rt; double negative_overlap, positive_overlap;
  float* labels; float* regression; float* transformation; float* coords;   // [B][N][C+1], [B][N][5], [B][N][rt+1], [B][N][64] (nullable)
};
void launch_anchor_targets(const AnchorTargetArgs&, hipStream_t);

// ---- training side: 6DoF augmentation + preprocess of the generator (generators/common.py:348-479, :543-607), k_augment.hip ----
#define AUG_MAX_K 16          // annotations per image
#define AUG_TILE_ROWS 8       // rows of one aug_mask workgroup
struct AugmentArgs {
  const uint8_t* rgb; const uint8_t* mask;                         // [B][H][W][3] ; [B][H][W]
  const double* xform; const float* camera_k;                      // [B][9] M (6), angle rad, scale, apply ; [B][4]
  const double* boxes; const int32_t* labels; const int32_t* mask_values;      // [B][kmax][4] ; [B][kmax] ; [B][kmax]
  const float* rvec; const float* tvec; const float* extra; const int32_t* num_gt;
  int B, H, W, S, kmax, tiles;                                     // tiles = ceil(H / AUG_TILE_ROWS)
  int resize, nh, nw; float tsn; double image_scale, inv_scale_x, inv_scale_y;
  float* image; uint8_t* mask_out; float* camera;                  // [B][3][S][S] ; [B][H][W] (nullable) ; [B][6]
  double* gt_boxes; int32_t* gt_labels; float* gt_transform; int32_t* gt_num; int32_t* applied;
  int32_t* partials; uint8_t* frame_u8;                            // workspace: [B][tiles][4 kmax + 1] ; [B][H][W][3]
};
void launch_augment(const AugmentArgs&, hipStream_t);

// ---- training side: colour augmentation of the generator (generators/randaug.py:244-279, common.py:334-341), k_colour.hip ----
#define COL_COUNTERS 769      // per image and slot: three 256-bin histograms and the luma sum
struct ColourArgs {
  const uint8_t* rgb; const int32_t* ops; const float* args;      // [B][H][W][3] ; [B][3][8] ; [B][3][2]
  int B, H, W;
  uint8_t* out;                                                    // [B][H][W][3]
  uint32_t* counters; uint8_t* frame0; uint8_t* frame1;            // workspace: [B][3][COL_COUNTERS] (zeroed per call) ; two frames
};
void launch_colour(const ColourArgs&, hipStream_t);

// ---- training side: optimiser update, gradient norm and the translation glue of the one-call step (k_train.hip) ----
#define OPT_MAX_BLOCKS 1024   // the fixed grid of the streaming passes: at most this many workgroups, one double partial each
struct OptimState { float norm, clip_coef, bias1, bias2_sqrt; int32_t step, skipped; int32_t pad[2]; };      // the 32-byte state block of include/hep.h
struct OptimArgs {
  float* params; const float* grad; float* m; float* v; const float* stats; const uint8_t* kind; int64_t n;
  int optimizer, blocks; float lr, beta1, beta2, eps, max_norm;
  OptimState* state; double* partials;                             // partials: [blocks] in the caller's workspace
};
int optim_grid(int64_t n);
void launch_optim_norm(const OptimArgs&, hipStream_t);
void launch_optim_update(const OptimArgs&, hipStream_t);
struct TransformArgs {
  const float* rotation; const float* raw; const float* camera; const float* anchors;      // [B][N][R] ; [B][N][3] ; [B][6] ; [N][3]
  float* transformation;                                           // [B][N][R+3]: written by pack, the gradient read by unpack
  float* g_rotation; float* g_raw;                                 // unpack: [B][N][R] ; [B][N][3]
  int B, N, R;
};
void launch_transformation_pack(const TransformArgs&, hipStream_t);
void launch_transformation_unpack_grad(const TransformArgs&, hipStream_t);

// ---- training side: the five losses of batch_iterate (hmdegopose/loss.py:54-99), forward values ----
#define LOSS_MAX_POINTS 2048
struct LossArgs {
  const float* gt_cls; const float* cls;        // [B][N][K+1] (labels, anchor state) ; [B][N][K] scores
  const float* gt_reg; const float* reg;        // [B][N][5] ; [B][N][4]
  const float* gt_tr; const float* tr;          // [B][N][R+3+3] (rotation, translation, is_symmetric, class, state) ; [B][N][R+3]
  const float* gt_hand; const float* hand;      // [B][N][H+1] ; [B][N][H] (both nullable: hand loss 0)
  const float* points;                          // [classes][P][3]
  int B, N, K, R, H, classes, P;
  float* per_image;                             // [B][5]: classification, regression, rotation, translation, hand
  float* losses;                                // [5]: batch means, regression x 50
};
void launch_losses(const LossArgs&, hipStream_t);
// ... and their backward (k_loss_grad.hip): the gradients of the predictions for an upstream gradient of the per-image losses
struct LossGradArgs {
  LossArgs f;                                   // the forward's inputs and sizes (per_image / losses unused)
  const float* u;                               // [B][5] upstream gradient of per_image
  float* g_cls; float* g_reg; float* g_tr; float* g_hand;   // [B][N][K], [B][N][4], [B][N][R+3], [B][N][H] (each nullable)
  int32_t* ws;                                  // [B][4] counts (n_c, n_r, n_t, n_h), then [B][N] object anchors of the transformation state
};
void launch_losses_backward(const LossGradArgs&, hipStream_t);

// ---- training side: forward and backward of the five head nets (k_head_grad.hip) ----
// Activations live as fp32 rows [R][W]: the pixels of level 0 (all images), then level 1, ...; R = batch * sum(s_l^2).
#define HG_SLOTS 6           // header separable convs: regressor, classifier, rotation, translation xy, translation z, hand
#define HG_NETS 5
#define HG_TILE_ROWS 32      // rows of one column-reduction tile (a tile never crosses a level)
#define HG_MAX_SLABS 32      // split-K slabs of the weight-gradient products
struct HGGeom {
  int B, W, D, R, S;         // batch, width, head depth, rows, pixels per image over the five levels
  int s[5];                  // side of each level
  int pixoff[6];             // pixels per image in front of each level
  int rowoff[6];             // rows in front of each level (= B * pixoff)
  int tileoff[6];            // column-reduction tiles in front of each level
  int ntiles, nslab, slab_rows;
};
struct HGPlan {
  HGGeom g;
  int num_classes;
  int C[HG_SLOTS], ld[HG_SLOTS];                        // header channels (9 * values per anchor) and their row pitch (C rounded up to 4)
  int net[HG_SLOTS], K[HG_SLOTS], kh[HG_SLOTS], koff[HG_SLOTS];   // owning net; values per anchor of the net's output, of this header, first column
  int64_t p_conv[HG_NETS], p_bn[HG_NETS], p_hdr[HG_SLOTS], nparams;   // float offsets into the flat parameter buffer
  int64_t o_x0, o_x, o_u, o_z, o_uh, o_cl, o_do[HG_SLOTS], o_g1, o_g2, o_pw[HG_SLOTS], o_pdw[HG_SLOTS], o_pbh[HG_SLOTS],
      o_pg[2], o_pb[2], o_pbi[2], ws_floats;            // float offsets into the workspace
  int bn_batch;                                         // HEP_BN_BATCH: batch-statistics BatchNorm (the passes of grad_dev.h)
  int64_t o_bne, o_bnp;                                 // ... its effective tables (layout of p_bn per net) and the statistics partials
  int bn_sync; int64_t o_xch;                           // synchronised statistics (with bn_batch): the exchange block of grad_dev.h's GDSync
};
// fills the plan; returns 0, or a negative HEP_ERR_* with a reason in *why (a static string)
int heads_plan(int phi, int num_classes, int size, int batch, HGPlan* p, const char** why, int bn_mode = 0, int sync = 0);
int heads_tensor_count(const HGPlan&);      // the tensors of the flat buffer in state_dict order: how many, and (below) the float offset of each; all three parts alike
void heads_tensor_offsets(const HGPlan&, int64_t* offsets);
// momentum, stats_out: batch statistics only (stats_out: layout of params, the running_mean / running_var slots written; NULL: no update)
// sync: the plan's bn_sync only (the hook the sums of every BatchNorm cross the replicas through; forward and backward alike, all three parts)
void launch_heads_forward(const HGPlan&, const float* params, const float* const feats[5], float* const outs[5], float* ws, hipStream_t,
                          float momentum = 0.0f, float* stats_out = nullptr, const hep_sync* sync = nullptr);
void launch_heads_backward(const HGPlan&, const float* params, const float* const grad_outs[5], float* grad_params, float* const grad_feats[5],
                           float* ws, hipStream_t, const hep_sync* sync = nullptr);

// ---- training side: forward and backward of the BiFPN neck (k_neck_grad.hip) ----
// Every map is fp32 rows [B * s_l * s_l][C] in a buffer of its own; the parameters are read from an aligned copy in the workspace.
#define NG_NODES 8           // conv6_up conv5_up conv4_up conv3_up conv4_down conv5_down conv6_down conv7_down
#define NG_LATERALS 6        // cell 0: p5_down_channel p4_down_channel p3_down_channel p5_to_p6 p4_down_channel_2 p5_down_channel_2
#define NG_MAX_CELLS 8
#define NG_FUSION_FLOATS 19  // the eight fusion vectors in front of every cell
#define NG_TILE_ROWS 8       // rows of one column-reduction tile: short serial walks, the maps are small (32 measured 3 x slower in gather / dw_bwd)
#define NG_MAX_SLABS 32      // split-K slabs of the weight-gradient products
#define NG_MAX_CONTRIB 4     // consumers of one map
struct NGPlan {
  int phi, W, cells, B;
  int tapc[3];                                          // channels of the taps P3, P4, P5
  int s[5], R[5], ntiles[5], slab_rows[5], nslab[5];    // per level: side, rows, column-reduction tiles, weight-gradient slabs
  int64_t p_cell[NG_MAX_CELLS + 1], p_lat[NG_LATERALS], nparams;   // float offsets into the flat parameter buffer
  // float offsets into the workspace: the aligned parameter copy of each cell; tap rows; lateral z / y; cell 0's pooled P6 / P7
  // and their argmax bytes; per node s, u, z, y (+ argmax bytes of the pool it reads); temporaries of the backward
  int64_t o_pp[NG_MAX_CELLS], o_tap[3], o_lz[NG_LATERALS], o_ly[NG_LATERALS], o_p6, o_p7, o_am6, o_am7;
  int64_t o_s[NG_MAX_CELLS][NG_NODES], o_u[NG_MAX_CELLS][NG_NODES], o_z[NG_MAX_CELLS][NG_NODES], o_y[NG_MAX_CELLS][NG_NODES], o_am[NG_MAX_CELLS][NG_NODES];
  int64_t o_x, o_dz, o_du, o_ds[2][NG_NODES], o_g6, o_g7, o_pw, o_pdw, o_pb[3], o_pf[3], o_dtap[NG_LATERALS], ws_floats;
  int bn_batch;                                         // HEP_BN_BATCH: batch-statistics BatchNorm (the passes of grad_dev.h)
  int64_t o_bne, o_bnp;                                 // ... an effective table per BatchNorm (laterals, then cell by cell); the statistics partials
  int bn_sync; int64_t o_xch;                           // synchronised statistics (with bn_batch): the exchange block of grad_dev.h's GDSync
};
// fills the plan (size == batch == 0: the parameter layout only); returns 0, or a negative HEP_ERR_* with a reason in *why.  The three plan
// functions have one signature: num_classes is the heads' alone and ignored here
int neck_plan(int phi, int num_classes, int size, int batch, NGPlan* p, const char** why, int bn_mode = 0, int sync = 0);
int neck_tensor_count(const NGPlan&);
void neck_tensor_offsets(const NGPlan&, int64_t* offsets);
// stage i of the workspace a forward leaves: its name, NHWC dims and float offset; -1 for an index past the end (neck and backbone alike)
int neck_stage_count(const NGPlan&);
int neck_stage(const NGPlan&, int i, char name[32], int64_t dims[4], int64_t* offset_floats);
// momentum, stats_out: batch statistics only (stats_out: layout of params, the running_mean / running_var slots written; NULL: no update)
void launch_neck_forward(const NGPlan&, const float* params, const float* const taps[3], float* const feats[5], float* ws, hipStream_t,
                         float momentum = 0.0f, float* stats_out = nullptr, const hep_sync* sync = nullptr);
void launch_neck_backward(const NGPlan&, const float* const grad_feats[5], float* grad_params, float* const grad_taps[3], float* ws, hipStream_t,
                          const hep_sync* sync = nullptr);

// ---- training side: forward and backward of the EfficientNet trunk (k_backbone_grad.hip) ----
// Every map is fp32 rows [B * s * s][C] in a buffer of its own; the parameters are read from an aligned copy in the workspace.
#define BG_MAX_BLOCKS 48     // phi 6 / 7 have 45 MBConv blocks
#define BG_MAX_SEGMENTS (2 * BG_MAX_BLOCKS + 1)   // aligned parameter copies: the stem, per block [expand .. se_expand bias] and [project, bn2]
#define BG_MAX_SLABS 256     // split-K slabs of the weight-gradient products (up to 16 * 128 * 128 rows at phi 0 / 256 / batch 16)
#define BG_MAX_CEXP 3456     // widest expanded map (phi 6 / 7) and squeeze width: the squeeze-excite kernels keep one image's vectors in LDS
#define BG_MAX_SE 144
struct BGBlock {
  int cin, cexp, k, stride, se, cout, expand, skip;
  int s_in, s_out, R_in, R_out;
  // float offsets into the flat parameter buffer (p_first: the block's first tensor, p_end: one past its last)
  int64_t p_first, p_w0, p_bn0, p_dw, p_bn1, p_wr, p_br, p_we, p_be, p_w2, p_bn2, p_end;
  // float offsets into the workspace: the two aligned parameter copies; what the forward keeps (conv outputs z0 z1 z2, swish(bn0(z0)),
  // the gated map, the block's output, per image the squeezed means, the reduce FC's output and the gate)
  int64_t q_a, q_b, o_z0, o_a0, o_z1, o_xg, o_z2, o_y, o_m, o_r, o_g;
  int64_t o_e0, o_e1, o_e2;                             // batch statistics: the effective tables of bn0, bn1, bn2
};
struct BGPlan {
  int phi, nblocks, stem, B, size, s0, R0;
  int taps[3], tapc[3];                                 // blocks whose outputs are P3, P4, P5 and their channels
  int64_t p_stem, p_bn_stem, nparams;
  BGBlock b[BG_MAX_BLOCKS];
  // workspace: stem parameters, the image, the stem's conv output and activation; temporaries of forward (a1) and backward
  int64_t q_stem, o_img, o_zs, o_as, o_a1, o_dy[2], o_dz2, o_dxg, o_da0, o_dx, o_pw, o_pcol[2], o_pdw, o_pse, o_dl, o_dr, o_dm, ws_floats;
  int bn_batch;                                         // HEP_BN_BATCH: batch-statistics BatchNorm (the passes of grad_dev.h)
  int64_t o_es, o_bnp;                                  // ... the stem's effective table; the statistics partials
  int bn_sync; int64_t o_xch;                           // synchronised statistics (with bn_batch): the exchange block of grad_dev.h's GDSync
};
// fills the plan (size == batch == 0: the parameter layout only); returns 0, or a negative HEP_ERR_* with a reason in *why
int backbone_plan(int phi, int num_classes, int size, int batch, BGPlan* p, const char** why, int bn_mode = 0, int sync = 0);      // (num_classes ignored, as neck_plan)
int backbone_tensor_count(const BGPlan&);
void backbone_tensor_offsets(const BGPlan&, int64_t* offsets);
int backbone_stage_count(const BGPlan&);
int backbone_stage(const BGPlan&, int i, char name[32], int64_t dims[4], int64_t* offset_floats);
// momentum, stats_out: batch statistics only (stats_out: layout of params, the running_mean / running_var slots written; NULL: no update)
void launch_backbone_forward(const BGPlan&, const float* params, const float* image, const float* branch_scale, float* const taps[3], float* ws, hipStream_t,
                             float momentum = 0.0f, float* stats_out = nullptr, const hep_sync* sync = nullptr);
void launch_backbone_backward(const BGPlan&, const float* const grad_taps[3], const float* branch_scale, float* grad_params, float* grad_image, float* ws,
                              hipStream_t, const hep_sync* sync = nullptr);
