/* hep.h - C ABI of libhep.so, the MI355X-native (gfx950) EfficientPose / HMD-EgoPose
 * inference path: EfficientNet-B{phi} MBConv backbone -> BiFPN -> box / class / rotation /
 * translation / hand heads -> anchor, box and translation decode -> detection filter.
 *
 * Drop-in boundary.  Every entry point names the reference interface it replaces
 * (paths relative to the reference repository root):
 *
 *   hep_create / hep_destroy   <- `new InferenceSession(ModelFilePath, sessionOptions)` / Dispose
 *                                 unity-sandbox/OpenCVDNNSandboxNetCore/Program.cs:39-61,
 *                                 unity-sandbox/WebRTCNetCoreSandbox/Program.cs:57-78;
 *                                 Python: HMDEgoPose(...)+load_state_dict, pytorch-sandbox/evaluate.py:84-119
 *   hep_run                    <- `Session.Run({"input": float[1,3,S,S]})` -> 10 outputs in the order fixed by
 *                                 pytorch-sandbox/hmdegopose/misc_utils.py:77-83 (feat1..5, regression,
 *                                 classification, rotation, translation_raw, hand); Program.cs:95-122 / :211-229
 *   hep_run_device             <- HMDEgoPose.forward, pytorch-sandbox/backbone.py:104-125 (device tensors,
 *                                 asynchronous on the caller's HIP stream; what the torch custom op calls)
 *   hep_anchors                <- anchors_for_shape, pytorch-sandbox/generators/utils/anchors.py:273-318 and the
 *                                 files anchors_256.txt / translation_anchors_256.txt the C# hosts load
 *                                 (Program.cs:26-28)
 *   hep_decode / _device       <- format_bboxes + format_translation, pytorch-sandbox/hmdegopose/loss.py:12-51
 *                                 (C# twins Program.cs:225-470)
 *   hep_filter / _device       <- FilterDetections / filter_detections, pytorch-sandbox/hmdegopose/layers.py:264-482
 *                                 (C# twin Program.cs:472-627)
 *   hep_top1_device            <- the ONE detection the streaming app keeps of filter_detections (WebRTCNetCoreSandbox/Program.cs:261-282):
 *                                 row 0 of hep_decode_device + hep_filter_device in one launch
 *   hep_pose_from_i420         <- the whole I420AVideoFrameReady callback, Program.cs:128-298 (frame bytes in host memory -> pose)
 *   hep_pose_from_input        <- the same from the float blob of OpenCVDNNSandboxNetCore/Program.cs:95-122
 *   hep_top_labels_device, hep_poses_from_i420, hep_poses_from_input <- the same three for a model of several objects
 *                                 (num_classes > 1, backbone.py:14): the top detection of EVERY label, class-specific as the
 *                                 reference constructs its filter (train.py:78-81)
 *   hep_pose_from_i420_tiled, hep_pose_from_i420_windows (and hep_poses_*) <- no twin: the callback's centre crop taken at several places of
 *                                 the frame in one call, best window reported (WHOLE-FRAME SEARCH below)
 *   hep_pose_from_i420_tiled_rectified, hep_pose_from_i420_windows_rectified (and hep_poses_*) <- no twin: the same search on windows resampled
 *                                 into the view of a camera rotated to look along their ray, poses rotated back (RECTIFIED WINDOWS below)
 *   hep_anchor_targets_device <- anchor_targets_bbox, pytorch-sandbox/generators/utils/anchors.py:69-221 (training side)
 *   hep_losses_device          <- batch_iterate, pytorch-sandbox/hmdegopose/loss.py:54-428 (training side, forward values)
 *   hep_losses_backward_device <- loss.backward() through batch_iterate (training side, gradients of the predictions)
 *   hep_heads_forward_device / hep_heads_backward_device <- the five head nets under those losses, trainable
 *   hep_neck_forward_device / hep_neck_backward_device <- the BiFPN neck in front of them, trainable
 *   hep_backbone_forward_device / hep_backbone_backward_device <- the EfficientNet trunk in front of the neck, trainable
 *   hep_pose_errors / _device  <- check_6d_pose_add / check_6d_pose_add_s, pytorch-sandbox/eval/common.py:682-746 with
 *                                 c_min_distances, pytorch-sandbox/generators/utils/calc_min_distances.h:24-35 (the
 *                                 metric arithmetic of evaluate.py's loop, eval/common.py:866-1121)
 *   hep_score_detections_device <- the per-image body of evaluate_model, eval/common.py:866-1121: matching (942-957) and the
 *                                 metrics of the matched pair (682-778, 646-679, 970-982) for a whole batch in one launch
 *   hep_score_scene_device     <- the same loop as the reference writes it (912-1030): every label, several annotations per
 *                                 image, each detection assigned to the annotation of its label it overlaps most
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a
 * negative hep_status, never throws (every entry point catches what its C++ body could raise -> HEP_ERR_INTERNAL) and never aborts; hep_last_error() gives a thread-local
 * message.  A handle serialises its own calls with an internal mutex (the C# frame callback
 * re-enters Run from WebRTC worker threads, Program.cs:128); several handles may coexist.
 * There is NO CPU fallback: without a usable gfx950 device hep_create fails.
 */
#ifndef HEP_H_
#define HEP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HEP_ABI_VERSION 1

typedef struct hep_handle hep_handle;

typedef enum hep_status {
  HEP_OK = 0,
  HEP_ERR_INVALID = -1,      /* bad argument                                  */
  HEP_ERR_PACK = -2,         /* weight pack missing / malformed / wrong shape  */
  HEP_ERR_DEVICE = -3,       /* HIP error or no gfx950 device                  */
  HEP_ERR_UNSUPPORTED = -4,  /* phi / size / batch outside the built range     */
  HEP_ERR_INTERNAL = -5      /* a C++ exception (out of host memory, ...) was caught at the ABI: nothing ever propagates into the caller */
} hep_status;

typedef enum hep_dtype {
  HEP_F32 = 0,   /* fp32 storage, exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): the parity mode        */
  HEP_BF16 = 1,  /* bf16 activations+weights, fp32 accumulate (v_mfma_f32_16x16x32_bf16): the bench */
  HEP_FP8 = 2    /* bf16 session whose backbone pointwise convs (expand / project, 62 % of the MACs) run with OCP e4m3
                    operands (v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulate): weights stored as e4m3 with one scale per
                    output channel behind the BN fold, activations converted on the fly with one power-of-two scale per
                    tensor calibrated at hep_create; depthwise, BiFPN and heads stay bf16 (BASELINE config 5).
                    OPT-IN BUILD (make -C hmd_ego_pose_amd/csrc fp8 -> libhep_fp8.so): on MI355X it measured slower than
                    HEP_BF16 at every batch size and ten times less accurate, so the default libhep.so answers
                    HEP_ERR_UNSUPPORTED to it (and says so in hep_last_error)                                       */
} hep_dtype;

/* hep_create flags */
#define HEP_FLAG_KEEP_INTERMEDIATES 1u   /* no activation-buffer reuse: hep_debug_tensor works for every stage */
#define HEP_FLAG_NO_GRAPH 2u             /* launch kernels eagerly instead of replaying a captured hipGraph    */

/* Output indices (the ONNX export order, misc_utils.py:77-83). */
enum { HEP_OUT_FEAT1 = 0, HEP_OUT_FEAT5 = 4, HEP_OUT_REGRESSION = 5, HEP_OUT_CLASSIFICATION = 6,
       HEP_OUT_ROTATION = 7, HEP_OUT_TRANSLATION_RAW = 8, HEP_OUT_HAND = 9, HEP_NUM_OUTPUTS = 10 };

int hep_abi_version(void);
/* Which build of the library this is: "libhep gfx950" followed by the optional parts it was compiled with - " alt" (the rejected plan
 * alternatives and their knobs: make alt), " fp8" (make fp8), " poison" (sanitizer build), " trace" (phase stamps).  Static storage. */
const char* hep_build_info(void);
const char* hep_last_error(void);

/* Number of HIP devices visible; does not initialise the runtime beyond counting. */
int hep_device_count(void);

/* Build a session: reads a HEPW weight pack (the reference state_dict by name, fp32;
 * see hmd_ego_pose_amd/weights.py), folds BatchNorm, lays weights out for the kernels
 * and allocates the activation arena for batches up to max_batch on HIP device `device`. */
int hep_create(const char* pack_path, int phi, int size, int max_batch, int dtype, int device,
               unsigned flags, hep_handle** out);
int hep_create_from_memory(const void* pack, size_t pack_bytes, int phi, int size, int max_batch,
                           int dtype, int device, unsigned flags, hep_handle** out);
void hep_destroy(hep_handle* h);

/* Geometry. */
int hep_num_anchors(const hep_handle* h);                       /* N = 9 * sum(level cells)          */
/* Classes of the classifier, read from the weights: its header holds 9 * num_classes channels (efficientdet/model.py:393;
 * backbone.py:14 `num_classes`, 1 at every reference call site).  1..63. */
int hep_num_classes(const hep_handle* h);
int hep_output_shape(const hep_handle* h, int index, int batch, int64_t dims[4], int* ndim);
/* The handle's OWN device buffer of head output `index` (HEP_OUT_REGRESSION .. HEP_OUT_HAND), fp32 [max_batch, N, K]:
 * where hep_run_device leaves its results when outs == NULL.  Valid until hep_destroy; rewritten by the next forward on
 * this handle (stream-ordered).  Lets a serving loop with several handles in flight hand out results without the
 * device-to-device copies that caller-provided outs[] cost (75 MB per batch of 16 at phi 0). */
int hep_output_device(const hep_handle* h, int index, float** ptr);

/* Session.Run replacement: host buffers in, host buffers out, synchronous.
 * input: fp32 NCHW [batch,3,S,S], already normalised.  feats may be NULL (or hold NULLs):
 * feature maps are then not exported.  Outputs are caller-allocated, fp32:
 * feats[l] NCHW [batch,W,s_l,s_l]; regression [batch,N,4]; classification [batch,N,num_classes] (post-sigmoid);
 * rotation [batch,N,3]; translation_raw [batch,N,3]; hand [batch,N,63]. */
int hep_run(hep_handle* h, const float* input_nchw, int batch, float* const feats[5],
            float* regression, float* classification, float* rotation, float* translation_raw, float* hand);

/* HMDEgoPose.forward on device memory, asynchronous on `stream` (a hipStream_t; NULL = default).
 * in_strides: element strides of (n,c,h,w) - an NHWC-memory view (eval/common.py:397) is accepted
 * as is; NULL = contiguous NCHW.  outs[5] = regression, classification, rotation, translation_raw,
 * hand (device, fp32; NULL = leave them in the handle's own buffers, read back through
 * hep_decode_device / hep_filter_device with NULL inputs).  feats may be NULL.  Every batch size replays
 * its own hipGraph.
 * A handle owns ONE activation arena: work enqueued through it is stream-ordered, so use a handle on one
 * stream at a time (or let the previous forward finish before switching streams).  For several batches in
 * flight create several handles from the same weight pack - see INTEGRATION.md section 4. */
int hep_run_device(hep_handle* h, const float* input, const int64_t in_strides[4], int batch,
                   float* const outs[5], float* const feats[5], void* stream);

/* anchors_for_shape((size,size)): host, float64 arithmetic, one cast to float32.
 * anchors [N,4] x1,y1,x2,y2; translation_anchors [N,3] cx,cy,stride.  Either may be NULL.
 * Returns N (or a negative status). */
int hep_anchors(int size, float* anchors, float* translation_anchors);

/* Box + translation decode.  camera [batch,6] = fx,fy,px,py,tz_scale,image_scale.
 * boxes [batch,N,4] = xmin,ymin,xmax,ymax clipped to [0,S-1]; translation [batch,N,3] = Tx,Ty,Tz. */
int hep_decode(hep_handle* h, const float* regression, const float* translation_raw, const float* camera,
               int batch, float* boxes, float* translation);
int hep_decode_device(hep_handle* h, const float* regression, const float* translation_raw, const float* camera,
                      int batch, float* boxes, float* translation, void* stream);

/* Detection filter per image: score > score_threshold -> greedy NMS (IoU strictly greater than
 * nms_threshold suppresses; candidates by descending score, ties by lower anchor index) -> first
 * max_detections survivors -> rows padded with -1.  classification is [batch,N,num_classes]; with more than one class
 * the filter is class-specific (layers.py:347-358, the reference's default and the only mode it constructs,
 * train.py:78-81): every class is thresholded and suppressed on its own, the (anchor, class) pairs of all classes are
 * concatenated class by class and the max_detections best scores are kept (ties: the earlier pair); det_labels holds
 * the class.  Unlike the reference (which returns only the
 * last batch item, layers.py:466-482) every image gets its rows.
 * det_boxes [batch,M,4], det_scores [batch,M], det_labels [batch,M] (int32), det_rotation [batch,M,3],
 * det_translation [batch,M,3], det_hand [batch,M,63], det_index [batch,M] (int32 anchor index),
 * det_count [batch] (int32).  Any output except det_count may be NULL. */
/* class_specific_filter of FilterDetections (layers.py:403-433, filter_detections :347-362).  on != 0 (the default, and the only mode
 * the reference constructs): as described above.  on == 0: ONE pass per image over every anchor's best class - score = max over the
 * class columns, det_labels = the first argmax - thresholded, suppressed and cut to max_detections like a single class.  With one
 * class both modes are the same pass.  Applies to the following hep_filter / hep_filter_device calls on this handle. */
int hep_set_class_specific_filter(hep_handle* h, int on);
int hep_filter(hep_handle* h, const float* boxes, const float* classification, const float* rotation,
               const float* translation, const float* hand, int batch, float score_threshold,
               float nms_threshold, int max_detections, float* det_boxes, float* det_scores,
               int32_t* det_labels, float* det_rotation, float* det_translation, float* det_hand,
               int32_t* det_index, int32_t* det_count);
int hep_filter_device(hep_handle* h, const float* boxes, const float* classification, const float* rotation,
                      const float* translation, const float* hand, int batch, float score_threshold,
                      float nms_threshold, int max_detections, float* det_boxes, float* det_scores,
                      int32_t* det_labels, float* det_rotation, float* det_translation, float* det_hand,
                      int32_t* det_index, int32_t* det_count, void* stream);

/* The top detection of every image - what the streaming app sends (unity-sandbox/WebRTCNetCoreSandbox/Program.cs:272-298 reads one
 * detection) - as ONE launch on the raw head outputs, with no decode of the other anchors, no sort and no NMS.
 * DEFINITION: the record of image b is row 0 of hep_decode_device -> hep_filter_device on the same inputs, bit for bit, for any
 * nms_threshold and any max_detections >= 1, in the handle's current hep_set_class_specific_filter mode (the best-scoring
 * candidate always survives greedy NMS).  As a rule: class-specific mode - the maximal score over all (anchor, class) pairs with
 * score > score_threshold, ties to the lower class, then to the lower anchor index; other mode - per anchor the maximum over the
 * class columns (label = first argmax), then the maximal such score above the threshold, ties to the lower anchor index.  A score
 * exactly at the threshold is no candidate.
 * regression, classification, rotation, translation_raw, hand: the RAW head outputs on the device (each may be NULL = the handle's
 * own output buffer, as for hep_decode_device / hep_filter_device); camera [batch,6] on the device.
 * records: device memory, batch x HEP_POSE_RECORD_WORDS 4-byte words:
 *   word 0      found, int32 0 / 1                    word 4       score
 *   word 1      label, int32                          words 5-8    box xmin, ymin, xmax, ymax
 *   word 2      anchor index, int32                   words 9-11   rotation (the network's output, as the filter returns it)
 *   word 3      0                                     words 12-14  translation Tx, Ty, Tz
 *   words 15-77 hand (63)                             words 78-79  0
 * With no candidate found is 0 and every other word holds the filter's padding (-1 / -1.0f); words 3, 78 and 79 stay 0.
 * Asynchronous on `stream`, no allocation, no host synchronisation.  NULL handle / camera / records or a batch outside
 * 1..max_batch: HEP_ERR_INVALID. */
#define HEP_POSE_RECORD_WORDS 80
int hep_top1_device(hep_handle* h, const float* regression, const float* classification, const float* rotation,
                    const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                    uint32_t* records, void* stream);

/* Frame to pose in one synchronous call on HOST memory - the whole frame callback of the streaming app (Program.cs:128-298):
 * yuv [batch][height * width * 3 / 2] I420 bytes as WebRTC delivers them -> the kernels of hep_preprocess_i420_device (same
 * arguments, same arithmetic) -> the forward -> the top-detection launch above -> one device-to-host copy of batch x 320 bytes.
 * No decode or filter launch, no head array on the host.  camera [batch,6] on the host.  Outputs on the host, per image:
 * found [batch] int32, scores [batch], labels [batch] int32, index [batch] int32 (anchor), boxes [batch,4], rotation [batch,3],
 * translation [batch,3], hand [batch,63]; any of them except found may be NULL.  An image with found == 0 gets the padding
 * (-1 / -1.0f) everywhere else.  rotation is the network's output as the filter returns it (the evaluator multiplies by pi,
 * eval/common.py:419-447; the app converts to a quaternion itself).
 * The handle's mutex is held from staging to the final synchronise (the callback may re-enter from worker threads).  The record
 * comes back through a pinned host buffer of the handle; the frame is handed to hipMemcpyAsync where it lies (measured faster than
 * a copy into a pinned buffer of the handle first, which HEP_POSE_UPLOAD=pinned in the environment still selects).  The handle's
 * buffers are allocated at first use and only ever grown: after the first call of a shape nothing is allocated or freed, on host
 * or device.  Every argument is checked before any HIP call: a NULL handle /
 * yuv / camera / found, a batch outside 1..max_batch, an odd height or width, a crop larger than the frame or resized < 1 is
 * HEP_ERR_INVALID with the reason in hep_last_error. */
int hep_pose_from_i420(hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop, int resized,
                       const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels,
                       int32_t* index, float* boxes, float* rotation, float* translation, float* hand);
/* The same from the normalised fp32 NCHW blob [batch,3,S,S] that hep_run takes (OpenCVDNNSandboxNetCore/Program.cs:95-122). */
int hep_pose_from_input(hep_handle* h, const float* input_nchw, int batch, const float* camera, float score_threshold,
                        int32_t* found, float* scores, int32_t* labels, int32_t* index, float* boxes, float* rotation,
                        float* translation, float* hand);

/* The top detection of EVERY label of every image, in one launch on the raw head outputs: the serving call of a model trained on several
 * objects (num_classes = K > 1; hep_top1_device reports only whichever object scores highest in the frame).
 * DEFINITION: record (b, c) is row 0 of hep_decode_device -> hep_filter_device in class-specific mode on image b with every
 * classification column but c set to -1, bit for bit, for any nms_threshold and any max_detections >= 1.  As a rule: the maximal
 * classification[b, n, c] over the anchors n with a score > score_threshold, ties to the lower anchor index; a score exactly at the
 * threshold is no candidate.  Where an image has no more than max_detections candidate pairs in all, record (b, c) is also the first
 * row with det_labels == c of the unmasked filter.
 * CLASS-SPECIFIC BY DEFINITION: hep_set_class_specific_filter is ignored.  In the other mode an anchor whose best class is c can be
 * suppressed by a box of another label, so "the top detection per label" has no NMS-free meaning there.
 * Arguments as for hep_top1_device (NULL head pointer = the handle's own output buffer; camera [batch,6] on the device).
 * records: device memory, batch x num_classes x HEP_POSE_RECORD_WORDS words, [batch][num_classes] records of the layout above; the label
 * word of record (b, c) is c when found.  A label without a candidate gets found = 0 and the filter's padding (-1 / -1.0f) everywhere
 * else; words 3, 78 and 79 stay 0.  Asynchronous on `stream`, no allocation, no host synchronisation.  NULL handle / camera / records or
 * a batch outside 1..max_batch: HEP_ERR_INVALID. */
int hep_top_labels_device(hep_handle* h, const float* regression, const float* classification, const float* rotation,
                          const float* translation_raw, const float* hand, const float* camera, int batch, float score_threshold,
                          uint32_t* records, void* stream);

/* hep_pose_from_i420 / hep_pose_from_input for several objects: the same staging, mutex, one pinned download (batch x num_classes x 320
 * bytes) and one synchronise, with the launch of hep_top_labels_device in place of the top-detection launch.  Every output has
 * [batch][num_classes] rows and slot c is label c, so there is no labels array: found [batch,K] int32, scores [batch,K], index [batch,K]
 * int32, boxes [batch,K,4], rotation [batch,K,3], translation [batch,K,3], hand [batch,K,63]; any of them except found may be NULL.  A
 * slot with found == 0 holds the padding (-1 / -1.0f).  The buffers for num_classes records per image belong to the handle, are allocated
 * at the first of these calls and only ever grown; hep_pose_from_* keep their own.  Argument checks as for hep_pose_from_*. */
int hep_poses_from_i420(hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop, int resized,
                        const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index, float* boxes,
                        float* rotation, float* translation, float* hand);
int hep_poses_from_input(hep_handle* h, const float* input_nchw, int batch, const float* camera, float score_threshold,
                         int32_t* found, float* scores, int32_t* index, float* boxes, float* rotation, float* translation,
                         float* hand);

/* WHOLE-FRAME SEARCH.  The frame path above shows the network the crop x crop square at the frame's centre, as the streaming app does;
 * an object held elsewhere in the field of view is not found.  These calls cover the frame with several such squares in ONE upload, one
 * forward at batch n and one download, and report the best of them.
 * A WINDOW is three int32 {frame, ox, oy}: the crop x crop square of frame `frame` whose top-left pixel is (ox, oy), 0 <= ox <= width - crop,
 * 0 <= oy <= height - crop, any parity.  Its pixels are converted exactly as the frame path converts the centre square (the chroma of a pixel
 * is that of its place in the full frame), then resized and normalised by the same two launches.
 * LIMITS of the plain (unrectified) calls: rotation is the network's output as the filter returns it, exactly as for the centre crop.  A
 * window's camera differs from the caller's by the principal point only (hep_window_cameras); no correction for the viewing ray of an off-axis
 * window is applied or claimed by them.  The RECTIFIED WINDOWS further below apply that correction exactly.
 *
 * The three functions below are host arithmetic: no handle, no HIP call.
 *
 * hep_tile_windows: the frames x ny x nx windows of a regular grid into windows_out [frames * ny * nx][3], frame-major, then row, then column.
 * Column i has ox = nx == 1 ? (width - crop) / 2 : (i * (width - crop)) / (nx - 1) in integer division, row r the same with height and ny: the
 * first and the last cell touch the frame's borders, and a 1 x 1 grid is the frame path's centre crop.  nx, ny or frames < 1, an odd height or
 * width, a crop larger than the frame, NULL: HEP_ERR_INVALID. */
int hep_tile_windows(int height, int width, int crop, int nx, int ny, int frames, int32_t* windows_out);
/* hep_window_cameras: camera [frames,6] holds the rows the caller passes for the CENTRE window of every frame (fx, fy, px, py, tz_scale,
 * image_scale); camera_out [n,6] gets, for window i, the row of its frame with
 *   px' = (float)((double)px - (double)(ox - (width - crop) / 2) * (double)resized / (double)crop)          py' likewise from oy and height,
 * the other four entries copied bit for bit.  hep_decode computes Tx = (cx / image_scale - px) * Tz / fx with cx / image_scale in pixels of the
 * resized image, so this shift is the exact pinhole statement of moving the window; the centre window's row is unchanged bit for bit.
 * camera must hold a row for every frame the table names.  NULL, n < 1, the frame geometry above, a window outside the frame: HEP_ERR_INVALID. */
int hep_window_cameras(const float* camera, const int32_t* windows, int n, int height, int width, int crop, int resized, float* camera_out);
/* hep_window_from_box: the window centred on a detection, for a loop that follows what it found.  box [4] = xmin, ymin, xmax, ymax in
 * network-input pixels (`size` = the session's size) of the window (ox, oy) it was found in, as the records carry it.  In double:
 *   cx = ox + 0.5 * (xmin + xmax) * crop / size;   *ox_out = clamp((int)floor(cx - 0.5 * crop + 0.5), 0, width - crop);   *oy_out likewise.
 * NULL, size < 1, the frame geometry above, (ox, oy) outside the frame: HEP_ERR_INVALID. */
int hep_window_from_box(const float* box, int ox, int oy, int height, int width, int crop, int size, int32_t* ox_out, int32_t* oy_out);

/* Best of the windows of every frame, one launch, no handle.  records: device memory, [n][slots][HEP_POSE_RECORD_WORDS] as hep_top1_device
 * (slots = 1) or hep_top_labels_device (slots = num_classes) writes them for a batch of n windows; windows [n][3] on the device.  For every
 * frame f < frames and slot c: among the windows i with windows[i].frame == f whose record (i, c) has found == 1, the one with the largest
 * score (float32 comparison) wins, ties to the lowest i; out_records [frames][slots] gets its record bit for bit and out_window [frames][slots]
 * gets i.  Without such a window - none found, or a frame no window names - the record is the not-found record of the two launches (found 0,
 * words 3, 78, 79 zero, the padding -1 / -1.0f elsewhere) and out_window is -1.  Windows of one frame need not be adjacent in the table.
 * Asynchronous on `stream`, no allocation, no host synchronisation.  NULL, slots outside 1..63, n < 1, frames < 1: HEP_ERR_INVALID. */
int hep_best_window_device(const uint32_t* records, int slots, const int32_t* windows, int n, int frames, uint32_t* out_records,
                           int32_t* out_window, void* stream);

/* hep_pose_from_i420 on n windows of `frames` frames in host memory: ONE upload (camera rows, table, frames), hep_preprocess_i420_windows_device's
 * launches, one forward at batch n, the top-detection launch, one download.  yuv [frames][height * width * 3 / 2]; windows [n][3] and
 * camera [n,6] on the host: one camera row PER WINDOW (hep_window_cameras makes them from per-frame rows).  Outputs as hep_pose_from_i420 with
 * one row per window; boxes are in network-input pixels of their window.  hep_poses_from_i420_windows: the per-label launch, outputs
 * [n][num_classes] as hep_poses_from_i420.  Mutex, pinned download and "allocated at first use, only ever grown" as for hep_pose_from_i420
 * (the staging buffer is shared with it).  Checked before any HIP call, HEP_ERR_INVALID with the reason in hep_last_error: NULL handle / yuv /
 * windows / camera / found, n or frames outside 1..max_batch, the frame geometry, a window whose frame index or offsets lie outside the frame. */
int hep_pose_from_i420_windows(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                               int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels,
                               int32_t* index, float* boxes, float* rotation, float* translation, float* hand);
int hep_poses_from_i420_windows(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                                int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index,
                                float* boxes, float* rotation, float* translation, float* hand);
/* The whole frame in one call: the grid of hep_tile_windows (frames * nx * ny <= max_batch windows) with the cameras of hep_window_cameras from
 * camera [frames,6] (the rows of the centre window, what hep_pose_from_i420 takes), the device work above, then hep_best_window_device and a
 * download of `frames` records.  Outputs as hep_pose_from_i420, one row per FRAME, plus window [frames]: the index of the winning window in
 * hep_tile_windows' order within the whole table (frame f's cell = window[f] - f * nx * ny; column = cell % nx, row = cell / nx), or -1.  Boxes
 * stay in the winning window's network-input pixels; translation is in the camera frame through the shifted principal point.  A 1 x 1 grid is
 * hep_pose_from_i420 bit for bit.  hep_poses_from_i420_tiled: per label, outputs and window are [frames][num_classes].  Checks as above, and
 * nx or ny < 1, a NULL window, frames * nx * ny > max_batch: HEP_ERR_INVALID. */
int hep_pose_from_i420_tiled(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                             const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels, int32_t* index,
                             float* boxes, float* rotation, float* translation, float* hand, int32_t* window);
int hep_poses_from_i420_tiled(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                              const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index, float* boxes,
                              float* rotation, float* translation, float* hand, int32_t* window);

/* RECTIFIED WINDOWS.  A plain window is a square cut out of the frame: 30 degrees off the optical axis it shows the object as a camera looking
 * along the axis sees it from the side, while the network - trained on crops whose principal point sits near their centre - reports the rotation
 * as if the camera looked straight at it.  The rectified window of {frame, ox, oy} is the frame RESAMPLED into the picture that a camera with the
 * caller's own intrinsics, rotated about the same centre to look along the window's viewing ray, would have taken (a pure rotation is a
 * homography: exact up to resampling).  The network sees a centre view with the centre camera row; its rotation, translation and hand joints are
 * then rotated back into the real camera's frame.  tests/_rectify.py states every rounding of what follows in numpy; all of it is float64.
 * CLAIMED: the geometry, up to resampling.  NOT MODELLED: lens distortion.  NOT MEASURED AND NOT CLAIMED: accuracy on trained weights.
 *
 * With s = resized / crop, ox_c = (width - crop) / 2, oy_c = (height - crop) / 2 (integer division) and (fx, fy, px, py) the frame's CENTRE camera
 * row (float32 widened): a = (ox - ox_c) s / fx, b = (oy - oy_c) s / fy, d = (a, b, 1) / sqrt(a a + b b + 1), k = 1 / (1 + d_z),
 *   R_w = [1 - d_x d_x k, -d_x d_y k, d_x;  -d_x d_y k, 1 - d_y d_y k, d_y;  -d_x, -d_y, d_z]
 * - the rotation about e_z x d that takes e_z to d, from + - * / sqrt alone; a point X_v of the virtual camera's frame is X_c = R_w X_v in the
 * real camera's.  The centre window gives the identity exactly.  A TABLE ROW is HEP_RECTIFY_ROW_DOUBLES doubles: R_w row-major, fx, fy, px, py.
 * Pixel (x, y) of the rectified crop: u = s (x + 0.5) - 0.5, v alike; q = ((u - px) / fx, (v - py) / fy, 1); p = R_w q; p_z <= 0 or not finite:
 * black.  Otherwise u' = fx p_x / p_z + px, X_f = (u' + 0.5) / s - 0.5 + ox_c (Y_f alike), sampled from the converted frame at 1/32 pixel with
 * integer bilinear weights that sum to 32768 and the four taps CLAMPED to the frame (replicate border).  The two resize launches of the frame path
 * follow unchanged.  The centre window's crop is the plain crop bit for bit.
 *
 * hep_rectify_windows (host arithmetic, no handle, no HIP call): camera [frames,6] = the centre rows, windows [n][3] -> table_out
 * [n][HEP_RECTIFY_ROW_DOUBLES].  NULL, n or frames < 1, the frame geometry, a window outside the frame or naming a frame >= frames, an fx or fy
 * that is not finite and positive: HEP_ERR_INVALID. */
#define HEP_RECTIFY_ROW_DOUBLES 13
int hep_rectify_windows(const float* camera, int frames, const int32_t* windows, int n, int height, int width, int crop, int resized,
                        double* table_out);
/* Going back to the frame (host arithmetic): pixel (x, y) of the network input (`size` pixels a side) of the rectified window `row` looks at
 * frame position xy_out[2] = (X_f, Y_f) - the chain above with size in place of crop in u = (resized / size) (x + 0.5) - 0.5; both NaN when the
 * ray points backwards.  BOXES OF THE RECTIFIED CALLS LIVE IN THE RECTIFIED WINDOW: map their corners or centre with this function, not with the
 * window's offsets.  hep_window_from_box_rectified: the plain window centred on a detection of a rectified window, for the follow loop - the
 * centre (0.5 (xmin + xmax), 0.5 (ymin + ymax)) of box [4] goes through the map above, then *ox_out = clamp((int)floor(X_f - 0.5 crop + 0.5), 0,
 * width - crop) and *oy_out likewise (a NaN gives 0).  NULL, size < 1, the frame geometry, a row whose fx or fy is not finite and positive:
 * HEP_ERR_INVALID. */
int hep_rectified_point_to_frame(const double* row, double x, double y, int height, int width, int crop, int resized, int size, double* xy_out);
int hep_window_from_box_rectified(const double* row, const float* box, int height, int width, int crop, int resized, int size, int32_t* ox_out,
                                  int32_t* oy_out);
/* Back-rotation of the records of n rectified windows, in place, one launch, no handle: records [n][slots][HEP_POSE_RECORD_WORDS] and table
 * [n][HEP_RECTIFY_ROW_DOUBLES] on the device.  For every record with found == 1, in double, each result rounded once to float32: the rotation
 * words hold the axis-angle vector in units of pi (the network's output), so R_out = R_w Rodrigues(pi rotation) and rotation' = Rodrigues^-1(R_out)
 * / pi; translation' = R_w translation; every hand joint' = R_w joint.  Words 0-8 (found, label, index, score, box - the box stays in
 * network-input pixels of the rectified window) and 78-79 are untouched; a record with found != 1 is untouched bit for bit, and so is every
 * record of a row whose R_w is exactly the identity.  Asynchronous on `stream`.  NULL, slots outside 1..63, n < 1: HEP_ERR_INVALID. */
int hep_derotate_records_device(uint32_t* records, int slots, const double* table, int n, void* stream);
/* The four one-call forms on rectified windows: ONE upload (camera rows, window table, the float64 table computed on the host, frames), the
 * rectified preprocess, one forward at batch n, the top-detection launch with every window's frame's CENTRE camera row unshifted, the
 * back-rotation launch, for the tiled calls hep_best_window_device, one download.  Arguments, outputs and checks as for the calls above, except:
 * camera is [frames,6] - the centre rows - for ALL FOUR, and an fx or fy that is not finite and positive is HEP_ERR_INVALID.  Boxes are in
 * network-input pixels of the RECTIFIED window; rotation, translation and hand are in the real camera's frame.  A 1 x 1 grid is
 * hep_pose_from_i420 bit for bit. */
int hep_pose_from_i420_windows_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                                         int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels,
                                         int32_t* index, float* boxes, float* rotation, float* translation, float* hand);
int hep_poses_from_i420_windows_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n, int crop,
                                          int resized, const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index,
                                          float* boxes, float* rotation, float* translation, float* hand);
int hep_pose_from_i420_tiled_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                                       const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* labels, int32_t* index,
                                       float* boxes, float* rotation, float* translation, float* hand, int32_t* window);
int hep_poses_from_i420_tiled_rectified(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, int crop, int resized, int nx, int ny,
                                        const float* camera, float score_threshold, int32_t* found, float* scores, int32_t* index, float* boxes,
                                        float* rotation, float* translation, float* hand, int32_t* window);

/* ADD and ADD-S of num_pairs (ground truth, prediction) poses over one object model: points [num_points,3]; rotations
 * as axis-angle vectors in radians (what _get_detections hands on: network output * pi), translations in the model's
 * unit.  add[i] = mean over ALL points of ||(R_gt p + t_gt) - (R_pr p + t_pr)|| (float64); add_s[i] = mean over the
 * ground-truth cloud subsampled with step = num_points / max_points + 1 (max_points = 1000 in the reference) of the
 * float32 distance to the nearest point of the equally subsampled predicted cloud.  A pose counts as correct when the
 * value is <= 0.1 * diameter (the caller's comparison).  The host variant copies through a temporary device buffer. */
int hep_pose_errors(int device, const float* points, int num_points, const float* rvec_gt, const float* t_gt,
                    const float* rvec_pred, const float* t_pred, int num_pairs, int max_points, double* add, double* add_s);
int hep_pose_errors_device(const float* points, int num_points, const float* rvec_gt, const float* t_gt,
                           const float* rvec_pred, const float* t_pred, int num_pairs, int max_points, double* add,
                           double* add_s, void* stream);

/* The per-image half of evaluate_model (pytorch-sandbox/eval/common.py:866-1121) for a whole batch in ONE launch on
 * device-resident detections: match the rows of every image against its ground truth and score the matched pose.
 * Stateless like hep_pose_errors_device: no handle, no allocation, no host synchronisation, asynchronous on `stream`.
 * One workgroup of 256 threads per image.
 * det_*: the rows of hep_filter_device, [batch][rows][4|1|1|3|3|63], padding -1, in descending score order; det_hand may
 * be NULL (the hand slot is then NaN).  points [num_points,3]: the object model.
 * gt: one row of HEP_SCORE_GT_DOUBLES = 88 doubles per image:
 *   0      has annotation (0 / 1)                      14-17  fx, fy, cx, cy
 *   1-4    box x1, y1, x2, y2, original-image pixels   18     image scale (network size / longer image side)
 *   5-7    axis-angle, radians                         19     has hand joints (0 / 1)
 *   8-10   translation                                 20-82  21 x 3 hand joints, metres
 *   11-13  drill-tip offset                            83-87  zero
 * DEFINITION, image b (what hmd_ego_pose_amd/evaluate.py::evaluate does for it):
 *   1. a candidate is a row with score > score_threshold (float32 compare); the first max_detections candidates are kept,
 *      THEN the rows whose label is not `label` are dropped (the cap counts every label)
 *   2. box = float32(box) / float32(scale), rotation = float32(r) * float32(pi), both in float32; IoU with the ground-truth
 *      box in float64 with the "+1" pixel convention of compute_overlap.pyx:33-73 (0 without intersection)
 *   3. the first candidate with IoU >= iou_threshold is the match (none when has annotation is 0).  Every considered
 *      candidate's score goes to out_scores [batch][max_detections] and its flag (1 matched, 0 not) to out_tp, compacted
 *      in order, padded with -1.0f / -1
 *   4. for the matched pair: ADD and ADD-S by the device code of hep_pose_errors_device (bit-identical to it on the same
 *      pair; the ground truth enters them ROUNDED TO FLOAT32, max_points as there) - and, on the table's float64 ground
 *      truth: |t_gt - t_pr|, the rotation difference in degrees (arccos of the clamped (trace(R_pr R_gt^T) - 1) / 2), the
 *      distance of the drill tips R tip + t, the mean pinhole reprojection distance over ALL model points in pixels, the
 *      mean distance of the 21 hand joints in mm
 * records: one row of HEP_SCORE_RECORD_DOUBLES = 16 doubles per image:
 *   0  considered count        4  matched IoU                  8   rotation difference, degrees
 *   1  matched (0 / 1)         5  ADD                          9   tip distance
 *   2  matched row, or -1      6  ADD-S                        10  reprojection distance, pixels
 *   3  matched score           7  translation difference       11  hand error, mm
 *   12-15 zero.  Slots 3-11 of an image without a match, and slot 11 without hand ground truth (or det_hand), hold NaN.
 * One annotation per image and one evaluated label (several of either: hep_score_scene_device below).  Checked before any HIP call, HEP_ERR_INVALID with the reason in
 * hep_last_error: a NULL pointer (except det_hand and stream), batch < 1, rows outside 1..256, max_detections outside
 * 1..rows, num_points < 1, max_points outside 1..1024 (what hep_pose_errors_device accepts). */
#define HEP_SCORE_GT_DOUBLES 88
#define HEP_SCORE_RECORD_DOUBLES 16
int hep_score_detections_device(const float* det_boxes, const float* det_scores, const int32_t* det_labels,
                                const float* det_rotation, const float* det_translation, const float* det_hand,
                                int batch, int rows, const double* gt, const float* points, int num_points, int max_points,
                                int label, float score_threshold, int max_detections, double iou_threshold,
                                double* records, float* out_scores, int32_t* out_tp, void* stream);

/* hep_score_detections_device for scenes: up to HEP_SCORE_MAX_ANNOTATIONS = 16 annotations per image over num_labels labels, every
 * label and every annotation scored in ONE launch (the generic loop of eval/common.py:912-1030 behind post_filter).  Stateless
 * like its sibling: no handle, no allocation, no host synchronisation, asynchronous on `stream`.  One workgroup of 256 threads
 * per (image, annotation slot).
 * det_*: as above; det_hand may be NULL.
 * gt: [batch][amax][HEP_SCORE_GT_DOUBLES], each row in the layout above with slot 83 = the annotation's label as an integral
 *   double; slot 0 marks a valid row, padding rows have slot 0 == 0.  Camera and scale (14-18) are repeated in every row of an
 *   image; the metrics of a pair read them from the pair's row, the image scale of the detection boxes comes from row 0.
 * points: the model clouds of all labels concatenated; point_offsets (HOST memory, [num_labels + 1], copied into the kernel
 *   argument): label l owns points [point_offsets[l], point_offsets[l+1]).
 * DEFINITION, image b (roundings as for hep_score_detections_device: float32 score compare, float32(box) / float32(scale),
 * float32(r) * float32(pi), float64 IoU with the "+1" convention compared with >=, ground truth rounded to float32 for ADD and
 * ADD-S only):
 *   1. a candidate is a row with score > score_threshold; the first max_detections candidates are kept (the cap counts every
 *      label), THEN the kept rows whose label is outside 0..num_labels-1 are dropped; the rest are the considered rows.  Their
 *      score, flag and label go to out_scores / out_tp / out_labels [batch][max_detections], compacted in row order and padded
 *      with -1.0f / -1 / -1; their number goes to out_count[b]
 *   2. each considered row of label l, in row order, looks at the valid annotations of label l: none - flag 0; otherwise the
 *      assigned annotation is the FIRST one with the maximal IoU (np.argmax), and the flag is 1 only when that IoU >=
 *      iou_threshold and the annotation has not been assigned before - then the annotation is taken.  A row whose best
 *      annotation is already taken is a false positive even if it overlaps another free annotation above the threshold
 *   3. every taken annotation's pair is scored exactly as hep_score_detections_device scores its pair, with the points of the
 *      annotation's label and that row's ground truth, tip offset, camera and hand joints; ADD and ADD-S are bit-identical to
 *      hep_pose_errors_device on the same pair with that label's cloud
 * records: [batch][amax][HEP_SCORE_RECORD_DOUBLES], one row per annotation slot:
 *   0  valid (0 / 1)           3  matched score                5-11  the seven metrics, as above
 *   1  matched (0 / 1)         4  matched IoU                  12    label
 *   2  matched row, or -1                                      13-15 zero
 *   Slots 3-11 of an unmatched row hold NaN, slot 11 also without hand ground truth or det_hand.  An invalid row has slots 0-1
 *   zero, slot 2 = -1, slots 3-11 NaN, slot 12 = -1; a valid row whose label is outside 0..num_labels-1 is treated as invalid
 *   (the device cannot refuse it without a synchronisation; hmd_ego_pose_amd.evaluate.gt_scene_table refuses it on the host).
 * Checked before any HIP call, HEP_ERR_INVALID with the reason in hep_last_error: a NULL pointer (except det_hand and stream),
 * batch < 1, rows outside 1..256, max_detections outside 1..rows, amax outside 1..16, num_labels outside 1..63,
 * point_offsets[0] != 0, an offset that does not increase (every label needs at least one point), max_points outside 1..1024. */
#define HEP_SCORE_MAX_ANNOTATIONS 16
int hep_score_scene_device(const float* det_boxes, const float* det_scores, const int32_t* det_labels,
                           const float* det_rotation, const float* det_translation, const float* det_hand,
                           int batch, int rows, const double* gt, int amax,
                           const float* points, const int32_t* point_offsets /* HOST, [num_labels + 1] */, int num_labels, int max_points,
                           float score_threshold, int max_detections, double iou_threshold,
                           double* records, float* out_scores, int32_t* out_tp, int32_t* out_labels, int32_t* out_count, void* stream);

/* Pose overlays: the valid annotations and the kept detections of every image of a batch drawn into the frames, in place, in ONE
 * launch - the step of eval/common.py:452-479 (projected cuboid with its centre point, optionally the 2D box and the hand skeleton:
 * generators/utils/visualization.py:85-117, 143-232, 234-290) from what the evaluators already hold on the device.  Stateless like
 * hep_score_scene_device: no handle, no allocation, no host synchronisation, asynchronous on `stream`.  The drawing is THIS
 * library's own definition in integer arithmetic (tests/_draw.py states it in numpy; the kernel matches it byte for byte): cv2's
 * line / circle rasterisers, LINE_AA and fonts are not restated (parity unpinned, as for the other cv2 conventions), no text.
 * frames: uint8 [batch][height][width][3], device memory, drawn in place; bytes are written in the channel order given.
 * gt: [batch][amax][HEP_SCORE_GT_DOUBLES] in the layout of hep_score_scene_device (0 valid, 1-4 box, 5-7 axis-angle in radians, 8-10
 *   translation, 19 has-hand, 20-82 joints, 83 label), or NULL: no annotation is drawn.  Rows with slot 0 == 0 or a label outside
 *   0..num_labels-1 (NaN included; the label is truncated to an integer) are skipped.
 * camera: [batch][5] float64 fx, fy, cx, cy, scale, or NULL: then slots 14-18 of row 0 of the image's gt rows.  Used when given.
 * det_*: the six arrays of hep_filter_device, [batch][rows][4|1|1|3|3|63]; all five of boxes, scores, labels, rotation, translation,
 *   or none (no detection is drawn; rows and max_detections are then not read); det_hand may be NULL: no detection hand is drawn.
 *   A candidate is a row with score > score_threshold (float32 compare; padding and NaN are none); the first max_detections
 *   candidates are kept, then the kept rows with a label outside 0..num_labels-1 are skipped.  Box = float32(box) / float32(scale),
 *   rotation = float32(r) * float32(pi) in float32: the roundings of hep_score_detections_device.
 * cuboids: device, float32 [num_labels][8][3], corner order of generators/colibri.py:121-151.  colours: HOST, uint8 [num_labels][3],
 *   copied into the kernel argument.
 * PROJECTION (float64, no contraction): R = Rodrigues of the axis-angle (float64 for an annotation, the float32 product for a
 *   detection; identity below an angle of 1e-12); cuboid corner p = ((R0 c0 + R1 c1) + R2 c2) + t per row of R, the centre is t, hand
 *   joints (annotation: slots 20-82, detection: det_hand) are camera-frame points as they are; u = (fx X) / Z + cx, v = (fy Y) / Z + cy.
 *   A point with Z <= 0 (or a NaN anywhere) is invalid.  Each coordinate - the box corners as well, unprojected - is saturated to
 *   [-8192, 8191], then truncated toward zero.
 * PRIMITIVES of a shape, in this order: (1) with HEP_DRAW_BOX2D the four segments (x1,y1)-(x2,y1)-(x2,y2)-(x1,y2)-(x1,y1); (2) with
 *   HEP_DRAW_CUBOID the twelve edges 0-1 1-2 2-3 0-3 4-5 5-6 6-7 4-7 0-4 1-5 2-6 3-7 (visualization.py:99-112), then the disc of radius 3
 *   at the centre; (3) with HEP_DRAW_HAND, for a shape that has joints, the 20 segments of the chains 0-1-2-3-4, 0-5-..-8, 0-9-..-12,
 *   0-13-..-16, 0-17-..-20.  A segment with an invalid end point and a disc with an invalid centre are skipped.
 * COVERAGE, exact in int64: pixel p = (x, y) belongs to the segment (a, b) of thickness t when its distance to the segment is at
 *   most t / 2: with d = b - a, L = d.d, s = (p - a).d:  s <= 0: 4 |p-a|^2 <= t^2;  s >= L: 4 |p-b|^2 <= t^2;  otherwise
 *   4 ((p-a) x d)^2 <= t^2 L  (a == b: the disc of radius t / 2).  Disc of radius 3: |p-c|^2 <= 9.  No gaps at t = 1; axis-aligned lines
 *   are 1, 3, 3, 5 pixels wide for t = 1..4.
 * ORDER AND COLOURS: per image the valid annotation slots in slot order, then the kept detections in row order; a later primitive
 *   overwrites an earlier one, a pixel nothing covers keeps its bytes.  Annotation: cuboid and disc (0,255,0), 2D box (0,127,0), hand
 *   (0,178,0).  Detection: cuboid, disc and hand the label's colour, 2D box (255,0,255).
 * One workgroup per 64 x 16 pixel tile; a thread writes only its own pixels (no atomics, deterministic), never outside
 * frames[0 .. batch*height*width*3).
 * Checked before any HIP call, HEP_ERR_INVALID with the reason in hep_last_error: NULL frames, cuboids or colours; gt and camera both
 * NULL; gt given with amax outside 1..16; a partial set of the five required det_* pointers (or det_hand alone); with detections, rows
 * outside 1..256 and max_detections outside 1..min(rows, HEP_DRAW_MAX_DETECTIONS); num_labels outside 1..63; thickness outside 1..8;
 * layer bits outside the three flags; batch < 1.  height or width outside 16..4096: HEP_ERR_UNSUPPORTED. */
#define HEP_DRAW_BOX2D 1
#define HEP_DRAW_CUBOID 2
#define HEP_DRAW_HAND 4
#define HEP_DRAW_MAX_DETECTIONS 64
int hep_draw_poses_device(uint8_t* frames, int batch, int height, int width,
                          const double* gt, int amax, const double* camera,
                          const float* det_boxes, const float* det_scores, const int32_t* det_labels,
                          const float* det_rotation, const float* det_translation, const float* det_hand, int rows,
                          float score_threshold, int max_detections,
                          const float* cuboids /* device [num_labels][8][3] */,
                          const uint8_t* colours /* HOST [num_labels][3], copied into the kernel argument */,
                          int num_labels, int ann_layers, int det_layers, int thickness, void* stream);

/* Object models rendered under poses: the uint8 instance mask (what hep_augment_6dof_device takes), the depth of the model and a filled
 * overlay of every image of a batch, from ONE z-buffered triangle rasteriser in three launches.  Stateless like hep_draw_poses_device: no
 * handle, no allocation, no host synchronisation, asynchronous on `stream`; the workspace is the caller's (hep_render_workspace_bytes:
 * batch * pmax * (num_vertices + 1) * 16 bytes, or a negative hep_status; 16-byte aligned).  The rendering is THIS library's own definition
 * (tests/_render.py states it in numpy and IS the definition; the kernels match it bit for bit).  No textures, shading, anti-aliasing,
 * near-plane clipping or non-triangle faces.
 * poses: device, float64 [batch][pmax][16], pmax in 1..HEP_RENDER_MAX_POSES: slot 0 valid, 1 the label, 2 the mask value, 3 reserved,
 *   4-12 the rotation MATRIX row-major, 13-15 the translation (the matrix, not the axis-angle: device code has only + - * /, floor and
 *   comparisons).  A row is skipped when slot 0 is 0, when the label is outside 0..num_labels-1 (NaN included) or when the mask value is
 *   outside 1..255 (tested as 1 <= value < 256); label and mask value are then truncated to integers.
 * camera: device, float64 [batch][5] fx, fy, cx, cy, scale - the layout of hep_draw_poses_device; scale is not used.
 * vertices: device, float32 [num_vertices][3]; faces: device, int32 [num_faces][3] indexing vertices; both counts in
 *   1..HEP_RENDER_MAX_ELEMENTS.  face_start: HOST, int32 [num_labels + 1], copied into the kernel argument: the faces of label c are
 *   face_start[c] .. face_start[c+1]; num_labels in 1..63.  A face with an index outside 0..num_vertices-1 is skipped, never read
 *   (the ABI cannot see device memory; hmd_ego_pose_amd.render.MeshSet checks every index on the host).
 * mask: uint8 [batch][height][width], 0 where nothing is rendered, else the winning pose's mask value; overwritten completely.
 * depth: float32 [batch][height][width], 0 where nothing is rendered, else float32 of the winning fragment's z; overwritten completely.
 * frames: uint8 [batch][height][width][3], blended in place where something is rendered, per channel
 *   out = (alpha * colour[label] + (256 - alpha) * old + 128) >> 8, alpha an integer in 0..256, colours HOST uint8 [num_labels][3];
 *   pixels that nothing covers keep their bytes.  Any of the three may be NULL, not all three.
 * PROJECTION, float64, no contraction: the camera-frame point is p = ((R0 v0 + R1 v1) + R2 v2) + t per row of R, with v the float32
 *   vertex widened; u = (fx X) / Z + cx, v = (fy Y) / Z + cy.  Sub-pixel integer coordinates: sx = floor(16 u + 0.5), with 16 u + 0.5
 *   saturated to [-8192*16, 8191*16] before the floor; sy alike.  A vertex with Z <= 0 or a NaN anywhere is invalid; a face with an
 *   invalid vertex is skipped whole.  There is NO near-plane clipping.
 * COVERAGE, exact in int64: pixel (x, y) has its centre at (16 x + 8, 16 y + 8).  With s the sign of the doubled area
 *   A' = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) the three edge functions are, for the edges (a, b) = (v1, v2), (v2, v0), (v0, v1) in
 *   this order, E_i(p) = dx (py - ay) - dy (px - ax) with (dx, dy) = s (b - a); they sum to A = |A'| > 0.  Faces of either winding are
 *   drawn, A' == 0 is skipped.  The pixel is inside when every E_i is positive, or zero on a top-left edge: dy < 0, or dy == 0 and
 *   dx > 0 (d and -d never both qualify and never both fail: two faces that share an edge never both own, and never both lose, a centre
 *   on it).
 * DEPTH, perspective-correct, float64: w_i = 1 / Z_i, invz = ((E0 w0 + E1 w1) + E2 w2) / A with E_i and A converted exactly, z = 1 / invz.
 * WINNER per pixel: the smallest (z as float64, pose slot, face index) in lexicographic order - equal depth goes to the lower slot, then
 *   to the lower face index; a NaN z never wins.  Deterministic: a thread keeps the winner of its own pixels, no atomics.
 * Never writes outside mask / depth [0 .. batch*height*width), frames [0 .. batch*height*width*3) and the workspace's stated bytes.
 * Checked before any HIP call, HEP_ERR_INVALID with the reason in hep_last_error: NULL poses, camera, vertices, faces, face_start or
 * workspace; all three outputs NULL; batch < 1; pmax outside 1..16; num_vertices or num_faces outside 1..HEP_RENDER_MAX_ELEMENTS;
 * num_labels outside 1..63; a face_start that starts below 0, decreases or ends beyond num_faces; frames without colours or with alpha
 * outside 0..256; a workspace that is misaligned or too small.  height or width outside 16..4096: HEP_ERR_UNSUPPORTED. */
#define HEP_RENDER_MAX_POSES 16
#define HEP_RENDER_MAX_ELEMENTS (1 << 24)
int64_t hep_render_workspace_bytes(int batch, int height, int width, int pmax, int num_vertices);
int hep_render_models_device(const double* poses, int batch, int pmax, const double* camera,
                             const float* vertices, int num_vertices, const int32_t* faces, int num_faces,
                             const int32_t* face_start /* HOST [num_labels + 1], copied into the kernel argument */, int num_labels,
                             int height, int width, uint8_t* mask, float* depth, uint8_t* frames,
                             const uint8_t* colours /* HOST [num_labels][3], or NULL without frames */, int alpha,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* Synthetic training frames: the models of hep_render_models_device SHADED from per-vertex colours and one light per image, composited
 * over the caller's backgrounds, and - in the same call - the labels hep_augment_6dof_device takes: the visible box of every pose slot from
 * the pixels that slot actually won, and the padded annotation tensors with hidden and off-frame objects dropped.  The same rasteriser
 * (one kernel, a compile-time switch), four launches (five with the annotation group).  Stateless like hep_render_models_device: no handle,
 * no allocation, no host synchronisation, asynchronous on `stream`; the workspace is the caller's (hep_synth_workspace_bytes: the bytes
 * and the refusals of hep_render_workspace_bytes; 16-byte aligned).  The definition is THIS library's own (tests/_synth.py states it in
 * numpy and IS the definition; the kernels match it bit for bit).  No textures, smooth shading, shadows or anti-aliasing.
 * poses, camera, vertices, faces, face_start, num_labels, height, width: those of hep_render_models_device, with the same row rule;
 *   PROJECTION, COVERAGE, DEPTH and the WINNER per pixel are exactly its.  mask, depth: its outputs, bit for bit; each may be NULL.
 * vertex_colours: device, uint8 [num_vertices][3].  face_normals: device, float64 [num_faces][3], indexed by the face's index in `faces`:
 *   plain data, computed by the caller (hmd_ego_pose_amd.synth.ShadedMeshSet: cross(v1 - v0, v2 - v0) / length in float64); a zero vector
 *   is legal.  lights: device, float64 [batch][8] = lx, ly, lz, ambient, diffuse, gain0, gain1, gain2; the direction is in the camera
 *   frame and the CALLER normalises it: device code has only + - * /, floor and comparisons.
 * SHADING of a pixel whose winner is face f of a slot, with vertices v0, v1, v2, the winner's edge values E0, E1, E2 at the pixel centre
 *   (exact int64) and w_i = 1 / Z_i of the vertex records; float64, no contraction, in this order:
 *   q_i = (double)E_i * w_i; den = (q0 + q1) + q2; b_i = q_i / den; c_k = (b0 C0k + b1 C1k) + b2 C2k, Cik the colour byte of vertex i
 *   widened, k = 0, 1, 2; with R the pose row's matrix and n the face's normal m_r = (R[r][0] n0 + R[r][1] n1) + R[r][2] n2;
 *   d = (m_0 lx + m_1 ly) + m_2 lz; d = d < 0 ? -d : d (two-sided: faces of either winding shade alike); s = ambient + diffuse * d;
 *   v_k = (c_k * s) * gain_k; t = v_k + 0.5; byte = !(t >= 0) ? 0 : (t >= 256 ? 255 : (int)floor(t)) - a NaN gives 0.
 * frames: uint8 [batch][height][width][3], REQUIRED, composited in place where something is rendered, per channel
 *   out = (alpha * byte + (256 - alpha) * old + 128) >> 8, alpha an integer in 0..256; pixels that nothing covers keep their bytes.
 * visible: int32 [batch][pmax][5], REQUIRED = min_x, min_y, max_x, max_y, count of the pixels slot k WON - the inclusive minimum and
 *   maximum of the pixel indices, per slot, not per mask value.  A slot that won none - a skipped row included - has count 0, INT_MAX
 *   in the two minima and INT_MIN in the two maxima.  Reduced in the workgroup, then by integer atomic min / max / add: the result does
 *   not depend on the order of arrival.
 * THE ANNOTATION GROUP, all eleven given or all NULL.  Inputs rvec, tvec float32 [batch][pmax][3], extra float32 [batch][pmax][2]: the
 *   caller's padded tensors, slot k belonging to pose row k.  Per image the slots are walked in order; a slot is KEPT when its row is
 *   rendered (the row rule) and count >= min_pixels (min_pixels >= 1); the n-th kept slot becomes row n of boxes float64 [batch][pmax][4]
 *   (the four integers of visible widened), labels, mask_values int32 [batch][pmax] (the pose row's values truncated as the renderer
 *   truncates them), out_rvec, out_tvec float32 [batch][pmax][3], out_extra float32 [batch][pmax][2] (gathered from slot k), slot_of
 *   int32 [batch][pmax] (k; -1 in the padding); num_gt int32 [batch] the number kept.  All padding is zeros.  The outputs must not
 *   overlap the inputs.
 * Never writes outside frames [0 .. batch*height*width*3), mask / depth [0 .. batch*height*width), visible [0 .. batch*pmax*5), the
 * annotation outputs' stated shapes and the workspace's stated bytes; never writes vertex_colours, face_normals, lights, rvec, tvec, extra.
 * Checked before any HIP call, HEP_ERR_INVALID with the reason in hep_last_error: NULL poses, camera, vertices, vertex_colours, faces,
 * face_normals, face_start, lights, frames, visible or workspace; a half-given annotation group; the ranges of hep_render_models_device
 * (batch, pmax, num_vertices, num_faces, num_labels, face_start); alpha outside 0..256; min_pixels < 1; a pointer that is not aligned
 * to its element; a workspace that is misaligned or too small.  height or width outside 16..4096: HEP_ERR_UNSUPPORTED. */
int64_t hep_synth_workspace_bytes(int batch, int height, int width, int pmax, int num_vertices);
int hep_synth_frames_device(const double* poses, int batch, int pmax, const double* camera,
                            const float* vertices, const uint8_t* vertex_colours, int num_vertices,
                            const int32_t* faces, const double* face_normals, int num_faces,
                            const int32_t* face_start /* HOST [num_labels + 1], copied into the kernel argument */, int num_labels,
                            const double* lights, int height, int width, uint8_t* frames, int alpha,
                            uint8_t* mask /* or NULL */, float* depth /* or NULL */, int32_t* visible,
                            const float* rvec, const float* tvec, const float* extra, int min_pixels,
                            double* boxes, int32_t* labels, int32_t* mask_values, float* out_rvec, float* out_tvec, float* out_extra,
                            int32_t* num_gt, int32_t* slot_of /* the annotation group: all or none */,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* BOP pose errors of matched (ground truth, estimate) pairs: MSSD and MSPD over a model's vertices and its set of symmetry transforms
 * from one entry point, VSD over rendered depth maps from a second.  Stateless like hep_render_models_device: no handle, no allocation, no
 * host synchronisation, asynchronous on `stream`.  This is BOP's mssd, mspd and vsd (bop19 visibility rule, step cost) RESTATED with this
 * library's own roundings: tests/_bop.py states them in numpy and IS the definition.  bop_toolkit is not part of this project's
 * environment: parity with it is UNPINNED, as it is for cv2.  Out of scope: BOP's error-based matching, the tlinear cost, depth PNGs.
 * pairs: device, float64 [n][HEP_BOP_PAIR_DOUBLES = 32], one row per pair:
 *   0      valid (0 / 1)                 4-12   R_gt, the rotation MATRIX row-major         16-24  R_est
 *   1      label                         13-15  t_gt                                        25-27  t_est
 *   2      image index (VSD's depth_test)                                                   28-31  fx, fy, cx, cy
 *   3      reserved
 *   A row is skipped and all of its outputs are NaN (its counts -1) when slot 0 is 0, when the label is outside 0..num_labels-1 (NaN
 *   included; the label is then truncated to an integer) or when a NaN sits anywhere in slots 4-27.
 * symmetries: device, float64 [num_symmetries][12], R row-major then t; symmetry_start: HOST, int32 [num_labels + 1], copied into the
 *   kernel argument: label c owns the transforms symmetry_start[c] .. symmetry_start[c+1], 1..HEP_BOP_MAX_SYMMETRIES = 64 of them.  Entry
 *   0 of every label must be the identity: hmd_ego_pose_amd.bop.SymmetrySet guarantees it, the ABI cannot see device memory.
 * vertices: device, float32 [num_vertices][3]; vertex_start: HOST, int32 [num_labels + 1]: label c owns vertex_start[c] .. vertex_start[c+1].
 * POINT ERRORS, float64, no contraction.  For pair i and symmetry s: R' = R_gt R_s, t' = R_gt t_s + t_gt, each element
 *   ((a0 b0 + a1 b1) + a2 b2) [+ t].  For vertex v widened: p = ((R0 v0 + R1 v1) + R2 v2) + t under the estimate, q alike under (R', t').
 *   mssd2(s) = max over v of ((dx dx + dy dy) + dz dz) with d = p - q; MSSD = sqrt(min over s of mssd2(s)): max and min are taken on the
 *   squared values - the selection is exact and independent of the order - and one sqrt comes at the end.  MSPD is the same with
 *   u = (fx X) / Z + cx, v = (fy Y) / Z + cy and du du + dv dv.  If any vertex has Z <= 0 (tested as not Z > 0) under the estimate or under any
 *   (R', t'), the pair's MSPD is NaN; MSSD is unaffected.  A NaN squared distance (non-finite input) makes the error it belongs to NaN.
 *   errors: float64 [n][2] MSSD, MSPD.  One workgroup per pair.
 * VSD.  depth_gt, depth_est: device, float32 [n][height][width]: what hep_render_models_device writes with batch = n and pmax = 1 for
 *   the pair's two poses, 0 where nothing is rendered.  depth_test: device, float32 [num_images][height][width] in the model's unit, 0 where
 *   there is no measurement, or NULL; pair i reads image slot 2; with a depth_test a row whose slot 2 is outside 0..num_images-1 is skipped
 *   too.  delta and taus (HOST, float64 [num_taus], 1..HEP_BOP_MAX_TAUS = 16) are in the model's unit.
 *   With zg, ze, zt the three depths of pixel (x, y) widened to float64 (zt = 0 without depth_test):
 *     a = (x - cx) / fx, b = (y - cy) / fy, k2 = (a a + b b) + 1: the squared ratio of distance-from-camera to depth - no sqrt anywhere;
 *     far(zm, zr, d): false when zm - zr <= 0, else k2 ((zm - zr)(zm - zr)) > d d;
 *     visible(zm): zm > 0 and (zt == 0 or not far(zm, zt, delta));  vis_gt = visible(zg);  vis_est = visible(ze) or (vis_gt and ze > 0);
 *     inter = vis_gt and vis_est, union = vis_gt or vis_est;  a pixel of inter costs 1 at tau when k2 ((zg - ze)(zg - ze)) >= tau tau;
 *     VSD(tau) = (cost_count(tau) + (union_count - inter_count)) / union_count, one float64 division of exactly converted integers;
 *     1.0 when union_count is 0.
 *   vsd: float64 [n][num_taus].  counts: int32 [n][2 + num_taus] union_count, inter_count, cost_count per tau.  The counters are summed in
 *   the caller's workspace (hep_bop_workspace_bytes: n * (2 + num_taus) * 4 bytes rounded up to 16, or a negative hep_status; 16-byte
 *   aligned) with integer atomics after a zeroing launch: the sums do not depend on the order.
 * Never writes outside errors [0 .. 2 n), vsd [0 .. n num_taus), counts [0 .. n (2 + num_taus)) and the workspace's stated bytes.
 * Checked before any HIP call, HEP_ERR_INVALID with the reason in hep_last_error: a NULL pointer (except depth_test and stream); n < 1;
 * num_labels outside 1..63; num_vertices or num_symmetries < 1; a start table that starts below 0, does not increase or ends past its
 * array; more than 64 symmetries for a label; num_taus outside 1..16; a tau or delta that is not finite and positive; num_images < 1 with a
 * depth_test; a workspace that is misaligned or too small.  height or width outside 16..4096: HEP_ERR_UNSUPPORTED. */
#define HEP_BOP_PAIR_DOUBLES 32
#define HEP_BOP_MAX_SYMMETRIES 64
#define HEP_BOP_MAX_TAUS 16
int hep_bop_point_errors_device(const double* pairs, int n, const float* vertices, int num_vertices,
                                const int32_t* vertex_start /* HOST [num_labels + 1] */,
                                const double* symmetries, int num_symmetries, const int32_t* symmetry_start /* HOST [num_labels + 1] */,
                                int num_labels, double* errors, void* stream);
int64_t hep_bop_workspace_bytes(int n, int num_taus);
int hep_bop_vsd_device(const double* pairs, int n, int num_labels, const float* depth_gt, const float* depth_est,
                       const float* depth_test /* or NULL */, int num_images, int height, int width, double delta,
                       const double* taus /* HOST [num_taus] */, int num_taus, double* vsd, int32_t* counts,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* Training side: anchor_targets_bbox, pytorch-sandbox/generators/utils/anchors.py:69-221 with the IoU
 * matrix of generators/utils/compute_overlap.pyx:33-73 and bbox_transform anchors.py:422-458, on device memory: per
 * image the ground-truth boxes [batch][kmax][4] (float64 x1,y1,x2,y2; the first num_gt[b] are valid), their labels,
 * transformation targets [batch][kmax][num_transform] and (optionally) hand coordinates [batch][kmax][63]; image_hw
 * [batch][2] = (height, width) of the unpadded image.  Outputs as the reference builds them (float32): labels
 * [batch][N][num_classes+1], regression [batch][N][5] = (ty,tx,th,tw,state), transformation [batch][N][num_transform+1],
 * coords [batch][N][64] (may be NULL); the last column is the anchor state: -1 ignore, 0 background, 1 object.
 * They feed hep_losses_device below. */
int hep_anchor_targets_device(const float* anchors, int num_anchors, const double* gt_boxes, const int32_t* gt_labels,
                              const float* gt_transform, const float* gt_coords, const int32_t* num_gt, const int32_t* image_hw,
                              int batch, int kmax, int num_classes, int num_transform, double negative_overlap, double positive_overlap,
                              float* labels, float* regression, float* transformation, float* coords, void* stream);

/* batch_iterate, pytorch-sandbox/hmdegopose/loss.py:54-99 - forward values of the five training losses on device
 * memory (float32, as torch computes them): focal classification loss (102-167), smooth-L1 box regression x 50
 * (170-219), rotation = mean (nearest, for symmetric objects) model-point distance between the predicted and the target
 * axis-angle rotation (273-428), translation = torch SmoothL1Loss on the object anchors (NaN when an image has none - the
 * reference's behaviour), smooth-L1 hand loss (222-271; gt_hand / hand may both be NULL).  Layouts as the generator and
 * the network produce them: gt_classification [batch][N][num_classes+1], classification [batch][N][num_classes]
 * (post-sigmoid), gt_regression [batch][N][5], regression [batch][N][4], gt_transformation [batch][N][num_rotation+3+3] =
 * (rotation, translation, is_symmetric, class index, anchor state), transformation [batch][N][num_rotation+3] =
 * cat(rotation head, decoded translation) (train.py:49), gt_hand [batch][N][num_hand+1], hand [batch][N][num_hand],
 * model_points [num_model_classes][num_points][3] (num_points <= 2048).  Outputs: per_image [batch][5] and losses [5] =
 * (classification, regression, rotation, translation, hand), the batch means.  The gradients are
 * hep_losses_backward_device below (the reference's optimiser loop, train.py:88-342, stays with the caller). */
int hep_losses_device(const float* gt_classification, const float* classification, const float* gt_regression, const float* regression,
                      const float* gt_transformation, const float* transformation, const float* gt_hand, const float* hand,
                      const float* model_points, int batch, int num_anchors, int num_classes, int num_rotation, int num_hand,
                      int num_model_classes, int num_points, float* per_image, float* losses, void* stream);

/* Backward of hep_losses_device: what the reference's autograd returns for batch_iterate.  Same inputs, sizes and
 * argument rules as hep_losses_device; grad_per_image [batch][5] is the upstream gradient of per_image (fold the
 * gradient of the batch means in first: grad_per_image[b][k] += grad_losses[k] * (k == 1 ? 50 : 1) / batch).  Outputs
 * (each may be NULL: that tensor is skipped; grad_hand needs hand): grad_classification [batch][N][num_classes],
 * grad_regression [batch][N][4], grad_transformation [batch][N][num_rotation+3] (rotation, then translation),
 * grad_hand [batch][N][num_hand].  Every element of a given output is written (zeros included): uninitialised memory
 * is fine.  workspace: int32 scratch of batch * (num_anchors + 4) entries on the device (per-image counts and the
 * compacted object anchors), owned by the caller and busy until the launches on `stream` end.  Asynchronous on
 * `stream`, no host synchronisation and no allocation; bit-reproducible (fixed reduction order, no float atomics).
 * Edges follow torch: the classification clamp passes the gradient at its bounds (inclusive), smooth-L1 gives 0 at a
 * zero residual, the translation gradient is 0 in an image without object anchors (whose translation loss is NaN).
 * An object anchor whose predicted or target rotation vector is exactly zero (no rotation axis; its forward distance
 * is NaN and the image's rotation loss 0) gets a rotation gradient of 0; the reference's autograd returns NaN there. */
int hep_losses_backward_device(const float* gt_classification, const float* classification, const float* gt_regression, const float* regression,
                               const float* gt_transformation, const float* transformation, const float* gt_hand, const float* hand,
                               const float* model_points, int batch, int num_anchors, int num_classes, int num_rotation, int num_hand,
                               int num_model_classes, int num_points, const float* grad_per_image, float* grad_classification,
                               float* grad_regression, float* grad_transformation, float* grad_hand, int32_t* workspace, void* stream);

/* The five head nets (regressor, classifier, rotation_net, translation_net, hand_net) as a TRAINABLE function of the five
 * BiFPN maps: forward and backward in HIP (csrc/k_head_grad.hip; the neck in front of them: hep_neck_*), so that the heads can be fitted on the device behind
 * hep_losses_device / hep_losses_backward_device.  Stateless: plain pointers and sizes, asynchronous on `stream`, no
 * allocation, no host synchronisation, argument checks before any HIP call, bit-reproducible (no float atomics).
 * BatchNorm uses its RUNNING statistics in forward and backward (the function the inference path computes; the
 * reference's freeze_bn): gamma and beta get gradients, the statistics never change.  Batch-statistics BatchNorm (the
 * reference's model.train()) is the hep_heads_*_bn group below with HEP_BN_BATCH.
 *
 * params: ONE flat fp32 device buffer (16-byte aligned) holding the head tensors in the reference's shapes and
 * state_dict order (regressor, classifier, rotation_net, translation_net, hand_net; per net conv_list.{i}.{depthwise
 * [W,1,3,3], pointwise [W,W,1,1], bias [W]}, bn_list.{level}.{i}.{weight, bias, running_mean, running_var},
 * then the header conv(s)); num_batches_tracked is not part of it.  hep_heads_param_count returns its length in
 * floats; hep_heads_param_layout writes the offset of every tensor in that order (offsets == NULL: returns how many).
 * feats[l]: the five maps, fp32 NCHW [batch][W][s_l][s_l] as hep_run_device exports them.  outs[k]: [batch][N][K_k] in
 * the inference layout (regression, classification post-sigmoid, rotation, translation raw, hand).
 * workspace: hep_heads_workspace_bytes bytes on the device, 16-byte aligned, owned by the caller.  The forward leaves
 * in it what the backward needs: hand the SAME workspace (untouched) and the same params to hep_heads_backward_device.
 * grad_outs[k]: cotangents [batch][N][K_k].  grad_params: same layout as params, every element written (running
 * statistics: zero).  grad_feats: five NCHW buffers, or NULL to skip the map gradients.
 * Supported: phi 0..7, num_classes 1..63, size a multiple of 128 in [128, 2048], batch >= 1 (HEP_ERR_UNSUPPORTED otherwise). */
int64_t hep_heads_param_count(int phi, int num_classes);
int hep_heads_param_layout(int phi, int num_classes, int64_t* offsets, int capacity);
int64_t hep_heads_workspace_bytes(int phi, int num_classes, int size, int batch);
int hep_heads_forward_device(const float* params, const float* const feats[5], int phi, int num_classes, int size, int batch,
                             float* const outs[5], void* workspace, size_t workspace_bytes, void* stream);
int hep_heads_backward_device(const float* params, const float* const grad_outs[5], int phi, int num_classes, int size, int batch,
                              float* grad_params, float* const grad_feats[5], void* workspace, size_t workspace_bytes, void* stream);

/* The same three calls with a BatchNorm mode.  HEP_BN_RUNNING: exactly the calls above (they are this one with that mode).
 * HEP_BN_BATCH: F.batch_norm(training = True) - what the reference's train.py computes under model.train().  Every BatchNorm
 * normalises with the mean and the biased variance of the rows it sees (one level's batch * s_l * s_l pixels: bn_list.{level}.{i}
 * is per level, the convs are shared), eps 1e-3; the backward is that function's:
 *   d beta = sum d a,  d gamma = sum d a x^,  d z = gamma rstd (d a - d beta / N - x^ d gamma / N);
 * the conv bias in front of a BatchNorm gets exactly zero (its gradient is analytically zero), the running statistics too.
 * stats_out (forward): a buffer in the layout of params, or NULL.  Its running_mean / running_var elements receive
 *   (1 - momentum) running + momentum batch   (the variance unbiased, N / (N - 1));
 * no other element is touched and params stays const; the caller owns num_batches_tracked.  The reference uses momentum 0.01.
 * A BatchNorm with N < 2 rows (size 128, batch 1: a 1 x 1 top level) is HEP_ERR_UNSUPPORTED, as torch raises there.
 * hep_heads_workspace_bytes_bn: the workspace of that mode (batch >= running); forward and backward take the same mode. */
#define HEP_BN_RUNNING 0
#define HEP_BN_BATCH 1
int64_t hep_heads_workspace_bytes_bn(int phi, int num_classes, int size, int batch, int bn_mode);
int hep_heads_forward_device_bn(const float* params, const float* const feats[5], int phi, int num_classes, int size, int batch,
                                float* const outs[5], void* workspace, size_t workspace_bytes, int bn_mode, float momentum, float* stats_out,
                                void* stream);
int hep_heads_backward_device_bn(const float* params, const float* const grad_outs[5], int phi, int num_classes, int size, int batch,
                                 float* grad_params, float* const grad_feats[5], void* workspace, size_t workspace_bytes, int bn_mode,
                                 void* stream);

/* The BiFPN neck (every cell of bifpn.{r}; reference efficientdet/model.py:194-266) as a TRAINABLE function of its parameters
 * and the three backbone taps P3 / P4 / P5: forward and backward in HIP (csrc/k_neck_grad.hip).  Same conventions as the
 * hep_heads_* group: stateless, asynchronous on `stream`, no allocation, no host synchronisation, argument checks before any
 * HIP call, bit-reproducible (no float atomics), BatchNorm with its RUNNING statistics in forward and backward (gamma and beta
 * get gradients, the statistics get exactly zero; batch statistics: hep_neck_*_bn below).  Fast-attention fusion w = relu(p) / (sum relu(p) + 1e-4); relu'(p) = 0 for
 * p <= 0.  Max-pool gradients go to the FIRST maximal element in row-major order of the zero-padded 3 x 3 window (padding:
 * one column right, one row below).  The taps are inputs; grad_taps gives their gradient (what hep_backbone_backward_device
 * takes).
 *
 * params: ONE flat fp32 device buffer (16-byte aligned) with every bifpn.* tensor in the reference's shapes and state_dict
 * order, num_batches_tracked left out (per cell the eight fusion vectors p6_w1 .. p7_w2, then per node depthwise [W,1,3,3],
 * pointwise [W,W,1,1], bias [W], bn weight / bias / running_mean / running_var; cell 0 ends with its six lateral convs:
 * weight [W,C,1,1], bias, BatchNorm).  hep_neck_param_count: its length in floats; hep_neck_param_layout: the offset of every
 * tensor in that order (offsets == NULL: returns how many).
 * taps[t]: fp32 NCHW [batch][tap_channels[t]][s][s], s = size/8, size/16, size/32.  feats[l]: fp32 NCHW [batch][W][s_l][s_l],
 * the layout hep_heads_forward_device takes.  workspace: hep_neck_workspace_bytes bytes, 16-byte aligned, owned by the caller;
 * the forward leaves in it what the backward needs (an aligned copy of params included): hand the SAME workspace, untouched, to
 * hep_neck_backward_device.  grad_feats[l]: cotangents of the five maps.  grad_params: layout of params, every element
 * written.  grad_taps: three NCHW buffers, or NULL to skip the tap gradients.
 * Supported: phi 0..5 (phi 6 / 7 fuse by plain sums: HEP_ERR_UNSUPPORTED), size a multiple of 128 in [128, 2048], batch >= 1.
 *
 * hep_neck_stage_*: introspection for tests.  Stage i names an fp32 tensor the forward leaves in the workspace at
 * offset_bytes, laid out NHWC: dims = {batch, s, s, W}, channels contiguous.  Names: "p6_pre" (the p5_to_p6 lateral's
 * output, pooled into P6 of cell 0), "bifpn0_p6_in" (that pool's result, pooled again into P7), and "bifpn{r}_p3" ..
 * "bifpn{r}_p7", the outputs of cell r (p3 .. p6 are pooled by the cell's down path).  *name points to thread-local storage. */
int64_t hep_neck_param_count(int phi);
int hep_neck_param_layout(int phi, int64_t* offsets, int capacity);
int64_t hep_neck_workspace_bytes(int phi, int size, int batch);
int hep_neck_forward_device(const float* params, const float* const taps[3], int phi, int size, int batch, float* const feats[5],
                            void* workspace, size_t workspace_bytes, void* stream);
int hep_neck_backward_device(const float* params, const float* const grad_feats[5], int phi, int size, int batch, float* grad_params,
                             float* const grad_taps[3], void* workspace, size_t workspace_bytes, void* stream);
/* With a BatchNorm mode, as hep_heads_*_bn: HEP_BN_RUNNING is exactly the calls above; HEP_BN_BATCH normalises every BatchNorm
 * (the six laterals and every node) with the statistics of its map's batch * s * s rows, the backward is that function's
 * (every conv bias feeds a BatchNorm: its gradient is written as exactly zero), stats_out (layout of params, or NULL) receives the
 * updated running_mean / running_var.  batch * (size / 128)^2 < 2 (P7 of one 128 image): HEP_ERR_UNSUPPORTED. */
int64_t hep_neck_workspace_bytes_bn(int phi, int size, int batch, int bn_mode);
int hep_neck_forward_device_bn(const float* params, const float* const taps[3], int phi, int size, int batch, float* const feats[5],
                               void* workspace, size_t workspace_bytes, int bn_mode, float momentum, float* stats_out, void* stream);
int hep_neck_backward_device_bn(const float* params, const float* const grad_feats[5], int phi, int size, int batch, float* grad_params,
                                float* const grad_taps[3], void* workspace, size_t workspace_bytes, int bn_mode, void* stream);
int hep_neck_stage_count(int phi);
int hep_neck_stage_info(int phi, int size, int batch, int i, const char** name, int64_t dims[4], int64_t* offset_bytes);

/* The EfficientNet trunk (backbone_net.model.*: stem conv + BN + swish and every MBConv block - expand 1x1, depthwise k3 / k5 at
 * stride 1 / 2 with TF-SAME padding, squeeze-excite, project 1x1, skip add; reference efficientnet/model.py:69-104,
 * efficientdet/model.py:436-458) as a TRAINABLE function image [batch][3][size][size] -> (P3, P4, P5): forward and backward in
 * HIP (csrc/k_backbone_grad.hip).  Same conventions as the hep_neck_* group: stateless, asynchronous on `stream`, no
 * allocation, no host synchronisation, argument checks before any HIP call, bit-reproducible (no float atomics), BatchNorm
 * with its RUNNING statistics in forward and backward (gamma and beta get gradients, the statistics get exactly zero; batch
 * statistics: hep_backbone_*_bn below).
 *
 * Drop-connect (efficientnet/utils.py:85-94) enters as data.  branch_scale: fp32 [blocks][batch] on the device, or NULL for
 * all ones; a block that adds its input computes y = bn2(project) * branch_scale[block][image] + input, the other blocks
 * ignore their row.  Hand the same table (or NULL) to forward and backward.
 *
 * params: ONE flat fp32 device buffer (16-byte aligned) with every float backbone_net.* tensor in the reference's shapes and
 * state_dict order, num_batches_tracked left out (_conv_stem weight [stem,3,3,3], _bn0 weight / bias / running_mean /
 * running_var, then per block [_expand_conv [cexp,cin,1,1], _bn0], _depthwise_conv [cexp,1,k,k], _bn1, _se_reduce weight
 * [se,cexp,1,1] and bias, _se_expand weight [cexp,se,1,1] and bias, _project_conv [cout,cexp,1,1], _bn2).
 * hep_backbone_param_count: its length in floats; hep_backbone_param_layout: the offset of every tensor in that order
 * (offsets == NULL: returns how many).
 * image: fp32 NCHW, contiguous.  taps[t]: fp32 NCHW [batch][tap_channels[t]][s][s], s = size/8, size/16, size/32: what
 * hep_neck_forward_device takes.  workspace: hep_backbone_workspace_bytes bytes, 16-byte aligned, owned by the caller; the
 * forward leaves in it what the backward needs (aligned copies of params and of the image included): hand the SAME workspace,
 * untouched, to hep_backbone_backward_device.  grad_taps[t]: cotangents of the three taps.  grad_params: layout of params,
 * every element written.  grad_image: an NCHW buffer like image, or NULL to skip the image gradient.
 * Supported: phi 0..7, size a multiple of 128 in [128, 2048], batch >= 1 (HEP_ERR_UNSUPPORTED otherwise).
 *
 * hep_backbone_stage_*: introspection for tests.  Stage i names an fp32 tensor the forward leaves in the workspace at
 * offset_bytes, laid out NHWC: dims = {batch, s, s, C}, channels contiguous.  Names: "stem" (after BN and swish) and
 * "block{i}", the output of MBConv block i.  *name points to thread-local storage. */
int64_t hep_backbone_param_count(int phi);
int hep_backbone_param_layout(int phi, int64_t* offsets, int capacity);
int64_t hep_backbone_workspace_bytes(int phi, int size, int batch);
int hep_backbone_forward_device(const float* params, const float* image, const float* branch_scale, int phi, int size, int batch,
                                float* const taps[3], void* workspace, size_t workspace_bytes, void* stream);
int hep_backbone_backward_device(const float* params, const float* const grad_taps[3], const float* branch_scale, int phi, int size, int batch,
                                 float* grad_params, float* grad_image, void* workspace, size_t workspace_bytes, void* stream);
/* With a BatchNorm mode, as hep_heads_*_bn: HEP_BN_RUNNING is exactly the calls above; HEP_BN_BATCH normalises the stem's
 * BatchNorm and every block's bn0 / bn1 / bn2 with the statistics of its map's batch * s * s rows (the squeeze-excite, the
 * branch scale and the skip add stay behind bn2 as they are), the backward is that function's, stats_out (layout of params, or
 * NULL) receives the updated running_mean / running_var.  The smallest map has batch * 16 rows, so no size is refused. */
int64_t hep_backbone_workspace_bytes_bn(int phi, int size, int batch, int bn_mode);
int hep_backbone_forward_device_bn(const float* params, const float* image, const float* branch_scale, int phi, int size, int batch,
                                   float* const taps[3], void* workspace, size_t workspace_bytes, int bn_mode, float momentum, float* stats_out,
                                   void* stream);
int hep_backbone_backward_device_bn(const float* params, const float* const grad_taps[3], const float* branch_scale, int phi, int size, int batch,
                                    float* grad_params, float* grad_image, void* workspace, size_t workspace_bytes, int bn_mode, void* stream);
int hep_backbone_stage_count(int phi);
int hep_backbone_stage_info(int phi, int size, int batch, int i, const char** name, int64_t dims[4], int64_t* offset_bytes);

/* Synchronised BatchNorm: HEP_BN_BATCH of the three parts with the row set of every BatchNorm being the UNION over all
 * replicas of a data-parallel step (the reference's utils/sync_batchnorm).  The function, its backward, stats_out and every
 * argument rule are those of the *_bn group with HEP_BN_BATCH; there is no bn_mode argument.  What crosses the replicas are
 * double sums, through a hook of the caller's:
 *   forward   per BatchNorm sum z [C], sum z^2 [C] and this replica's row count R; mean = S / N, var = max((Q - mean S) / N, 0)
 *             in double from the global sums, the running-statistics update with the unbiased N / (N - 1) of the GLOBAL N:
 *             every replica writes the same values to stats_out.
 *   backward  per BatchNorm this replica's d gamma [C], d beta [C] (before their rounding to float) and R; the d z correction
 *             uses the global sums, rounded once, and the global N.  grad_params holds this replica's LOCAL contribution in
 *             EVERY element (d gamma and d beta included): the plain sum of grad_params over the replicas is the gradient of
 *             the global-batch function.
 * All sums of one launch (25 BatchNorms in the heads, 1 in the neck and the backbone) lie in ONE contiguous, 16-byte aligned
 * block of doubles inside the workspace; sum is called once per block:
 *   data      device memory inside the workspace handed to the call; count elements, double (is_double != 0; float otherwise)
 *   contract  when the work that sum enqueued on stream has run, every element holds the sum over all replicas; it may
 *             enqueue and return.  All replicas make the same sequence of calls with the same counts; the sequence depends on
 *             phi, num_classes and size, never on batch: shards may be uneven (the row counts travel in the block).
 *   failure   a non-zero return: the entry point launches nothing further and returns HEP_ERR_DEVICE, the error text names the hook.
 * sync == NULL or sync->sum == NULL: HEP_ERR_INVALID before any HIP call.  A replica cannot know the global row count, so any
 * local batch >= 1 is accepted here; "at least 2 rows per BatchNorm" is the caller's to check on the global batch.
 * An identity hook (one replica) gives HEP_BN_BATCH bit for bit.  The *_workspace_bytes_sync size is >= the batch-mode size. */
typedef int (*hep_sum_fn)(void* ctx, void* data, int64_t count, int is_double, void* stream);
typedef struct hep_sync { hep_sum_fn sum; void* ctx; } hep_sync;
int64_t hep_heads_workspace_bytes_sync(int phi, int num_classes, int size, int batch);
int hep_heads_forward_device_sync(const float* params, const float* const feats[5], int phi, int num_classes, int size, int batch,
                                  float* const outs[5], void* workspace, size_t workspace_bytes, float momentum, float* stats_out,
                                  const hep_sync* sync, void* stream);
int hep_heads_backward_device_sync(const float* params, const float* const grad_outs[5], int phi, int num_classes, int size, int batch,
                                   float* grad_params, float* const grad_feats[5], void* workspace, size_t workspace_bytes,
                                   const hep_sync* sync, void* stream);
int64_t hep_neck_workspace_bytes_sync(int phi, int size, int batch);
int hep_neck_forward_device_sync(const float* params, const float* const taps[3], int phi, int size, int batch, float* const feats[5],
                                 void* workspace, size_t workspace_bytes, float momentum, float* stats_out, const hep_sync* sync, void* stream);
int hep_neck_backward_device_sync(const float* params, const float* const grad_feats[5], int phi, int size, int batch, float* grad_params,
                                  float* const grad_taps[3], void* workspace, size_t workspace_bytes, const hep_sync* sync, void* stream);
int64_t hep_backbone_workspace_bytes_sync(int phi, int size, int batch);
int hep_backbone_forward_device_sync(const float* params, const float* image, const float* branch_scale, int phi, int size, int batch,
                                     float* const taps[3], void* workspace, size_t workspace_bytes, float momentum, float* stats_out,
                                     const hep_sync* sync, void* stream);
int hep_backbone_backward_device_sync(const float* params, const float* const grad_taps[3], const float* branch_scale, int phi, int size,
                                      int batch, float* grad_params, float* grad_image, void* workspace, size_t workspace_bytes,
                                      const hep_sync* sync, void* stream);

/* preprocess_image (reference generators/colibri_common.py:622-656): device uint8 RGB [batch, height, width, 3] ->
 * device float32 [batch, size, size, 3]: resize by scale = size / max(height, width) (8-bit bilinear, OpenCV
 * INTER_LINEAR fixed-point convention - restated, parity unpinned: cv2 is absent here; skipped when scale == 1, every
 * 256x256 syn_colibri frame), then ((x / 255) - mean) / std with numpy's float64 intermediate steps (the no-resize
 * output is bit-identical to the numpy code), zero-padded at the bottom / right.  Hand the result to hep_run_device as
 * the NCHW view of NHWC memory (strides {size*size*3, 1, size*3, 3}), exactly what eval/common.py:397 does; the camera
 * vector's image_scale entry is size / max(height, width). */
int hep_preprocess_u8_device(hep_handle* h, const uint8_t* rgb_hwc, int batch, int height, int width,
                             float* out_hwc, void* stream);

/* The frame callback of the reference's streaming app (unity-sandbox/WebRTCNetCoreSandbox/Program.cs:140-205, 381-445) on
 * the device: 4:2:0 planar frames [batch][height * width * 3 / 2] bytes as WebRTC delivers them -> cvtColor(YUV2BGR_YV12)
 * (the app reads its I420 bytes as YV12: U and V exchanged, kept) -> centre crop `crop` x `crop` -> resize to `resized` x
 * `resized` -> ResizeAndNormalizeMat to the session's size (float32 / 255, - mean, / std applied to B, G, R in that order as
 * the C# Scalars meet a BGR Mat, zero-padded) -> out_hwc float32 [batch, size, size, 3] in B, G, R channel order, the
 * NHWC memory of blobFromImage(swapRB = false)'s NCHW result (hand it to hep_run_device with strides
 * {size*size*3, 1, size*3, 3}).  The app uses crop 256, resized 512.  OpenCV's BT.601 fixed-point conversion and 8-bit
 * INTER_LINEAR are restated from its source: parity unpinned (cv2 is absent from the build image).
 * Not for stream capture (the handle orders its scratch frames across streams with an event of its own): HEP_ERR_UNSUPPORTED
 * when `stream` is capturing. */
int hep_preprocess_i420_device(hep_handle* h, const uint8_t* yuv, int batch, int height, int width, int crop, int resized,
                               float* out_hwc, void* stream);
/* The same for n windows of a table (WHOLE-FRAME SEARCH above): yuv [frames][height * width * 3 / 2] and windows [n][3] int32
 * {frame, ox, oy} on the device, out_hwc float32 [n, size, size, 3].  Image i is bit for bit the frame path's arithmetic with the crop
 * taken at (ox, oy) of frame `frame`.  The table lives in device memory and is TRUSTED, as every device table of this ABI is (a window
 * outside its frame reads outside the frames; the host calls check their table before the upload).  n <= max_batch: the handle's
 * scratch frames, their event across streams and the refusal under stream capture are those of hep_preprocess_i420_device.
 * NULL, frames < 1, the frame geometry, n outside 1..max_batch: HEP_ERR_INVALID before any HIP call. */
int hep_preprocess_i420_windows_device(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows, int n,
                                       int crop, int resized, float* out_hwc, void* stream);

/* The same for n RECTIFIED windows (RECTIFIED WINDOWS above): table [n][HEP_RECTIFY_ROW_DOUBLES] on the device next to windows [n][3], of which
 * only the frame index is read.  Both tables are trusted device memory; every tap is clamped to its frame, so no value of `table` - a NaN row
 * included - reads outside it.  Scratch frames, event, refusal under stream capture and the n <= max_batch rule as above.
 * NULL, frames < 1, the frame geometry, n outside 1..max_batch: HEP_ERR_INVALID before any HIP call. */
int hep_preprocess_i420_rectified_device(hep_handle* h, const uint8_t* yuv, int frames, int height, int width, const int32_t* windows,
                                         const double* table, int n, int crop, int resized, float* out_hwc, void* stream);

/* Introspection used by tests, bench.py and DESIGN.md tables. */
int hep_debug_tensor_count(const hep_handle* h);
int hep_debug_tensor_info(const hep_handle* h, int i, const char** name, int64_t dims[4] /* B,H,W,C */);
/* Copy stage tensor `name` of the last run (as fp32, NHWC) into host memory. */
int hep_debug_tensor(hep_handle* h, const char* name, int batch, float* out, size_t capacity_floats);
int hep_kernel_count(const hep_handle* h, int batch);      /* launches in one forward                      */
/* Per-launch description of the forward plan: name, algorithmic bytes and flops for `batch`. */
int hep_kernel_info(const hep_handle* h, int batch, int i, const char** name, double* bytes, double* flops);
/* fp8 sessions: the calibrated per-tensor activation scale of launch i (0 when the launch has no e4m3 operands). */
int hep_fp8_scale(const hep_handle* h, int i, float* a_scale);
/* HEP_FP8 sessions fix one power-of-two scale per quantised GEMM input at hep_create, from the amax of that tensor on two
 * frames of pseudo-normal noise with 2x headroom; the e4m3 conversion SATURATES silently at +-448 * scale.  Real frames
 * (normalised to about [-2.1, 2.6], structured, zero-padded) through trained weights can exceed that range in the deeper
 * layers: recalibrate on representative frames before serving.  frames: contiguous fp32 [batch,3,S,S] on the session's
 * device (the first min(batch, frames per lane) frames are used: all of max_batch with the default single lane, max_batch / HEP_LANES otherwise).  Not to be called while a run is in flight on this handle.
 * Replaces the fixed scales of ONNXRuntime's static quantisation tables, which the reference does not use (fp32 ORT). */
int hep_calibrate_fp8(hep_handle* h, const float* frames_nchw_device, int batch);
/* Device function (as rocprofv3 --kernel-trace names it, e.g. "sep_kernel<true>") behind launch i. */
int hep_kernel_symbol(const hep_handle* h, int i, const char** symbol);
/* The launch list of the session that hep_create_from_memory(pack, ..., phi, size, max_batch, dtype, device, flags) would build,
 * planned on the host alone: no HIP call is made, so it works on a machine without a GPU.  The plan knobs are read from the
 * environment as at hep_create (HEP_LANES included); the compute-unit count, which a session asks its device for, is 256.
 * Text, one line per launch in launch order, each "<device function> | <launch name>\n" with the strings of hep_kernel_symbol and
 * hep_kernel_info, NUL-terminated.  *needed (optional) receives the byte count including the NUL; out may be NULL to ask for
 * it, otherwise capacity must be at least that.  The weights decide nothing but the class count (read from the classifier header). */
int hep_plan_launch_list(const void* pack, size_t pack_bytes, int phi, int size, int max_batch, int dtype, unsigned flags,
                         char* out, size_t capacity, size_t* needed);
/* Time `iters` replays of the forward at `batch` with HIP events on the handle's own stream; when
 * per_kernel_ms is non-NULL (length hep_kernel_count) also run the forward eagerly with a HIP event
 * in front of every launch and return each launch's average in-sequence duration. */
int hep_profile(hep_handle* h, int batch, int iters, float* total_ms_per_iter, float* per_kernel_ms);
/* Throughput cost of every launch: launch i is issued `iters` times on each of `nstreams` HIP streams
 * at once and per_kernel_ms[i] = wall time / (iters * nstreams).  A launch that fills the chip costs
 * its full duration, one that leaves CUs idle costs less than it takes alone (bench.py keeps several
 * batches in flight, so this - not the stand-alone duration - is what a launch costs the pipeline). */
int hep_profile_concurrent(hep_handle* h, int batch, int iters, int nstreams, float* per_kernel_ms);

/* Training input (the reference's host generator in front of the training step, pytorch-sandbox/generators/common.py:348-479
 * augment_6DoF_image_and_annotations / augmentation_6DoF and :543-607 preprocess_group_entry), on device memory, in three launches
 * (four when max(height, width) != size), with no host synchronisation and no allocation: the caller owns the workspace
 * (hep_augment_workspace_bytes; >= 0, or a negative hep_status).
 * Inputs: rgb_hwc uint8 [batch][height][width][3]; mask uint8 [batch][height][width]; xform float64 [batch][9] = the forward matrix
 * of cv2.getRotationMatrix2D((cx, cy), -angle, scale) (6, row major, computed by the caller on the host), the angle in radians, the
 * scale, apply (0: leave this image alone); camera_k [batch][4] = fx, fy, px, py; per annotation (the first num_gt[b] of kmax):
 * boxes float64 x1,y1,x2,y2, labels, mask_values (the mask byte of the object), rvec / tvec float32 [3], extra [2] = is_symmetric,
 * class index.
 * Per image: the mask is warped (INTER_NEAREST); when the warped mask has no non-zero pixel, when apply is 0, or when the scale on
 * the device is outside [0.25, 4], the image, boxes and poses pass through unchanged and applied[b] = 0.  Otherwise applied[b] = 1:
 * the image is warped (INTER_LINEAR, constant border 0), each annotation's box is the extent of its mask value in the warped mask
 * (an annotation with no pixel left is removed, the order of the rest is kept), its pose becomes R' = Rz(angle) R(rvec),
 * t' = Rz t, t'_z /= scale (float32 in, double arithmetic, float32 out).  Then preprocess_group_entry: image_scale = size /
 * max(height, width), boxes * image_scale, rotation / pi, the frame resized when max(height, width) != size (the 8-bit resize of
 * hep_preprocess_u8_device), normalised with that entry point's arithmetic and zero-padded.
 * Outputs: image_nchw float32 [batch][3][size][size] (16-byte aligned; what hep_backbone_forward_device takes); mask_out (may be
 * NULL) uint8 [batch][height][width], the mask that goes with the image; camera [batch][6] = fx, fy, px, py,
 * translation_scale_norm, image_scale; gt_boxes float64 [batch][kmax][4], gt_labels [batch][kmax], gt_transform [batch][kmax][8] =
 * (rotation / pi [3], translation [3], is_symmetric, class index), gt_num [batch] - exactly the inputs of hep_anchor_targets_device,
 * rows at and beyond gt_num[b] zero; applied [batch].
 * PARITY-UNPINNED: OpenCV's conventions (the double inverse in warpAffine's order, the AB_BITS = 10 / INTER_BITS = 5 fixed-point map,
 * the int32 bilinear weights that sum to 32768, Rodrigues) are restated from its source, cv2 is not available to this project; the
 * definition is the numpy oracle tests/_augment.py, which the kernels reproduce bit for bit (image, mask, boxes, labels, camera).
 * What OpenCV's int16 table does with a weight of 32768 is not restated.  Not reproduced: coords_3d is not touched (the reference
 * does not rotate hand joints), translations_x_y_2D is not produced (anchor_targets_bbox never reads it).  The reference's colour augmentation runs BEFORE
 * this call, on the uint8 frames: hep_colour_augment_device below.
 * Supported: height, width in [16, 4096], size a multiple of 4 in [16, 4096], kmax in 1..16 (HEP_ERR_UNSUPPORTED otherwise, with
 * the reason, before any HIP call); a NULL required pointer, batch < 1, a misaligned image_nchw or a short workspace is
 * HEP_ERR_INVALID.  The scale lives in device memory: the ABI cannot refuse it without a synchronisation, so an out-of-range scale
 * shows as applied[b] = 0 (hmd_ego_pose_amd.augment refuses it on the host). */
int64_t hep_augment_workspace_bytes(int batch, int height, int width, int size, int kmax);
int hep_augment_6dof_device(
    const uint8_t* rgb_hwc, const uint8_t* mask, const double* xform, const float* camera_k,
    const double* boxes, const int32_t* labels, const int32_t* mask_values,
    const float* rvec, const float* tvec, const float* extra,
    const int32_t* num_gt, int batch, int height, int width, int size, int kmax, float translation_scale_norm,
    float* image_nchw, uint8_t* mask_out, float* camera,
    double* gt_boxes, int32_t* gt_labels, float* gt_transform, int32_t* gt_num, int32_t* applied,
    void* workspace, int64_t workspace_bytes, void* stream);

/* Colour augmentation of the training input (the reference's RandAugment(n=(1, 3), m=(1, 14)), generators/randaug.py:244-279, applied
 * to the RGB frame in front of the 6DoF augmentation, generators/common.py:334-341), on device memory: up to three operations per image
 * from a table, at most four launches and one memset of the counters, stateless, no allocation, no host synchronisation; the caller owns
 * the workspace (hep_colour_workspace_bytes; >= 0, or a negative hep_status; it is at least two frames).
 * rgb_hwc, out_hwc: uint8 [batch][height][width][3] (out_hwc != rgb_hwc).  ops int32 [batch][3][8]: per slot (id, or -1 for an empty
 * slot; i0, i1, i2, i3; seed_lo, seed_hi; 0).  args float32 [batch][3][2]: per slot (f or sigma, 0).  An image's operations are its
 * leading slots up to the first id of -1, applied in order; none: the image is copied.  Ids, in the reference's order:
 *    0 Identity            1 Autocontrast (cutoff 0)    2 Equalize             3 Invert
 *    4 Posterize, i0 = bits kept, 2..8                  5 Solarize, i0 = threshold, 0..256 (v < threshold stays, else 255 - v)
 *    6 EnhanceColor        7 EnhanceContrast            8 EnhanceBrightness    9 EnhanceSharpness: f in [0.1, 1.9], Image.blend of
 *      the degenerate image (luma; the rounded mean luma; 0; the smoothed image) and the image
 *   10 Cutout: the rectangle [i1, i3) x [i0, i2) = rows [y1, y2), columns [x1, x2) inside the frame becomes 128
 *   11 FilterBlur (5 x 5 ring, scale 16, 2-pixel border copied)   12 FilterSmooth (3 x 3, centre 5, scale 13, 1-pixel border copied)
 *   13 AdditiveGaussianNoise per channel: v + rint(sigma z) clipped, sigma in [0, 255], z from Philox4x32-10 with the slot's 64-bit seed
 *      as the key and the counter (e / 4, 0, image, slot), e the element index in [height][width][3] order; Box-Muller in float32.
 * The definition is the numpy oracle tests/_colour.py, which the kernels reproduce bit for bit for ids 0-12; for id 13 an element whose
 * sigma z lies within 1e-3 of a half-integer may differ by 1 from the oracle's float64 evaluation.  Pinned: tests/test_colour_cpu.py
 * holds the oracle to PIL with zero differing bytes for ids 1, 2, 4, 5, 6, 7, 8, 9, 11, 12 (imgaug's pillike augmenters call PIL).
 * PARITY-UNPINNED: imgaug is not available to this project, so Cutout's rectangle convention, Invert and the noise's rounding are
 * restated, and imgaug's random stream is not reproduced (hmd_ego_pose_amd.augment.draw_colour defines the project's draws).
 * Supported: height, width in [16, 4096], batch <= 65535 (HEP_ERR_UNSUPPORTED otherwise, with the reason, before any HIP call); a NULL
 * pointer, batch < 1, out_hwc == rgb_hwc, a workspace that is short or not 16-byte aligned: HEP_ERR_INVALID.  The table lives in device
 * memory: the ABI cannot refuse it without a synchronisation, so a slot with an unknown id or an out-of-range argument runs as
 * Identity (hmd_ego_pose_amd.augment.colour_augment refuses it on the host). */
int64_t hep_colour_workspace_bytes(int batch, int height, int width);
int hep_colour_augment_device(
    const uint8_t* rgb_hwc, const int32_t* ops, const float* args, int batch, int height, int width,
    uint8_t* out_hwc, void* workspace, int64_t workspace_bytes, void* stream);

/* The training step between the parts (csrc/k_train.hip): the optimiser, the gradient norm and the translation glue over the flat
 * buffers of the hep_{backbone,neck,heads}_*_device_bn calls, so that one object can own params | grad | stats for the whole model
 * and run the reference's step (train.py:88-342) as plain calls on one stream.  Conventions of the hep_heads_* group: stateless,
 * asynchronous on `stream`, no allocation, no host synchronisation, argument checks before any HIP call, bit-reproducible (fixed
 * reduction order, no float atomics).
 *
 * kind: one uint8 per element of the flat buffer (4-byte aligned):
 *   HEP_PK_TRAIN   updated by the optimiser
 *   HEP_PK_STAT    running_mean / running_var: never touched by the optimiser; takes the value of `stats` when stats != NULL
 *   HEP_PK_FROZEN  left bit-unchanged (padding between parts, a frozen part); any other value is treated like it
 * state: 32 bytes on the device (16-byte aligned), owned by the caller and zeroed once:
 *   float norm, clip_coef, bias1, bias2_sqrt; int32 step, skipped; int32 pad[2].
 *
 * hep_optim_grad_norm_device: the 2-norm of the HEP_PK_TRAIN elements of grad.  Pass 1: a fixed grid (a function of n only), each
 * thread sums its squares in double, a fixed-order tree per workgroup, one double partial per workgroup in the workspace
 * (hep_optim_workspace_bytes(n) bytes, 16-byte aligned).  Pass 2: one workgroup sums the partials in index order and writes the
 * state block: norm = sqrt(sum); when it is finite (as a float) step += 1, clip_coef = max_norm > 0 ? min(1, max_norm / (norm +
 * 1e-6)) : 1 (torch.nn.utils.clip_grad_norm_), bias1 = 1 - beta1^step, bias2_sqrt = sqrt(1 - beta2^step) (in double); otherwise
 * skipped += 1, clip_coef = 0 and step stays.
 *
 * hep_optim_update_device: one pass over the buffer, after hep_optim_grad_norm_device of the same gradient (it reads the state
 * block).  When that norm was not finite it writes nothing: params, m, v and the statistics stay bit-identical.  Otherwise, with
 * g' = clip_coef g, for HEP_PK_TRAIN:
 *   HEP_OPT_ADAM (torch.optim.Adam's defaults)   m += (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *                                                p -= (lr / bias1) m / (sqrt(v) / bias2_sqrt + eps)
 *   HEP_OPT_SGD_NESTEROV (train.py:103)          m = beta1 m + g';  p = fma(-lr, fma(beta1, m, g'), p)      (v may be NULL; from m = 0
 *                                                the first step is torch's buf = g)
 * HEP_PK_STAT: p = stats[i] when stats != NULL.  m and v of the other kinds are not touched.  29 bytes per trainable element move.
 * lr is a host argument (a scheduler on the host keeps working).  params, grad, m, v, stats: 16-byte aligned, n floats.
 * NULL (but stats, and v under SGD), n <= 0, a misaligned pointer or a short workspace: HEP_ERR_INVALID; an unknown optimiser:
 * HEP_ERR_UNSUPPORTED with the reason. */
#define HEP_PK_TRAIN 0
#define HEP_PK_STAT 1
#define HEP_PK_FROZEN 2
#define HEP_OPT_ADAM 0
#define HEP_OPT_SGD_NESTEROV 1
int64_t hep_optim_workspace_bytes(int64_t n);
int hep_optim_grad_norm_device(const float* grad, const uint8_t* kind, int64_t n, int optimizer, float beta1, float beta2, float max_norm,
                               void* state, void* workspace, size_t workspace_bytes, void* stream);
int hep_optim_update_device(float* params, const float* grad, float* m, float* v, const float* stats, const uint8_t* kind, int64_t n,
                            int optimizer, float lr, float beta1, float beta2, float eps, const void* state, void* stream);

/* transformation = cat(rotation head, format_translation(translation head)) - hmdegopose/loss.py:30-51, train.py:39,49 - and the
 * backward of that map.  rotation [batch][N][num_rotation], translation_raw [batch][N][3], camera [batch][6] = fx, fy, px, py,
 * tz_scale, image_scale, translation_anchors [N][3] = cx, cy, stride (hep_anchors, on the device):
 *   x = (cx + raw0 stride) / image_scale - px, y alike, tz = raw2 tz_scale, translation = (x tz / fx, y tz / fy, tz).
 * pack writes transformation [batch][N][num_rotation + 3] (what hep_losses_device takes); unpack takes its gradient (what
 * hep_losses_backward_device writes) and writes grad_rotation and grad_translation_raw (two of the cotangents of
 * hep_heads_backward_device).  NULL, batch < 1, num_anchors < 1 or num_rotation outside 1..8: HEP_ERR_INVALID. */
int hep_transformation_pack_device(const float* rotation, const float* translation_raw, const float* camera, const float* translation_anchors,
                                   int batch, int num_anchors, int num_rotation, float* transformation, void* stream);
int hep_transformation_unpack_grad_device(const float* grad_transformation, const float* translation_raw, const float* camera,
                                          const float* translation_anchors, int batch, int num_anchors, int num_rotation,
                                          float* grad_rotation, float* grad_translation_raw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HEP_H_ */
