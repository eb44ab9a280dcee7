/* Argument checks of the frame-to-pose entry points (hep_top1_device, hep_pose_from_i420, hep_pose_from_input, and their per-label
 * twins hep_top_labels_device, hep_poses_from_i420, hep_poses_from_input) as a stand-alone
 * program: every call below must be refused with HEP_ERR_INVALID and a reason before any HIP call, so it runs without a device and
 * suits a host sanitizer build.  The checks in front of the first read of the handle - NULL pointers, a batch below 1, the frame
 * geometry - are walked with a stand-in address for the handle that is never dereferenced; a batch above max_batch needs a real
 * handle and is the GPU tests' (tests/test_gpu_top1.py, tests/test_gpu_top_labels.py).  It sees the host argument paths only, never a kernel.
 *   make -C hmd_ego_pose_amd/csrc OUT=$PWD/build_san/libhep_san.so OBJDIR=$PWD/build_san/obj \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   clang -fsanitize=address,undefined -Iinclude tools/pose_abi_check.c -o build_san/pose_abi_check -Lbuild_san -lhep_san -Wl,-rpath,$PWD/build_san
 *   build_san/pose_abi_check
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hep.h"

static int failures = 0;
#define REFUSED(call, reason) do { \
    hep_anchors(100, NULL, NULL);      /* another message in between: the text checked below is never a stale one */ \
    long long rc_ = (long long)(call); \
    if (rc_ != HEP_ERR_INVALID || strstr(hep_last_error(), reason) == NULL) { \
      printf("FAIL line %d: %s = %lld (%s), expected HEP_ERR_INVALID with \"%s\"\n", __LINE__, #call, rc_, hep_last_error(), reason); failures++; } } while (0)

int main(void) {
  float* f = calloc(64, sizeof(float));           /* camera / input / outputs: never read, the calls are refused first */
  uint8_t* yuv = calloc(64, 1);
  int32_t* found = calloc(4, sizeof(int32_t));
  uint32_t* rec = calloc(HEP_POSE_RECORD_WORDS, sizeof(uint32_t));
  hep_handle* h = calloc(1, 1 << 16);             /* a stand-in, zeroed: the checks walked with it come before the handle is read, but for
                                                     the batch of the two device calls, whose one range check reads max_batch (here 0) */

  REFUSED(hep_top1_device(NULL, NULL, NULL, NULL, NULL, NULL, f, 1, 0.5f, rec, NULL), "handle is NULL");
  REFUSED(hep_top1_device(h, NULL, NULL, NULL, NULL, NULL, NULL, 1, 0.5f, rec, NULL), "camera is NULL");
  REFUSED(hep_top1_device(h, NULL, NULL, NULL, NULL, NULL, f, 1, 0.5f, NULL, NULL), "records is NULL");
  REFUSED(hep_top1_device(h, NULL, NULL, NULL, NULL, NULL, f, 0, 0.5f, rec, NULL), "batch");
  REFUSED(hep_top1_device(h, NULL, NULL, NULL, NULL, NULL, f, -3, 0.5f, rec, NULL), "batch");

  REFUSED(hep_pose_from_input(NULL, f, 1, f, 0.5f, found, NULL, NULL, NULL, NULL, NULL, NULL, NULL), "handle is NULL");
  REFUSED(hep_pose_from_input(h, NULL, 1, f, 0.5f, found, NULL, NULL, NULL, NULL, NULL, NULL, NULL), "input_nchw is NULL");
  REFUSED(hep_pose_from_input(h, f, 1, NULL, 0.5f, found, NULL, NULL, NULL, NULL, NULL, NULL, NULL), "camera is NULL");
  REFUSED(hep_pose_from_input(h, f, 1, f, 0.5f, NULL, f, NULL, NULL, NULL, NULL, NULL, NULL), "found is NULL");
  REFUSED(hep_pose_from_input(h, f, 0, f, 0.5f, found, NULL, NULL, NULL, NULL, NULL, NULL, NULL), "batch");

#define I420(hh, yy, b, H, W, crop, rs, cam, fnd) hep_pose_from_i420(hh, yy, b, H, W, crop, rs, cam, 0.5f, fnd, NULL, NULL, NULL, NULL, NULL, NULL, NULL)
  REFUSED(I420(NULL, yuv, 1, 480, 640, 256, 512, f, found), "handle is NULL");
  REFUSED(I420(h, NULL, 1, 480, 640, 256, 512, f, found), "yuv is NULL");
  REFUSED(I420(h, yuv, 1, 480, 640, 256, 512, NULL, found), "camera is NULL");
  REFUSED(I420(h, yuv, 1, 480, 640, 256, 512, f, NULL), "found is NULL");
  REFUSED(I420(h, yuv, 0, 480, 640, 256, 512, f, found), "batch");
  REFUSED(I420(h, yuv, 1, 481, 640, 256, 512, f, found), "even");
  REFUSED(I420(h, yuv, 1, 480, 641, 256, 512, f, found), "even");
  REFUSED(I420(h, yuv, 1, 0, 640, 256, 512, f, found), "even");
  REFUSED(I420(h, yuv, 1, 480, 640, 482, 512, f, found), "crop");
  REFUSED(I420(h, yuv, 1, 480, 640, 0, 512, f, found), "crop");
  REFUSED(I420(h, yuv, 1, 480, 640, 256, 0, f, found), "resized");

  /* the top detection of every label: the same checks, each with its own name in the reason */
  REFUSED(hep_top_labels_device(NULL, NULL, NULL, NULL, NULL, NULL, f, 1, 0.5f, rec, NULL), "hep_top_labels_device: handle is NULL");
  REFUSED(hep_top_labels_device(h, NULL, NULL, NULL, NULL, NULL, NULL, 1, 0.5f, rec, NULL), "hep_top_labels_device: camera is NULL");
  REFUSED(hep_top_labels_device(h, NULL, NULL, NULL, NULL, NULL, f, 1, 0.5f, NULL, NULL), "hep_top_labels_device: records is NULL");
  REFUSED(hep_top_labels_device(h, NULL, NULL, NULL, NULL, NULL, f, 0, 0.5f, rec, NULL), "hep_top_labels_device: batch");
  REFUSED(hep_top_labels_device(h, NULL, NULL, NULL, NULL, NULL, f, -3, 0.5f, rec, NULL), "hep_top_labels_device: batch");

  REFUSED(hep_poses_from_input(NULL, f, 1, f, 0.5f, found, NULL, NULL, NULL, NULL, NULL, NULL), "hep_poses_from_input: handle is NULL");
  REFUSED(hep_poses_from_input(h, NULL, 1, f, 0.5f, found, NULL, NULL, NULL, NULL, NULL, NULL), "hep_poses_from_input: input_nchw is NULL");
  REFUSED(hep_poses_from_input(h, f, 1, NULL, 0.5f, found, NULL, NULL, NULL, NULL, NULL, NULL), "hep_poses_from_input: camera is NULL");
  REFUSED(hep_poses_from_input(h, f, 1, f, 0.5f, NULL, f, NULL, NULL, NULL, NULL, NULL), "hep_poses_from_input: found is NULL");
  REFUSED(hep_poses_from_input(h, f, 0, f, 0.5f, found, NULL, NULL, NULL, NULL, NULL, NULL), "hep_poses_from_input: batch");

#define I420S(hh, yy, b, H, W, crop, rs, cam, fnd) hep_poses_from_i420(hh, yy, b, H, W, crop, rs, cam, 0.5f, fnd, NULL, NULL, NULL, NULL, NULL, NULL)
  REFUSED(I420S(NULL, yuv, 1, 480, 640, 256, 512, f, found), "hep_poses_from_i420: handle is NULL");
  REFUSED(I420S(h, NULL, 1, 480, 640, 256, 512, f, found), "hep_poses_from_i420: yuv is NULL");
  REFUSED(I420S(h, yuv, 1, 480, 640, 256, 512, NULL, found), "hep_poses_from_i420: camera is NULL");
  REFUSED(I420S(h, yuv, 1, 480, 640, 256, 512, f, NULL), "hep_poses_from_i420: found is NULL");
  REFUSED(I420S(h, yuv, 0, 480, 640, 256, 512, f, found), "hep_poses_from_i420: batch");
  REFUSED(I420S(h, yuv, 1, 481, 640, 256, 512, f, found), "even");
  REFUSED(I420S(h, yuv, 1, 480, 641, 256, 512, f, found), "even");
  REFUSED(I420S(h, yuv, 1, 0, 640, 256, 512, f, found), "even");
  REFUSED(I420S(h, yuv, 1, 480, 640, 482, 512, f, found), "crop");
  REFUSED(I420S(h, yuv, 1, 480, 640, 0, 512, f, found), "crop");
  REFUSED(I420S(h, yuv, 1, 480, 640, 256, 0, f, found), "resized");

  free(f); free(yuv); free(found); free(rec); free(h);
  printf(failures ? "%d check(s) failed\n" : "all argument checks returned as documented\n", failures);
  return failures != 0;
}
