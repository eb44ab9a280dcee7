/* Host-side argument checks of hep_score_scene_device as a stand-alone program: every call below must return before any HIP call, so it
 * runs without a device and suits a host sanitizer build (the point_offsets array is read on the host: the sanitizer sees those reads):
 *   make -C hmd_ego_pose_amd/csrc OUT=$PWD/build_san/libhep_san.so OBJDIR=$PWD/build_san/obj \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   clang -fsanitize=address,undefined -Iinclude tools/score_scene_abi_check.c -o build_san/score_scene_abi_check -Lbuild_san -lhep_san -Wl,-rpath,$PWD/build_san
 *   build_san/score_scene_abi_check
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hep.h"

static int failures = 0;
#define EXPECT(call, want) do { int rc_ = (int)(call); if (rc_ != (want)) { printf("FAIL %s = %d, expected %d (%s)\n", #call, rc_, (want), hep_last_error()); failures++; } } while (0)
#define REFUSED(call, reason) do { EXPECT(call, HEP_ERR_INVALID); \
  if (!strstr(hep_last_error(), "hep_score_scene_device") || !strstr(hep_last_error(), reason)) { printf("FAIL %s: message '%s' lacks '%s'\n", #call, hep_last_error(), reason); failures++; } } while (0)

int main(void) {
  float* f = malloc(4096);
  double* d = malloc(4096);
  int32_t* i = malloc(4096);
  /* exactly num_labels + 1 offsets on the heap: a read past them is an error under the sanitizer */
  int32_t* off = malloc(4 * sizeof(int32_t));
  int32_t* flat = malloc(4 * sizeof(int32_t));
  int32_t* back = malloc(4 * sizeof(int32_t));
  int32_t* one = malloc(4 * sizeof(int32_t));
  int32_t* full = malloc(64 * sizeof(int32_t));
  off[0] = 0; off[1] = 1; off[2] = 38; off[3] = 1039;
  flat[0] = 0; flat[1] = 1; flat[2] = 1; flat[3] = 1039;
  back[0] = 0; back[1] = 38; back[2] = 1; back[3] = 1039;
  one[0] = 1; one[1] = 2; one[2] = 38; one[3] = 1039;
  for (int k = 0; k < 64; k++) full[k] = k;
#define CALL(boxes, scores, labels, rot, trans, batch, rows, gt, amax, points, offsets, nl, maxp, maxdet, rec, os, ot, ol, oc) \
  hep_score_scene_device(boxes, scores, labels, rot, trans, NULL, batch, rows, gt, amax, points, offsets, nl, maxp, 0.05f, maxdet, 0.5, rec, os, ot, ol, oc, NULL)
  REFUSED(CALL(NULL, f, i, f, f, 2, 12, d, 4, f, off, 3, 1000, 10, d, f, i, i, i), "det_boxes is NULL");
  REFUSED(CALL(f, NULL, i, f, f, 2, 12, d, 4, f, off, 3, 1000, 10, d, f, i, i, i), "det_scores is NULL");
  REFUSED(CALL(f, f, NULL, f, f, 2, 12, d, 4, f, off, 3, 1000, 10, d, f, i, i, i), "det_labels is NULL");
  REFUSED(CALL(f, f, i, NULL, f, 2, 12, d, 4, f, off, 3, 1000, 10, d, f, i, i, i), "det_rotation is NULL");
  REFUSED(CALL(f, f, i, f, NULL, 2, 12, d, 4, f, off, 3, 1000, 10, d, f, i, i, i), "det_translation is NULL");
  REFUSED(CALL(f, f, i, f, f, 2, 12, NULL, 4, f, off, 3, 1000, 10, d, f, i, i, i), "gt is NULL");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, NULL, off, 3, 1000, 10, d, f, i, i, i), "points is NULL");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, NULL, 3, 1000, 10, d, f, i, i, i), "point_offsets is NULL");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 3, 1000, 10, NULL, f, i, i, i), "records is NULL");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 3, 1000, 10, d, NULL, i, i, i), "out_scores is NULL");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 3, 1000, 10, d, f, NULL, i, i), "out_tp is NULL");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 3, 1000, 10, d, f, i, NULL, i), "out_labels is NULL");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 3, 1000, 10, d, f, i, i, NULL), "out_count is NULL");
  REFUSED(CALL(f, f, i, f, f, 0, 12, d, 4, f, off, 3, 1000, 10, d, f, i, i, i), "batch");
  REFUSED(CALL(f, f, i, f, f, -5, 12, d, 4, f, off, 3, 1000, 10, d, f, i, i, i), "batch");
  REFUSED(CALL(f, f, i, f, f, 2, 0, d, 4, f, off, 3, 1000, 10, d, f, i, i, i), "rows outside 1..256");
  REFUSED(CALL(f, f, i, f, f, 2, 257, d, 4, f, off, 3, 1000, 257, d, f, i, i, i), "rows outside 1..256");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 3, 1000, 0, d, f, i, i, i), "max_detections outside 1..rows");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 3, 1000, 13, d, f, i, i, i), "max_detections outside 1..rows");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 0, f, off, 3, 1000, 10, d, f, i, i, i), "amax outside 1..16");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 17, f, off, 3, 1000, 10, d, f, i, i, i), "amax outside 1..16");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 0, 1000, 10, d, f, i, i, i), "num_labels outside 1..63");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, -1, 1000, 10, d, f, i, i, i), "num_labels outside 1..63");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 64, 1000, 10, d, f, i, i, i), "num_labels outside 1..63");      /* refused before off[4..64] is read */
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, one, 3, 1000, 10, d, f, i, i, i), "point_offsets[0] must be 0");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, flat, 3, 1000, 10, d, f, i, i, i), "point_offsets must increase");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, back, 3, 1000, 10, d, f, i, i, i), "point_offsets must increase");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 3, 0, 10, d, f, i, i, i), "max_points");
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, off, 3, 1025, 10, d, f, i, i, i), "max_points");
  /* the largest label count walks exactly 64 offsets and is then refused for another reason */
  REFUSED(CALL(f, f, i, f, f, 2, 12, d, 4, f, full, 63, 0, 10, d, f, i, i, i), "max_points");
  EXPECT(hep_abi_version(), 1);
  free(f); free(d); free(i); free(off); free(flat); free(back); free(one); free(full);
  printf(failures ? "%d check(s) failed\n" : "all argument checks returned as documented\n", failures);
  return failures != 0;
}
