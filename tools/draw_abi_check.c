/* Host-side argument checks of hep_draw_poses_device as a stand-alone program: every call below must return before any HIP call, so it
 * runs without a device and suits a host sanitizer build (the colours array is HOST memory and is copied only after every check):
 *   make -C hmd_ego_pose_amd/csrc OUT=$PWD/build_san/libhep_san.so OBJDIR=$PWD/build_san/obj \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   clang -fsanitize=address,undefined -Iinclude tools/draw_abi_check.c -o build_san/draw_abi_check -Lbuild_san -lhep_san -Wl,-rpath,$PWD/build_san
 *   build_san/draw_abi_check
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hep.h"

static int failures = 0;
#define EXPECT(call, want) do { int rc_ = (int)(call); if (rc_ != (want)) { printf("FAIL %s = %d, expected %d (%s)\n", #call, rc_, (want), hep_last_error()); failures++; } } while (0)
#define REFUSED_AS(call, code, reason) do { EXPECT(call, code); \
  if (!strstr(hep_last_error(), "hep_draw_poses_device") || !strstr(hep_last_error(), reason)) { printf("FAIL %s: message '%s' lacks '%s'\n", #call, hep_last_error(), reason); failures++; } } while (0)
#define REFUSED(call, reason) REFUSED_AS(call, HEP_ERR_INVALID, reason)

int main(void) {
  uint8_t* u = malloc(4096);
  float* f = malloc(4096);
  double* d = malloc(4096);
  int32_t* i = malloc(4096);
  uint8_t* col = malloc(3 * 3);      /* exactly num_labels x 3 bytes on the heap */
  memset(col, 7, 9);
#define CALL(frames, batch, h, w, gt, amax, cam, boxes, scores, labels, rot, trans, hand, rows, maxdet, cub, colours, nl, al, dl, t) \
  hep_draw_poses_device(frames, batch, h, w, gt, amax, cam, boxes, scores, labels, rot, trans, hand, rows, 0.5f, maxdet, cub, colours, nl, al, dl, t, NULL)
  REFUSED(CALL(NULL, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), "frames is NULL");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, NULL, col, 3, 2, 7, 2), "cuboids is NULL");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, NULL, 3, 2, 7, 2), "colours is NULL");
  REFUSED(CALL(u, 2, 48, 64, NULL, 4, NULL, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), "gt and camera are both NULL");
  REFUSED(CALL(u, 2, 48, 64, d, 0, d, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), "amax outside 1..16");
  REFUSED(CALL(u, 2, 48, 64, d, 17, NULL, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), "amax outside 1..16");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, NULL, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), "must all be given or all be NULL");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, NULL, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), "must all be given or all be NULL");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, NULL, f, f, f, 12, 10, f, col, 3, 2, 7, 2), "must all be given or all be NULL");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, NULL, f, f, 12, 10, f, col, 3, 2, 7, 2), "must all be given or all be NULL");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, NULL, f, 12, 10, f, col, 3, 2, 7, 2), "must all be given or all be NULL");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, NULL, NULL, NULL, NULL, NULL, f, 12, 10, f, col, 3, 2, 7, 2), "det_hand without the other det_* arrays");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, NULL, 0, 10, f, col, 3, 2, 7, 2), "rows outside 1..256");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, NULL, 257, 10, f, col, 3, 2, 7, 2), "rows outside 1..256");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 0, f, col, 3, 2, 7, 2), "max_detections outside 1..min(rows, 64)");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 13, f, col, 3, 2, 7, 2), "max_detections outside 1..min(rows, 64)");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 256, 65, f, col, 3, 2, 7, 2), "max_detections outside 1..min(rows, 64)");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 0, 2, 7, 2), "num_labels outside 1..63");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 64, 2, 7, 2), "num_labels outside 1..63");      /* refused before col[9..191] is read */
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 0), "thickness outside 1..8");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 9), "thickness outside 1..8");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 3, 8, 7, 2), "layer bits");
  REFUSED(CALL(u, 2, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 3, 2, -1, 2), "layer bits");
  REFUSED(CALL(u, 0, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), "batch must be >= 1");
  REFUSED(CALL(u, -4, 48, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), "batch must be >= 1");
  REFUSED_AS(CALL(u, 2, 15, 64, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  REFUSED_AS(CALL(u, 2, 48, 4097, d, 4, d, f, f, i, f, f, f, 12, 10, f, col, 3, 2, 7, 2), HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  /* the size check comes last: everything before it, the widest label count included, has passed when it refuses */
  REFUSED_AS(CALL(u, 2, 4097, 64, NULL, 0, d, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, f, col, 3, 0, 0, 8), HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  EXPECT(hep_abi_version(), 1);
  free(u); free(f); free(d); free(i); free(col);
  printf(failures ? "%d check(s) failed\n" : "all argument checks returned as documented\n", failures);
  return failures != 0;
}
