/* Host-side argument checks of hep_render_models_device / hep_render_workspace_bytes as a stand-alone program: every call below must
 * return before any HIP call, so it runs without a device and suits a host sanitizer build (face_start and colours are HOST memory:
 * face_start is read - num_labels + 1 entries, after num_labels has passed - by the checks, colours is copied only after every check):
 *   make -C hmd_ego_pose_amd/csrc OUT=$PWD/build_san/libhep_san.so OBJDIR=$PWD/build_san/obj \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   clang -fsanitize=address,undefined -Iinclude tools/render_abi_check.c -o build_san/render_abi_check -Lbuild_san -lhep_san -Wl,-rpath,$PWD/build_san
 *   build_san/render_abi_check
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hep.h"

static int failures = 0;
#define EXPECT(call, want) do { long long rc_ = (long long)(call); if (rc_ != (long long)(want)) { printf("FAIL %s = %lld, expected %lld (%s)\n", #call, rc_, (long long)(want), hep_last_error()); failures++; } } while (0)
#define REFUSED_AS(call, code, reason) do { EXPECT(call, code); \
  if (!strstr(hep_last_error(), "hep_render_models_device") || !strstr(hep_last_error(), reason)) { printf("FAIL %s: message '%s' lacks '%s'\n", #call, hep_last_error(), reason); failures++; } } while (0)
#define REFUSED(call, reason) REFUSED_AS(call, HEP_ERR_INVALID, reason)

int main(void) {
  uint8_t* u = malloc(4096);
  float* f = malloc(4096);
  double* d = malloc(4096);
  int32_t* i = malloc(4096);
  void* ws = NULL;
  if (posix_memalign(&ws, 16, 4096)) return 2;
  uint8_t* col = malloc(2 * 3);                      /* exactly num_labels x 3 bytes on the heap */
  int32_t* fs = malloc(3 * sizeof(int32_t));         /* exactly num_labels + 1 entries */
  int32_t* fs_down = malloc(3 * sizeof(int32_t));
  int32_t* fs_beyond = malloc(3 * sizeof(int32_t));
  int32_t* fs_below = malloc(3 * sizeof(int32_t));
  memset(col, 7, 6);
  fs[0] = 0; fs[1] = 12; fs[2] = 16;
  fs_down[0] = 0; fs_down[1] = 16; fs_down[2] = 12;
  fs_beyond[0] = 0; fs_beyond[1] = 12; fs_beyond[2] = 17;
  fs_below[0] = -1; fs_below[1] = 12; fs_below[2] = 16;
  const int64_t need = 2 * 4 * (12 + 1) * 16;        /* batch x pmax x (vertices + 1) x 16 bytes */
  EXPECT(hep_render_workspace_bytes(2, 48, 80, 4, 12), need);
#define CALL(poses, batch, pmax, cam, v, nv, fc, nf, start, nl, h, w, mask, depth, frames, colours, alpha, wsp, bytes) \
  hep_render_models_device(poses, batch, pmax, cam, v, nv, fc, nf, start, nl, h, w, mask, depth, frames, colours, alpha, wsp, bytes, NULL)
  REFUSED(CALL(NULL, 2, 4, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "poses is NULL");
  REFUSED(CALL(d, 2, 4, NULL, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "camera is NULL");
  REFUSED(CALL(d, 2, 4, d, NULL, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "vertices is NULL");
  REFUSED(CALL(d, 2, 4, d, f, 12, NULL, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "faces is NULL");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, NULL, 2, 48, 80, u, f, u, col, 128, ws, need), "face_start is NULL");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, NULL, need), "workspace is NULL");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 48, 80, NULL, NULL, NULL, col, 128, ws, need), "mask, depth and frames are all NULL");
  REFUSED(CALL(d, 0, 4, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "batch must be >= 1");
  REFUSED(CALL(d, 2, 0, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "pmax outside 1..16");
  REFUSED(CALL(d, 2, 17, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "pmax outside 1..16");
  REFUSED(CALL(d, 2, 4, d, f, 0, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "num_vertices outside");
  REFUSED(CALL(d, 2, 4, d, f, HEP_RENDER_MAX_ELEMENTS + 1, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "num_vertices outside");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 0, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "num_faces outside");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, HEP_RENDER_MAX_ELEMENTS + 1, fs, 2, 48, 80, u, f, u, col, 128, ws, need), "num_faces outside");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 0, 48, 80, u, f, u, col, 128, ws, need), "num_labels outside 1..63");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 64, 48, 80, u, f, u, col, 128, ws, need), "num_labels outside 1..63");      /* refused before fs[3..64] is read */
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs_down, 2, 48, 80, u, f, u, col, 128, ws, need), "face_start decreases");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs_beyond, 2, 48, 80, u, f, u, col, 128, ws, need), "face_start leaves 0..num_faces");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs_below, 2, 48, 80, u, f, u, col, 128, ws, need), "face_start leaves 0..num_faces");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, NULL, 128, ws, need), "frames without colours");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, -1, ws, need), "alpha outside 0..256");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 257, ws, need), "alpha outside 0..256");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, (char*)ws + 8, need), "workspace must be 16-byte aligned");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, need - 1), "workspace too small");
  REFUSED(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 48, 80, u, f, u, col, 128, ws, 0), "workspace too small");
  REFUSED_AS(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 15, 80, u, f, u, col, 128, ws, need), HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  REFUSED_AS(CALL(d, 2, 4, d, f, 12, i, 16, fs, 2, 48, 4097, u, NULL, NULL, NULL, 0, ws, need), HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  REFUSED_AS(hep_render_workspace_bytes(2, 4097, 80, 4, 12), HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  REFUSED(hep_render_workspace_bytes(2, 48, 80, 17, 12), "pmax outside 1..16");
  REFUSED(hep_render_workspace_bytes(0, 48, 80, 4, 12), "batch must be >= 1");
  EXPECT(hep_render_workspace_bytes(1024, 4096, 4096, 16, HEP_RENDER_MAX_ELEMENTS), (int64_t)1024 * 16 * ((int64_t)HEP_RENDER_MAX_ELEMENTS + 1) * 16);      /* no 32-bit overflow */
  EXPECT(hep_abi_version(), 1);
  free(u); free(f); free(d); free(i); free(ws); free(col); free(fs); free(fs_down); free(fs_beyond); free(fs_below);
  printf(failures ? "%d check(s) failed\n" : "all argument checks returned as documented\n", failures);
  return failures != 0;
}
