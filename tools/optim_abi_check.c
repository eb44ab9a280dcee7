/* Host-side argument checks of the hep_optim_* and hep_transformation_* entry points, as a stand-alone program: every call below must
 * return before any HIP call, so it runs without a device and suits a host sanitizer build:
 *   make -C hmd_ego_pose_amd/csrc OUT=$PWD/build_san/libhep_san.so OBJDIR=$PWD/build_san/obj \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   clang -fsanitize=address,undefined -Iinclude tools/optim_abi_check.c -o build_san/optim_abi_check -Lbuild_san -lhep_san -Wl,-rpath,$PWD/build_san
 *   build_san/optim_abi_check
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hep.h"

static int failures = 0;
#define EXPECT(call, want) do { int rc_ = (int)(call); if (rc_ != (want)) { printf("FAIL %s = %d, expected %d (%s)\n", #call, rc_, (want), hep_last_error()); failures++; } } while (0)

int main(void) {
  const int64_t n = 1000;
  char* raw = malloc(6 * 4096 + 64);
  char* base = (char*)(((uintptr_t)raw + 15) & ~(uintptr_t)15);
  float *a = (float*)base, *b = (float*)(base + 4096), *c = (float*)(base + 2 * 4096), *d = (float*)(base + 3 * 4096);
  void* ws = base + 4 * 4096;
  uint8_t* kind = (uint8_t*)(base + 5 * 4096);
  void* state = base + 5 * 4096 + 2048;
  const int64_t nws = hep_optim_workspace_bytes(n);
  EXPECT(nws > 0 && nws % 16 == 0, 1);
  EXPECT(hep_optim_workspace_bytes(0), HEP_ERR_INVALID);
  EXPECT(hep_optim_workspace_bytes(-1), HEP_ERR_INVALID);
  EXPECT(hep_optim_grad_norm_device(NULL, kind, n, 0, .9f, .999f, 1.f, state, ws, nws, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_grad_norm_device(a, NULL, n, 0, .9f, .999f, 1.f, state, ws, nws, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_grad_norm_device(a, kind, n, 0, .9f, .999f, 1.f, NULL, ws, nws, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_grad_norm_device(a, kind, n, 0, .9f, .999f, 1.f, state, NULL, nws, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_grad_norm_device(a, kind, 0, 0, .9f, .999f, 1.f, state, ws, nws, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_grad_norm_device(a + 1, kind, n, 0, .9f, .999f, 1.f, state, ws, nws, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_grad_norm_device(a, kind + 1, n, 0, .9f, .999f, 1.f, state, ws, nws, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_grad_norm_device(a, kind, n, 0, .9f, .999f, 1.f, state, ws, nws - 1, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_grad_norm_device(a, kind, n, 7, .9f, .999f, 1.f, state, ws, nws, NULL), HEP_ERR_UNSUPPORTED);
  EXPECT(strstr(hep_last_error(), "optimizer 7") != NULL, 1);
  EXPECT(hep_optim_update_device(NULL, b, c, d, NULL, kind, n, 0, 1e-3f, .9f, .999f, 1e-8f, state, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_update_device(a, b, c, NULL, NULL, kind, n, 0, 1e-3f, .9f, .999f, 1e-8f, state, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_update_device(a, b, c + 1, d, NULL, kind, n, 0, 1e-3f, .9f, .999f, 1e-8f, state, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_update_device(a, b, c, d, a + 1, kind, n, 0, 1e-3f, .9f, .999f, 1e-8f, state, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_update_device(a, b, c, d, NULL, kind, -3, 0, 1e-3f, .9f, .999f, 1e-8f, state, NULL), HEP_ERR_INVALID);
  EXPECT(hep_optim_update_device(a, b, c, d, NULL, kind, n, 7, 1e-3f, .9f, .999f, 1e-8f, state, NULL), HEP_ERR_UNSUPPORTED);
  EXPECT(hep_transformation_pack_device(NULL, b, c, d, 1, 10, 3, a, NULL), HEP_ERR_INVALID);
  EXPECT(hep_transformation_pack_device(a, b, c, d, 0, 10, 3, a, NULL), HEP_ERR_INVALID);
  EXPECT(hep_transformation_pack_device(a, b, c, d, 1, 10, 9, a, NULL), HEP_ERR_INVALID);
  EXPECT(hep_transformation_unpack_grad_device(a, b, c, d, 1, 10, 3, NULL, a, NULL), HEP_ERR_INVALID);
  EXPECT(hep_transformation_unpack_grad_device(a, b, c, d, 1, 0, 3, a, b, NULL), HEP_ERR_INVALID);
  free(raw);
  printf(failures ? "%d check(s) failed\n" : "all argument checks returned as documented\n", failures);
  return failures != 0;
}
