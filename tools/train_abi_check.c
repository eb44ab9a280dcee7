/* Host-side planning and argument checks of the three trainable parts (hep_heads_*, hep_neck_*, hep_backbone_*), as a stand-alone
 * program: every call below must return before any HIP call, so it runs without a device and suits a host sanitizer build.  The
 * planners fill fixed-size tables (BG_MAX_BLOCKS, NG_MAX_CELLS, HG_SLOTS) and the layout calls write into the caller's array:
 * that indexing is what the sanitizer watches here.  It sees the host planning and argument paths only, never a kernel.
 *   make -C hmd_ego_pose_amd/csrc OUT=$PWD/build_san/libhep_san.so OBJDIR=$PWD/build_san/obj \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   clang -fsanitize=address,undefined -Iinclude tools/train_abi_check.c -o build_san/train_abi_check -Lbuild_san -lhep_san -Wl,-rpath,$PWD/build_san
 *   build_san/train_abi_check
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hep.h"

static int failures = 0;
#define EXPECT(call, want) do { long long rc_ = (long long)(call); if (rc_ != (long long)(want)) { printf("FAIL line %d: %s = %lld, expected %lld (%s)\n", __LINE__, #call, rc_, (long long)(want), hep_last_error()); failures++; } } while (0)

enum { HEADS, NECK, BACKBONE, PARTS };
static const char* const kName[PARTS] = {"heads", "neck", "backbone"};
static const int kMaxPhi[PARTS] = {7, 5, 7};
static const int kSizes[5] = {128, 256, 2048, 0, 200};      /* the last two are refused */

static int64_t param_count(int part, int phi) { return part == HEADS ? hep_heads_param_count(phi, 1) : part == NECK ? hep_neck_param_count(phi) : hep_backbone_param_count(phi); }
static int param_layout(int part, int phi, int64_t* o, int cap) {
  return part == HEADS ? hep_heads_param_layout(phi, 1, o, cap) : part == NECK ? hep_neck_param_layout(phi, o, cap) : hep_backbone_param_layout(phi, o, cap);
}
static int64_t ws_bytes(int part, int phi, int size, int batch, int mode) {
  return part == HEADS ? hep_heads_workspace_bytes_bn(phi, 1, size, batch, mode) : part == NECK ? hep_neck_workspace_bytes_bn(phi, size, batch, mode)
                                                                                                 : hep_backbone_workspace_bytes_bn(phi, size, batch, mode);
}
static int64_t ws_bytes_plain(int part, int phi, int size, int batch) {
  return part == HEADS ? hep_heads_workspace_bytes(phi, 1, size, batch) : part == NECK ? hep_neck_workspace_bytes(phi, size, batch) : hep_backbone_workspace_bytes(phi, size, batch);
}
static int stage_count(int part, int phi) { return part == NECK ? hep_neck_stage_count(phi) : hep_backbone_stage_count(phi); }
static int stage_info(int part, int phi, int size, int batch, int i, const char** name, int64_t dims[4], int64_t* off) {
  return part == NECK ? hep_neck_stage_info(phi, size, batch, i, name, dims, off) : hep_backbone_stage_info(phi, size, batch, i, name, dims, off);
}

/* forward / backward of a part on one never-dereferenced address; `hole` leaves the middle pointer of every pointer array NULL */
struct call { void* params; void* ws; int64_t nbytes; int phi, size, batch, mode; float momentum; int hole, no_arrays; };
static int run(int part, int backward, struct call c) {
  void* a = c.ws ? c.ws : c.params;
  void* five[5] = {a, a, c.hole ? NULL : a, a, a};
  void* three[3] = {a, c.hole ? NULL : a, a};
  const float* const* in5 = c.no_arrays ? NULL : (const float* const*)five;
  const float* const* in3 = c.no_arrays ? NULL : (const float* const*)three;
  float* const* out5 = c.no_arrays ? NULL : (float* const*)five;
  float* const* out3 = c.no_arrays ? NULL : (float* const*)three;
  const float* p = c.params;
  const size_t n = (size_t)c.nbytes;
  if (part == HEADS)
    return backward ? hep_heads_backward_device_bn(p, in5, c.phi, 1, c.size, c.batch, (float*)a, NULL, c.ws, n, c.mode, NULL)
                    : hep_heads_forward_device_bn(p, in5, c.phi, 1, c.size, c.batch, out5, c.ws, n, c.mode, c.momentum, NULL, NULL);
  if (part == NECK)
    return backward ? hep_neck_backward_device_bn(p, in5, c.phi, c.size, c.batch, (float*)a, NULL, c.ws, n, c.mode, NULL)
                    : hep_neck_forward_device_bn(p, in3, c.phi, c.size, c.batch, out5, c.ws, n, c.mode, c.momentum, NULL, NULL);
  return backward ? hep_backbone_backward_device_bn(p, in3, NULL, c.phi, c.size, c.batch, (float*)a, NULL, c.ws, n, c.mode, NULL)
                  : hep_backbone_forward_device_bn(p, (const float*)a, NULL, c.phi, c.size, c.batch, out3, c.ws, n, c.mode, c.momentum, NULL, NULL);
}

int main(void) {
  char* raw = malloc(256);
  char* a = (char*)(((uintptr_t)raw + 15) & ~(uintptr_t)15);
  for (int part = 0; part < PARTS; part++) {
    for (int phi = -1; phi <= 8; phi++) {
      const int ok = phi >= 0 && phi <= kMaxPhi[part];
      const int64_t count = param_count(part, phi);
      const int n = param_layout(part, phi, NULL, 0);
      if (!ok) {
        EXPECT(count, HEP_ERR_UNSUPPORTED); EXPECT(n, HEP_ERR_UNSUPPORTED);
        if (part != HEADS) EXPECT(stage_count(part, phi), HEP_ERR_UNSUPPORTED);
        EXPECT(ws_bytes(part, phi, 256, 2, HEP_BN_RUNNING), HEP_ERR_UNSUPPORTED);
        continue;
      }
      EXPECT(count > 0, 1); EXPECT(n > 0, 1);
      if (count <= 0 || n <= 0) continue;
      /* the fill writes exactly n offsets (the array has no slack: a walk past the end is the sanitizer's), ascending from 0 */
      int64_t* off = malloc((size_t)n * sizeof(int64_t));
      memset(off, 0xff, (size_t)n * sizeof(int64_t));
      EXPECT(param_layout(part, phi, off, n), n);
      EXPECT(off[0], 0);
      for (int i = 1; i < n; i++) if (off[i] <= off[i - 1]) { printf("FAIL %s phi %d: tensor offsets do not ascend at %d\n", kName[part], phi, i); failures++; break; }
      EXPECT(off[n - 1] < count, 1);
      EXPECT(param_layout(part, phi, off, n - 1), HEP_ERR_INVALID);
      free(off);
      for (int mode = HEP_BN_RUNNING; mode <= HEP_BN_BATCH; mode++)
        for (int s = 0; s < 5; s++) {
          const int64_t b = ws_bytes(part, phi, kSizes[s], 2, mode);
          if (s < 3) EXPECT(b > 0 && b % 16 == 0, 1); else EXPECT(b, HEP_ERR_UNSUPPORTED);
          if (mode == HEP_BN_RUNNING) EXPECT(ws_bytes_plain(part, phi, kSizes[s], 2), b);
        }
      EXPECT(ws_bytes(part, phi, 0, 0, HEP_BN_RUNNING), HEP_ERR_UNSUPPORTED);
      EXPECT(ws_bytes(part, phi, 256, 0, HEP_BN_RUNNING), HEP_ERR_UNSUPPORTED);
      EXPECT(ws_bytes(part, phi, 256, 2, 5), HEP_ERR_INVALID);
      if (part == HEADS) continue;
      /* every stage lies inside the workspace; one index past the end is refused */
      const int stages = stage_count(part, phi);
      const int64_t need = ws_bytes(part, phi, 256, 2, HEP_BN_RUNNING);
      EXPECT(stages > 0, 1);
      for (int i = 0; i < stages; i++) {
        const char* name = NULL; int64_t dims[4] = {0, 0, 0, 0}, at = -1;
        EXPECT(stage_info(part, phi, 256, 2, i, &name, dims, &at), 0);
        EXPECT(name != NULL && name[0] != 0 && strlen(name) < 32, 1);
        EXPECT(dims[0] == 2 && dims[1] > 0 && dims[1] == dims[2] && dims[3] > 0, 1);
        EXPECT(at >= 0 && at % 16 == 0 && at + 4 * dims[0] * dims[1] * dims[2] * dims[3] <= need, 1);
      }
      EXPECT(stage_info(part, phi, 256, 2, stages, NULL, NULL, NULL), HEP_ERR_INVALID);
      EXPECT(stage_info(part, phi, 256, 2, -1, NULL, NULL, NULL), HEP_ERR_INVALID);
      EXPECT(stage_info(part, phi, 0, 0, 0, NULL, NULL, NULL), HEP_ERR_UNSUPPORTED);
      EXPECT(stage_info(part, phi, 200, 2, 0, NULL, NULL, NULL), HEP_ERR_UNSUPPORTED);
    }
    /* the refusals of the part's two _bn calls, in both BatchNorm modes */
    for (int backward = 0; backward < 2; backward++)
      for (int mode = HEP_BN_RUNNING; mode <= HEP_BN_BATCH; mode++) {
        const int64_t need = ws_bytes(part, 0, 256, 2, mode);
        const struct call good = {a, a, need, 0, 256, 2, mode, 0.01f, 0, 0};
        struct call c;
        c = good; c.params = NULL; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        c = good; c.ws = NULL; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        c = good; c.hole = 1; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        c = good; c.no_arrays = 1; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        c = good; c.ws = a + 4; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        EXPECT(strstr(hep_last_error(), "aligned") != NULL, 1);
        if (part == HEADS) { c = good; c.params = a + 4; EXPECT(run(part, backward, c), HEP_ERR_INVALID); EXPECT(strstr(hep_last_error(), "params") != NULL, 1); }
        c = good; c.nbytes = need - 4; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        EXPECT(strstr(hep_last_error(), "workspace is smaller") != NULL, 1);
        c = good; c.nbytes = 0; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        c = good; c.mode = 5; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        EXPECT(strstr(hep_last_error(), "mode") != NULL, 1);
        c = good; c.mode = -1; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        if (!backward && mode == HEP_BN_BATCH) {
          c = good; c.momentum = 1.5f; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
          EXPECT(strstr(hep_last_error(), "momentum") != NULL, 1);
          c = good; c.momentum = -0.5f; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
          c = good; c.momentum = NAN; EXPECT(run(part, backward, c), HEP_ERR_INVALID);
        }
        c = good; c.size = 200; EXPECT(run(part, backward, c), HEP_ERR_UNSUPPORTED);
        EXPECT(strstr(hep_last_error(), "multiple of 128") != NULL, 1);
        c = good; c.size = 0; c.batch = 0; EXPECT(run(part, backward, c), HEP_ERR_UNSUPPORTED);
        EXPECT(strstr(hep_last_error(), "multiple of 128") != NULL, 1);
        c = good; c.batch = 0; EXPECT(run(part, backward, c), HEP_ERR_UNSUPPORTED);
        c = good; c.phi = 8; EXPECT(run(part, backward, c), HEP_ERR_UNSUPPORTED);
        c = good; c.phi = -1; EXPECT(run(part, backward, c), HEP_ERR_UNSUPPORTED);
      }
  }
  free(raw);
  printf(failures ? "%d check(s) failed\n" : "all planning and argument checks returned as documented\n", failures);
  return failures != 0;
}
