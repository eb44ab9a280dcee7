/* Host-side argument checks of hep_synth_frames_device / hep_synth_workspace_bytes as a stand-alone program: every call below must
 * return before any HIP call, so it runs without a device and suits a host sanitizer build (face_start is HOST memory, exactly
 * num_labels + 1 entries on the heap, read by the checks only after num_labels has passed; every other pointer is only looked at, never
 * followed):
 *   make -C hmd_ego_pose_amd/csrc OUT=$PWD/build_san/libhep_san.so OBJDIR=$PWD/build_san/obj \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   clang -fsanitize=address,undefined -Iinclude tools/synth_abi_check.c -o build_san/synth_abi_check -Lbuild_san -lhep_san -Wl,-rpath,$PWD/build_san
 *   build_san/synth_abi_check
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hep.h"

typedef struct {
  const double* poses; int batch, pmax; const double* camera; const float* vertices; const uint8_t* vertex_colours; int num_vertices;
  const int32_t* faces; const double* face_normals; int num_faces; const int32_t* face_start; int num_labels; const double* lights;
  int height, width; uint8_t* frames; int alpha; uint8_t* mask; float* depth; int32_t* visible;
  const float* rvec; const float* tvec; const float* extra; int min_pixels;
  double* boxes; int32_t* labels; int32_t* mask_values; float* out_rvec; float* out_tvec; float* out_extra; int32_t* num_gt; int32_t* slot_of;
  void* workspace; int64_t workspace_bytes;
} Args;

static int run(const Args* a) {
  return hep_synth_frames_device(a->poses, a->batch, a->pmax, a->camera, a->vertices, a->vertex_colours, a->num_vertices, a->faces, a->face_normals,
                                 a->num_faces, a->face_start, a->num_labels, a->lights, a->height, a->width, a->frames, a->alpha, a->mask, a->depth,
                                 a->visible, a->rvec, a->tvec, a->extra, a->min_pixels, a->boxes, a->labels, a->mask_values, a->out_rvec, a->out_tvec,
                                 a->out_extra, a->num_gt, a->slot_of, a->workspace, a->workspace_bytes, NULL);
}

static int failures = 0;
static Args good;
#define EXPECT(call, want) do { long long rc_ = (long long)(call); if (rc_ != (long long)(want)) { printf("FAIL %s = %lld, expected %lld (%s)\n", #call, rc_, (long long)(want), hep_last_error()); failures++; } } while (0)
#define MESSAGE(what, reason) do { if (!strstr(hep_last_error(), "hep_synth_frames_device: ") || !strstr(hep_last_error(), reason)) { \
  printf("FAIL %s: message '%s' lacks '%s'\n", what, hep_last_error(), reason); failures++; } } while (0)
/* the good call with one member changed */
#define REFUSED_AS(change, code, reason) do { Args a = good; change; EXPECT(run(&a), code); MESSAGE(#change, reason); } while (0)
#define REFUSED(change, reason) REFUSED_AS(change, HEP_ERR_INVALID, reason)

int main(void) {
  uint8_t* u = malloc(4096);
  float* f = malloc(4096);
  double* d = malloc(4096);
  int32_t* i = malloc(4096);
  void* ws = NULL;
  if (posix_memalign(&ws, 16, 4096)) return 2;
  int32_t* fs = malloc(3 * sizeof(int32_t));         /* exactly num_labels + 1 entries */
  int32_t* fs_down = malloc(3 * sizeof(int32_t));
  int32_t* fs_beyond = malloc(3 * sizeof(int32_t));
  int32_t* fs_below = malloc(3 * sizeof(int32_t));
  fs[0] = 0; fs[1] = 12; fs[2] = 16;
  fs_down[0] = 0; fs_down[1] = 16; fs_down[2] = 12;
  fs_beyond[0] = 0; fs_beyond[1] = 12; fs_beyond[2] = 17;
  fs_below[0] = -1; fs_below[1] = 12; fs_below[2] = 16;
  const int64_t need = 2 * 4 * (12 + 1) * 16;        /* batch x pmax x (vertices + 1) x 16 bytes: the renderer's */
  EXPECT(hep_synth_workspace_bytes(2, 48, 80, 4, 12), need);
  EXPECT(hep_synth_workspace_bytes(2, 48, 80, 4, 12), hep_render_workspace_bytes(2, 48, 80, 4, 12));
  const Args g = {d, 2, 4, d, f, u, 12, i, d, 16, fs, 2, d, 48, 80, u, 256, u, f, i, f, f, f, 16, d, i, i, f, f, f, i, i, ws, need};
  good = g;

  REFUSED(a.poses = NULL, "poses is NULL");
  REFUSED(a.camera = NULL, "camera is NULL");
  REFUSED(a.vertices = NULL, "vertices is NULL");
  REFUSED(a.vertex_colours = NULL, "vertex_colours is NULL");
  REFUSED(a.faces = NULL, "faces is NULL");
  REFUSED(a.face_normals = NULL, "face_normals is NULL");
  REFUSED(a.face_start = NULL, "face_start is NULL");
  REFUSED(a.lights = NULL, "lights is NULL");
  REFUSED(a.frames = NULL, "frames is NULL");
  REFUSED(a.visible = NULL, "visible is NULL");
  REFUSED(a.workspace = NULL, "workspace is NULL");
  /* the annotation group: each of the eleven missing alone, and each given alone */
  REFUSED(a.rvec = NULL, "half given"); REFUSED(a.tvec = NULL, "half given"); REFUSED(a.extra = NULL, "half given");
  REFUSED(a.boxes = NULL, "half given"); REFUSED(a.labels = NULL, "half given"); REFUSED(a.mask_values = NULL, "half given");
  REFUSED(a.out_rvec = NULL, "half given"); REFUSED(a.out_tvec = NULL, "half given"); REFUSED(a.out_extra = NULL, "half given");
  REFUSED(a.num_gt = NULL, "half given"); REFUSED(a.slot_of = NULL, "half given");
#define NO_GROUP a.rvec = a.tvec = a.extra = NULL; a.boxes = NULL; a.labels = a.mask_values = a.num_gt = a.slot_of = NULL; a.out_rvec = a.out_tvec = a.out_extra = NULL
  REFUSED(NO_GROUP; a.rvec = f, "half given");
  REFUSED(NO_GROUP; a.num_gt = i, "half given");
  REFUSED(NO_GROUP; a.boxes = d, "half given");
  REFUSED(a.batch = 0, "batch must be >= 1");
  REFUSED(a.pmax = 0, "pmax outside 1..16");
  REFUSED(a.pmax = 17, "pmax outside 1..16");
  REFUSED(a.num_vertices = 0, "num_vertices outside");
  REFUSED(a.num_vertices = HEP_RENDER_MAX_ELEMENTS + 1, "num_vertices outside");
  REFUSED(a.num_faces = 0, "num_faces outside");
  REFUSED(a.num_faces = HEP_RENDER_MAX_ELEMENTS + 1, "num_faces outside");
  REFUSED(a.num_labels = 0, "num_labels outside 1..63");
  REFUSED(a.num_labels = 64, "num_labels outside 1..63");      /* refused before fs[3..64] is read */
  REFUSED(a.face_start = fs_down, "face_start decreases");
  REFUSED(a.face_start = fs_beyond, "face_start leaves 0..num_faces");
  REFUSED(a.face_start = fs_below, "face_start leaves 0..num_faces");
  REFUSED(a.alpha = -1, "alpha outside 0..256");
  REFUSED(a.alpha = 257, "alpha outside 0..256");
  REFUSED(a.min_pixels = 0, "min_pixels must be >= 1");
  REFUSED(a.min_pixels = -3, "min_pixels must be >= 1");
  REFUSED(a.poses = (const double*)((const char*)d + 4), "poses must be 8-byte aligned");
  REFUSED(a.camera = (const double*)((const char*)d + 4), "camera must be 8-byte aligned");
  REFUSED(a.face_normals = (const double*)((const char*)d + 4), "face_normals must be 8-byte aligned");
  REFUSED(a.lights = (const double*)((const char*)d + 2), "lights must be 8-byte aligned");
  REFUSED(a.vertices = (const float*)((const char*)f + 2), "vertices must be 4-byte aligned");
  REFUSED(a.faces = (const int32_t*)((const char*)i + 1), "faces must be 4-byte aligned");
  REFUSED(a.depth = (float*)((char*)f + 2), "depth must be 4-byte aligned");
  REFUSED(a.visible = (int32_t*)((char*)i + 2), "visible must be 4-byte aligned");
  REFUSED(a.boxes = (double*)((char*)d + 4), "boxes must be 8-byte aligned");
  REFUSED(a.rvec = (const float*)((const char*)f + 1), "rvec must be 4-byte aligned");
  REFUSED(a.tvec = (const float*)((const char*)f + 2), "tvec must be 4-byte aligned");
  REFUSED(a.extra = (const float*)((const char*)f + 3), "extra must be 4-byte aligned");
  REFUSED(a.labels = (int32_t*)((char*)i + 2), "labels must be 4-byte aligned");
  REFUSED(a.mask_values = (int32_t*)((char*)i + 2), "mask_values must be 4-byte aligned");
  REFUSED(a.out_rvec = (float*)((char*)f + 2), "out_rvec must be 4-byte aligned");
  REFUSED(a.out_tvec = (float*)((char*)f + 2), "out_tvec must be 4-byte aligned");
  REFUSED(a.out_extra = (float*)((char*)f + 2), "out_extra must be 4-byte aligned");
  REFUSED(a.num_gt = (int32_t*)((char*)i + 2), "num_gt must be 4-byte aligned");
  REFUSED(a.slot_of = (int32_t*)((char*)i + 2), "slot_of must be 4-byte aligned");
  REFUSED(a.workspace = (char*)ws + 8, "workspace must be 16-byte aligned");
  REFUSED(a.workspace_bytes = need - 1, "workspace too small");
  REFUSED(a.workspace_bytes = 0, "workspace too small");
  REFUSED_AS(a.height = 15, HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  REFUSED_AS(a.width = 4097, HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  EXPECT(hep_synth_workspace_bytes(2, 4097, 80, 4, 12), HEP_ERR_UNSUPPORTED); MESSAGE("workspace_bytes height", "height and width must be in 16..4096");
  EXPECT(hep_synth_workspace_bytes(2, 48, 80, 17, 12), HEP_ERR_INVALID); MESSAGE("workspace_bytes pmax", "pmax outside 1..16");
  EXPECT(hep_synth_workspace_bytes(0, 48, 80, 4, 12), HEP_ERR_INVALID); MESSAGE("workspace_bytes batch", "batch must be >= 1");
  EXPECT(hep_synth_workspace_bytes(1024, 4096, 4096, 16, HEP_RENDER_MAX_ELEMENTS), (int64_t)1024 * 16 * ((int64_t)HEP_RENDER_MAX_ELEMENTS + 1) * 16);      /* no 32-bit overflow */
  EXPECT(hep_abi_version(), 1);
  free(u); free(f); free(d); free(i); free(ws); free(fs); free(fs_down); free(fs_beyond); free(fs_below);
  printf(failures ? "%d check(s) failed\n" : "all argument checks returned as documented\n", failures);
  return failures != 0;
}
