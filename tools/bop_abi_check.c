/* Host-side argument checks of hep_bop_point_errors_device / hep_bop_vsd_device / hep_bop_workspace_bytes as a stand-alone program: every
 * call below must return before any HIP call, so it runs without a device and suits a host sanitizer build (vertex_start, symmetry_start
 * and taus are HOST memory: the start tables are read - num_labels + 1 entries, after num_labels has passed - and the taus - num_taus
 * entries, after num_taus has passed - by the checks; the tables here are heap blocks of exactly that size):
 *   make -C hmd_ego_pose_amd/csrc OUT=$PWD/build_san/libhep_san.so OBJDIR=$PWD/build_san/obj \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   clang -fsanitize=address,undefined -Iinclude tools/bop_abi_check.c -o build_san/bop_abi_check -Lbuild_san -lhep_san -Wl,-rpath,$PWD/build_san
 *   build_san/bop_abi_check
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hep.h"

static int failures = 0;
#define EXPECT(call, want) do { long long rc_ = (long long)(call); if (rc_ != (long long)(want)) { printf("FAIL %s = %lld, expected %lld (%s)\n", #call, rc_, (long long)(want), hep_last_error()); failures++; } } while (0)
#define REFUSED_AS(who, call, code, reason) do { EXPECT(call, code); \
  if (!strstr(hep_last_error(), who) || !strstr(hep_last_error(), reason)) { printf("FAIL %s: message '%s' lacks '%s'\n", #call, hep_last_error(), reason); failures++; } } while (0)
#define P_REFUSED(call, reason) REFUSED_AS("hep_bop_point_errors_device", call, HEP_ERR_INVALID, reason)
#define V_REFUSED(call, reason) REFUSED_AS("hep_bop_vsd_device", call, HEP_ERR_INVALID, reason)

static int32_t* table(int32_t a, int32_t b, int32_t c) {          /* exactly num_labels + 1 = 3 entries on the heap */
  int32_t* t = malloc(3 * sizeof(int32_t));
  t[0] = a; t[1] = b; t[2] = c;
  return t;
}

int main(void) {
  float* f = malloc(4096);
  double* d = malloc(4096);
  int32_t* i = malloc(4096);
  void* ws = NULL;
  if (posix_memalign(&ws, 16, 4096)) return 2;
  int32_t *vs = table(0, 8, 12), *ss = table(0, 1, 3), *below = table(-1, 1, 3), *flat = table(0, 0, 3), *down = table(0, 2, 1), *past = table(0, 8, 13),
          *many = table(0, 65, 66);
  double* taus = malloc(2 * sizeof(double));                       /* exactly num_taus entries */
  taus[0] = 5.0; taus[1] = 20.0;
  double* bad_tau = malloc(2 * sizeof(double));

  /* ---- MSSD / MSPD ---- */
  P_REFUSED(hep_bop_point_errors_device(NULL, 3, f, 12, vs, d, 3, ss, 2, d, NULL), "pairs is NULL");
  P_REFUSED(hep_bop_point_errors_device(d, 3, NULL, 12, vs, d, 3, ss, 2, d, NULL), "vertices is NULL");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, NULL, d, 3, ss, 2, d, NULL), "vertex_start is NULL");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, NULL, 3, ss, 2, d, NULL), "symmetries is NULL");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, d, 3, NULL, 2, d, NULL), "symmetry_start is NULL");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, d, 3, ss, 2, NULL, NULL), "errors is NULL");
  P_REFUSED(hep_bop_point_errors_device(d, 0, f, 12, vs, d, 3, ss, 2, d, NULL), "n must be >= 1");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, d, 3, ss, 0, d, NULL), "num_labels outside 1..63");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, d, 3, ss, 64, d, NULL), "num_labels outside 1..63");      /* the tables are not read */
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 0, vs, d, 3, ss, 2, d, NULL), "must be >= 1");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, d, 0, ss, 2, d, NULL), "must be >= 1");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, below, d, 3, ss, 2, d, NULL), "vertex_start starts below 0");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, flat, d, 3, ss, 2, d, NULL), "vertex_start must increase");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, down, d, 3, ss, 2, d, NULL), "vertex_start must increase");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, past, d, 3, ss, 2, d, NULL), "vertex_start ends past the array");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, d, 3, below, 2, d, NULL), "symmetry_start starts below 0");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, d, 3, flat, 2, d, NULL), "symmetry_start must increase");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, d, 3, vs, 2, d, NULL), "symmetry_start ends past the array");
  P_REFUSED(hep_bop_point_errors_device(d, 3, f, 12, vs, d, 66, many, 2, d, NULL), "more than 64");

  /* ---- VSD ---- */
  EXPECT(hep_bop_workspace_bytes(3, 2), 48);
  EXPECT(hep_bop_workspace_bytes(1, 1), 16);
  EXPECT(hep_bop_workspace_bytes(17, 16), 1232);
  EXPECT(hep_bop_workspace_bytes(0, 2), HEP_ERR_INVALID);
  EXPECT(hep_bop_workspace_bytes(3, 0), HEP_ERR_INVALID);
  EXPECT(hep_bop_workspace_bytes(3, 17), HEP_ERR_INVALID);
  V_REFUSED(hep_bop_vsd_device(NULL, 3, 2, f, f, NULL, 0, 48, 64, 15.0, taus, 2, d, i, ws, 48, NULL), "pairs is NULL");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, NULL, f, NULL, 0, 48, 64, 15.0, taus, 2, d, i, ws, 48, NULL), "depth_gt is NULL");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, NULL, NULL, 0, 48, 64, 15.0, taus, 2, d, i, ws, 48, NULL), "depth_est is NULL");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 15.0, NULL, 2, d, i, ws, 48, NULL), "taus is NULL");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 15.0, taus, 2, NULL, i, ws, 48, NULL), "vsd is NULL");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 15.0, taus, 2, d, NULL, ws, 48, NULL), "counts is NULL");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 15.0, taus, 2, d, i, NULL, 48, NULL), "workspace is NULL");
  V_REFUSED(hep_bop_vsd_device(d, 0, 2, f, f, NULL, 0, 48, 64, 15.0, taus, 2, d, i, ws, 48, NULL), "n must be >= 1");
  V_REFUSED(hep_bop_vsd_device(d, 3, 0, f, f, NULL, 0, 48, 64, 15.0, taus, 2, d, i, ws, 48, NULL), "num_labels outside 1..63");
  V_REFUSED(hep_bop_vsd_device(d, 3, 64, f, f, NULL, 0, 48, 64, 15.0, taus, 2, d, i, ws, 48, NULL), "num_labels outside 1..63");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 15.0, taus, 0, d, i, ws, 48, NULL), "num_taus outside 1..16");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 15.0, taus, 17, d, i, ws, 48, NULL), "num_taus outside 1..16");      /* taus is not read */
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, f, 0, 48, 64, 15.0, taus, 2, d, i, ws, 48, NULL), "num_images must be >= 1");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 0.0, taus, 2, d, i, ws, 48, NULL), "delta must be finite and positive");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, -1.0, taus, 2, d, i, ws, 48, NULL), "delta must be finite and positive");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, NAN, taus, 2, d, i, ws, 48, NULL), "delta must be finite and positive");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, INFINITY, taus, 2, d, i, ws, 48, NULL), "delta must be finite and positive");
  const double wrong[4] = {0.0, -1.0, NAN, INFINITY};
  for (int k = 0; k < 4; k++) {
    bad_tau[0] = 5.0; bad_tau[1] = wrong[k];
    V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 15.0, bad_tau, 2, d, i, ws, 48, NULL), "tau 1 must be finite and positive");
  }
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 15.0, taus, 2, d, i, (char*)ws + 8, 48, NULL), "workspace must be 16-byte aligned");
  V_REFUSED(hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 64, 15.0, taus, 2, d, i, ws, 47, NULL), "workspace too small");
  REFUSED_AS("hep_bop_vsd_device", hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 15, 64, 15.0, taus, 2, d, i, ws, 48, NULL), HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  REFUSED_AS("hep_bop_vsd_device", hep_bop_vsd_device(d, 3, 2, f, f, NULL, 0, 48, 4097, 15.0, taus, 2, d, i, ws, 48, NULL), HEP_ERR_UNSUPPORTED, "height and width must be in 16..4096");
  EXPECT(hep_abi_version(), 1);

  free(f); free(d); free(i); free(ws); free(vs); free(ss); free(below); free(flat); free(down); free(past); free(many); free(taus); free(bad_tau);
  printf(failures ? "%d check(s) FAILED\n" : "all argument checks returned as documented\n", failures);
  return failures ? 1 : 0;
}
