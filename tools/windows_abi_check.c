/* The whole-frame search's host side as a stand-alone program: the argument checks of its entry points, plain and rectified, - every call below must return
 * before any HIP call, so it runs without a device - and the host arithmetic of hep_tile_windows / hep_window_cameras / hep_window_from_box on
 * exactly sized heap blocks (hep_rectify_windows, hep_rectified_point_to_frame and hep_window_from_box_rectified likewise).  It suits a host
 * sanitizer build:
 *   make -C hmd_ego_pose_amd/csrc OUT=$PWD/build_san/libhep_san.so OBJDIR=$PWD/build_san/obj \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   clang -fsanitize=address,undefined -Iinclude tools/windows_abi_check.c -o build_san/windows_abi_check -Lbuild_san -lhep_san -Wl,-rpath,$PWD/build_san
 *   build_san/windows_abi_check
 * Where a case needs a non-NULL handle, a zeroed block stands in: the checks that do not read the handle come first (and max_batch would read as 0).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hep.h"

static int failures = 0;
#define EXPECT(call, want) do { int rc_ = (int)(call); if (rc_ != (want)) { printf("FAIL %s = %d, expected %d (%s)\n", #call, rc_, (want), hep_last_error()); failures++; } } while (0)
#define REFUSED(call, text) do { EXPECT(call, HEP_ERR_INVALID); if (!strstr(hep_last_error(), text)) { printf("FAIL %s: \"%s\" lacks \"%s\"\n", #call, hep_last_error(), text); failures++; } } while (0)

int main(void) {
  const int H = 504, W = 896, C = 256, R = 512;
  hep_handle* fake = calloc(1, 1 << 16);
  float* cam = calloc(6 * 2, sizeof(float));
  float* f = calloc(64, sizeof(float));
  int32_t* found = calloc(16, sizeof(int32_t));
  uint8_t* yuv = calloc(16, 1);      /* never read: every call is refused first */
  uint32_t* rec = calloc(80, 4);
  int32_t ox, oy;

  /* the arithmetic, into blocks of exactly the documented sizes */
  int32_t* grid = malloc(2 * 2 * 4 * 3 * sizeof(int32_t));
  EXPECT(hep_tile_windows(H, W, C, 4, 2, 2, grid), 0);
  EXPECT(grid[3 * 3 + 1] == W - C && grid[7 * 3 + 2] == H - C && grid[15 * 3] == 1 && grid[1 * 3 + 1] == 213, 1);
  int32_t one[3];
  EXPECT(hep_tile_windows(H, W, C, 1, 1, 1, one), 0);
  EXPECT(one[0] == 0 && one[1] == (W - C) / 2 && one[2] == (H - C) / 2, 1);
  for (int i = 0; i < 2; i++) { cam[i * 6] = 480.f + i; cam[i * 6 + 1] = 470.f; cam[i * 6 + 2] = 61.f; cam[i * 6 + 3] = 66.f; cam[i * 6 + 4] = 1000.f; cam[i * 6 + 5] = .5f; }
  float* wcam = malloc(16 * 6 * sizeof(float));
  EXPECT(hep_window_cameras(cam, grid, 16, H, W, C, R, wcam), 0);
  EXPECT(wcam[0 * 6 + 2] == 61.f + 640.f && wcam[3 * 6 + 2] == 61.f - 640.f && wcam[15 * 6] == 481.f && wcam[4 * 6 + 3] == 66.f - 248.f, 1);
  float centre[6];
  EXPECT(hep_window_cameras(cam + 6, one, 1, H, W, C, R, centre), 0);      /* (frame 0 of a table given its second row) */
  EXPECT(memcmp(centre, cam + 6, 24) == 0, 1);
  const float box[4] = {374.f, 246.f, 394.f, 266.f};
  EXPECT(hep_window_from_box(box, 100, 100, H, W, C, R, &ox, &oy), 0);
  EXPECT(ox == 164 && oy == 100, 1);
  const float far_box[4] = {1e30f, -1e30f, 1e30f, -1e30f};
  EXPECT(hep_window_from_box(far_box, 0, 0, H, W, C, R, &ox, &oy), 0);
  EXPECT(ox == W - C && oy == 0, 1);

  /* refusals of the host arithmetic */
  REFUSED(hep_tile_windows(H, W, C, 4, 2, 2, NULL), "windows_out is NULL");
  REFUSED(hep_tile_windows(H, W, C, 0, 2, 2, grid), "nx must be >= 1");
  REFUSED(hep_tile_windows(H, W, C, 4, -1, 2, grid), "ny must be >= 1");
  REFUSED(hep_tile_windows(H, W, C, 4, 2, 0, grid), "frames must be >= 1");
  REFUSED(hep_tile_windows(H + 1, W, C, 4, 2, 2, grid), "even");
  REFUSED(hep_tile_windows(H, W, H + 2, 4, 2, 2, grid), "crop");
  const int32_t outside[3] = {0, W - C + 1, 0}, below[3] = {0, 0, -1};
  REFUSED(hep_window_cameras(NULL, grid, 16, H, W, C, R, wcam), "camera is NULL");
  REFUSED(hep_window_cameras(cam, grid, 0, H, W, C, R, wcam), "n must be >= 1");
  REFUSED(hep_window_cameras(cam, outside, 1, H, W, C, R, wcam), "outside the frame");
  REFUSED(hep_window_cameras(cam, below, 1, H, W, C, R, wcam), "outside the frame");
  REFUSED(hep_window_cameras(cam, grid, 16, H, W + 1, C, R, wcam), "even");
  REFUSED(hep_window_from_box(NULL, 0, 0, H, W, C, R, &ox, &oy), "box is NULL");
  REFUSED(hep_window_from_box(box, 0, 0, H, W, C, R, &ox, NULL), "oy_out is NULL");
  REFUSED(hep_window_from_box(box, 0, H - C + 1, H, W, C, R, &ox, &oy), "outside the frame");
  REFUSED(hep_window_from_box(box, 0, 0, H, W, C, 0, &ox, &oy), "size must be >= 1");

  /* the device entry points */
  REFUSED(hep_preprocess_i420_windows_device(NULL, yuv, 1, H, W, grid, 1, C, R, f, NULL), "handle is NULL");
  REFUSED(hep_preprocess_i420_windows_device(fake, NULL, 1, H, W, grid, 1, C, R, f, NULL), "yuv is NULL");
  REFUSED(hep_preprocess_i420_windows_device(fake, yuv, 1, H, W, NULL, 1, C, R, f, NULL), "windows is NULL");
  REFUSED(hep_preprocess_i420_windows_device(fake, yuv, 1, H, W, grid, 1, C, R, NULL, NULL), "out_hwc is NULL");
  REFUSED(hep_preprocess_i420_windows_device(fake, yuv, 0, H, W, grid, 1, C, R, f, NULL), "frames must be >= 1");
  REFUSED(hep_preprocess_i420_windows_device(fake, yuv, 1, H, W - 1, grid, 1, C, R, f, NULL), "even");
  REFUSED(hep_preprocess_i420_windows_device(fake, yuv, 1, H, W, grid, 1, W, R, f, NULL), "crop");
  REFUSED(hep_preprocess_i420_windows_device(fake, yuv, 1, H, W, grid, 1, C, R, f, NULL), "n outside 1..max_batch");      /* the zeroed handle: max_batch 0 */
  REFUSED(hep_best_window_device(NULL, 1, grid, 1, 1, rec, found, NULL), "records is NULL");
  REFUSED(hep_best_window_device(rec, 1, NULL, 1, 1, rec, found, NULL), "windows is NULL");
  REFUSED(hep_best_window_device(rec, 1, grid, 1, 1, NULL, found, NULL), "out_records is NULL");
  REFUSED(hep_best_window_device(rec, 1, grid, 1, 1, rec, NULL, NULL), "out_window is NULL");
  REFUSED(hep_best_window_device(rec, 64, grid, 1, 1, rec, found, NULL), "slots outside 1..63");
  REFUSED(hep_best_window_device(rec, 1, grid, 0, 1, rec, found, NULL), "n must be >= 1");
  REFUSED(hep_best_window_device(rec, 1, grid, 1, 0, rec, found, NULL), "frames outside");

  /* the host calls: every output but found may be NULL */
#define WIN(h, y, fr, hh, ww, wi, n, c, cm, fo) hep_pose_from_i420_windows(h, y, fr, hh, ww, wi, n, c, R, cm, .5f, fo, NULL, NULL, NULL, NULL, NULL, NULL, NULL)
#define WINS(h, y, fr, hh, ww, wi, n, c, cm, fo) hep_poses_from_i420_windows(h, y, fr, hh, ww, wi, n, c, R, cm, .5f, fo, NULL, NULL, NULL, NULL, NULL, NULL)
#define TIL(h, y, fr, hh, ww, c, nx, ny, cm, fo, wo) hep_pose_from_i420_tiled(h, y, fr, hh, ww, c, R, nx, ny, cm, .5f, fo, NULL, NULL, NULL, NULL, NULL, NULL, NULL, wo)
#define TILS(h, y, fr, hh, ww, c, nx, ny, cm, fo, wo) hep_poses_from_i420_tiled(h, y, fr, hh, ww, c, R, nx, ny, cm, .5f, fo, NULL, NULL, NULL, NULL, NULL, NULL, wo)
#define WINR(h, y, fr, hh, ww, wi, n, c, cm, fo) hep_pose_from_i420_windows_rectified(h, y, fr, hh, ww, wi, n, c, R, cm, .5f, fo, NULL, NULL, NULL, NULL, NULL, NULL, NULL)
#define TILR(h, y, fr, hh, ww, c, nx, ny, cm, fo, wo) hep_pose_from_i420_tiled_rectified(h, y, fr, hh, ww, c, R, nx, ny, cm, .5f, fo, NULL, NULL, NULL, NULL, NULL, NULL, NULL, wo)
  const int32_t frame1[3] = {1, 0, 0};
  REFUSED(WIN(NULL, yuv, 1, H, W, grid, 1, C, cam, found), "hep_pose_from_i420_windows: handle is NULL");
  REFUSED(WINS(NULL, yuv, 1, H, W, grid, 1, C, cam, found), "hep_poses_from_i420_windows: handle is NULL");
  REFUSED(WIN(fake, NULL, 1, H, W, grid, 1, C, cam, found), "yuv is NULL");
  REFUSED(WIN(fake, yuv, 1, H, W, NULL, 1, C, cam, found), "windows is NULL");
  REFUSED(WIN(fake, yuv, 1, H, W, grid, 1, C, NULL, found), "camera is NULL");
  REFUSED(WINS(fake, yuv, 1, H, W, grid, 1, C, cam, NULL), "found is NULL");
  REFUSED(WIN(fake, yuv, 1, H, W, grid, 0, C, cam, found), "n outside 1..max_batch");
  REFUSED(WIN(fake, yuv, 0, H, W, grid, 1, C, cam, found), "frames must be >= 1");
  REFUSED(WIN(fake, yuv, 1, H + 1, W, grid, 1, C, cam, found), "even");
  REFUSED(WINS(fake, yuv, 1, H, W, grid, 1, H + 2, cam, found), "crop");
  REFUSED(WIN(fake, yuv, 1, H, W, outside, 1, C, cam, found), "outside the frame");
  REFUSED(WINS(fake, yuv, 1, H, W, below, 1, C, cam, found), "outside the frame");
  REFUSED(WIN(fake, yuv, 1, H, W, frame1, 1, C, cam, found), "outside the frame");      /* frame 1 of one frame */
  REFUSED(WIN(fake, yuv, 2, H, W, grid, 16, C, cam, found), "n outside 1..max_batch");   /* a good table; the zeroed handle: max_batch 0 */
  REFUSED(TIL(NULL, yuv, 1, H, W, C, 4, 2, cam, found, found), "hep_pose_from_i420_tiled: handle is NULL");
  REFUSED(TILS(NULL, yuv, 1, H, W, C, 4, 2, cam, found, found), "hep_poses_from_i420_tiled: handle is NULL");
  REFUSED(TIL(fake, NULL, 1, H, W, C, 4, 2, cam, found, found), "yuv is NULL");
  REFUSED(TIL(fake, yuv, 1, H, W, C, 4, 2, NULL, found, found), "camera is NULL");
  REFUSED(TILS(fake, yuv, 1, H, W, C, 4, 2, cam, NULL, found), "found is NULL");
  REFUSED(TIL(fake, yuv, 1, H, W, C, 4, 2, cam, found, NULL), "window is NULL");
  REFUSED(TIL(fake, yuv, 1, H, W, C, 0, 2, cam, found, found), "nx must be >= 1");
  REFUSED(TILS(fake, yuv, 1, H, W, C, 4, 0, cam, found, found), "ny must be >= 1");
  REFUSED(TIL(fake, yuv, 0, H, W, C, 4, 2, cam, found, found), "frames must be >= 1");
  REFUSED(TIL(fake, yuv, 1, H, W + 1, C, 4, 2, cam, found, found), "even");
  REFUSED(TILS(fake, yuv, 1, H, W, W, 4, 2, cam, found, found), "crop");
  REFUSED(TIL(fake, yuv, 1, H, W, C, 4, 2, cam, found, found), "frames * nx * ny outside 1..max_batch");      /* the zeroed handle: max_batch 0 */
  REFUSED(TIL(fake, yuv, 2147483647, H, W, C, 2147483647, 2147483647, cam, found, found), "frames * nx * ny outside 1..max_batch");      /* no overflow on the way */

  /* rectified windows: the host arithmetic into exactly sized blocks, then the refusals */
  double* table = malloc(16 * HEP_RECTIFY_ROW_DOUBLES * sizeof(double));
  EXPECT(hep_rectify_windows(cam, 2, grid, 16, H, W, C, R, table), 0);
  EXPECT(table[0 * 13 + 2] < 0 && table[3 * 13 + 2] > 0 && table[3 * 13 + 8] > 0 && table[15 * 13 + 9] == 481. && table[12] == 66., 1);
  double* id = malloc(HEP_RECTIFY_ROW_DOUBLES * sizeof(double));
  EXPECT(hep_rectify_windows(cam, 1, one, 1, H, W, C, R, id), 0);
  EXPECT(id[0] == 1. && id[4] == 1. && id[8] == 1. && id[1] == 0. && id[2] == 0. && id[5] == 0. && id[6] == 0., 1);
  double* xy = malloc(2 * sizeof(double));
  EXPECT(hep_rectified_point_to_frame(id, 255.5, 255.5, H, W, C, R, 512, xy), 0);
  EXPECT(xy[0] == 320. + 127.5 && xy[1] == 124. + 127.5, 1);      /* the identity row: the centre crop's own pixel */
  EXPECT(hep_window_from_box_rectified(table + 3 * 13, box, H, W, C, R, 512, &ox, &oy), 0);
  EXPECT(ox >= 0 && ox <= W - C && oy >= 0 && oy <= H - C, 1);
  EXPECT(hep_window_from_box_rectified(table, far_box, H, W, C, R, 512, &ox, &oy), 0);
  EXPECT(ox >= 0 && ox <= W - C && oy >= 0 && oy <= H - C, 1);
  REFUSED(hep_rectify_windows(NULL, 2, grid, 16, H, W, C, R, table), "camera is NULL");
  REFUSED(hep_rectify_windows(cam, 2, grid, 16, H, W, C, R, NULL), "table_out is NULL");
  REFUSED(hep_rectify_windows(cam, 2, grid, 0, H, W, C, R, table), "n must be >= 1");
  REFUSED(hep_rectify_windows(cam, 1, grid, 16, H, W, C, R, table), "outside the frame");      /* the grid names frame 1: no camera row */
  REFUSED(hep_rectify_windows(cam, 2, outside, 1, H, W, C, R, table), "outside the frame");
  REFUSED(hep_rectify_windows(cam, 2, grid, 16, H + 1, W, C, R, table), "even");
  cam[0] = 0.f;
  REFUSED(hep_rectify_windows(cam, 2, grid, 16, H, W, C, R, table), "fx and fy must be finite and positive");
  REFUSED(WINR(fake, yuv, 2, H, W, grid, 16, C, cam, found), "hep_pose_from_i420_windows_rectified: camera row 0: fx and fy must be finite and positive");
  cam[0] = 480.f;
  id[10] = -1.;
  REFUSED(hep_rectified_point_to_frame(id, 1., 1., H, W, C, R, 512, xy), "fx and fy must be finite and positive");
  REFUSED(hep_window_from_box_rectified(id, box, H, W, C, R, 512, &ox, &oy), "fx and fy must be finite and positive");
  REFUSED(hep_rectified_point_to_frame(NULL, 1., 1., H, W, C, R, 512, xy), "row is NULL");
  REFUSED(hep_window_from_box_rectified(table, box, H, W, C, R, 0, &ox, &oy), "size must be >= 1");
  REFUSED(hep_preprocess_i420_rectified_device(fake, yuv, 1, H, W, grid, NULL, 1, C, R, f, NULL), "table is NULL");
  REFUSED(hep_preprocess_i420_rectified_device(fake, yuv, 1, H, W, grid, table, 1, C, R, f, NULL), "n outside 1..max_batch");
  REFUSED(hep_derotate_records_device(NULL, 1, table, 1, NULL), "records is NULL");
  REFUSED(hep_derotate_records_device(rec, 1, NULL, 1, NULL), "table is NULL");
  REFUSED(hep_derotate_records_device(rec, 64, table, 1, NULL), "slots outside 1..63");
  REFUSED(WINR(NULL, yuv, 1, H, W, grid, 1, C, cam, found), "hep_pose_from_i420_windows_rectified: handle is NULL");
  REFUSED(WINR(fake, yuv, 1, H, W, frame1, 1, C, cam, found), "outside the frame");
  REFUSED(WINR(fake, yuv, 2, H, W, grid, 16, C, cam, found), "n outside 1..max_batch");
  REFUSED(TILR(fake, yuv, 1, H, W, C, 4, 2, cam, found, NULL), "window is NULL");
  REFUSED(TILR(fake, yuv, 1, H, W, C, 4, 2, cam, found, found), "hep_pose_from_i420_tiled_rectified: frames * nx * ny outside 1..max_batch");

  free(fake); free(cam); free(f); free(found); free(yuv); free(rec); free(grid); free(wcam); free(table); free(id); free(xy);
  printf(failures ? "%d check(s) failed\n" : "all argument checks returned as documented\n", failures);
  return failures != 0;
}
