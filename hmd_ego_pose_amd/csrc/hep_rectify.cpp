// hep_rectify.cpp - the host arithmetic of the rectified windows (include/hep.h: hep_rectify_windows, hep_rectified_point_to_frame,
// hep_window_from_box_rectified; their argument checks live with the other whole-frame entry points in hep_api_pose.cpp).  Built with
// -ffp-contract=off (Makefile): tests/_rectify.py states every product and sum in this order and is reproduced bit for bit.
#include <math.h>
#include <stdint.h>

#include "hep_host.h"

namespace hep {

// R_w: the rotation about e_z x d that takes e_z to the window's viewing ray d, in its trig-free closed form.  A negation is a subtraction
// from zero, so the centre window (a = b = 0) gives the identity with +0.0 everywhere.
void rectify_row(const float* camera_row, const int32_t* w, int height, int width, int crop, int resized, double* row) {
  const double fx = (double)camera_row[0], fy = (double)camera_row[1];
  const double s = (double)resized / (double)crop;
  const double a = ((double)(w[1] - (width - crop) / 2) * s) / fx, b = ((double)(w[2] - (height - crop) / 2) * s) / fy;
  const double n = sqrt((a * a + b * b) + 1.0);
  const double dx = a / n, dy = b / n, dz = 1.0 / n;
  const double k = 1.0 / (1.0 + dz), m = (dx * dy) * k;
  row[0] = 1.0 - (dx * dx) * k; row[1] = 0.0 - m;               row[2] = dx;
  row[3] = 0.0 - m;               row[4] = 1.0 - (dy * dy) * k; row[5] = dy;
  row[6] = 0.0 - dx;              row[7] = 0.0 - dy;              row[8] = dz;
  row[9] = fx; row[10] = fy; row[11] = (double)camera_row[2]; row[12] = (double)camera_row[3];
}

// the chain of yv12_rectified_windows_kernel (k_rectify.hip) up to the frame coordinates, for an image of side x side pixels
bool rectified_point(const double* row, double x, double y, int height, int width, int crop, int resized, int side, double* xy) {
  const double fx = row[9], fy = row[10], px = row[11], py = row[12];
  const double s = (double)resized / (double)crop, sn = (double)resized / (double)side;
  const double u = sn * (x + 0.5) - 0.5, v = sn * (y + 0.5) - 0.5;
  const double qx = (u - px) / fx, qy = (v - py) / fy;
  const double p0 = (row[0] * qx + row[1] * qy) + row[2], p1 = (row[3] * qx + row[4] * qy) + row[5], p2 = (row[6] * qx + row[7] * qy) + row[8];
  if (!(p2 > 0.0) || !isfinite(p2)) { xy[0] = xy[1] = NAN; return false; }
  const double u2 = (fx * p0) / p2 + px, v2 = (fy * p1) / p2 + py;
  xy[0] = ((u2 + 0.5) / s - 0.5) + (double)((width - crop) / 2);
  xy[1] = ((v2 + 0.5) / s - 0.5) + (double)((height - crop) / 2);
  return true;
}

}  // namespace hep
