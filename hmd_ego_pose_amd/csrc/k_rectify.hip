// Rectified windows of the whole-frame search (include/hep.h: hep_preprocess_i420_rectified_device, hep_derotate_records_device).
// A plain window is a square cut out of the frame; off the optical axis it shows the object from the side while the record reports the
// rotation as if the camera looked straight at it.  The rectified window is the frame resampled into the view of a camera with the
// caller's intrinsics, rotated about the same centre by R_w to look along the window's ray (a homography), and the pose the network
// returns for it is rotated back by R_w.  The definition both kernels reproduce is the numpy oracle tests/_rectify.py; this file is built
// with -ffp-contract=off (Makefile), every product and sum below is written in the oracle's order.
//   yv12_rectified_windows_kernel   one thread per crop pixel, one window per blockIdx.y - the window's table row (13 doubles: R_w row-major,
//                                   fx, fy, px, py) and its frame index have block-uniform addresses, so they are read once per wave by
//                                   scalar loads.  The float64 chain gives the frame position in 1/32 pixel; four taps, each CLAMPED to the
//                                   frame and converted with yv12_windows_kernel's integer arithmetic (three byte loads per tap: neighbouring
//                                   lanes read neighbouring bytes, a line of the frame serves a row of the window), then the integer blend.
//   derotate_records_kernel         one wave per record; lanes 0-20 rotate a hand joint each, lane 21 the translation, lane 22 the rotation
//                                   through both Rodrigues conversions in double.  In place: a lane reads and writes its own three words only.
//                                   A record that is not found, and every record of a row whose R_w is exactly the identity, is left alone.
// No LDS, no atomics, no allocation.
#include "hep_dev.h"
#include "hep_internal.h"
#include "rodrigues_dev.h"

#include <cstdint>

// lrint, half to even, saturating to int32; fmax(NaN, lo) = lo: a NaN becomes INT32_MIN
__device__ __forceinline__ int rect_lrint(double v) {
  return (int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0);
}

// B, G, R of frame pixel (sy, sx): yv12_windows_kernel's conversion
__device__ __forceinline__ void rect_tap(const uint8_t* f, int W, int hw, int q, int sy, int sx, int* bgr) {
  const int Y = f[(int64_t)sy * W + sx];
  const int V = f[hw + (sy / 2) * (W / 2) + sx / 2], U = f[hw + q + (sy / 2) * (W / 2) + sx / 2];      // YV12: Y, V, U planes
  const int yy = max(0, Y - 16) * 1220542, uu = U - 128, vv = V - 128, half = 1 << 19;
  bgr[0] = min(255, max(0, (yy + half + 2116026 * uu) >> 20));
  bgr[1] = min(255, max(0, (yy + half - 852492 * vv - 409993 * uu) >> 20));
  bgr[2] = min(255, max(0, (yy + half + 1673527 * vv) >> 20));
}

__global__ __launch_bounds__(256) void yv12_rectified_windows_kernel(Yv12RectArgs a) {
  const int i = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= a.crop * a.crop) return;
  const int x = pix % a.crop, y = pix / a.crop;
  const double* t = a.table + (int64_t)i * RECTIFY_ROW_DOUBLES;
  const double fx = t[9], fy = t[10], px = t[11], py = t[12];
  const double s = (double)a.resized / (double)a.crop;
  const double u = s * ((double)x + 0.5) - 0.5, v = s * ((double)y + 0.5) - 0.5;
  const double qx = (u - px) / fx, qy = (v - py) / fy;
  const double p0 = (t[0] * qx + t[1] * qy) + t[2], p1 = (t[3] * qx + t[4] * qy) + t[5], p2 = (t[6] * qx + t[7] * qy) + t[8];
  int out[3] = {0, 0, 0};
  if (p2 > 0.0 && p2 <= 1.7976931348623157e308) {                // in front of the camera and finite (a NaN compares false)
    const double u2 = (fx * p0) / p2 + px, v2 = (fy * p1) / p2 + py;
    const double Xf = ((u2 + 0.5) / s - 0.5) + (double)((a.W - a.crop) / 2), Yf = ((v2 + 0.5) / s - 0.5) + (double)((a.H - a.crop) / 2);
    const int XI = rect_lrint(Xf * 32.0), YI = rect_lrint(Yf * 32.0);
    const int sx = XI >> 5, sy = YI >> 5, ax = XI & 31, ay = YI & 31;      // |sx| < 2^26: sx + 1 cannot wrap
    const int x0 = min(max(sx, 0), a.W - 1), x1 = min(max(sx + 1, 0), a.W - 1), y0 = min(max(sy, 0), a.H - 1), y1 = min(max(sy + 1, 0), a.H - 1);
    const int hw = a.H * a.W, q = (a.H / 2) * (a.W / 2);
    const uint8_t* f = a.in + (int64_t)a.windows[(int64_t)i * 3] * (hw + 2 * q);
    int p00[3], p01[3], p10[3], p11[3];
    rect_tap(f, a.W, hw, q, y0, x0, p00); rect_tap(f, a.W, hw, q, y0, x1, p01);
    rect_tap(f, a.W, hw, q, y1, x0, p10); rect_tap(f, a.W, hw, q, y1, x1, p11);
    const int w00 = (32 - ay) * (32 - ax) * 32, w01 = (32 - ay) * ax * 32, w10 = ay * (32 - ax) * 32, w11 = ay * ax * 32;      // sum 32768
    for (int c = 0; c < 3; c++) out[c] = (w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 16384) >> 15;
  }
  uint8_t* o = a.bgr + ((int64_t)i * a.crop * a.crop + pix) * 3;
  o[0] = (uint8_t)out[0]; o[1] = (uint8_t)out[1]; o[2] = (uint8_t)out[2];
}
void launch_yv12_rectified_windows(const Yv12RectArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(yv12_rectified_windows_kernel, dim3((unsigned)((a.crop * a.crop + 255) / 256), (unsigned)a.n), dim3(256), 0, s, a);
}

__global__ __launch_bounds__(64) void derotate_records_kernel(DerotateArgs a) {
  const int lane = threadIdx.x;
  uint32_t* r = a.records + (int64_t)blockIdx.x * POSE_RECORD_WORDS;
  if (r[0] != 1u || lane > 22) return;                             // a record that is not found stays as it is, bit for bit
  const double* R = a.table + (int64_t)(blockIdx.x / a.slots) * RECTIFY_ROW_DOUBLES;
  bool identity = true;                                            // the centre window: R_w is the identity exactly and the record stays, bit for bit
  for (int k = 0; k < 9; k++) identity = identity && R[k] == (k % 4 == 0 ? 1.0 : 0.0);
  if (identity) return;
  float* w = reinterpret_cast<float*>(r) + (lane < 21 ? 15 + 3 * lane : (lane == 21 ? 12 : 9));
  const double v[3] = {(double)w[0], (double)w[1], (double)w[2]};
  double o[3];
  if (lane < 22) {                                                  // a hand joint or the translation: R_w v
    for (int k = 0; k < 3; k++) o[k] = (R[3 * k] * v[0] + R[3 * k + 1] * v[1]) + R[3 * k + 2] * v[2];
  } else {                                                          // the rotation: the record holds the axis-angle vector in units of pi
    const double pi = 3.141592653589793;
    const double rv[3] = {v[0] * pi, v[1] * pi, v[2] * pi};
    double Rn[9], Ro[9];
    rodrigues_to_matrix(rv, Rn);
    for (int k = 0; k < 3; k++)
      for (int j = 0; j < 3; j++) Ro[3 * k + j] = (R[3 * k] * Rn[j] + R[3 * k + 1] * Rn[3 + j]) + R[3 * k + 2] * Rn[6 + j];
    rodrigues_to_vector(Ro, o);
    for (int k = 0; k < 3; k++) o[k] = o[k] / pi;
  }
  w[0] = (float)o[0]; w[1] = (float)o[1]; w[2] = (float)o[2];
}
void launch_derotate_records(const DerotateArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(derotate_records_kernel, dim3((unsigned)(a.n * a.slots)), dim3(64), 0, s, a);
}
