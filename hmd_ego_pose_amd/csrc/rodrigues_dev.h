// rodrigues_dev.h - cv2.Rodrigues in both directions as device functions, shared by aug_annot_kernel (k_augment.hip) and
// derotate_records_kernel (k_rectify.hip).
#pragma once

// cv2.Rodrigues both ways as hmd_ego_pose_amd/evaluate.py restates them (axis_angle_to_matrix, matrix_to_axis_angle), in double
__device__ inline void rodrigues_to_matrix(const double r[3], double R[9]) {
  const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (th < 1e-12) { for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
  const double k[3] = {r[0] / th, r[1] / th, r[2] / th}, c = cos(th), s = sin(th);
  const double K[9] = {0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[i * 3 + j] = (i == j ? c : 0.0) + (1.0 - c) * k[i] * k[j] + s * K[i * 3 + j];
}
__device__ inline void rodrigues_to_vector(const double R[9], double r[3]) {
  const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) / 2.0, c = (R[0] + R[4] + R[8] - 1.0) / 2.0;
  const double th = atan2(s, c);
  if (s < 1e-10) {
    if (c > 0) { for (int i = 0; i < 3; i++) r[i] = v[i] / 2.0; return; }
    // theta -> pi: the axis comes from R + I = 2 k k^T
    double d[3], A[9];
    for (int i = 0; i < 9; i++) A[i] = (R[i] + ((i % 4 == 0) ? 1.0 : 0.0)) / 2.0;
    for (int i = 0; i < 3; i++) d[i] = sqrt(fmax(A[i * 4], 0.0));
    int m = 0;
    if (d[1] > d[m]) m = 1;
    if (d[2] > d[m]) m = 2;
    const double dm = fmax(d[m], 1e-300);
    double k[3] = {A[m * 3] / dm, A[m * 3 + 1] / dm, A[m * 3 + 2] / dm};
    if (k[0] * v[0] + k[1] * v[1] + k[2] * v[2] < 0) { k[0] = -k[0]; k[1] = -k[1]; k[2] = -k[2]; }
    const double nk = sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
    for (int i = 0; i < 3; i++) r[i] = k[i] / nk * th;
    return;
  }
  for (int i = 0; i < 3; i++) r[i] = v[i] / (2.0 * s) * th;
}
