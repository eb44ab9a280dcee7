// loss_dev.h - device helpers shared by the forward of the training losses (k_eval.hip) and their backward
// (k_loss_grad.hip): both must rotate the model points with the same float32 expressions, so that the backward picks
// the nearest target point the forward measured.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float smooth_l1_sigma3(float d) {
#pragma clang fp contract(off)
  const float s2 = 9.0f;
  d = fabsf(d);
  return d <= 1.0f / s2 ? 0.5f * s2 * (d * d) : d - 0.5f / s2;
}

struct AxisAngle { float ax, ay, az, c, s; };
__device__ __forceinline__ AxisAngle axis_angle(const float* r) {
#pragma clang fp contract(off)
  const float pi = 3.14159265358979323846f;
  const float x = r[0] * pi, y = r[1] * pi, z = r[2] * pi;
  const float angle = sqrtf((x * x + y * y) + z * z);
  AxisAngle q; q.ax = x / angle; q.ay = y / angle; q.az = z / angle; q.c = cosf(angle); q.s = sinf(angle);
  return q;
}
// point * cos + cross(axis, point) * sin + axis * dot(axis, point) * (1 - cos)      (loss.py:570-609)
__device__ __forceinline__ void rotate_pt(const AxisAngle& q, const float* p, float o[3]) {
#pragma clang fp contract(off)
  const float dt = (q.ax * p[0] + q.ay * p[1]) + q.az * p[2], omc = 1.0f - q.c;
  const float cx = q.ay * p[2] - q.az * p[1], cy = q.az * p[0] - q.ax * p[2], cz = q.ax * p[1] - q.ay * p[0];
  o[0] = (p[0] * q.c + cx * q.s) + (q.ax * dt) * omc;
  o[1] = (p[1] * q.c + cy * q.s) + (q.ay * dt) * omc;
  o[2] = (p[2] * q.c + cz * q.s) + (q.az * dt) * omc;
}
