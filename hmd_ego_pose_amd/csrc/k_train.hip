// The training step between the parts (hep_optim_*_device, hep_transformation_*_device): what the reference does with
// torch.optim.Adam / SGD (train.py:100,103), clip_grad_norm_ (train.py:210) and format_translation + cat (loss.py:30-51,
// train.py:39,49), over ONE flat fp32 buffer in the layout of the hep_{backbone,neck,heads}_*_device calls.
//   optim_norm_partial  fixed grid, grid-stride float4 + scalar tail: squares of the kind-0 gradients in double, a fixed-order tree
//                       per workgroup, one double partial per workgroup at a fixed place in the caller's workspace
//   optim_norm_finish   one workgroup: the partials summed in index order, the state block written (norm, clip_coef, bias terms,
//                       step / skipped)
//   optim_update        one pass over the buffer: 16 bytes read of p, g, m, v and 1 of kind, 12 written - 29 bytes per element
//   transformation_pack / transformation_unpack_grad   one thread per (image, anchor)
// All streaming and memory-bound.  No atomics, no allocation; every result is an ordinary vector store.  This file is compiled with
// -ffp-contract=off (Makefile): every operation below rounds once, so the float32 restatement (tests/_optim.py) describes the rounding
// of every step and the translation glue equals the torch ops it replaces bit for bit.
#include "hep.h"
#include "hep_train.h"

#include <cstdint>

#define OPT_THREADS 256

// fixed-order sum of one double per thread; the result is valid in thread 0
__device__ __forceinline__ double optim_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = OPT_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(OPT_THREADS) void optim_norm_partial_kernel(OptimArgs a) {
  __shared__ double red[OPT_THREADS];
  const int64_t quads = a.n >> 2, stride = (int64_t)gridDim.x * OPT_THREADS;
  const float4* g4 = reinterpret_cast<const float4*>(a.grad);
  const uint32_t* k4 = reinterpret_cast<const uint32_t*>(a.kind);
  double acc = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; q < quads; q += stride) {      // q < n / 4: inside both buffers
    const uint32_t k = k4[q];
    if (k == 0x02020202u || k == 0x01010101u) continue;
    const float4 g = g4[q];
    if ((k & 0xffu) == 0) acc += (double)g.x * (double)g.x;                                         // (a non-finite value outside kind 0 is never touched)
    if (((k >> 8) & 0xffu) == 0) acc += (double)g.y * (double)g.y;
    if (((k >> 16) & 0xffu) == 0) acc += (double)g.z * (double)g.z;
    if ((k >> 24) == 0) acc += (double)g.w * (double)g.w;
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (a.n & 3)) {                                        // the scalar tail: elements 4 quads .. n - 1
    const int64_t i = (quads << 2) + threadIdx.x;
    if (a.kind[i] == HEP_PK_TRAIN) acc += (double)a.grad[i] * (double)a.grad[i];
  }
  const double s = optim_block_sum(acc, red);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_norm_finish_kernel(OptimArgs a) {
  __shared__ double part[OPT_MAX_BLOCKS];
  for (int i = threadIdx.x; i < a.blocks; i += OPT_THREADS) part[i] = a.partials[i];                // a.blocks <= OPT_MAX_BLOCKS
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int i = 0; i < a.blocks; i++) sum += part[i];                                                // index order
  const double norm = sqrt(sum);
  OptimState st = *a.state;
  st.norm = (float)norm;
  if (isfinite(norm) && isfinite(st.norm)) {
    st.step += 1;
    st.clip_coef = a.max_norm > 0.f ? (float)fmin(1.0, (double)a.max_norm / (norm + 1e-6)) : 1.f;   // clip_grad_norm_
    st.bias1 = (float)(1.0 - pow((double)a.beta1, (double)st.step));
    st.bias2_sqrt = (float)sqrt(1.0 - pow((double)a.beta2, (double)st.step));
  } else {
    st.skipped += 1;
    st.clip_coef = 0.f;
  }
  *a.state = st;
}

struct OptimCoef { float lr, b1, b2, eps, clip, step_size, bias2_sqrt; };

template <int OPT>
__device__ __forceinline__ void optim_one(float& p, float g, float& m, float& v, const OptimCoef& c) {
  g = c.clip * g;
  if (OPT == HEP_OPT_ADAM) {
    m = m + (1.f - c.b1) * (g - m);
    v = c.b2 * v + (1.f - c.b2) * (g * g);
    p = p - c.step_size * (m / (sqrtf(v) / c.bias2_sqrt + c.eps));
  } else {
    m = c.b1 * m + g;
    p = fmaf(-c.lr, fmaf(c.b1, m, g), p);       // both multiply-adds fused, as torch's add(alpha = ...) kernels compute them: torch.optim.SGD's bits
  }
}

template <int OPT>
__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(OptimArgs a) {
  const OptimState st = *a.state;
  if (!isfinite(st.norm)) return;                              // this step was skipped: nothing is written
  OptimCoef c;
  c.lr = a.lr; c.b1 = a.beta1; c.b2 = a.beta2; c.eps = a.eps; c.clip = st.clip_coef; c.bias2_sqrt = st.bias2_sqrt;
  c.step_size = OPT == HEP_OPT_ADAM ? a.lr / st.bias1 : a.lr;
  const bool has_v = OPT == HEP_OPT_ADAM;
  const int64_t quads = a.n >> 2, stride = (int64_t)gridDim.x * OPT_THREADS;
  const uint32_t* k4 = reinterpret_cast<const uint32_t*>(a.kind);
  for (int64_t q = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; q < quads; q += stride) {      // q < n / 4: inside every buffer
    const uint32_t k = k4[q];
    if (k == 0x02020202u) continue;
    if (k == 0) {                                              // the vector body: four trainable elements
      float4 p = reinterpret_cast<float4*>(a.params)[q];
      const float4 g = reinterpret_cast<const float4*>(a.grad)[q];
      float4 m = reinterpret_cast<float4*>(a.m)[q];
      float4 v = has_v ? reinterpret_cast<float4*>(a.v)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
      optim_one<OPT>(p.x, g.x, m.x, v.x, c); optim_one<OPT>(p.y, g.y, m.y, v.y, c);
      optim_one<OPT>(p.z, g.z, m.z, v.z, c); optim_one<OPT>(p.w, g.w, m.w, v.w, c);
      reinterpret_cast<float4*>(a.params)[q] = p;
      reinterpret_cast<float4*>(a.m)[q] = m;
      if (has_v) reinterpret_cast<float4*>(a.v)[q] = v;
      continue;
    }
    if (k == 0x01010101u && a.stats) {                         // four running statistics
      reinterpret_cast<float4*>(a.params)[q] = reinterpret_cast<const float4*>(a.stats)[q];
      continue;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {                              // a run of another kind starts or ends inside this quad
      const int64_t i = (q << 2) + j;
      const uint32_t kj = (k >> (8 * j)) & 0xffu;
      if (kj == HEP_PK_TRAIN) {
        float p = a.params[i], m = a.m[i], v = has_v ? a.v[i] : 0.f;
        optim_one<OPT>(p, a.grad[i], m, v, c);
        a.params[i] = p; a.m[i] = m;
        if (has_v) a.v[i] = v;
      } else if (kj == HEP_PK_STAT && a.stats) {
        a.params[i] = a.stats[i];
      }
    }
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (a.n & 3)) {                                        // the scalar tail
    const int64_t i = (quads << 2) + threadIdx.x;
    const uint8_t kj = a.kind[i];
    if (kj == HEP_PK_TRAIN) {
      float p = a.params[i], m = a.m[i], v = has_v ? a.v[i] : 0.f;
      optim_one<OPT>(p, a.grad[i], m, v, c);
      a.params[i] = p; a.m[i] = m;
      if (has_v) a.v[i] = v;
    } else if (kj == HEP_PK_STAT && a.stats) {
      a.params[i] = a.stats[i];
    }
  }
}

int optim_grid(int64_t n) {
  const int64_t blocks = ((n >> 2) + OPT_THREADS - 1) / OPT_THREADS;
  return (int)(blocks < 1 ? 1 : blocks > OPT_MAX_BLOCKS ? OPT_MAX_BLOCKS : blocks);
}

void launch_optim_norm(const OptimArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(optim_norm_partial_kernel, dim3(a.blocks), dim3(OPT_THREADS), 0, s, a);
  hipLaunchKernelGGL(optim_norm_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, s, a);
}

void launch_optim_update(const OptimArgs& a, hipStream_t s) {
  if (a.optimizer == HEP_OPT_ADAM) hipLaunchKernelGGL(optim_update_kernel<HEP_OPT_ADAM>, dim3(a.blocks), dim3(OPT_THREADS), 0, s, a);
  else hipLaunchKernelGGL(optim_update_kernel<HEP_OPT_SGD_NESTEROV>, dim3(a.blocks), dim3(OPT_THREADS), 0, s, a);
}

// ---- cat(rotation, format_translation(raw)) and its backward -------------------------------------------------------------------
// format_translation (loss.py:30-51), in the order of training.format_translation:
//   x = (ax + r0 stride) / image_scale - px,  y alike,  tz = r2 tz_scale,  out = (x tz / fx, y tz / fy, tz)
__global__ __launch_bounds__(OPT_THREADS) void transformation_pack_kernel(TransformArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  if (idx >= (int64_t)a.B * a.N) return;
  const int b = (int)(idx / a.N), n = (int)(idx % a.N);
  const float* cam = a.camera + (int64_t)b * 6;
  const float* ta = a.anchors + (int64_t)n * 3;
  const float* raw = a.raw + idx * 3;
  float* o = a.transformation + idx * (a.R + 3);
  for (int r = 0; r < a.R; r++) o[r] = a.rotation[idx * a.R + r];
  const float x = (ta[0] + raw[0] * ta[2]) / cam[5] - cam[2];
  const float y = (ta[1] + raw[1] * ta[2]) / cam[5] - cam[3];
  const float tz = raw[2] * cam[4];
  o[a.R] = x * tz / cam[0]; o[a.R + 1] = y * tz / cam[1]; o[a.R + 2] = tz;
}

__global__ __launch_bounds__(OPT_THREADS) void transformation_unpack_grad_kernel(TransformArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  if (idx >= (int64_t)a.B * a.N) return;
  const int b = (int)(idx / a.N), n = (int)(idx % a.N);
  const float* cam = a.camera + (int64_t)b * 6;
  const float* ta = a.anchors + (int64_t)n * 3;
  const float* raw = a.raw + idx * 3;
  const float* g = a.transformation + idx * (a.R + 3);
  for (int r = 0; r < a.R; r++) a.g_rotation[idx * a.R + r] = g[r];
  const float x = (ta[0] + raw[0] * ta[2]) / cam[5] - cam[2];
  const float y = (ta[1] + raw[1] * ta[2]) / cam[5] - cam[3];
  const float tz = raw[2] * cam[4];
  const float gx = g[a.R] / cam[0], gy = g[a.R + 1] / cam[1];        // d out0 / d (x tz), d out1 / d (y tz)
  float* o = a.g_raw + idx * 3;
  o[0] = gx * tz / cam[5] * ta[2];
  o[1] = gy * tz / cam[5] * ta[2];
  o[2] = ((g[a.R + 2] + gy * y) + gx * x) * cam[4];                  // the order in which autograd accumulates the three uses of tz
}

void launch_transformation_pack(const TransformArgs& a, hipStream_t s) {
  const int64_t rows = (int64_t)a.B * a.N;
  hipLaunchKernelGGL(transformation_pack_kernel, dim3((unsigned)((rows + OPT_THREADS - 1) / OPT_THREADS)), dim3(OPT_THREADS), 0, s, a);
}

void launch_transformation_unpack_grad(const TransformArgs& a, hipStream_t s) {
  const int64_t rows = (int64_t)a.B * a.N;
  hipLaunchKernelGGL(transformation_unpack_grad_kernel, dim3((unsigned)((rows + OPT_THREADS - 1) / OPT_THREADS)), dim3(OPT_THREADS), 0, s, a);
}
