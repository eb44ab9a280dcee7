// Training input on the GPU (hep_augment_6dof_device): the reference's host generator in front of `for frames, targets in loader`
// (pytorch-sandbox/generators/common.py:348-479 augment_6DoF_image_and_annotations / augmentation_6DoF, :543-607
// preprocess_group_entry) as three launches, plus one when the frame has to be resized:
//   aug_mask   cv2.warpAffine(mask, M, INTER_NEAREST) and, per workgroup, the min / max x / y of every annotation's mask value
//   aug_annot  one workgroup per image: boxes from the partials, valid / applied, the pose update in double, compaction, tables
//   aug_image  cv2.warpAffine(image, M) (INTER_LINEAR, BORDER_CONSTANT 0) or a plain copy, normalised, planar NCHW float32
//   aug_resize only when max(H, W) != S: aug_image leaves the uint8 HWC frame in the workspace, this resizes and normalises it
// OpenCV's conventions are RESTATED from its source (imgproc/imgwarp.cpp; cv2 is not available to this project: PARITY-UNPINNED,
// DESIGN.md section 7e).  The definition the kernels reproduce bit for bit is the numpy oracle tests/_augment.py:
//   inverse of M in double in warpAffine's order, contraction off;
//   X = lrint((A01 y + A02) 1024) + rd + lrint(A00 x 1024) (AB_BITS = 10), Y alike; lrint is half-to-even and saturates to int32
//   (NaN -> INT32_MIN), the sum wraps - every source address is bounds-checked, so no value of M can read outside the frame;
//   nearest: rd = 512, source = X >> 10; bilinear: rd = 16, X >>= 5, source = X >> 5, fraction X & 31 (INTER_BITS = 5), int32
//   weights (32-fy)(32-fx)32, (32-fy)fx 32, fy(32-fx)32, fy fx 32 (sum 32768), out = (sum w p + 16384) >> 15.
// No atomics on global memory, no float atomics, no allocation: the partials have a fixed place per workgroup in the caller's workspace.
#include "hep_train.h"
#include "rodrigues_dev.h"

#include <cstdint>

#define AUG_THREADS 256
#define AUG_ANNOT_THREADS 128      // >= 4 * AUG_MAX_K + 1 reduction slots

struct AugInv { double a00, a01, a02, a10, a11, a12; };

__device__ __forceinline__ bool aug_apply(const double* xf) {
  return xf[8] != 0.0 && xf[7] >= 0.25 && xf[7] <= 4.0;      // (a NaN scale compares false: not applied)
}

__device__ __forceinline__ AugInv aug_invert(const double* M) {
#pragma clang fp contract(off)      // warpAffine (and the oracle) round every product before the sum
  AugInv r;
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0.0 ? 1.0 / D : 0.0;
  r.a00 = M[4] * D; r.a11 = M[0] * D; r.a01 = -M[1] * D; r.a10 = -M[3] * D;
  r.a02 = -r.a00 * M[2] - r.a01 * M[5];
  r.a12 = -r.a10 * M[2] - r.a11 * M[5];
  return r;
}

__device__ __forceinline__ int64_t aug_lrint(double v) {
  const double r = rint(v);
  return (int64_t)fmin(fmax(r, -2147483648.0), 2147483647.0);      // fmax(NaN, lo) = lo
}
// the row part lrint((a1 y + a2) 1024) and the column part lrint(a0 x 1024) of one fixed-point coordinate
__device__ __forceinline__ int64_t aug_row_term(double a1, double a2, int y) {
#pragma clang fp contract(off)
  const double t = a1 * (double)y + a2;
  return aug_lrint(t * 1024.0);
}
__device__ __forceinline__ int64_t aug_col_term(double a0, int x) {
#pragma clang fp contract(off)
  const double t = a0 * (double)x;
  return aug_lrint(t * 1024.0);
}
__device__ __forceinline__ int aug_wrap32(int64_t v) { return (int)(uint32_t)(uint64_t)v; }

// ---- launch 1: warped mask + per-workgroup box partials -----------------------------------------------------------------------
// grid (tiles, B): workgroup (t, b) owns rows [t * AUG_TILE_ROWS, ...) of image b - a tile never crosses an image.  Partials of the
// workgroup: int32 [4 * kmax + 1] = (min x, min y, max x, max y) per annotation, then "any non-zero pixel"; identity INT_MAX / -1 / 0.
__device__ __forceinline__ void aug_flush(int* red, const int* mv, int n, int kmax, int v, int x0, int x1, int y0, int y1) {
  if (v != 0) red[4 * kmax] = 1;                                   // (every writer stores the same 1)
  for (int k = 0; k < n; k++)
    if (mv[k] == v) {
      atomicMin(&red[4 * k + 0], x0); atomicMin(&red[4 * k + 1], y0);      // integer LDS atomics: order-independent
      atomicMax(&red[4 * k + 2], x1); atomicMax(&red[4 * k + 3], y1);
    }
}

__global__ __launch_bounds__(AUG_THREADS) void aug_mask_kernel(AugmentArgs a) {
  __shared__ int red[4 * AUG_MAX_K + 1];
  __shared__ int mv[AUG_MAX_K];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int y_begin = tile * AUG_TILE_ROWS, y_end = min(a.H, y_begin + AUG_TILE_ROWS);
  const double* xf = a.xform + (int64_t)b * 9;
  const uint8_t* src = a.mask + (int64_t)b * a.H * a.W;
  uint8_t* dst = a.mask_out ? a.mask_out + (int64_t)b * a.H * a.W : nullptr;
  if (!aug_apply(xf)) {                                            // not augmented: the mask passes through; aug_annot reads no partials of this image
    if (dst)
      for (int64_t i = (int64_t)y_begin * a.W + tid; i < (int64_t)y_end * a.W; i += AUG_THREADS) dst[i] = src[i];
    return;
  }
  const int nred = 4 * a.kmax + 1;
  const int n = min(max(a.num_gt[b], 0), a.kmax);
  if (tid < nred) red[tid] = tid == nred - 1 ? 0 : ((tid & 3) < 2 ? 0x7fffffff : -1);
  if (tid < n) mv[tid] = a.mask_values[(int64_t)b * a.kmax + tid];
  __syncthreads();
  const AugInv A = aug_invert(xf);
  // a lane walks a column strip downwards, so the interior of an object is one run: it reaches the LDS once per run, not per pixel
  int cur = -1, rx0 = 0, rx1 = 0, ry0 = 0, ry1 = 0;
  for (int x = tid; x < a.W; x += AUG_THREADS) {
    const int64_t cx = aug_col_term(A.a00, x), cy = aug_col_term(A.a10, x);
    for (int y = y_begin; y < y_end; y++) {
      const int X = aug_wrap32(aug_row_term(A.a01, A.a02, y) + 512 + cx), Y = aug_wrap32(aug_row_term(A.a11, A.a12, y) + 512 + cy);
      const int sx = X >> 10, sy = Y >> 10;
      int v = 0;
      if (sx >= 0 && sx < a.W && sy >= 0 && sy < a.H) v = src[(int64_t)sy * a.W + sx];
      if (dst) dst[(int64_t)y * a.W + x] = (uint8_t)v;
      if (v == cur && x == rx1) ry1 = y;                           // the run goes on (same value, same column, next row)
      else {
        if (cur >= 0) aug_flush(red, mv, n, a.kmax, cur, rx0, rx1, ry0, ry1);
        cur = v; rx0 = rx1 = x; ry0 = ry1 = y;
      }
    }
  }
  if (cur >= 0) aug_flush(red, mv, n, a.kmax, cur, rx0, rx1, ry0, ry1);
  __syncthreads();
  if (tid < nred) a.partials[((int64_t)b * a.tiles + tile) * nred + tid] = red[tid];
}

// ---- launch 2: annotations ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_ANNOT_THREADS) void aug_annot_kernel(AugmentArgs a) {
  __shared__ int red[4 * AUG_MAX_K + 1];
  __shared__ int keep[AUG_MAX_K];
  const int b = blockIdx.x, tid = threadIdx.x, kmax = a.kmax, nred = 4 * kmax + 1;
  const double* xf = a.xform + (int64_t)b * 9;
  const bool apply = aug_apply(xf);
  if (tid < nred) {
    int acc = tid == nred - 1 ? 0 : ((tid & 3) < 2 ? 0x7fffffff : -1);
    if (apply) {
      const int32_t* p = a.partials + (int64_t)b * a.tiles * nred + tid;
      for (int t = 0; t < a.tiles; t++) {                        // in index order
        const int v = p[(int64_t)t * nred];
        acc = tid == nred - 1 ? (acc | v) : ((tid & 3) < 2 ? min(acc, v) : max(acc, v));
      }
    }
    red[tid] = acc;
  }
  __syncthreads();
  const bool applied = apply && red[nred - 1] != 0;               // common.py:441-444: an empty warped mask keeps the original
  const int n = min(max(a.num_gt[b], 0), kmax);
  if (tid < kmax) keep[tid] = tid < n && (!applied || red[4 * tid + 2] >= 0);
  __syncthreads();
  int total = 0, pos = 0;
  for (int j = 0; j < kmax; j++) { total += keep[j]; if (j < tid) pos += keep[j]; }
  if (tid == 0) {
    a.gt_num[b] = total; a.applied[b] = applied ? 1 : 0;
    float* cam = a.camera + (int64_t)b * 6;
    const float* ck = a.camera_k + (int64_t)b * 4;
    cam[0] = ck[0]; cam[1] = ck[1]; cam[2] = ck[2]; cam[3] = ck[3]; cam[4] = a.tsn; cam[5] = (float)a.image_scale;
  }
  if (tid >= kmax) return;
  const int64_t in = (int64_t)b * kmax + tid;
  if (keep[tid]) {
    const int64_t o = (int64_t)b * kmax + pos;
    double box[4];
    float rot[3], t[3];
    if (applied) {
      for (int i = 0; i < 4; i++) box[i] = (double)red[4 * tid + i];
      const double r0[3] = {(double)a.rvec[in * 3], (double)a.rvec[in * 3 + 1], (double)a.rvec[in * 3 + 2]};
      const double t0[3] = {(double)a.tvec[in * 3], (double)a.tvec[in * 3 + 1], (double)a.tvec[in * 3 + 2]};
      const double c = cos(xf[6]), s = sin(xf[6]);                  // Rz: +angle about z (common.py:461-466)
      double R[9], R2[9], r2[3];
      rodrigues_to_matrix(r0, R);
      for (int j = 0; j < 3; j++) { R2[j] = c * R[j] - s * R[3 + j]; R2[3 + j] = s * R[j] + c * R[3 + j]; R2[6 + j] = R[6 + j]; }
      rodrigues_to_vector(R2, r2);
      for (int i = 0; i < 3; i++) rot[i] = (float)r2[i];
      t[0] = (float)(c * t0[0] - s * t0[1]); t[1] = (float)(s * t0[0] + c * t0[1]); t[2] = (float)(t0[2] / xf[7]);
    } else {
      for (int i = 0; i < 4; i++) box[i] = a.boxes[in * 4 + i];
      for (int i = 0; i < 3; i++) { rot[i] = a.rvec[in * 3 + i]; t[i] = a.tvec[in * 3 + i]; }
    }
    for (int i = 0; i < 4; i++) a.gt_boxes[o * 4 + i] = box[i] * a.image_scale;      // common.py:559
    a.gt_labels[o] = a.labels[in];
    float* row = a.gt_transform + o * 8;
    for (int i = 0; i < 3; i++) row[i] = __fdiv_rn(rot[i], 3.14159274101257324f);      // :562 on a float32 array: float32(pi)
    for (int i = 0; i < 3; i++) row[3 + i] = t[i];
    row[6] = a.extra[in * 2]; row[7] = a.extra[in * 2 + 1];
  }
  if (tid >= total) {                                              // rows at and beyond gt_num[b]
    const int64_t o = (int64_t)b * kmax + tid;
    for (int i = 0; i < 4; i++) a.gt_boxes[o * 4 + i] = 0.0;
    a.gt_labels[o] = 0;
    for (int i = 0; i < 8; i++) a.gt_transform[o * 8 + i] = 0.f;
  }
}

// ---- launch 3: image ------------------------------------------------------------------------------------------------------------
// preprocess_kernel's arithmetic (k_post.hip), restated: numpy divides the float32 image by 255. in float32 and evaluates the two
// in-place operations with the float64 lists in double, rounding to float32 each time
__device__ __forceinline__ float aug_normalise(int u8, int c) {
  const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
  const float r1 = __fdiv_rn((float)u8, 255.0f);
  const float r2 = (float)((double)r1 - mean[c]);
  return (float)((double)r2 / sd[c]);
}

// a lane owns four adjacent pixels of one output row: the planes are written as 16-byte stores and the taps of neighbours share lines
__global__ __launch_bounds__(AUG_THREADS) void aug_image_kernel(AugmentArgs a) {
  const int b = blockIdx.y;
  const int OW = a.resize ? a.W : a.S, OH = a.resize ? a.H : a.S, Q = (OW + 3) >> 2;
  const int64_t idx = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x;
  if (idx >= (int64_t)Q * OH) return;
  const int y = (int)(idx / Q), x0 = (int)(idx % Q) * 4;
  const double* xf = a.xform + (int64_t)b * 9;
  const bool applied = a.applied[b] != 0;
  const uint8_t* src = a.rgb + (int64_t)b * a.H * a.W * 3;
  int px[4][3];
  AugInv A = {};
  int64_t ry_x = 0, ry_y = 0;
  if (applied) { A = aug_invert(xf); ry_x = aug_row_term(A.a01, A.a02, y) + 16; ry_y = aug_row_term(A.a11, A.a12, y) + 16; }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = x0 + j;
    px[j][0] = px[j][1] = px[j][2] = 0;
    if (y >= a.H || x >= a.W) continue;
    if (!applied) {
      const uint8_t* p = src + ((int64_t)y * a.W + x) * 3;
      px[j][0] = p[0]; px[j][1] = p[1]; px[j][2] = p[2];
      continue;
    }
    const int X = aug_wrap32(ry_x + aug_col_term(A.a00, x)) >> 5, Y = aug_wrap32(ry_y + aug_col_term(A.a10, x)) >> 5;
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    const int w[4] = {(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32};
    int acc[3] = {16384, 16384, 16384};
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int tx = sx + (t & 1), ty = sy + (t >> 1);
      if (tx >= 0 && tx < a.W && ty >= 0 && ty < a.H) {             // BORDER_CONSTANT 0; checked before the load
        const uint8_t* p = src + ((int64_t)ty * a.W + tx) * 3;
        acc[0] += w[t] * p[0]; acc[1] += w[t] * p[1]; acc[2] += w[t] * p[2];
      }
    }
    px[j][0] = acc[0] >> 15; px[j][1] = acc[1] >> 15; px[j][2] = acc[2] >> 15;
  }
  // an augmentation that turned out invalid: aug_mask wrote the (empty) warped mask, the image keeps the original - so does the mask
  if (a.mask_out && !applied && aug_apply(xf) && y < a.H) {
    const int64_t m = (int64_t)b * a.H * a.W + (int64_t)y * a.W;
    for (int j = 0; j < 4; j++)
      if (x0 + j < a.W) a.mask_out[m + x0 + j] = a.mask[m + x0 + j];
  }
  if (a.resize) {                                                  // the uint8 HWC frame for aug_resize
    uint8_t* o = a.frame_u8 + (((int64_t)b * a.H + y) * a.W + x0) * 3;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (x0 + j < a.W) { o[j * 3] = (uint8_t)px[j][0]; o[j * 3 + 1] = (uint8_t)px[j][1]; o[j * 3 + 2] = (uint8_t)px[j][2]; }
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float4 v;
    v.x = (y < a.H && x0 + 0 < a.W) ? aug_normalise(px[0][c], c) : 0.f;
    v.y = (y < a.H && x0 + 1 < a.W) ? aug_normalise(px[1][c], c) : 0.f;
    v.z = (y < a.H && x0 + 2 < a.W) ? aug_normalise(px[2][c], c) : 0.f;
    v.w = (y < a.H && x0 + 3 < a.W) ? aug_normalise(px[3][c], c) : 0.f;
    *reinterpret_cast<float4*>(a.image + (((int64_t)b * 3 + c) * a.S + y) * a.S + x0) = v;      // S % 4 == 0, base 16-byte aligned (checked at the ABI)
  }
}

// ---- launch 4: resize (only when max(H, W) != S) ---------------------------------------------------------------------------------
// OpenCV's 8-bit INTER_LINEAR resize exactly as preprocess_kernel (k_post.hip) restates it; kept as a copy here so that the inference
// preprocess does not move (tests/test_gpu_augment.py holds the two together bit for bit)
__device__ __forceinline__ void aug_resize_tap(int o, double inv_scale, int n, int* s0, int* s1, int* w0, int* w1) {
#pragma clang fp contract(off)
  float f = (float)(((double)o + 0.5) * inv_scale - 0.5);
  int i = (int)floorf(f);
  f -= (float)i;
  if (i < 0) { f = 0.f; i = 0; }
  if (i >= n - 1) { f = 0.f; i = n - 1; }
  *s0 = i; *s1 = min(i + 1, n - 1);
  *w0 = (int)lrintf((1.f - f) * 2048.f); *w1 = (int)lrintf(f * 2048.f);
}

__global__ __launch_bounds__(AUG_THREADS) void aug_resize_kernel(AugmentArgs a) {
  const int b = blockIdx.y, Q = a.S >> 2;
  const int64_t idx = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x;
  if (idx >= (int64_t)Q * a.S) return;
  const int y = (int)(idx / Q), x0 = (int)(idx % Q) * 4;
  const uint8_t* img = a.frame_u8 + (int64_t)b * a.H * a.W * 3;
  float out[3][4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = x0 + j;
    out[0][j] = out[1][j] = out[2][j] = 0.f;
    if (y >= a.nh || x >= a.nw) continue;
    int xa, xb, a0, a1, ya, yb, b0, b1;
    aug_resize_tap(x, a.inv_scale_x, a.W, &xa, &xb, &a0, &a1);      // taps are clamped into [0, n - 1]
    aug_resize_tap(y, a.inv_scale_y, a.H, &ya, &yb, &b0, &b1);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int S0 = img[((int64_t)ya * a.W + xa) * 3 + c] * a0 + img[((int64_t)ya * a.W + xb) * 3 + c] * a1;
      const int S1 = img[((int64_t)yb * a.W + xa) * 3 + c] * a0 + img[((int64_t)yb * a.W + xb) * 3 + c] * a1;
      out[c][j] = aug_normalise(min(255, max(0, (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2)), c);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; c++)
    *reinterpret_cast<float4*>(a.image + (((int64_t)b * 3 + c) * a.S + y) * a.S + x0) = make_float4(out[c][0], out[c][1], out[c][2], out[c][3]);
}

void launch_augment(const AugmentArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(aug_mask_kernel, dim3(a.tiles, a.B), dim3(AUG_THREADS), 0, s, a);
  hipLaunchKernelGGL(aug_annot_kernel, dim3(a.B), dim3(AUG_ANNOT_THREADS), 0, s, a);
  const int OW = a.resize ? a.W : a.S, OH = a.resize ? a.H : a.S;
  const int64_t quads = (int64_t)((OW + 3) >> 2) * OH;
  hipLaunchKernelGGL(aug_image_kernel, dim3((unsigned)((quads + AUG_THREADS - 1) / AUG_THREADS), a.B), dim3(AUG_THREADS), 0, s, a);
  if (a.resize) {
    const int64_t q2 = (int64_t)(a.S >> 2) * a.S;
    hipLaunchKernelGGL(aug_resize_kernel, dim3((unsigned)((q2 + AUG_THREADS - 1) / AUG_THREADS), a.B), dim3(AUG_THREADS), 0, s, a);
  }
}
