// Colour augmentation on the GPU (hep_colour_augment_device): the 14 operations of the reference's RandAugment
// (pytorch-sandbox/generators/randaug.py:244-279, applied in generators/common.py:334-341 in front of the 6DoF warp) on uint8 HWC frames,
// up to three operations per image from a table in device memory.  The definition is the numpy oracle tests/_colour.py, reproduced bit for
// bit (the noise, id 13, up to the float32 evaluation of its normals).  tests/test_colour_cpu.py pins that oracle against PIL for the ten
// operations that are PIL's; Cutout, Invert and the noise are restated (PARITY-UNPINNED).
// One kernel, four launches (launch_colour):
//   slot -1  "stats0": the histograms / luma sum that slot 0 needs, from rgb; images whose slot 0 needs none exit at once
//   slot k   apply the image's operation k; accumulate what slot k + 1 needs from the bytes being written (LDS histogram per workgroup,
//            the non-empty bins flushed with uint32 atomicAdd: integer sums do not depend on the order of arrival)
// An image's first operation reads rgb, its last writes out, the ones between ping-pong through two workspace frames; an image without an
// operation is copied by the last launch.  Every rounding of the blend and of the autocontrast table is stated: this file is compiled with
// -ffp-contract=off (Makefile).  No float atomics, no allocation, no host synchronisation.
#include "hep_train.h"

#include <cstdint>

#define COL_THREADS 256
#define COL_QUADS 4      // quads (four adjacent pixels of a row) per lane: a workgroup covers 4096 pixels

struct ColSlot { int op, i0, i1, i2, i3; uint32_t seed_lo, seed_hi; float f; };

__device__ __forceinline__ int col_count(const int32_t* ops_b) {
  int n = 0;
  while (n < 3 && ops_b[n * 8] != -1) n++;
  return n;
}

// a slot the device does not accept (unknown id, argument out of range, NaN) runs as Identity: the ABI cannot refuse device data
__device__ __forceinline__ ColSlot col_slot(const ColourArgs& a, int b, int k) {
  const int32_t* o = a.ops + ((int64_t)b * 3 + k) * 8;
  ColSlot s;
  s.op = o[0]; s.i0 = o[1]; s.i1 = o[2]; s.i2 = o[3]; s.i3 = o[4]; s.seed_lo = (uint32_t)o[5]; s.seed_hi = (uint32_t)o[6];
  s.f = a.args[((int64_t)b * 3 + k) * 2];
  bool ok;
  switch (s.op) {
    case 0: case 1: case 2: case 3: case 11: case 12: ok = true; break;
    case 4: ok = s.i0 >= 2 && s.i0 <= 8; break;
    case 5: ok = s.i0 >= 0 && s.i0 <= 256; break;
    case 6: case 7: case 8: case 9: ok = s.f >= 0.1f && s.f <= 1.9f; break;
    case 10: ok = 0 <= s.i0 && s.i0 <= s.i2 && s.i2 <= a.W && 0 <= s.i1 && s.i1 <= s.i3 && s.i3 <= a.H; break;
    case 13: ok = s.f >= 0.f && s.f <= 255.f; break;
    default: ok = false;
  }
  if (!ok) s.op = 0;
  return s;
}

__device__ __forceinline__ int col_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend: t = float32(d + float32(f * float32(x - d))); truncated inside 0 <= f <= 1, clipped outside
__device__ __forceinline__ int col_blend(int d, int x, float f, bool inside) {
#pragma clang fp contract(off)
  const float p = f * (float)(x - d);
  const float t = (float)d + p;
  if (inside) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// ImageFilter.SMOOTH (R = 1: 3 x 3, centre 5, scale 13) and BLUR (R = 2: the outer ring of 5 x 5, scale 16) of the four pixels of a quad;
// an R-pixel border keeps v.  Window addresses are clamped into the frame, so no load leaves it; clamped values reach border pixels only.
template <int R>
__device__ __forceinline__ void col_filter(const uint8_t* src, int H, int W, int x0, int y, const int (&v)[12], int (&fv)[12]) {
  constexpr int NR = 2 * R + 1, NC = 4 + 2 * R, SCALE = R == 1 ? 13 : 16;
  const bool yin = y >= R && y < H - R;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    int win[NR][NC];
#pragma unroll
    for (int r = 0; r < NR; r++) {
      const int yy = min(max(y + r - R, 0), H - 1);
#pragma unroll
      for (int q = 0; q < NC; q++) {
        const int xx = min(max(x0 + q - R, 0), W - 1);
        win[r][q] = src[((int64_t)yy * W + xx) * 3 + c];
      }
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
      int acc = 0;
#pragma unroll
      for (int r = 0; r < NR; r++)
#pragma unroll
        for (int q = 0; q < NR; q++) {
          const int w = R == 1 ? ((r == 1 && q == 1) ? 5 : 1) : ((r == 0 || r == 4 || q == 0 || q == 4) ? 1 : 0);
          if (w) acc += w * win[r][p + q];
        }
      const int o = min((2 * acc + SCALE) / (2 * SCALE), 255);
      const int x = x0 + p;
      fv[p * 3 + c] = (yin && x >= R && x < W - R) ? o : v[p * 3 + c];
    }
  }
}

// Philox4x32-10 (Salmon et al., SC11)
__device__ __forceinline__ void col_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// four normals of one block: u = ((x >> 8) + 0.5) 2^-24, Box-Muller on (u0, u1) and (u2, u3) with the accurate float32 functions
__device__ __forceinline__ void col_normals(uint32_t q, uint32_t image, uint32_t slot, uint32_t k0, uint32_t k1, float* z) {
  uint32_t x[4];
  col_philox(q, 0u, image, slot, k0, k1, x);
#pragma unroll
  for (int a = 0; a < 4; a += 2) {
    const float ua = ((float)(x[a] >> 8) + 0.5f) * 5.9604644775390625e-8f, ub = ((float)(x[a + 1] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.f * logf(ua));
    float s, c;
    sincospif(2.f * ub, &s, &c);
    z[a] = r * c; z[a + 1] = r * s;
  }
}

// grid (workgroups per image, B), slot -1 .. 2
__global__ __launch_bounds__(COL_THREADS) void colour_kernel(ColourArgs a, int k) {
  __shared__ uint32_t hist[COL_COUNTERS];
  __shared__ uint32_t scan[256];
  __shared__ uint8_t lut[3][256];
  __shared__ int lohi[2];
  const int b = blockIdx.y, tid = threadIdx.x, H = a.H, W = a.W;
  const int n = col_count(a.ops + (int64_t)b * 24);
  const bool copy_only = n == 0 && k == 2;                        // an image without an operation: copied by the last launch
  if (k >= n && !copy_only) return;
  ColSlot s;
  s.op = 0; s.i0 = s.i1 = s.i2 = s.i3 = 0; s.seed_lo = s.seed_hi = 0u; s.f = 1.f;
  if (k >= 0 && !copy_only) s = col_slot(a, b, k);
  int next = 0;                                                   // the id of slot k + 1 when it needs statistics of this launch's output
  if (!copy_only && k + 1 < n) {
    const int t = col_slot(a, b, k + 1).op;
    if (t == 1 || t == 2 || t == 7) next = t;
  }
  if (k < 0 && !next) return;
  const int64_t frame = (int64_t)H * W * 3;
  const uint8_t* src = (k <= 0 || copy_only) ? a.rgb + b * frame : (((k - 1) & 1) ? a.frame1 : a.frame0) + b * frame;
  uint8_t* dst = (k == n - 1 || copy_only) ? a.out + b * frame : ((k & 1) ? a.frame1 : a.frame0) + b * frame;
  const int op = s.op;

  // the per-image tables of this slot, from the counters the previous launch summed
  const uint32_t* cnt = a.counters + ((int64_t)b * 3 + max(k, 0)) * COL_COUNTERS;
  int grey = 0;
  if (op == 7) grey = (int)((double)cnt[768] / (double)((int64_t)H * W) + 0.5);
  if (op == 1 || op == 2) {
    for (int c = 0; c < 3; c++) {
      const uint32_t h = cnt[c * 256 + tid];
      if (tid < 2) lohi[tid] = op == 1 ? (tid == 0 ? 256 : -1) : (tid == 0 ? 0 : -1);
      scan[tid] = h;
      __syncthreads();
      int v = tid;
      if (op == 1) {                                              // autocontrast: first and last non-empty bin
        if (h) { atomicMin(&lohi[0], tid); atomicMax(&lohi[1], tid); }
        __syncthreads();
        const int lo = lohi[0], hi = lohi[1];
        if (hi > lo) {
          const double scale = 255.0 / (double)(hi - lo);
          const double offset = -(double)lo * scale;
          const double t = (double)tid * scale;                   // two roundings (contraction is off in this file)
          v = min(max((int)(t + offset), 0), 255);
        }
      } else {                                                    // equalize: the number of non-empty bins, the last one, a 256-wide prefix sum
        if (h) { atomicAdd(&lohi[0], 1); atomicMax(&lohi[1], tid); }
        for (int d = 1; d < 256; d <<= 1) {
          const uint32_t t = tid >= d ? scan[tid - d] : 0u;
          __syncthreads();
          scan[tid] += t;
          __syncthreads();
        }
        const int bins = lohi[0], last = lohi[1];
        if (bins > 1) {
          const uint32_t step = (scan[255] - cnt[c * 256 + last]) / 255u;
          if (step) v = (int)min((step / 2u + (scan[tid] - h)) / step, 255u);
        }
      }
      lut[c][tid] = (uint8_t)v;
      __syncthreads();                                            // lohi and scan are reused by the next channel
    }
  }
  for (int i = tid; i < COL_COUNTERS; i += COL_THREADS) hist[i] = 0u;
  __syncthreads();

  const int Q = (W + 3) >> 2;
  const int64_t quads = (int64_t)Q * H;
  const bool inside = s.f >= 0.f && s.f <= 1.f;
#pragma unroll 1
  for (int it = 0; it < COL_QUADS; it++) {
    const int64_t idx = ((int64_t)blockIdx.x * COL_QUADS + it) * COL_THREADS + tid;
    if (idx >= quads) break;
    const int y = (int)(idx / Q), x0 = (int)(idx % Q) * 4, nb = min(4, W - x0) * 3;
    const int64_t off = ((int64_t)y * W + x0) * 3;
    // a full quad at a 4-byte aligned address moves as three dwords; the head and tail of a row whose 3 W bytes do not keep that alignment move as bytes
    const bool wide = nb == 12 && ((uintptr_t)(src + off) & 3) == 0 && ((uintptr_t)(dst + off) & 3) == 0;
    int v[12];
    if (wide) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(src + off);
      const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
#pragma unroll
      for (int j = 0; j < 4; j++) { v[j] = (w0 >> (8 * j)) & 255; v[4 + j] = (w1 >> (8 * j)) & 255; v[8 + j] = (w2 >> (8 * j)) & 255; }
    } else {
#pragma unroll
      for (int j = 0; j < 12; j++) v[j] = j < nb ? src[off + j] : 0;
    }
    switch (op) {
      case 1: case 2:
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] = lut[j % 3][v[j]];
        break;
      case 3:
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] = 255 - v[j];
        break;
      case 4: {
        const int m = ~((1 << (8 - s.i0)) - 1) & 255;
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] &= m;
        break;
      }
      case 5:
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] = v[j] < s.i0 ? v[j] : 255 - v[j];
        break;
      case 6:
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const int l = col_luma(v[p * 3], v[p * 3 + 1], v[p * 3 + 2]);
#pragma unroll
          for (int c = 0; c < 3; c++) v[p * 3 + c] = col_blend(l, v[p * 3 + c], s.f, inside);
        }
        break;
      case 7:
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] = col_blend(grey, v[j], s.f, inside);
        break;
      case 8:
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] = col_blend(0, v[j], s.f, inside);
        break;
      case 9: {
        int fv[12];
        col_filter<1>(src, H, W, x0, y, v, fv);
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] = col_blend(fv[j], v[j], s.f, inside);
        break;
      }
      case 10:
#pragma unroll
        for (int p = 0; p < 4; p++)
          if (y >= s.i1 && y < s.i3 && x0 + p >= s.i0 && x0 + p < s.i2) v[p * 3] = v[p * 3 + 1] = v[p * 3 + 2] = 128;
        break;
      case 11: {
        int fv[12];
        col_filter<2>(src, H, W, x0, y, v, fv);
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] = fv[j];
        break;
      }
      case 12: {
        int fv[12];
        col_filter<1>(src, H, W, x0, y, v, fv);
#pragma unroll
        for (int j = 0; j < 12; j++) v[j] = fv[j];
        break;
      }
      case 13: {
        // element e of the image (in [H][W][3] order) takes output e % 4 of block e / 4: the quad's 12 elements span up to four blocks
        const uint32_t q0 = (uint32_t)(off >> 2);
        const int r0 = (int)(off & 3);
        float z[16];
#pragma unroll
        for (int j = 0; j < 4; j++) col_normals(q0 + j, (uint32_t)b, (uint32_t)k, s.seed_lo, s.seed_hi, z + 4 * j);
#pragma unroll
        for (int j = 0; j < 12; j++) {
          const float zj = r0 == 0 ? z[j] : (r0 == 1 ? z[j + 1] : (r0 == 2 ? z[j + 2] : z[j + 3]));
          v[j] = min(max(v[j] + (int)rintf(s.f * zj), 0), 255);
        }
        break;
      }
      default: break;
    }
    if (k >= 0) {
      if (wide) {
        uint32_t w[3];
#pragma unroll
        for (int i = 0; i < 3; i++) w[i] = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) | ((uint32_t)v[4 * i + 3] << 24);
        uint32_t* p = reinterpret_cast<uint32_t*>(dst + off);
        p[0] = w[0]; p[1] = w[1]; p[2] = w[2];
      } else {
#pragma unroll
        for (int j = 0; j < 12; j++)
          if (j < nb) dst[off + j] = (uint8_t)v[j];
      }
    }
    if (next == 7) {
      uint32_t l = 0;
#pragma unroll
      for (int p = 0; p < 4; p++)
        if (p * 3 < nb) l += (uint32_t)col_luma(v[p * 3], v[p * 3 + 1], v[p * 3 + 2]);
      atomicAdd(&hist[768], l);
    } else if (next) {
#pragma unroll
      for (int j = 0; j < 12; j++)
        if (j < nb) atomicAdd(&hist[(j % 3) * 256 + v[j]], 1u);
    }
  }
  if (!next) return;                                              // (uniform in the workgroup)
  __syncthreads();
  uint32_t* out_cnt = a.counters + ((int64_t)b * 3 + k + 1) * COL_COUNTERS;
  for (int i = tid; i < COL_COUNTERS; i += COL_THREADS)
    if (hist[i]) atomicAdd(&out_cnt[i], hist[i]);
}

void launch_colour(const ColourArgs& a, hipStream_t s) {
  const int64_t quads = (int64_t)((a.W + 3) >> 2) * a.H;
  const dim3 grid((unsigned)((quads + COL_THREADS * COL_QUADS - 1) / (COL_THREADS * COL_QUADS)), a.B);
  for (int k = -1; k < 3; k++) hipLaunchKernelGGL(colour_kernel, grid, dim3(COL_THREADS), 0, s, a, k);
}
