// k_draw.hip - pose overlays: the valid annotations and the kept detections of every image of a batch drawn into the uint8 frames in
// place, one launch (hep_draw_poses_device; the step of eval/common.py:452-479 with the shapes of generators/utils/visualization.py:85-117,
// 143-232, 234-290).  The drawing is the project's own definition in integer arithmetic - include/hep.h states it in full, tests/_draw.py
// states it in numpy and the kernel reproduces that byte for byte; cv2's line and circle rasterisers are NOT restated.
//
// One workgroup of 256 threads owns one tile of 64 x 16 pixels of one image (thread t: column t % 64, rows t / 64 + 4 k):
//   1. the candidates (score > threshold, float32) are ranked in row order by ballots, the first max_detections are kept;
//   2. one thread per shape (annotation slot, then kept detection) makes its rotation matrix and translation in float64 (rodrigues_f64);
//   3. the threads project the 34 points of every shape - four corners of the 2D box, eight cuboid corners, the centre, 21 joints - into
//      LDS as saturated, truncated integers with a validity byte;
//   4. one thread per shape marks the primitives (of the enabled layers, with valid end points) whose padded bounding box meets the tile:
//      a 37-bit mask per shape in LDS;
//   5. every thread walks the shapes and the set bits in order (wave-uniform: the masks are the tile's) and tests its own four pixels with
//      the int64 coverage rule; the last hit wins; a thread stores the three bytes of the pixels that were hit and nothing else.
// No atomics, no pixel has two writers, no floating point after step 3: the result is deterministic by construction.  The file is built
// with -ffp-contract=off (Makefile), so the projection's statements round as tests/_draw.py's do.
#include "hep_dev.h"
#include "hep_eval.h"
#include "eval_dev.h"

#define DRAW_THREADS 256
#define DRAW_TW 64
#define DRAW_TH 16
#define DRAW_ROWS_PER_THREAD (DRAW_TH / (DRAW_THREADS / DRAW_TW))
#define DRAW_SHAPES (SCORE_MAX_ANN + DRAW_MAX_DET)
#define DRAW_PTS 34                  // 0-3 box corners, 4-11 cuboid corners, 12 centre, 13-33 hand joints
#define DRAW_PRIMS 37                // 0-3 box, 4-15 cuboid edges (visualization.py:99-112), 16 centre disc, 17-36 hand chains
#define DRAW_SAT_LO (-8192.0)
#define DRAW_SAT_HI 8191.0

// end points of primitive i as point indices
__device__ __forceinline__ void draw_prim_points(int i, int& pa, int& pb) {
  if (i < 4) { pa = i; pb = (i + 1) & 3; return; }
  if (i < 16) {
    const int e = i - 4;
    if (e < 8) { const int base = 4 + (e & 4), k = e & 3; pa = base + (k == 3 ? 0 : k); pb = base + (k == 3 ? 3 : k + 1); }   // 0-1 1-2 2-3 0-3, then 4-5 5-6 6-7 4-7
    else { pa = 4 + (e - 8); pb = pa + 4; }                                                                                    // 0-4 1-5 2-6 3-7
    return;
  }
  if (i == 16) { pa = pb = 12; return; }
  const int h = i - 17, f = h >> 2, k = h & 3;                    // finger f, link k: joints (k == 0 ? 0 : 4 f + k) - (4 f + k + 1)
  pa = 13 + (k == 0 ? 0 : 4 * f + k);
  pb = 13 + 4 * f + k + 1;
}

__device__ __forceinline__ int draw_sat_trunc(double v) {
  v = v < DRAW_SAT_LO ? DRAW_SAT_LO : (v > DRAW_SAT_HI ? DRAW_SAT_HI : v);
  return (int)v;                                                  // toward zero, numpy's astype(int)
}

// pixel (px, py) against the segment a-b of thickness t (tt = t * t): exact in int64 (include/hep.h)
__device__ __forceinline__ bool draw_segment_covers(int px, int py, int ax, int ay, int bx, int by, int64_t tt) {
  const int64_t dx = bx - ax, dy = by - ay, qx = px - ax, qy = py - ay;
  const int64_t L = dx * dx + dy * dy, s = qx * dx + qy * dy;
  if (s <= 0) return 4 * (qx * qx + qy * qy) <= tt;
  if (s >= L) { const int64_t rx = px - bx, ry = py - by; return 4 * (rx * rx + ry * ry) <= tt; }
  const int64_t c = qx * dy - qy * dx;
  return 4 * (c * c) <= tt * L;
}

__global__ __launch_bounds__(DRAW_THREADS) void draw_kernel(DrawArgs a) {
  __shared__ double s_pose[DRAW_SHAPES][12];                      // R (9, row-major), t (3)
  __shared__ short2 s_pt[DRAW_SHAPES][DRAW_PTS];
  __shared__ uint8_t s_ok[DRAW_SHAPES][DRAW_PTS];
  __shared__ unsigned long long s_hit[DRAW_SHAPES];
  __shared__ int s_label[DRAW_SHAPES], s_row[DRAW_SHAPES];        // label (-1: nothing to draw); annotation slot or detection row
  __shared__ int s_detrow[DRAW_MAX_DET], s_wcnt[DRAW_THREADS / 64];
  const int t = threadIdx.x;
  const int tiles_x = (a.W + DRAW_TW - 1) / DRAW_TW;
  const int x0 = (int)(blockIdx.x % tiles_x) * DRAW_TW, y0 = (int)(blockIdx.x / tiles_x) * DRAW_TH;
  const int x1 = min(x0 + DRAW_TW, a.W) - 1, y1 = min(y0 + DRAW_TH, a.H) - 1;      // the tile, inclusive
  const int nann = a.gt ? a.amax : 0;
  const int64_t tt = (int64_t)a.thickness * a.thickness;
  const int pad = (a.thickness + 1) / 2;

  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const double* gt0 = a.gt ? a.gt + (int64_t)b * a.amax * SCORE_GT_DOUBLES : nullptr;
    const double* cam = a.camera ? a.camera + (int64_t)b * 5 : gt0 + 14;
    const int64_t r0 = (int64_t)b * a.rows;

    // 1. candidates in row order, the first max_det kept
    bool flag = false;
    if (a.scores && t < a.rows) flag = a.scores[r0 + t] > a.score_thr;       // padding (-1) and NaN are no candidates
    const unsigned long long bal = __ballot(flag);
    if ((t & 63) == 0) s_wcnt[t >> 6] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < DRAW_THREADS / 64; w++) { const int c = s_wcnt[w]; if (w < (t >> 6)) before += c; total += c; }
    const int rank = before + __popcll(bal & ((1ull << (t & 63)) - 1ull));
    if (flag && rank < a.max_det) s_detrow[rank] = t;
    const int ndet = min(total, a.max_det), nshapes = nann + ndet;
    __syncthreads();

    // 2. one thread per shape: label, rotation matrix, translation
    if (t < nshapes) {
      int lab = -1, row;
      double* P = s_pose[t];
      if (t < nann) {
        const double* g = gt0 + (int64_t)t * SCORE_GT_DOUBLES;
        row = t;
        const double l = g[83];
        if (g[0] != 0.0 && l >= 0.0 && l < (double)a.num_labels) lab = (int)l;      // NaN fails both compares
        if (lab >= 0) { rodrigues_f64(g + 5, P); for (int k = 0; k < 3; k++) P[9 + k] = g[8 + k]; }
      } else {
        row = s_detrow[t - nann];
        const int l = a.labels[r0 + row];
        if (l >= 0 && l < a.num_labels) lab = l;
        if (lab >= 0) {
          float rv[3];
          for (int k = 0; k < 3; k++) rv[k] = a.rotation[(r0 + row) * 3 + k] * 3.14159274f;      // np.float32(math.pi), in float32
          rodrigues_f64(rv, P);
          for (int k = 0; k < 3; k++) P[9 + k] = (double)a.translation[(r0 + row) * 3 + k];
        }
      }
      s_label[t] = lab; s_row[t] = row;
    }
    __syncthreads();

    // 3. the points of every shape
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    const float scale = (float)cam[4];
    for (int idx = t; idx < nshapes * DRAW_PTS; idx += DRAW_THREADS) {
      const int s = idx / DRAW_PTS, p = idx - s * DRAW_PTS;
      const int lab = s_label[s], row = s_row[s];
      const bool ann = s < nann;
      const double* g = ann ? gt0 + (int64_t)row * SCORE_GT_DOUBLES : nullptr;
      bool ok = lab >= 0;
      double u = 0.0, v = 0.0;
      if (ok && p < 4) {                                          // 2D box corners: (x1,y1) (x2,y1) (x2,y2) (x1,y2)
        const int ix = (p == 1 || p == 2) ? 2 : 0, iy = (p >= 2) ? 3 : 1;
        if (ann) { u = g[1 + ix]; v = g[1 + iy]; }
        else { u = (double)(a.boxes[(r0 + row) * 4 + ix] / scale); v = (double)(a.boxes[(r0 + row) * 4 + iy] / scale); }
      } else if (ok) {
        const double* P = s_pose[s];
        double X, Y, Z;
        if (p < 12) {
          const float* c = a.cuboids + ((int64_t)lab * 8 + (p - 4)) * 3;
          const double c0 = c[0], c1 = c[1], c2 = c[2];
          X = ((P[0] * c0 + P[1] * c1) + P[2] * c2) + P[9];
          Y = ((P[3] * c0 + P[4] * c1) + P[5] * c2) + P[10];
          Z = ((P[6] * c0 + P[7] * c1) + P[8] * c2) + P[11];
        } else if (p == 12) {
          X = P[9]; Y = P[10]; Z = P[11];
        } else {
          const int j = p - 13;
          if (ann) {
            ok = g[19] != 0.0;
            X = g[20 + 3 * j]; Y = g[21 + 3 * j]; Z = g[22 + 3 * j];
          } else {
            ok = a.hand != nullptr;
            const float* h = ok ? a.hand + (r0 + row) * 63 + 3 * j : nullptr;
            X = ok ? (double)h[0] : 0.0; Y = ok ? (double)h[1] : 0.0; Z = ok ? (double)h[2] : 1.0;
          }
        }
        ok = ok && Z > 0.0;                                       // NaN fails
        if (ok) { u = (fx * X) / Z + cx; v = (fy * Y) / Z + cy; }
      }
      ok = ok && u == u && v == v;
      s_pt[s][p] = make_short2((short)(ok ? draw_sat_trunc(u) : 0), (short)(ok ? draw_sat_trunc(v) : 0));
      s_ok[s][p] = ok ? 1 : 0;
    }
    __syncthreads();

    // 4. per shape: the primitives that can touch this tile
    if (t < nshapes) {
      unsigned long long m = 0;
      const int layers = t < nann ? a.ann_layers : a.det_layers;
      if (s_label[t] >= 0)
        for (int i = 0; i < DRAW_PRIMS; i++) {
          const int layer = i < 4 ? DRAW_BOX2D : (i < 17 ? DRAW_CUBOID : DRAW_HAND);
          if (!(layers & layer)) continue;
          int pa, pb;
          draw_prim_points(i, pa, pb);
          if (!s_ok[t][pa] || !s_ok[t][pb]) continue;
          const short2 A = s_pt[t][pa], B = s_pt[t][pb];
          const int pd = i == 16 ? 3 : pad;
          if (min(A.x, B.x) - pd > x1 || max(A.x, B.x) + pd < x0 || min(A.y, B.y) - pd > y1 || max(A.y, B.y) + pd < y0) continue;
          m |= 1ull << i;
        }
      s_hit[t] = m;
    }
    __syncthreads();

    // 5. every thread: its pixels against the tile's primitives, in order
    const int px = x0 + (t & (DRAW_TW - 1)), py0 = y0 + (t >> 6);
    uint32_t col[DRAW_ROWS_PER_THREAD];
    for (int k = 0; k < DRAW_ROWS_PER_THREAD; k++) col[k] = 0;
    for (int s = 0; s < nshapes; s++) {
      const unsigned long long hm = s_hit[s];
      uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)hm), hi = __builtin_amdgcn_readfirstlane((uint32_t)(hm >> 32));     // the same in every lane: said so
      if ((lo | hi) == 0) continue;
      const bool ann = s < nann;
      const int lab = s_label[s];
      const uint32_t own = ann ? 0x0000ff00u : ((uint32_t)a.colours[3 * lab] | (uint32_t)a.colours[3 * lab + 1] << 8 | (uint32_t)a.colours[3 * lab + 2] << 16);
      while (lo | hi) {
        const int i = lo ? __builtin_ctz(lo) : 32 + __builtin_ctz(hi);
        if (lo) lo &= lo - 1; else hi &= hi - 1;
        int pa, pb;
        draw_prim_points(i, pa, pb);
        const short2 A = s_pt[s][pa], B = s_pt[s][pb];
        uint32_t c = own;
        if (i < 4) c = ann ? 0x00007f00u : 0x00ff00ffu;           // (0,127,0) / (255,0,255)
        else if (i > 16 && ann) c = 0x0000b200u;                  // (0,178,0)
        c |= 1u << 24;
        for (int k = 0; k < DRAW_ROWS_PER_THREAD; k++) {
          const int py = py0 + k * (DRAW_THREADS / DRAW_TW);
          bool hit;
          if (i == 16) { const int64_t qx = px - A.x, qy = py - A.y; hit = qx * qx + qy * qy <= 9; }
          else hit = draw_segment_covers(px, py, A.x, A.y, B.x, B.y, tt);
          if (hit) col[k] = c;
        }
      }
    }
    if (px <= x1)
      for (int k = 0; k < DRAW_ROWS_PER_THREAD; k++) {
        const int py = py0 + k * (DRAW_THREADS / DRAW_TW);
        if (py > y1 || !(col[k] >> 24)) continue;
        uint8_t* o = a.frames + (((int64_t)b * a.H + py) * a.W + px) * 3;        // inside [0, B*H*W*3): b < B, py < H, px < W
        o[0] = (uint8_t)col[k]; o[1] = (uint8_t)(col[k] >> 8); o[2] = (uint8_t)(col[k] >> 16);
      }
    __syncthreads();                                              // the LDS is the next image's
  }
}

void launch_draw(const DrawArgs& a, hipStream_t s) {
  const int tiles = ((a.W + DRAW_TW - 1) / DRAW_TW) * ((a.H + DRAW_TH - 1) / DRAW_TH);
  hipLaunchKernelGGL(draw_kernel, dim3(tiles, a.B < 65535 ? a.B : 65535), dim3(DRAW_THREADS), 0, s, a);
}
