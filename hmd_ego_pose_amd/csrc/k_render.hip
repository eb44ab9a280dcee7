// k_render.hip - object models rendered under poses: the instance mask, the depth and a filled overlay of every image of a batch from one
// z-buffered triangle rasteriser (hep_render_models_device).  The definition is the project's own, in float64 and exact integers -
// include/hep.h states it in full, tests/_render.py states it in numpy and the kernels reproduce that bit for bit:
//
//   PROJECTION, float64, no contraction (the file is built with -ffp-contract=off, Makefile).  The camera-frame point is
//     p = ((R0 v0 + R1 v1) + R2 v2) + t per row of R, with v the float32 vertex widened; u = (fx X) / Z + cx, v = (fy Y) / Z + cy.
//     Sub-pixel integer coordinates: sx = floor(16 u + 0.5), with 16 u + 0.5 saturated to [-8192*16, 8191*16] before the floor; sy alike.
//     A vertex with Z <= 0 or a NaN anywhere is invalid; a face with an invalid vertex is skipped whole.  There is NO near-plane clipping.
//   COVERAGE, exact in int64.  Pixel (x, y) has its centre at (16 x + 8, 16 y + 8).  With s the sign of the doubled area
//     A' = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) the three edge functions are, for the edges (a, b) = (v1, v2), (v2, v0), (v0, v1) in this order,
//     E_i(p) = dx (py - ay) - dy (px - ax) with (dx, dy) = s (b - a); they sum to A = |A'| > 0.  Faces of either winding are drawn, A' == 0 is
//     skipped.  The pixel is inside when every E_i is positive, or zero on a top-left edge: dy < 0, or dy == 0 and dx > 0.  (d and -d
//     never both qualify and never both fail, so two faces that share an edge never both own, and never both lose, a centre on it.)
//   DEPTH, perspective-correct, float64.  w_i = 1 / Z_i, invz = ((E0 w0 + E1 w1) + E2 w2) / A with E_i and A converted exactly, z = 1 / invz.
//   WINNER per pixel: the smallest (z as float64, pose slot, face index) in lexicographic order; a NaN z never wins.
//
// Launch 1 (render_project_kernel): one thread per (image, slot, vertex) writes sx, sy, 1 / Z - negative: invalid - to the caller's
// workspace [batch][pmax][V] (16 bytes each); threads of a skipped row write nothing, and the later launches read only the rows that are
// not skipped.
// Launch 2 (render_bounds_kernel): one workgroup per (image, slot) reduces the valid vertices' sx, sy to the slot's sub-pixel bounding box
// (integer min / max in a fixed tree: deterministic) behind the vertex records, so that a tile the model does not reach skips the slot's
// faces altogether - every face's box lies inside the slot's, so the rendering is the same.
// Launch 3 (render_raster_kernel): one workgroup of 256 threads per (image, tile of 32 x 8 pixels), one pixel per thread; a wave owns
// two rows, so that a small face is turned away by whole waves after one box test.  (A covered tile's
// workgroup is a serial walk - bin, shade, bin - so small tiles, many workgroups per CU, are what hides its latency.)  All threads walk the valid slots' faces, 256 at a time, and append the faces whose vertices are valid and in
// range, whose area is not zero and whose sub-pixel bounding box meets the tile's pixel centres to an LDS list of RENDER_LIST faces
// (positions by wave ballots and a four-entry prefix: no atomics, the list order is fixed).  When fewer than 256 places are left, and at
// the end, every thread shades ITS OWN pixels against the list and keeps its running winner in registers: no pixel has two writers.  The
// winner is a minimum over a total order, so the result does not depend on where the list was cut.  Tiles that no face meets still write
// the zeros of mask and depth.
#include "hep_dev.h"
#include "hep_eval.h"

#define RENDER_THREADS 256
#define RENDER_TW 32
#define RENDER_TH 8
#define RENDER_PPT 1                                               // pixels of a thread
static_assert(RENDER_TW * RENDER_TH == RENDER_THREADS * RENDER_PPT, "one thread per pixel of the tile");
#define RENDER_LIST 512                                            // 512 x (32 + 24) bytes = 28 KiB of LDS: five workgroups per CU
#define RENDER_SAT_LO (-8192.0 * 16.0)
#define RENDER_SAT_HI (8191.0 * 16.0)
#define RENDER_NO_KEY 0xffffffffu
static_assert(RENDER_LIST >= 2 * RENDER_THREADS && RENDER_LIST <= 4096, "a round of appends always fits behind the flush threshold");
static_assert(RENDER_MAX_POSES * (int64_t)RENDER_MAX_ELEMS <= (1ll << 31), "slot << 24 | face stays below the orientation bit");

// the row of a pose table: is it rendered, and with which label
__device__ __forceinline__ bool render_row(const double* P, int num_labels, int& lab) {
  const double l = P[1], m = P[2];
  if (!(P[0] != 0.0) || !(l >= 0.0 && l < (double)num_labels) || !(m >= 1.0 && m < 256.0)) return false;      // NaN label / value fails
  lab = (int)l;
  return true;
}

__device__ __forceinline__ int render_snap(double u) {
  double t = 16.0 * u + 0.5;
  t = t < RENDER_SAT_LO ? RENDER_SAT_LO : (t > RENDER_SAT_HI ? RENDER_SAT_HI : t);
  return (int)floor(t);
}

__global__ __launch_bounds__(RENDER_THREADS) void render_project_kernel(RenderArgs a) {
  const int v = blockIdx.x * RENDER_THREADS + threadIdx.x, slot = blockIdx.y;
  if (v >= a.V) return;
  const double c0 = (double)a.vertices[3 * (int64_t)v], c1 = (double)a.vertices[3 * (int64_t)v + 1], c2 = (double)a.vertices[3 * (int64_t)v + 2];
  for (int b = blockIdx.z; b < a.B; b += gridDim.z) {
    const double* P = a.poses + ((int64_t)b * a.pmax + slot) * 16;
    int lab;
    if (!render_row(P, a.num_labels, lab)) continue;
    const double* cam = a.camera + (int64_t)b * 5;
    const double X = ((P[4] * c0 + P[5] * c1) + P[6] * c2) + P[13];
    const double Y = ((P[7] * c0 + P[8] * c1) + P[9] * c2) + P[14];
    const double Z = ((P[10] * c0 + P[11] * c1) + P[12] * c2) + P[15];
    RenderVertex o;
    o.sx = 0; o.sy = 0; o.w = -1.0;
    if (Z > 0.0) {                                                // NaN fails
      const double pu = (cam[0] * X) / Z + cam[2], pv = (cam[1] * Y) / Z + cam[3];
      if (pu == pu && pv == pv) { o.sx = render_snap(pu); o.sy = render_snap(pv); o.w = 1.0 / Z; }
    }
    a.ws[((int64_t)b * a.pmax + slot) * a.V + v] = o;             // inside [0, B * pmax * V): b < B, slot < pmax, v < V
  }
}

__global__ __launch_bounds__(RENDER_THREADS) void render_bounds_kernel(RenderArgs a) {
  __shared__ int s_box[4][RENDER_THREADS];
  const int t = threadIdx.x, slot = blockIdx.x;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    int lab;
    if (!render_row(a.poses + ((int64_t)b * a.pmax + slot) * 16, a.num_labels, lab)) continue;      // the same for every thread
    const RenderVertex* wsp = a.ws + ((int64_t)b * a.pmax + slot) * a.V;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
    for (int v = t; v < a.V; v += RENDER_THREADS) {
      const RenderVertex p = wsp[v];
      if (p.w >= 0.0) { x0 = min(x0, p.sx); y0 = min(y0, p.sy); x1 = max(x1, p.sx); y1 = max(y1, p.sy); }
    }
    s_box[0][t] = x0; s_box[1][t] = y0; s_box[2][t] = x1; s_box[3][t] = y1;
    __syncthreads();
    for (int n = RENDER_THREADS / 2; n > 0; n >>= 1) {
      if (t < n) {
        s_box[0][t] = min(s_box[0][t], s_box[0][t + n]); s_box[1][t] = min(s_box[1][t], s_box[1][t + n]);
        s_box[2][t] = max(s_box[2][t], s_box[2][t + n]); s_box[3][t] = max(s_box[3][t], s_box[3][t + n]);
      }
      __syncthreads();
    }
    if (t == 0)                                                    // record B * pmax * V + (b * pmax + slot) of the workspace's B * pmax * (V + 1)
      a.boxes[(int64_t)b * a.pmax + slot] = make_int4(s_box[0][0], s_box[1][0], s_box[2][0], s_box[3][0]);
    __syncthreads();                                               // s_box is the next image's
  }
}

// every thread: its pixel (centre (pcx, pcy0)) against the first n faces of the list
__device__ __forceinline__ void render_shade(const int (*s_v)[8], const double (*s_w)[3], int n, int pcx, int pcy0, double* bz, uint32_t* bkey) {
  for (int e = 0; e < n; e++) {
    const int x0 = s_v[e][0], y0 = s_v[e][1], x1 = s_v[e][2], y1 = s_v[e][3], x2 = s_v[e][4], y2 = s_v[e][5];
    if (pcx < min(x0, min(x1, x2)) || pcx > max(x0, max(x1, x2)) || pcy0 < min(y0, min(y1, y2)) || pcy0 > max(y0, max(y1, y2))) continue;
    const uint32_t keys = (uint32_t)s_v[e][6];
    const int s = (keys >> 31) ? -1 : 1;
    const int dx[3] = {s * (x2 - x1), s * (x0 - x2), s * (x1 - x0)}, dy[3] = {s * (y2 - y1), s * (y0 - y2), s * (y1 - y0)};
    const int ax[3] = {x1, x2, x0}, ay[3] = {y1, y2, y0};
    int64_t E[3];
    bool tl[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      E[i] = (int64_t)dx[i] * (pcy0 - ay[i]) - (int64_t)dy[i] * (pcx - ax[i]);
      tl[i] = dy[i] < 0 || (dy[i] == 0 && dx[i] > 0);
    }
#pragma unroll
    for (int k = 0; k < RENDER_PPT; k++) {
      const int64_t e0 = E[0] - 16 * k * dy[0], e1 = E[1] - 16 * k * dy[1], e2 = E[2] - 16 * k * dy[2];      // one pixel to the right: px + 16
      if (!((e0 > 0 || (e0 == 0 && tl[0])) && (e1 > 0 || (e1 == 0 && tl[1])) && (e2 > 0 || (e2 == 0 && tl[2])))) continue;
      const double invz = (((double)e0 * s_w[e][0] + (double)e1 * s_w[e][1]) + (double)e2 * s_w[e][2]) / (double)(e0 + e1 + e2);
      const double z = 1.0 / invz;
      const uint32_t key = keys & 0x7fffffffu;
      if (z < bz[k] || (z == bz[k] && key < bkey[k])) { bz[k] = z; bkey[k] = key; }
    }
  }
}

__global__ __launch_bounds__(RENDER_THREADS) void render_raster_kernel(RenderArgs a) {
  __shared__ __attribute__((aligned(16))) int s_v[RENDER_LIST][8];          // x0 y0 x1 y1 x2 y2, orientation << 31 | slot << 24 | face, 0
  __shared__ double s_w[RENDER_LIST][3];                                    // 1 / Z of the three vertices
  __shared__ int s_wcnt[2][RENDER_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tiles_x = (a.W + RENDER_TW - 1) / RENDER_TW;
  const int tx0 = (int)(blockIdx.x % tiles_x) * RENDER_TW, ty0 = (int)(blockIdx.x / tiles_x) * RENDER_TH;
  const int tx1 = min(tx0 + RENDER_TW, a.W) - 1, ty1 = min(ty0 + RENDER_TH, a.H) - 1;      // the tile, inclusive
  const int cx0 = 16 * tx0 + 8, cx1 = 16 * tx1 + 8, cy0 = 16 * ty0 + 8, cy1 = 16 * ty1 + 8; // its pixel centres
  const int px = tx0 + (t & (RENDER_TW - 1)), py0 = ty0 + t / RENDER_TW;      // the thread's pixel
  const int pcx = 16 * px + 8, pcy0 = 16 * py0 + 8;

  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    double bz[RENDER_PPT];
    uint32_t bkey[RENDER_PPT];
#pragma unroll
    for (int k = 0; k < RENDER_PPT; k++) { bz[k] = __builtin_inf(); bkey[k] = RENDER_NO_KEY; }
    int count = 0, par = 0;                                       // the same in every thread
    for (int slot = 0; slot < a.pmax; slot++) {
      int lab;
      if (!render_row(a.poses + ((int64_t)b * a.pmax + slot) * 16, a.num_labels, lab)) continue;
      const int4 box = a.boxes[(int64_t)b * a.pmax + slot];       // x0 y0 x1 y1 of the slot's valid vertices; none: an empty box
      if (box.z < cx0 || box.x > cx1 || box.w < cy0 || box.y > cy1) continue;
      const RenderVertex* wsp = a.ws + ((int64_t)b * a.pmax + slot) * a.V;
      const int f1 = a.face_start[lab + 1];
      for (int fb = a.face_start[lab]; fb < f1; fb += RENDER_THREADS) {
        if (count > RENDER_LIST - RENDER_THREADS) {
          __syncthreads();                                        // the list is written
          render_shade(s_v, s_w, count, pcx, pcy0, bz, bkey);
          __syncthreads();                                        // ... and read
          count = 0;
        }
        const int f = fb + t;
        bool pass = false;
        RenderVertex A, B, C;
        int sgn = 0;
        if (f < f1) {                                             // f < F: face_start is checked on the host
          const int i0 = a.faces[3 * (int64_t)f], i1 = a.faces[3 * (int64_t)f + 1], i2 = a.faces[3 * (int64_t)f + 2];
          if ((unsigned)i0 < (unsigned)a.V && (unsigned)i1 < (unsigned)a.V && (unsigned)i2 < (unsigned)a.V) {
            A = wsp[i0]; B = wsp[i1]; C = wsp[i2];
            if (A.w >= 0.0 && B.w >= 0.0 && C.w >= 0.0 &&
                !(max(A.sx, max(B.sx, C.sx)) < cx0 || min(A.sx, min(B.sx, C.sx)) > cx1 || max(A.sy, max(B.sy, C.sy)) < cy0 || min(A.sy, min(B.sy, C.sy)) > cy1)) {
              const int64_t area = (int64_t)(B.sx - A.sx) * (C.sy - A.sy) - (int64_t)(B.sy - A.sy) * (C.sx - A.sx);
              sgn = area > 0 ? 1 : (area < 0 ? -1 : 0);
              pass = sgn != 0;
            }
          }
        }
        const unsigned long long bal = __ballot(pass);
        if (lane == 0) s_wcnt[par][wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RENDER_THREADS / 64; w++) { const int c = s_wcnt[par][w]; if (w < wave) before += c; total += c; }
        if (pass) {
          const int e = count + before + __popcll(bal & ((1ull << lane) - 1ull));      // < count + 256 <= RENDER_LIST
          s_v[e][0] = A.sx; s_v[e][1] = A.sy; s_v[e][2] = B.sx; s_v[e][3] = B.sy; s_v[e][4] = C.sx; s_v[e][5] = C.sy;
          s_v[e][6] = (int)((sgn < 0 ? 0x80000000u : 0u) | (uint32_t)slot << 24 | (uint32_t)f);
          s_v[e][7] = 0;
          s_w[e][0] = A.w; s_w[e][1] = B.w; s_w[e][2] = C.w;
        }
        count += total;
        par ^= 1;                                                 // the counts of round i + 2 are written after everyone passed round i + 1's barrier
      }
    }
    __syncthreads();
    render_shade(s_v, s_w, count, pcx, pcy0, bz, bkey);

#pragma unroll
    for (int k = 0; k < RENDER_PPT; k++) {
      const int qx = px + k, py = py0;
      if (qx > tx1 || py > ty1) continue;
      const int64_t o = ((int64_t)b * a.H + py) * a.W + qx;       // inside [0, B * H * W): b < B, py < H, qx < W
      const bool hit = bkey[k] != RENDER_NO_KEY;
      const double* P = a.poses + ((int64_t)b * a.pmax + (hit ? (bkey[k] >> 24) : 0)) * 16;
      if (a.mask) a.mask[o] = hit ? (uint8_t)(int)P[2] : (uint8_t)0;
      if (a.depth) a.depth[o] = hit ? (float)bz[k] : 0.0f;
      if (a.frames && hit) {
        const uint8_t* c = a.colours + 3 * (int)P[1];
        uint8_t* q = a.frames + 3 * o;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) q[ch] = (uint8_t)((a.alpha * (int)c[ch] + (256 - a.alpha) * (int)q[ch] + 128) >> 8);
      }
    }
    __syncthreads();                                              // the list is the next image's
  }
}

void launch_render(const RenderArgs& a, hipStream_t s) {
  const int B = a.B < 65535 ? a.B : 65535;
  hipLaunchKernelGGL(render_project_kernel, dim3((a.V + RENDER_THREADS - 1) / RENDER_THREADS, a.pmax, B), dim3(RENDER_THREADS), 0, s, a);
  hipLaunchKernelGGL(render_bounds_kernel, dim3(a.pmax, B), dim3(RENDER_THREADS), 0, s, a);
  const int tiles = ((a.W + RENDER_TW - 1) / RENDER_TW) * ((a.H + RENDER_TH - 1) / RENDER_TH);
  hipLaunchKernelGGL(render_raster_kernel, dim3(tiles, B), dim3(RENDER_THREADS), 0, s, a);
}
