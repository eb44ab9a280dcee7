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
//
// Synthetic frames (hep_synth_frames_device, launch_synth): the SAME launches with SynthArgs for RenderArgs - launches 2 and 3 are templates
// over their argument, and the renderer's instantiation is the code it always was.  The shaded variant of launch 2 also writes the empty
// visible record of its (image, slot); that of launch 3 shades each pixel's winner ONCE, after the face walk (synth_shade: float64, every
// rounding stated in include/hep.h and tests/_synth.py), composites it and reduces min / max / count of the pixels each slot won - in LDS
// first, then one integer atomicMin / atomicMax / atomicAdd set per (workgroup, slot that won a pixel): only commutative integer operations
// cross workgroups, so the record does not depend on arrival order.  Launch 4 (synth_annotate_kernel): one thread per image compacts the
// kept slots into the padded annotation tensors.
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

// the kernel argument of a variant: RenderArgs itself, or SynthArgs around it (SHADE)
__device__ __forceinline__ const RenderArgs& render_args(const RenderArgs& a) { return a; }
__device__ __forceinline__ const RenderArgs& render_args(const SynthArgs& a) { return a.r; }
template <class Args> struct RenderShades { static constexpr bool value = false; };
template <> struct RenderShades<SynthArgs> { static constexpr bool value = true; };

template <class Args>
__global__ __launch_bounds__(RENDER_THREADS) void render_bounds_kernel(Args args) {
  __shared__ int s_box[4][RENDER_THREADS];
  const RenderArgs& a = render_args(args);
  const int t = threadIdx.x, slot = blockIdx.x;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    int lab;
    if constexpr (RenderShades<Args>::value) {                      // the empty visible record of EVERY (image, slot), skipped rows included
      if (t < SYNTH_VISIBLE_INTS)                                   // inside [0, B * pmax * 5): b < B, slot < pmax
        args.visible[((int64_t)b * a.pmax + slot) * SYNTH_VISIBLE_INTS + t] = t < 2 ? INT_MAX : (t < 4 ? INT_MIN : 0);
    }
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

// SHADE: the winner of pixel (px, py) of image b shaded from its three vertex colours and its face's normal under the image's light -
// once per pixel, after the face walk; include/hep.h (hep_synth_frames_device) states every rounding, tests/_synth.py in numpy
__device__ __forceinline__ void synth_shade(const SynthArgs& x, int b, uint32_t key, int pcx, int pcy, int out[3]) {
  const RenderArgs& a = x.r;
  const int slot = (int)(key >> 24), f = (int)(key & 0xffffffu);  // a winner's face passed the index test of the walk: f < F, indices < V
  const double* P = a.poses + ((int64_t)b * a.pmax + slot) * 16;
  const RenderVertex* wsp = a.ws + ((int64_t)b * a.pmax + slot) * a.V;
  const int i0 = a.faces[3 * (int64_t)f], i1 = a.faces[3 * (int64_t)f + 1], i2 = a.faces[3 * (int64_t)f + 2];
  const RenderVertex A = wsp[i0], B = wsp[i1], C = wsp[i2];
  const int64_t area = (int64_t)(B.sx - A.sx) * (C.sy - A.sy) - (int64_t)(B.sy - A.sy) * (C.sx - A.sx);
  const int s = area < 0 ? -1 : 1;
  const int64_t e0 = (int64_t)(s * (C.sx - B.sx)) * (pcy - B.sy) - (int64_t)(s * (C.sy - B.sy)) * (pcx - B.sx);
  const int64_t e1 = (int64_t)(s * (A.sx - C.sx)) * (pcy - C.sy) - (int64_t)(s * (A.sy - C.sy)) * (pcx - C.sx);
  const int64_t e2 = (int64_t)(s * (B.sx - A.sx)) * (pcy - A.sy) - (int64_t)(s * (B.sy - A.sy)) * (pcx - A.sx);
  const double q0 = (double)e0 * A.w, q1 = (double)e1 * B.w, q2 = (double)e2 * C.w;
  const double den = (q0 + q1) + q2;
  const double b0 = q0 / den, b1 = q1 / den, b2 = q2 / den;
  const double* n = x.face_normals + 3 * (int64_t)f;
  const double n0 = n[0], n1 = n[1], n2 = n[2];
  const double m0 = (P[4] * n0 + P[5] * n1) + P[6] * n2, m1 = (P[7] * n0 + P[8] * n1) + P[9] * n2, m2 = (P[10] * n0 + P[11] * n1) + P[12] * n2;
  const double* L = x.lights + (int64_t)b * SYNTH_LIGHT_DOUBLES;
  double d = (m0 * L[0] + m1 * L[1]) + m2 * L[2];
  d = d < 0.0 ? -d : d;                                           // two-sided
  const double sh = L[3] + L[4] * d;
  const uint8_t* c0 = x.vertex_colours + 3 * (int64_t)i0;
  const uint8_t* c1 = x.vertex_colours + 3 * (int64_t)i1;
  const uint8_t* c2 = x.vertex_colours + 3 * (int64_t)i2;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double c = (b0 * (double)c0[k] + b1 * (double)c1[k]) + b2 * (double)c2[k];
    const double v = (c * sh) * L[5 + k];
    const double t = v + 0.5;
    out[k] = !(t >= 0.0) ? 0 : (t >= 256.0 ? 255 : (int)floor(t));      // NaN: 0
  }
}

template <class Args>
__global__ __launch_bounds__(RENDER_THREADS) void render_raster_kernel(Args args) {
  constexpr bool SHADE = RenderShades<Args>::value;
  const RenderArgs& a = render_args(args);
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

  __shared__ int s_vis[SHADE ? RENDER_MAX_POSES : 1][SYNTH_VISIBLE_INTS];    // SHADE: min_x, min_y, max_x, max_y, count of the tile's pixels each slot won

  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    if constexpr (SHADE) {                                        // read back before the barrier that ends the previous image; the walk's barriers follow
      if (t < RENDER_MAX_POSES * SYNTH_VISIBLE_INTS) s_vis[t / SYNTH_VISIBLE_INTS][t % SYNTH_VISIBLE_INTS] = t % SYNTH_VISIBLE_INTS < 2 ? INT_MAX : (t % SYNTH_VISIBLE_INTS < 4 ? INT_MIN : 0);
    }
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
      if constexpr (SHADE) {
        if (hit) {
          int c[3];
          synth_shade(args, b, bkey[k], 16 * qx + 8, 16 * py + 8, c);
          uint8_t* q = a.frames + 3 * o;
#pragma unroll
          for (int ch = 0; ch < 3; ch++) q[ch] = (uint8_t)((a.alpha * c[ch] + (256 - a.alpha) * (int)q[ch] + 128) >> 8);
          int* v = s_vis[bkey[k] >> 24];                          // slot < pmax <= RENDER_MAX_POSES
          atomicMin(&v[0], qx); atomicMin(&v[1], py); atomicMax(&v[2], qx); atomicMax(&v[3], py); atomicAdd(&v[4], 1);
        }
      } else if (a.frames && hit) {
        const uint8_t* c = a.colours + 3 * (int)P[1];
        uint8_t* q = a.frames + 3 * o;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) q[ch] = (uint8_t)((a.alpha * (int)c[ch] + (256 - a.alpha) * (int)q[ch] + 128) >> 8);
      }
    }
    if constexpr (SHADE) {
      // the workgroup's pixels per slot are reduced; integer min / max / add commute, so the global record does not depend on which tile arrives first
      __syncthreads();
      if (t < a.pmax && s_vis[t][4] > 0) {
        int32_t* g = args.visible + ((int64_t)b * a.pmax + t) * SYNTH_VISIBLE_INTS;      // inside [0, B * pmax * 5)
        atomicMin(&g[0], s_vis[t][0]); atomicMin(&g[1], s_vis[t][1]); atomicMax(&g[2], s_vis[t][2]); atomicMax(&g[3], s_vis[t][3]); atomicAdd(&g[4], s_vis[t][4]);
      }
    }
    __syncthreads();                                              // the list is the next image's
  }
}

// SHADE's last launch: one thread per image walks the slots in order and keeps a slot whose row is rendered and whose visible count reaches
// min_pixels; the n-th kept slot becomes row n of the padded annotation tensors (augment.pad_annotations' layout), the rest is zeros
__global__ __launch_bounds__(64) void synth_annotate_kernel(SynthArgs x) {
  const RenderArgs& a = x.r;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  int n = 0;                                                     // rows written so far: n <= slot < pmax, so every index below stays inside [B][pmax][.]
  for (int slot = 0; slot < a.pmax; slot++) {
    const int64_t src = (int64_t)b * a.pmax + slot, o = (int64_t)b * a.pmax + n;
    const double* P = a.poses + src * 16;
    const int32_t* vis = x.visible + src * SYNTH_VISIBLE_INTS;
    int lab;
    if (!render_row(P, a.num_labels, lab) || vis[4] < x.min_pixels) continue;
    for (int k = 0; k < 4; k++) x.out_boxes[4 * o + k] = (double)vis[k];
    x.out_labels[o] = lab;
    x.out_mask_values[o] = (int)P[2];
    for (int k = 0; k < 3; k++) { x.out_rvec[3 * o + k] = x.rvec[3 * src + k]; x.out_tvec[3 * o + k] = x.tvec[3 * src + k]; }
    for (int k = 0; k < 2; k++) x.out_extra[2 * o + k] = x.extra[2 * src + k];
    x.slot_of[o] = slot;
    n++;
  }
  for (int r = n; r < a.pmax; r++) {                             // the padding: zeros, and no source slot
    const int64_t o = (int64_t)b * a.pmax + r;
    for (int k = 0; k < 4; k++) x.out_boxes[4 * o + k] = 0.0;
    x.out_labels[o] = 0;
    x.out_mask_values[o] = 0;
    for (int k = 0; k < 3; k++) { x.out_rvec[3 * o + k] = 0.0f; x.out_tvec[3 * o + k] = 0.0f; }
    for (int k = 0; k < 2; k++) x.out_extra[2 * o + k] = 0.0f;
    x.slot_of[o] = -1;
  }
  x.num_gt[b] = n;
}

template <class Args>
static void launch_raster(const Args& args, const RenderArgs& a, hipStream_t s) {
  const int B = a.B < 65535 ? a.B : 65535;
  hipLaunchKernelGGL(render_project_kernel, dim3((a.V + RENDER_THREADS - 1) / RENDER_THREADS, a.pmax, B), dim3(RENDER_THREADS), 0, s, a);
  hipLaunchKernelGGL(render_bounds_kernel<Args>, dim3(a.pmax, B), dim3(RENDER_THREADS), 0, s, args);
  const int tiles = ((a.W + RENDER_TW - 1) / RENDER_TW) * ((a.H + RENDER_TH - 1) / RENDER_TH);
  hipLaunchKernelGGL(render_raster_kernel<Args>, dim3(tiles, B), dim3(RENDER_THREADS), 0, s, args);
}

void launch_render(const RenderArgs& a, hipStream_t s) { launch_raster(a, a, s); }

void launch_synth(const SynthArgs& x, hipStream_t s) {
  launch_raster(x, x.r, s);
  if (x.num_gt) hipLaunchKernelGGL(synth_annotate_kernel, dim3((x.r.B + 63) / 64), dim3(64), 0, s, x);
}
