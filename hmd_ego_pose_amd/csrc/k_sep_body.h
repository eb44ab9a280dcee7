// k_sep_body.h - the body of the separable-conv kernels, included by k_sep_impl.h into sep_kernel (D = 0) and sep_shape_kernel (D > 0);
// it expects BF16, MODE, WL, W8, D and the kernel argument `a` in scope.  Text and not a function: behind a force-inlined function that
// takes the arguments by reference the generic kernels' code changed (k_chain_body.h).
  static_assert(!W8 || (BF16 && MODE == 0 && !WL), "eight-wave form: single bf16 nodes without staged weights");
  static_assert(!D || W8, "shape rows: the eight-wave single-node form");
  constexpr int SEP_THREADS = W8 ? 512 : SEP_THREADS_OF(MODE, BF16), SEP_WAVES = SEP_THREADS / 64;
  constexpr bool SINGLE = MODE == 0;
  constexpr SepShape SH = sep_shape(D);
  constexpr SepLds L = SEP_SHAPE_LDS;
  typedef Vec8<BF16> V;
  typedef typename V::elem T;
  typedef Frag<BF16> F;
  typedef typename F::raw raw_t;
  constexpr int KSTEP = F::KSTEP, KLANE = F::KLANE, PAD = BF16 ? 8 : 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  HEP_POISON(smem, D ? L.lds_bytes : a.lds_bytes);
#ifdef HEP_TOWER_TRACE
  unsigned long long sstamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  SSTAMP_NOWAIT(0);
#endif
  // the segment descriptor is never re-read from global memory: single-segment launches (BiFPN
  // nodes) take it from the kernel arguments (scalar loads), multi-segment launches (heads) copy
  // theirs into LDS once
  __shared__ SepSeg seg_s;
  for (int chain_i = 0; chain_i < (MODE == 2 ? a.nseg : 1); chain_i++) {
  if (!SINGLE) {
    const int si = MODE == 2 ? chain_i : a.tile_seg[blockIdx.x];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.segs + si);
    if (threadIdx.x < sizeof(SepSeg) / 4) reinterpret_cast<uint32_t*>(&seg_s)[threadIdx.x] = src[threadIdx.x];
    __syncthreads();
  }
  const SepSeg& sg = SINGLE ? a.seg0 : seg_s;
  const int C = D ? SEP_SHAPE_C : sg.C, CG = C >> 3, h = D ? SH.h : sg.h, w = D ? SH.w : sg.w, TS = D ? SEP_SHAPE_TS : sg.ts, HS = TS + 2;
  const int tilesN = D ? SEP_SHAPE_C / 16 : sg.tilesN;
  const int tiles_x = D ? SH.w / SEP_SHAPE_TS : sg.tiles_x;
  const uint32_t tiles_x_rcp = D ? rcp_u32(SH.w / SEP_SHAPE_TS) : sg.tiles_x_rcp;
  const int t = MODE == 2 ? 0 : (D ? (int)blockIdx.x : blockIdx.x - sg.tile_begin);
  const int b = blockIdx.y;                 // grid = (tiles of one image over all segments, batch)
  const int tile_y = udiv_rcp(t, tiles_x_rcp);
  const int y0 = tile_y * TS, x0 = (t - tile_y * tiles_x) * TS;
  const int CH = C + PAD;                   // halo and operand-tile row pitch (elements)
  T* halo = reinterpret_cast<T*>(smem);
  T* atile = reinterpret_cast<T*>(smem + (D ? L.off_atile : a.off_atile));
  float* wdw_s = reinterpret_cast<float*>(smem + (D ? L.off_wdw : a.off_wdw));
  float* bias_s = reinterpret_cast<float*>(smem + (D ? L.off_bias : a.off_bias));

  // (index arithmetic below: channel groups and tile sides are split with shifts and masks, the halo
  //  side with a compile-time divisor per tile size - a run-time integer division costs ~30 VALU
  //  instructions and this kernel used to issue half a dozen of them per work item)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  // (a row's maps are whole tiles: every tile row and column is valid)
  static_assert(SH.h % SEP_SHAPE_TS == 0 && SH.w % SEP_SHAPE_TS == 0, "SEP_SHAPES: maps of whole 8x8 tiles");
  const int rows_valid = D ? SEP_SHAPE_TS : min(TS, h - y0), cols_valid = D ? SEP_SHAPE_TS : min(TS, w - x0);
  const int mtv = TS == 16 ? rows_valid : (TS == 8 ? (rows_valid + 1) >> 1 : 1);   // 16-pixel m-tiles holding a valid pixel (TS 4: the whole tile)
  const int ksteps = (C + KSTEP - 1) / KSTEP;
  const T* W = reinterpret_cast<const T*>(sg.wpw);
  const int cgsh = CG <= 1 ? 0 : 32 - __builtin_clz(CG - 1);
  const int tssh = TS == 16 ? 4 : (TS == 8 ? 3 : 2);
  const int mtsh = mtv <= 1 ? 0 : 32 - __builtin_clz(mtv - 1);
  // ---- phase 0: everything that does not depend on the activations is REQUESTED here and parked in LDS once the
  //      gathers are in flight: depthwise weights, bias (16-byte vectors; were two dword loops = two round trips in
  //      front of the gathers) and the weight fragments of this wave's first (m-tile, n-tile) pair of phase 3 (were
  //      a global round trip between the depthwise conv and the MFMAs) ----
  const int nwv = (9 * C) >> 2, nbv = tilesN * 4;
  const f32x4* wdw_g = reinterpret_cast<const f32x4*>(sg.wdw);
  const f32x4 wv0 = wdw_g[min((int)threadIdx.x, nwv - 1)];
  const f32x4 bv = reinterpret_cast<const f32x4*>(sg.bias)[min((int)threadIdx.x, nbv - 1)];
  constexpr int WPRE = 2;                                 // k-steps of prefetched weight fragments (all of them for C = 64 in bf16)
  raw_t wpre[WPRE];
  if constexpr (!WL) {
    const T* wrow = W + (int64_t)(min(wave >> mtsh, tilesN - 1) * 16 + r) * C;
#pragma unroll
    for (int q = 0; q < WPRE; q++) {
      wpre[q] = *reinterpret_cast<const raw_t*>(wrow + min(q * KSTEP + KLANE * g, C - KLANE));   // (k >= C meets a zero activation fragment)
    }
  }
  auto park = [&]() {
    f32x4* wd = reinterpret_cast<f32x4*>(wdw_s);
    if ((int)threadIdx.x < nwv) wd[threadIdx.x] = wv0;
    for (int i = threadIdx.x + SEP_THREADS; i < nwv; i += SEP_THREADS) wd[i] = wdw_g[i];      // (C > 455 / 227 only)
    if ((int)threadIdx.x < nbv) reinterpret_cast<f32x4*>(bias_s)[threadIdx.x] = bv;
  };

  // ---- phase 1: fused (+swish) halo of the depthwise input, zero outside the image ----
  // (thread -> (position, channel group): an exact split by CG through a float reciprocal - with the power-of-two split a 160-channel
  //  node used 20 of every 32 lanes: four sweeps over its 100 halo positions instead of two)
  //  (single nodes only: in the multi-segment and chain instantiations the extra live values spilled)
  //  (measured and left out: two halo items in flight per lane for the two-source top-down nodes - one global round trip instead of
  //   two at widths above 64 - changed no launch by more than 0.5 us: sixteen waves per CU already overlap the sweeps)
  //  (shape rows: CG is 8 - the exact split IS the shift and the mask)
  constexpr bool EXACT = MODE == 0 && !D;
  const float cg_rinv = __builtin_amdgcn_rcpf((float)CG);
  const int t_pos = EXACT ? udiv_f((int)threadIdx.x, CG, cg_rinv) : (int)(threadIdx.x >> cgsh);
  const int t_cg = EXACT ? (int)threadIdx.x - t_pos * CG : (int)(threadIdx.x & ((1 << cgsh) - 1));
  const int t_stride = EXACT ? udiv_f(SEP_THREADS, CG, cg_rinv) : (SEP_THREADS >> cgsh);
  {
    const int cg = t_pos < t_stride ? t_cg : CG;                      // (the last SEP_THREADS % CG threads idle)
    if (cg < CG)
      for (int pos = t_pos; pos < HS * HS; pos += t_stride) {
        const int hy = TS == 16 ? pos / 18 : (TS == 8 ? pos / 10 : pos / 6), hx = pos - hy * HS;
        const int y = y0 + hy - 1, x = x0 + hx - 1;
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (y >= 0 && y < h && x >= 0 && x < w) gather_fuse<BF16, D>(sg, b, y, x, cg * 8, v);
        V::store(halo, (int64_t)pos * CH + cg * 8, v);
      }
  }
  SSTAMP(1);                            // gather done (halo stored)
  park();
  __syncthreads();
  SSTAMP_NOWAIT(2);
  // staged pointwise weights (a.off_wpw): requested here, under the depthwise phase, parked before the MFMA phase
  T* wpw_s = reinterpret_cast<T*>(smem + a.off_wpw);
  constexpr int NWST = WL ? 4 : 1;
  static_assert(!WL || SEP_THREADS == 1024, "sep_lds_layout admits up to 4 x 1024 staged weight vectors");
  raw_t wst[NWST];
  const int wvecs = tilesN * 16 * CG;                                             // 16-byte vectors of [16 * tilesN rows][C] (rows >= C are the pack's zero padding)
  if constexpr (WL) {
#pragma unroll
    for (int j = 0; j < NWST; j++) wst[j] = reinterpret_cast<const raw_t*>(W)[min((int)threadIdx.x + j * SEP_THREADS, wvecs - 1)];
  }

  // ---- phase 2: depthwise 3x3 -> operand tile [TS*TS pixels][C] ----
  {
    const int cg = t_pos < t_stride ? t_cg : CG;
    if (cg < CG)
      for (int p = t_pos; p < TS * TS; p += t_stride) {
        const int py = p >> tssh, px = p & (TS - 1);
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int ky = 0; ky < 3; ky++)
#pragma unroll
          for (int kx = 0; kx < 3; kx++) {
            float hv[8];
            V::load(halo, (int64_t)((py + ky) * HS + px + kx) * CH + cg * 8, hv);
            const f32x4* wp = reinterpret_cast<const f32x4*>(wdw_s + (ky * 3 + kx) * C + cg * 8);
            const f32x4 w0 = wp[0], w1 = wp[1];
#pragma unroll
            for (int c = 0; c < 4; c++) { acc[c] = fmaf(hv[c], w0[c], acc[c]); acc[4 + c] = fmaf(hv[4 + c], w1[c], acc[4 + c]); }
          }
        V::store(atile, (int64_t)p * CH + cg * 8, acc);
      }
  }
  SSTAMP(3);                            // depthwise done
  if constexpr (WL) {
    const float cg_inv = __builtin_amdgcn_rcpf((float)CG);
#pragma unroll
    for (int j = 0; j < NWST; j++) {
      const int i = threadIdx.x + j * SEP_THREADS, row = (int)(((float)i + 0.5f) * cg_inv), v = i - row * CG;    // i < 4096, CG <= 20
      if (i < wvecs) *reinterpret_cast<raw_t*>(wpw_s + row * CH + v * 8) = wst[j];
    }
  }
  __syncthreads();      // halo is dead from here on: its LDS becomes the output tile
  SSTAMP_NOWAIT(4);                     // staged weights parked, barrier passed

  // ---- phase 3: pointwise conv, D[n, pixel] = W[n,:] . tile[pixel,:] -> LDS output tile ----
  const int Nc = D ? SEP_SHAPE_C : sg.N;                  // columns of this segment
  const int act = D ? (int)ACT_NONE : sg.act, out_f32 = D ? 0 : sg.out_f32;
  float* otile_f = reinterpret_cast<float*>(smem);        // [TS*TS][Nc] fp32 (head outputs)
  T* otile_t = reinterpret_cast<T*>(smem);                // [TS*TS][Nc] dtype (maps)
  // (m-tile, n-tile) pairs are dealt round-robin to the waves; pair -> (nt, mt) is a shift and a mask
  for (int pair = wave; pair < (tilesN << mtsh); pair += SEP_WAVES) {
    const int nt = pair >> mtsh, mt = pair & ((1 << mtsh) - 1);
    if (mt >= mtv) continue;
    const int m = mt * 16 + r;
    const T* arow = atile + (int64_t)m * CH + KLANE * g;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    // The weight fragments of a pair come straight from global memory (L2): up to WGRP k-steps are requested together,
    // unconditionally on clamped addresses (k >= C meets a zero activation fragment).  Two at a time - the prefetch
    // depth of the prologue - made a 160-wide layer (5 k-steps) three dependent round trips per pair: at phi 3 @ 512 the
    // nodes on the 64x64 level spent about half of their 13 us per workgroup there.
    // (narrow layers - 2 k-steps at width 64 - keep groups of two: clamped extra loads are not free)
    auto kloop = [&](auto grp) {
      constexpr int WGRP = decltype(grp)::value;
      for (int ks0 = 0; ks0 < ksteps; ks0 += WGRP) {        // (a trailing partial group multiplies zeros)
        raw_t wfr[WGRP];
#pragma unroll
        for (int q = 0; q < WGRP; q++) {
          if constexpr (WL) wfr[q] = *reinterpret_cast<const raw_t*>(wpw_s + (nt * 16 + r) * CH + min((ks0 + q) * KSTEP + KLANE * g, C - KLANE));
          else if (!WL && q < WPRE && pair == wave && ks0 == 0) wfr[q] = wpre[q];       // (uniform) requested at kernel start
          else wfr[q] = *reinterpret_cast<const raw_t*>(W + (int64_t)(nt * 16 + r) * C + min((ks0 + q) * KSTEP + KLANE * g, C - KLANE));
        }
#pragma unroll
        for (int q = 0; q < WGRP; q++) {
          const int ks = ks0 + q;
          if (ks < ksteps) {                                  // (uniform)
            raw_t xa = {};
            if (ks * KSTEP + KLANE * g < C) xa = *reinterpret_cast<const raw_t*>(arow + ks * KSTEP);
            acc = F::mma(wfr[q], xa, acc);
          }
        }
      }
    };
    if constexpr (BF16) {
      if (WL || ksteps > 2) kloop(std::integral_constant<int, 6>()); else kloop(std::integral_constant<int, 2>());
    } else {
      // fp32 sessions: two k-steps at a time as before (wider groups spill in this kernel's fp32 instantiations)
      const T* wrow = W + (int64_t)(nt * 16 + r) * C + KLANE * g;
      for (int ks0 = 0; ks0 < ksteps; ks0 += WPRE) {        // (a trailing partial group multiplies zeros)
#pragma unroll
        for (int q = 0; q < WPRE; q++) {
          const int ks = ks0 + q;
          raw_t wf = {}, xa = {};
          if (ks * KSTEP + KLANE * g < C) {
            xa = *reinterpret_cast<const raw_t*>(arow + ks * KSTEP);
            if (pair == wave && ks0 == 0) wf = wpre[q];       // (uniform) requested at kernel start
            else wf = *reinterpret_cast<const raw_t*>(wrow + ks * KSTEP);
          }
          acc = F::mma(wf, xa, acc);
        }
      }
    }
    const int n = nt * 16 + 4 * g;          // lane: 4 consecutive columns of pixel m
    if (n < Nc) {
      const f32x4 bias = *reinterpret_cast<const f32x4*>(bias_s + n);
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; q++) v[q] = acc[q] + bias[q];
      if (act == ACT_SWISH) swish_n<BF16, 4>(v);                    // (uniform branches: BiFPN nodes have no activation behind the conv - the
      else if (act == ACT_SIGMOID) sigmoid_n<BF16, 4>(v);           //  branch-free select computed both transcendental forms for nothing)
      if (out_f32) {
#pragma unroll
        for (int q = 0; q < 4; q++) if (n + q < Nc) otile_f[(int64_t)m * Nc + n + q] = v[q];
      } else {
        V::store4(otile_t, (int64_t)m * Nc + n, v);     // Nc is a multiple of 8 for every map-producing layer
      }
    }
  }
  SSTAMP(5);                            // MFMA pairs done
  __syncthreads();
  SSTAMP_NOWAIT(6);

  // ---- phase 4: coalesced copy-out ----
  if (out_f32) {
    // head result [B, N_anchors, K]: pixel p owns 9*K consecutive floats; this segment's Nc columns
    float* o = reinterpret_cast<float*>(sg.out) + (int64_t)b * sg.out_bstride + sg.out_off;
    const int npx = rows_valid * cols_valid;
    for (int pp = wave; pp < npx; pp += SEP_WAVES) {
      const int py = pp / cols_valid, px = pp % cols_valid;
      const int m = py * TS + px;
      float* orow = o + ((int64_t)(y0 + py) * w + x0 + px) * sg.out_rowstride;
      for (int c = lane; c < Nc; c += 64) {
        const int nn = c + sg.n_base;
        orow[(nn / sg.col_kin) * sg.col_kout + nn % sg.col_kin + sg.col_off] = otile_f[(int64_t)m * Nc + c];
      }
    }
  } else {
    // NHWC map (possibly a column chunk [out_off, out_off+Nc) of a wider map): consecutive lanes
    // write consecutive 16-byte vectors of a pixel, then the next pixel of the tile row
    const int64_t out_bstride = D ? (int64_t)SH.h * SH.w * SEP_SHAPE_C : sg.out_bstride, out_off = D ? 0 : sg.out_off, out_rowstride = D ? SEP_SHAPE_C : sg.out_rowstride;
    T* o = reinterpret_cast<T*>(sg.out) + (int64_t)b * out_bstride + out_off;
    const int vpp = Nc >> 3;
    const int vsh = vpp <= 1 ? 0 : 32 - __builtin_clz(vpp - 1);
    const int cv = threadIdx.x & ((1 << vsh) - 1);
    if (cv < vpp)
      for (int pix = threadIdx.x >> vsh; pix < TS * TS; pix += SEP_THREADS >> vsh) {
        const int py = pix >> tssh, px = pix & (TS - 1);
        if (py >= rows_valid || px >= cols_valid) continue;
        const unsigned char* src = reinterpret_cast<const unsigned char*>(otile_t) + ((int64_t)pix * Nc + cv * 8) * sizeof(T);
        T* dst = o + ((int64_t)(y0 + py) * w + x0 + px) * out_rowstride + cv * 8;
        *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        if constexpr (!BF16) *reinterpret_cast<u32x4*>(dst + 4) = *reinterpret_cast<const u32x4*>(src + 16);
      }
  }
  // chain mode: this node's stores must have landed (and every LDS reader be done) before the next
  // node of the chain gathers them - same workgroup, same CU, so a barrier after vmcnt(0) suffices
  if (MODE == 2) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); }
#ifdef HEP_TOWER_TRACE
  if (MODE == 0) {
    SSTAMP(7);                          // stores acknowledged
    if (g_sep_trace && (threadIdx.x & 63) == 0 && h == g_sep_trace_hw) {
      unsigned long long* o = g_sep_trace + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * SEP_WAVES + (threadIdx.x >> 6)) * 8;
      for (int i = 0; i < 8; i++) o[i] = sstamps[i];
    }
  }
#endif
  }   // chain loop
