// k_chain_body.h - the body of the chain kernels, included by k_chain_impl.h into chain_kernel (D = 0) and chain_shape_kernel (D > 0); it
// expects BF16, WMODE, D and the kernel argument `a` in scope.  Text and not a function: with the body behind a force-inlined function
// that takes the arguments by reference the generic kernels grew by 6-8 % (static count, bf16 resident form 5632 -> 6067 instructions).
  static_assert(!D || (BF16 && WMODE == 0), "shape rows: bf16 chains with resident weights");
  constexpr bool STREAM = WMODE == 1, WGLOBAL = WMODE == 2;
  constexpr ChainShape SH = chain_shape(D);
  const int a_next = D ? SH.next : a.next, a_nnodes = D ? SH.nnodes : a.nnodes, a_nconv = D ? SH.nconv : a.nconv;
  const int a_wnode_bytes = D ? CHAIN_SHAPE_WNODE_BYTES : a.wnode_bytes;
  const uint32_t a_nt_rcp = D ? rcp_u32(CHAIN_SHAPE_C / 16) : a.nt_rcp;
  typedef Vec8<BF16> V;
  typedef typename V::elem T;
  typedef Raw8<BF16> R8;
  typedef Frag<BF16> F;
  typedef typename F::raw frag_t;
  constexpr int PAD = BF16 ? 8 : 4, KSTEP = F::KSTEP, KLANE = F::KLANE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  HEP_POISON(smem, D ? SH.lds_bytes : a.lds_bytes);
  T* slots = reinterpret_cast<T*>(smem);
  unsigned char* wreg = smem + (D ? SH.off_w : a.off_w);
  T* halo = reinterpret_cast<T*>(smem + (D ? SH.off_halo : a.off_halo));
  T* atile = reinterpret_cast<T*>(smem + (D ? SH.off_atile : a.off_atile));
  const int C = D ? CHAIN_SHAPE_C : a.C, CG = C >> 3, CH = C + PAD;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 15, g = lane >> 4;
  int cgsh = 0; while ((1 << cgsh) < CG) cgsh++;
  const int cg = tid & ((1 << cgsh) - 1), prow = tid >> cgsh, pstride = CHAIN_THREADS >> cgsh;
#ifdef HEP_MBF_TRACE
  unsigned long long st_buf[60]; int nst = 0;
  const unsigned long long clk0 = __builtin_amdgcn_s_memtime();
#endif
  CSTAMP();
  kernarg_warm<(int)sizeof(ChainArgs)>();      // (hep_dev.h: the prologue below fetched its eight argument lines one miss after the other)

  // ---- 1. one burst: node descriptors, all weights and all external maps -> LDS.  Every load is issued before the
  //         first LDS store that waits for it, so the whole prologue is about one memory round trip. ----
  {
    // the chain's weights: one contiguous blob already in the LDS layout (per node [9*C] f32 depthwise | [C] f32 bias |
    // [C][C+PAD] bf16 pointwise rows)
    constexpr int WB = 4096 / CHAIN_THREADS;
    // (WGLOBAL: the first 10 * C floats of every node - depthwise weights and bias - packed node after node)
    const int svecs = (10 * C * 4) >> 4;
    const int wvecs = WGLOBAL ? a_nconv * svecs : (int)(((size_t)(STREAM ? 1 : a_nconv) * a_wnode_bytes) >> 4);
    auto wsrc_of = [&](int i) -> const u32x4* {
      if constexpr (WGLOBAL) { const int nd_ = i / svecs, o = i - nd_ * svecs; return reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(a.wblob) + (size_t)nd_ * a_wnode_bytes) + o; }
      else return reinterpret_cast<const u32x4*>(a.wblob) + i;
    };
    u32x4 wv[WB];
#pragma unroll
    for (int j = 0; j < WB; j++) { const int i = tid + j * CHAIN_THREADS; if (i < wvecs) wv[j] = *wsrc_of(i); }
    // external maps that are copied as they are (their own resolution)
    constexpr int EPF = BF16 ? CH_MAX_EXT : 4;          // maps whose first row of vectors is prefetched (fp32: 8 registers each)
    R8 ev[EPF];
    // (a row's external maps: sizes, kind, pool pad and slot are the row's constants; only the pointers come from the arguments)
#define CHAIN_EXT(e) \
      const ChainExt& x = a.ext[e]; \
      const int x_sh = D ? SH.ext[e].sh : x.sh, x_sw = D ? SH.ext[e].sw : x.sw, x_kind = D ? SH.ext[e].kind : x.kind, x_h = D ? SH.ext[e].h : x.h, x_w = D ? SH.ext[e].w : x.w; \
      [[maybe_unused]] const int x_pad = D ? SH.ext[e].pool_pad : x.pool_pad, x_off = D ? SH.ext[e].off : x.off
#pragma unroll
    for (int e = 0; e < EPF; e++) {
      CHAIN_EXT(e);
      ev[e].zero();
      if (e < a_next && x_kind != SRC_DOWN && cg < CG && prow < x_h * x_w)
        ev[e] = R8::load(reinterpret_cast<const T*>(x.src) + ((int64_t)b * x_sh * x_sw + prow) * C + cg * 8);
    }
    // The node descriptors are read by scalar loads at the head of every node (below): a scalar-cache miss there is ~0.4 us in
    // front of every node, for all sixteen waves (per-wave stamps: waves without an item spend 0.5 us per node).  Every descriptor
    // line is touched HERE - every load of the prologue has been issued, the first LDS store below waits for them anyway - so that
    // the later loads hit the scalar cache.
    {
      typedef const __attribute__((address_space(4))) uint32_t* cptr;
      const int nbytes = a_nnodes * (int)sizeof(ChainNode);
      cptr np = (cptr)a.nodes;
#pragma unroll
      for (int o = 0; o < CH_MAX_NODES * (int)sizeof(ChainNode); o += 256) {
        if (o < nbytes) {                                       // (uniform)
          cptr q = np + o / 4;
          uint32_t t0, t1, t2, t3;
          asm volatile("s_load_dword %0, %4, 0x0\n\ts_load_dword %1, %4, 0x40\n\ts_load_dword %2, %4, 0x80\n\ts_load_dword %3, %4, 0xc0\n\ts_waitcnt lgkmcnt(0)"
                       : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3) : "s"(q) : "memory");
        }
      }
    }
#pragma unroll
    for (int j = 0; j < WB; j++) { const int i = tid + j * CHAIN_THREADS; if (i < wvecs) reinterpret_cast<u32x4*>(wreg)[i] = wv[j]; }
    for (int i = tid + WB * CHAIN_THREADS; i < wvecs; i += CHAIN_THREADS) reinterpret_cast<u32x4*>(wreg)[i] = *wsrc_of(i);   // (more nodes / wider maps)
#pragma unroll
    for (int e = 0; e < CH_MAX_EXT; e++) {
      CHAIN_EXT(e);
      if (e >= a_next || cg >= CG) continue;
      T* dst = slots + x_off;
      const T* src = reinterpret_cast<const T*>(x.src) + (int64_t)b * x_sh * x_sw * C;
      if (x_kind != SRC_DOWN) {
        if (e < EPF && prow < x_h * x_w) ev[e < EPF ? e : 0].store(dst + (int64_t)prow * C + cg * 8);
        for (int p = prow + (e < EPF ? pstride : 0); p < x_h * x_w; p += pstride) R8::load(src + (int64_t)p * C + cg * 8).store(dst + (int64_t)p * C + cg * 8);
      } else {       // pooled while it is loaded (zero-padded 3x3 / 2 max-pool); optionally also a map of its own (p6_in)
        for (int p = prow; p < x_h * x_w; p += pstride) {
          float m[8];
          slot_pool<BF16>(src, x_sh, x_sw, C, x_pad, p / x_w, p % x_w, cg * 8, m);
          V::store(dst, (int64_t)p * C + cg * 8, m);                                    // exact: the values are session-dtype numbers already
          if (D ? SH.ext[e].store != 0 : x.store != nullptr) V::store(x.store, ((int64_t)b * x_h * x_w + p) * C + cg * 8, m);
        }
      }
    }
#undef CHAIN_EXT
  }
  __syncthreads();
  CSTAMP();

  // ---- 2. the nodes, out of LDS (descriptors included); pixel
  //         indices are split with a reciprocal multiply (a run-time integer division is ~30 instructions on the one
  //         item a lane has per phase). ----
#pragma unroll 1      // a real loop: the body runs once per node, unrolled it would be fetched cold every time (measured +20 %)
  for (int n = 0; n < a_nnodes; n++) {
    // the descriptor is copied to registers once and made wave-uniform (scalar registers): read field by field from LDS
    // inside the phases it cost a load + wait per use (the gather phase took 2 us of a 3 us node)
    // (the descriptor arrives as a few wide scalar loads from constant memory; copied from LDS and made uniform dword by
    //  dword it was a chain of ~25 LDS round trips at the head of every node, paid by all 16 waves: per-wave stamps showed
    //  0.5-1.0 us per node in waves that had no item at all)
    ChainNode nd;
    {
      typedef const __attribute__((address_space(4))) uint32_t* cptr;
      cptr sp = (cptr)(a.nodes + n);
      uint32_t* dp = reinterpret_cast<uint32_t*>(&nd);
#pragma unroll
      for (int i = 0; i < (int)(sizeof(ChainNode) / 4); i++) dp[i] = sp[i];
    }
    const int h = nd.h, w = nd.w, hw = h * w;
    const uint32_t w_rcp = nd.w_rcp, hs_rcp = nd.hs_rcp;     // (host-made reciprocals: the 64-bit divisions were part of a ~0.6 us fixed cost per node)
    T* oslot = slots + nd.out_off;
    if (nd.pool_only) {          // p7_in = pool(p6_in): a map of its own, no convolution
      const ChainSrc& s0 = nd.src[0];
      if (cg < CG)
        for (int p = prow; p < hw; p += pstride) {
          float m[8];
          const int py = (int)__umulhi((uint32_t)p, w_rcp);
          slot_pool<BF16>(slots + s0.off, s0.sh, s0.sw, C, nd.pool_pad, py, p - py * w, cg * 8, m);
          V::store(oslot, (int64_t)p * C + cg * 8, m);
          V::store(nd.out, ((int64_t)b * hw + p) * C + cg * 8, m);
        }
      __syncthreads();
      continue;
    }
    const float* wdw_s = reinterpret_cast<const float*>(wreg + (WGLOBAL ? (size_t)nd.widx * (10 * C * 4) : (size_t)(STREAM ? (nd.widx & 1) : nd.widx) * a_wnode_bytes));
    const float* bias_s = wdw_s + 9 * C;
    const T* wpw_s = reinterpret_cast<const T*>(bias_s + C);                       // (resident / streamed forms)
    const T* wpw_g = reinterpret_cast<const T*>(reinterpret_cast<const unsigned char*>(a.wblob) + (size_t)nd.widx * a_wnode_bytes + (size_t)10 * C * 4);
    // streamed weights: the NEXT node's go straight from global memory into the other LDS buffer (LDS-DMA, no registers: held in
    // registers under the node they spilled); that buffer was last read by the previous node, which every wave has left
    // (its closing barrier).  1 KB per wave instruction; the host pads a node's weights to whole KB.
    if constexpr (STREAM) {
      if (nd.widx + 1 < a.nconv) {
        const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(a.wblob) + (size_t)(nd.widx + 1) * a.wnode_bytes;
        unsigned char* wdst = wreg + (size_t)((nd.widx + 1) & 1) * a.wnode_bytes;
        for (int c = wave; c * 1024 < a.wnode_bytes; c += CHAIN_WAVES)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + c * 1024 + lane * 16),
                                           (__attribute__((address_space(3))) void*)(wdst + c * 1024), 16, 0, 0);
      }
    }
    const int HS = w + 2;
    // fused + swished input with its one-pixel zero halo
    if (cg < CG)
      for (int pos = prow; pos < (h + 2) * HS; pos += pstride) {
        const int hy = (int)__umulhi((uint32_t)pos, hs_rcp);
        const int y = hy - 1, x = pos - hy * HS - 1;
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (y >= 0 && y < h && x >= 0 && x < w) {
#pragma unroll
          for (int i = 0; i < HEP_MAX_SRC; i++) {
            if (i >= nd.nsrc) break;
            const ChainSrc& s = nd.src[i];
            float t[8];
            if (s.kind == SRC_DOWN) slot_pool<BF16>(slots + s.off, s.sh, s.sw, C, nd.pool_pad, y, x, cg * 8, t);
            else if (s.kind == SRC_UP) slot_load<BF16>(slots + s.off, s.sh, s.sw, C, y >> 1, x >> 1, cg * 8, t);
            else slot_load<BF16>(slots + s.off, s.sh, s.sw, C, y, x, cg * 8, t);
#pragma unroll
            for (int c = 0; c < 8; c++) v[c] = fmaf(s.fw, t[c], v[c]);
          }
          swish_n<BF16, 8>(v);
        }
        V::store(halo, (int64_t)pos * CH + cg * 8, v);
      }
    CSTAMP();
    if constexpr (STREAM) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's share of the node's weights (requested one node ago) has landed
    __syncthreads();
    CSTAMP();
    // depthwise 3x3 -> MFMA operand tile [pixels][C]; rows beyond the map are zeroed (their products are discarded)
    if (cg < CG)
      for (int p = prow; p < ((hw + 15) & ~15); p += pstride) {
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (p < hw) {
          const int py = (int)__umulhi((uint32_t)p, w_rcp), px = p - py * w;
#pragma unroll
          for (int q = 0; q < 9; q++) {
            float hv[8];
            V::load(halo, (int64_t)((py + q / 3) * HS + px + q % 3) * CH + cg * 8, hv);
            const f32x4* wp = reinterpret_cast<const f32x4*>(wdw_s + q * C + cg * 8);
            const f32x4 w0 = wp[0], w1 = wp[1];
#pragma unroll
            for (int c = 0; c < 4; c++) { acc[c] = fmaf(hv[c], w0[c], acc[c]); acc[4 + c] = fmaf(hv[4 + c], w1[c], acc[4 + c]); }
          }
        }
        V::store(atile, (int64_t)p * CH + cg * 8, acc);
      }
    CSTAMP();
    __syncthreads();
    CSTAMP();
    // pointwise: D[n, pixel] = W[n, :] . tile[pixel, :]; (m-tile, n-tile) pairs dealt to the waves; lane ends with 4
    // consecutive channels of one pixel -> its slot in LDS
    const int mt_n = (hw + 15) >> 4, nt_n = (C + 15) >> 4, ksteps = (C + KSTEP - 1) / KSTEP;      // (widths like 88: the last n-tile is half used)
    for (int pair = wave; pair < mt_n * nt_n; pair += CHAIN_WAVES) {
      const int mt = udiv_rcp(pair, a_nt_rcp), nt = pair - mt * nt_n;      // (host-made reciprocal: a 64-bit division sat here)
      const int m = mt * 16 + r;
      // (WGLOBAL: at widths that are no multiple of 16 the last n-tile's rows past C would lie behind the node's [C][C + pad] weights
      //  in the blob - for the last node behind the blob itself; their products are never stored: clamp the row)
      const T* wrow = (WGLOBAL ? wpw_g : wpw_s) + (int64_t)(WGLOBAL ? min(nt * 16 + r, C - 1) : nt * 16 + r) * CH + KLANE * g;
      const T* arow = atile + (int64_t)m * CH + KLANE * g;
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (WGLOBAL) {
        // every k-step's weight fragment of the pair is requested before the first MFMA (one L2 round trip per pair, not per
        // k-step); unconditional loads on clamped offsets, k >= C meets a zeroed activation fragment
        constexpr int KSG = 6;                                                   // C <= 192 (bf16) / 96 (fp32): host-checked
        frag_t wfr[KSG];
#pragma unroll
        for (int ks = 0; ks < KSG; ks++) wfr[ks] = *reinterpret_cast<const frag_t*>(wrow + min(ks * KSTEP, C - KLANE - KLANE * g));
#pragma unroll
        for (int ks = 0; ks < KSG; ks++) {
          if (ks < ksteps) {
            frag_t xa = {};
            if (ks * KSTEP + KLANE * g < C) xa = *reinterpret_cast<const frag_t*>(arow + ks * KSTEP);
            acc = F::mma(wfr[ks], xa, acc);
          }
        }
      } else
      for (int ks = 0; ks < ksteps; ks++) {
        frag_t wf = {}, xa = {};
        if (ks * KSTEP + KLANE * g < C) { wf = *reinterpret_cast<const frag_t*>(wrow + ks * KSTEP); xa = *reinterpret_cast<const frag_t*>(arow + ks * KSTEP); }
        acc = F::mma(wf, xa, acc);
      }
      const int nn = nt * 16 + 4 * g;
      if (m < hw && nn < C) {
        const f32x4 bias = *reinterpret_cast<const f32x4*>(bias_s + nn);
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = acc[q] + bias[q];
        V::store4(oslot, (int64_t)m * C + nn, v);
      }
    }
    CSTAMP();
    __syncthreads();
    CSTAMP();
    // the finished map leaves as full 16-byte vectors; nobody in this launch reads it from global memory
    if (cg < CG)
      for (int p = prow; p < hw; p += pstride) R8::load(oslot + (int64_t)p * C + cg * 8).store(reinterpret_cast<T*>(nd.out) + ((int64_t)b * hw + p) * C + cg * 8);
    CSTAMP();
  }
#ifdef HEP_MBF_TRACE
  if (g_chain_trace && lane == 0) { unsigned long long* o = g_chain_trace + ((size_t)b * CHAIN_WAVES + wave) * 64; for (int i = 0; i < 60; i++) o[i] = i < nst ? st_buf[i] : 0; o[63] = (unsigned long long)nst; o[62] = __builtin_amdgcn_s_memtime() - clk0; }
#endif
