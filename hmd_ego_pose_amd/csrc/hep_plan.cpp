// hep_plan.cpp - the launch plan of a session: one Op per kernel launch, the tensor table, the host copy of the weight blob,
// the pointer references, and a liveness-based activation arena.  Host arithmetic only: no device is touched here
// (hep_session.cpp realises the plan).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>

#include "hep.h"
#include "hep_plan.h"

namespace hep {

static const float kFusionEps = 1e-4f;  // efficientdet/model.py:60

// a fused front's partial squeeze-excite rows: written by the front, read back by its own tail (alt build: HEP_SE_TAIL)
static void mbf_hpart_slot(Op& o, int seg, int idx, void* p) { SLOT(mbf.hpart)(o, seg, idx, p); SLOT(mbf.tail.hpart)(o, seg, idx, p); }

// ---- plan builder ----
struct Planner {
  Session* s; const Pack& pk; std::string* err; WBuilder wb; bool ok = true;
  std::vector<Ref>& refs;
  int& ntails;                        // fused fronts that finish their squeeze-excite in their tail (one counter block each)
  const Knobs kn;                     // plan knobs as the environment had them when the session was created (hep_knobs.h)
  std::map<int, int> front_of_out, front_of_part;   // tensor -> the fused front (OP_MBF) that writes it as its output / its partial squeeze-excite rows
  Planner(Session* s_, const Pack& p, Plan* plan, std::string* e) : s(s_), pk(p), err(e), refs(plan->refs), ntails(plan->ntails), kn(s_->knobs) { wb.dtype = s_->dtype; wb.layout_only = plan->layout_only; }

  int tensor(const std::string& name, int H, int W, int C, bool f32 = false) {
    TensorDesc t; t.name = name; t.H = H; t.W = W; t.C = C; t.f32 = f32;
    t.bytes_per_image = (size_t)H * W * C * (f32 ? 4 : s->esize());
    s->tensors.push_back(t);
    s->tensor_by_name[name] = (int)s->tensors.size() - 1;
    return (int)s->tensors.size() - 1;
  }
  const PackTensor* get(const std::string& n, std::initializer_list<int64_t> d) {
    const PackTensor* t = pk.get(n, d, err);
    if (!t) ok = false;
    return t;
  }
  // references: a weight at byte woff of the blob, an arena tensor (recorded as read or written by the op), head output k
  void wref(int op, Slot set, size_t woff, int seg = -1, int idx = 0) { refs.push_back({op, set, seg, idx, TO_WEIGHT, woff}); }
  void tref(int op, Slot set, int tensor, bool write, int seg = -1, int idx = 0) {
    refs.push_back({op, set, seg, idx, TO_TENSOR, (size_t)tensor});
    Op& o = s->ops[op];
    (write ? o.writes : o.reads).push_back(tensor);
  }
  void href(int op, Slot set, int k, int seg) { refs.push_back({op, set, seg, 0, TO_HEAD_OUT, (size_t)k}); }
  int new_op(OpKind k, const std::string& name) {
    Op o{};                           // every argument struct all-zero
    o.kind = k; o.name = name;
    s->ops.push_back(o);
    return (int)s->ops.size() - 1;
  }
  double es() const { return (double)s->esize(); }

  // ---- pointwise conv (weights [N][K] as in the state_dict; optional conv bias; optional BN) ----
  // squeeze-excite of a project conv: the front kernel's partial reduce-FC rows + the rest of the two FCs
  struct SeSpec { int hpart_t = -1, rows = 0, sq = 0, sqp = 0; float inv_hw = 0.f; size_t br = 0, we = 0, be = 0; };
  int add_pw(const std::string& name, int in_t, int HW, int K, int N, const std::string& wkey, const std::string& bkey,
             const std::string& bnkey, int act, const SeSpec* se, int res_t, const std::string& out_name, int H, int W, bool quant = false, int out_pre = -1) {
    const PackTensor* w = get(wkey, {N, K, 1, 1});
    const PackTensor* cb = bkey.empty() ? nullptr : get(bkey, {N});
    BnFold bn;
    if (!bnkey.empty() && !fold_bn(pk, bnkey, N, &bn, err)) ok = false;
    if (!ok) return -1;
    const int tilesN = (N + 15) / 16;
    const bool quant_fp8 = quant && s->dtype == 2;
    const FoldedPw f = fold_pw(w, K, cb, bnkey.empty() ? nullptr : &bn, 0, N, tilesN * 16);
    const std::vector<float>&wf = f.w, &bf = f.b;
    // tile shape: as many n-tiles per wave as fit (<= 8) so the activation rows are streamed
    // as few times as possible; two m-tiles per wave when the layer has rows to spare
    int pmode, pMT, pNT;
    const int64_t Mmax = (int64_t)HW * s->lane_batch;      // rows one launch sees (one lane of the batch)
    {
      const int64_t strips = (Mmax + 15) / 16;             // 16-row strips
      const int ksteps = (K + (s->dtype ? 32 : 16) - 1) / (s->dtype ? 32 : 16);
      auto clampi = [](int64_t v, int lo, int hi) { return (int)std::max<int64_t>(lo, std::min<int64_t>(hi, v)); };
      if (Mmax >= 16384) {          // big maps: waves along M, >= 256 workgroups anyway
        const int chunks = (tilesN + 7) / 8;
        pmode = 0; pNT = (tilesN + chunks - 1) / chunks;
        pMT = (Mmax >= 65536 && pNT <= 4) ? 2 : 1;
      } else if (ksteps >= 8) {     // small maps, deep K (project): split K over the 4 waves
        // widest split-K tile (alt build: HEP_PW_NT2).  Measured at phi 0 b16 (two m-tiles per wave): 4 / 2 / 1 n-tiles ->
        // one batch 0.6312 / 0.6259 / 0.6360 ms, four in flight 48.2k / 48.3k / 47.0k frames/s: 2
        const int nt2_max = kn.pw_nt2;
        pmode = 2; pMT = 1; pNT = clampi(strips * tilesN / 256, 1, std::min(std::min(8, nt2_max), tilesN));
      } else {                      // small maps, wide N (expand / lateral): waves side by side in N
        pmode = 1; pMT = 1; pNT = clampi(strips * tilesN / (4 * 256), 1, std::min(8, (tilesN + 3) / 4));
      }
      // Two m-tiles per wave in modes 1/2 (every weight fragment feeds two MFMAs, half the weight re-reads
      // from L2): no effect on a single batch in flight, but -2.5 % on the step with 4 batches in flight and
      // at batch 64, where these layers are bound by L2 traffic and not by latency.  (alt build: HEP_PW_MT2=0 disables.)
      {
        if (pmode != 0 && strips >= 8 && kn.pw_mt2 != 0) { pMT = 2; pNT = std::min(pNT, 4); }
        if (pmode == 2) pNT = std::min(pNT, std::max(1, kn.pw_nt2));
        // One more n-tile per wave where that brings the launch from two rounds of workgroups to one (the last project conv of phi 0:
        // 1152 -> 320 on the 8x8 maps, 32 x 10 = 320 workgroups with two n-tiles, 32 x 7 = 224 with three).  Round 4 selected it for fp32
        // sessions (one batch -5 us); re-measured with round 6's kernels it costs throughput: fp32 four in flight 28.84k -> 29.01k frames/s
        // WITHOUT it (four interleaved runs, one batch 17.03k -> 17.06k): the three-tile form runs four waves where the two-tile one
        // runs eight.  Off since; alt build: HEP_PW_NT3=1 selects it.
        if (pmode == 2 && kn.pw_nt3 > 0) {
          const int64_t mblocks = (strips + pMT - 1) / pMT;
          auto wgs = [&](int nt) { return mblocks * ((tilesN + nt - 1) / nt); };
          if (wgs(pNT) > 256 && wgs(pNT) <= 512 && pNT < 8 && wgs(pNT + 1) <= 256) pNT++;
        }
      }
    }
    // (alt build A/B, HEP_PW_WIDE=cap: fewest column chunks - fewer, fatter workgroups, fewer copies of the squeeze-excite prologue.  Measured,
    //  round 6: cap 8 -> 52.4k against 53.3k frames/s, with every squeeze-excite finish in the prologue 51.9k (against 50.4k with the default tiles):
    //  a 6-7 n-tile workgroup takes 11-15 us where the 2 n-tile one takes 6)
    if (pmode == 2 && kn.pw_wide > 0 && se) {
      const int cap = std::min(8, kn.pw_wide), ch = (tilesN + cap - 1) / cap;
      pNT = (tilesN + ch - 1) / ch;
    }
    // Squeeze-excite: finished in this GEMM's prologue (no launch) while the K x sq expand-FC matrix re-read by every
    // workgroup stays below HEP_SE_MAXMB (default 4) MB per launch; beyond that a small launch finishes it once per
    // image (k_dw.hip).  Measured at phi 0, batch 16 (same box, 2 x 300 steps): threshold 1000 / 12 / 8 / 4 / 0 MB ->
    // 40.7k / 41.0k / 41.3k / 41.7k / 41.8k frames/s with four batches in flight and 20.9k / 20.9k / 20.9k / 20.9k /
    // 20.6k with one (55 / 59 / 61 / 65 / 71 launches): the redundant L2 traffic of the prologue costs throughput on the
    // late blocks, the extra launches cost latency on the early ones.  phi 3 @ 512: 3.20k / 3.31k (24 MB) / 3.39k (0).
    int scale_t = -1;
    // weight bytes and flops of the expand FC, whichever launch runs it
    const double se_wbytes = se ? (double)K * se->sq * es() + ((double)K + se->sq) * 4 : 0.0, se_flops = se ? 2.0 * K * se->sq : 0.0;
    if (se) {
      const int rows_wg = pmode == 0 ? 64 * pMT : 16 * pMT, per_n = pmode == 1 ? 4 * pNT : pNT;
      const double wgs = (double)((Mmax + rows_wg - 1) / rows_wg) * ((tilesN + per_n - 1) / per_n);
      const bool own_launch = wgs * K * se->sqp * es() > kn.se_maxmb * 1e6;
#ifdef HEP_ALT
      // ... or no launch at all (HEP_SE_TAIL=1, NOT the default): the fused front that produced the partial rows finishes it in its tail
      // (k_mbf.hip: last workgroup of an image to arrive).  Measured, round 5, phi 0 b16: 59 -> 49 launches, bit-identical, four in flight
      // 51.4k against 51.3k frames/s, one batch 0.600 -> 0.605 ms, fp32 one batch 0.980 -> 1.021 ms, phi 3 one batch +2.3 %: the tail
      // (stores acknowledged, ticket, rows and weight rows fetched past L2 by ONE workgroup) costs 6-9 us against the ~5 us of a launch
      // and its boundary - the price list's "5-13 us per seam inside a launch" again.
      const int tail_op = kn.se_tail != 0 && front_of_part.count(se->hpart_t) ? front_of_part[se->hpart_t] : -1;
      if (own_launch && tail_op >= 0 && ntails < 64) {
        scale_t = tensor(name + ".se_scale", 1, 1, K, true);
        MbfArgs& m = s->ops[tail_op].mbf;
        m.se_tail = 1 + ntails++;          // (1 + index of its counter block; the pointers are patched per lane)
        m.tail.C = K; m.tail.sq = se->sq; m.tail.sqp = se->sqp; m.tail.rows = se->rows; m.tail.bf16 = s->dtype; m.tail.inv_hw = se->inv_hw;
        tref(tail_op, SLOT(mbf.tail.scale), scale_t, true);
        wref(tail_op, SLOT(mbf.tail.br), se->br); wref(tail_op, SLOT(mbf.tail.we), se->we); wref(tail_op, SLOT(mbf.tail.be), se->be);
        s->ops[tail_op].name += "+se";      // (the launch list shows which fronts carry the finish)
        s->ops[tail_op].weight_bytes += se_wbytes; s->ops[tail_op].flops_per_image += se_flops;
      } else
#endif
      if (own_launch) {
        scale_t = tensor(name + ".se_scale", 1, 1, K, true);
        const int sop = new_op(OP_SE, name.substr(0, name.find('.')) + ".se");
        Op& so = s->ops[sop];
        so.se.C = K; so.se.sq = se->sq; so.se.sqp = se->sqp; so.se.rows = se->rows; so.se.bf16 = s->dtype; so.se.inv_hw = se->inv_hw;
        tref(sop, SLOT(se.hpart), se->hpart_t, false); tref(sop, SLOT(se.scale), scale_t, true);
        wref(sop, SLOT(se.br), se->br); wref(sop, SLOT(se.we), se->we); wref(sop, SLOT(se.be), se->be);
        so.act_bytes_per_image = ((double)se->rows * se->sqp + K) * 4; so.weight_bytes = se_wbytes; so.flops_per_image = se_flops;
      }
    }
    const int out_t = out_pre >= 0 ? out_pre : tensor(out_name, H, W, N);
    const int op = new_op(OP_PW, name);
    Op& o = s->ops[op];
    o.pw.K = K; o.pw.N = N; o.pw.tilesN = tilesN; o.pw.HW = HW; o.pw.act = act; o.pw.bf16 = s->dtype;
    o.pw.mode = pmode; o.pw.MT = pMT; o.pw.NT = pNT;
    // fp32 split-K GEMMs deep enough for eight K slices of two load batches each (alt build: HEP_PW_W8=0, four waves as before)
    o.pw.nwv = (s->dtype == 0 && pmode == 2 && pNT <= 2 && K >= kn.pw_w8_mink && kn.pw_w8 != 0) ? 8 : 4;
    tref(op, SLOT(pw.A), in_t, false); tref(op, SLOT(pw.out), out_t, true);     // (reads[0] is the GEMM's activation operand: fp8 calibration)
    if (quant && s->dtype == 2) {     // fp8 session: e4m3 weights, one scale per output channel behind the BN fold
      std::vector<float> sc;
      wref(op, SLOT(pw.W), wb.put_fp8(wf, tilesN * 16, K, K, &sc)); wref(op, SLOT(pw.wscale), wb.put_f32(sc));
      o.pw.fp8 = 1; o.pw.a_scale = 1.f;
    } else {
      // Fragment-ordered operands (k_pw_impl.h FRAG; HEP_PW_FRAG=0 disables): the split-K project convs whose scale comes from
      // se_finish_kernel and whose activations come from a fused front (k_mbf.hip), K a multiple of the k-step, whole m-tiles per image
      const int producer = front_of_out.count(in_t) ? front_of_out[in_t] : -1;
      const bool frag = s->dtype != 2 && !quant_fp8 && pmode == 2 && pMT == 2 && pNT <= PW_FRAG_MAX_NT && act != ACT_SWISH && se && HW % 16 == 0 && producer >= 0 &&
                        kn.pw_frag != 0;
      if (frag) {
        const int kstep = s->dtype ? 32 : 16, klane = s->dtype ? 8 : 4, kst = (K + kstep - 1) / kstep;
        std::vector<float> wfr((size_t)tilesN * kst * 64 * klane, 0.f);      // K padded to whole k-steps with zeros
        for (int nt = 0; nt < tilesN; nt++) for (int ks = 0; ks < kst; ks++) for (int lane = 0; lane < 64; lane++) for (int e = 0; e < klane; e++) {
          const int k = ks * kstep + klane * (lane >> 4) + e;
          if (k < K) wfr[(((size_t)nt * kst + ks) * 64 + lane) * klane + e] = wf[(size_t)(nt * 16 + (lane & 15)) * K + k];
        }
        wref(op, SLOT(pw.W), wb.put_typed(wfr));
        s->ops[op].pw.frag = 1; s->ops[producer].mbf.out_frag = 1; s->tensors[in_t].frag = true;
      } else wref(op, SLOT(pw.W), wb.put_typed(wf));
    }
    wref(op, SLOT(pw.bias), wb.put_f32(bf));
    if (res_t >= 0) tref(op, SLOT(pw.res), res_t, false);
    o.act_bytes_per_image = ((double)HW * K + (double)HW * N * (res_t >= 0 ? 2 : 1)) * es();
    o.weight_bytes = (double)N * K * (o.pw.fp8 ? 1.0 : es());
    o.flops_per_image = 2.0 * HW * K * N;
    if (se) {
      o.pw.sq = se->sq; o.pw.sqp = se->sqp;
      // images a workgroup's rows can belong to (its scale table in LDS holds that many): rows per workgroup
      // and HW are multiples of 16 and workgroups start at multiples of their row count
      const int rows_wg = o.pw.mode == 0 ? 64 * o.pw.MT : 16 * o.pw.MT;
      o.pw.se_nimg = HW % rows_wg == 0 ? 1 : (rows_wg + HW - 1) / HW + 1;
      if (scale_t >= 0) {      // finished by an earlier launch
        o.pw.se_from_tensor = 1;
        tref(op, SLOT(pw.se_scale), scale_t, false);
        o.act_bytes_per_image += (double)K * 4;
      } else {                 // finished in this GEMM's prologue
        tref(op, SLOT(pw.hpart), se->hpart_t, false);
        wref(op, SLOT(pw.se_br), se->br); wref(op, SLOT(pw.se_we), se->we); wref(op, SLOT(pw.se_be), se->be);
        o.pw.se_rows = se->rows; o.pw.inv_hw = se->inv_hw;
        o.act_bytes_per_image += ((double)se->rows * se->sqp + se->sq) * 4;
        o.weight_bytes += se_wbytes; o.flops_per_image += se_flops;
      }
    }
    return out_t;
  }

  // ---- several independent pointwise convs (conv bias + BN folded, no activation) as ONE launch ----
  struct PwSpec { std::string name, wkey, bkey, bnkey, out_name; int in_t, HW, K, H, W; };
  std::vector<int> add_pw_group(const std::string& name, const std::vector<PwSpec>& specs, int N) {
    std::vector<int> outs;
    const int op = new_op(OP_PWG, name);
    int strips = 0;
    double bytes = 0, wbytes = 0, flops = 0;
    for (size_t i = 0; i < specs.size(); i++) {
      const PwSpec& sp = specs[i];
      const PackTensor* w = get(sp.wkey, {N, sp.K, 1, 1});
      const PackTensor* cb = sp.bkey.empty() ? nullptr : get(sp.bkey, {N});
      BnFold bn;
      if (!sp.bnkey.empty() && !fold_bn(pk, sp.bnkey, N, &bn, err)) ok = false;
      if (!ok) return outs;
      const int tilesN = (N + 15) / 16;
      const FoldedPw f = fold_pw(w, sp.K, cb, sp.bnkey.empty() ? nullptr : &bn, 0, N, tilesN * 16);
      const int out_t = tensor(sp.out_name, sp.H, sp.W, N);
      outs.push_back(out_t);
      PwgSeg& g = s->ops[op].pwg.seg[i];
      g.HW = sp.HW; g.K = sp.K; g.N = N; g.tilesN = tilesN; g.blk_begin = strips;
      strips += (sp.HW + 15) / 16;
      wref(op, SLOT(pwg.seg[seg].W), wb.put_typed(f.w), (int)i); wref(op, SLOT(pwg.seg[seg].bias), wb.put_f32(f.b), (int)i);
      tref(op, SLOT(pwg.seg[seg].A), sp.in_t, false, (int)i); tref(op, SLOT(pwg.seg[seg].out), out_t, true, (int)i);
      bytes += ((double)sp.HW * sp.K + (double)sp.HW * N) * es(); wbytes += (double)N * sp.K * es(); flops += 2.0 * sp.HW * sp.K * N;
    }
    Op& o = s->ops[op];
    o.pwg.nseg = (int)specs.size(); o.pwg.bf16 = s->dtype; o.pwg.strips_per_image = strips;
    o.act_bytes_per_image = bytes; o.weight_bytes = wbytes; o.flops_per_image = flops;
    return outs;
  }

  // ---- MBConv block ----
  // The project conv of a block is DEFERRED until the next block is planned: on the big maps it is fused with that
  // block's expand + depthwise convs into one boundary launch (k_xbf.hip); otherwise flush_project() emits it as a GEMM.
  struct Deferred { bool active = false; int i = 0; MBConv b; int dw_t = -1, inp = -1, out_t = -1, Ho = 0, Wo = 0; SeSpec se; std::string p; } defer;
  void flush_project() {
    if (!defer.active) return;
    defer.active = false;
    char nm[64]; snprintf(nm, sizeof nm, "b%d.project", defer.i);
    add_pw(nm, defer.dw_t, defer.Ho * defer.Wo, defer.b.cexp, defer.b.cout, defer.p + "._project_conv.conv.weight", "", defer.p + "._bn2", ACT_NONE, &defer.se,
           defer.b.skip ? defer.inp : -1, std::string("block") + std::to_string(defer.i), defer.Ho, defer.Wo, true, defer.out_t);
  }
  // boundary launch: [SE + project of the deferred block] + [expand + depthwise + SE partial sums of block i] (k_xbf.hip)
  bool try_xbf(int i, const MBConv& b, int dw_t, const std::vector<float>& wdw, const std::vector<float>& bdw, size_t wr_off, int sqp2,
               int Hin, int Win, int Ho, int Wo, int pt, int pl, bool mid_needed, int* part_t, int* nblk) {
    const int minh = kn.xbf_minh;     // smallest input map that takes the boundary kernel (64; alt build: HEP_XBF_MINH, HEP_XBF=0)
    if (kn.xbf == 0) return false;
    const MBConv& pb = defer.b;
    if (s->dtype == 2 || !b.expand || Hin < minh || !xbf_supports(b.k, b.stride) || pb.cout > 16 * XBF_MAXNT1 || b.cexp % 16 != 0 || pb.cexp % 8 != 0 ||
        (defer.se.sqp != 8 && defer.se.sqp != 16) || pb.cexp > 512) return false;
    XbfArgs xa; memset(&xa, 0, sizeof xa);
    xa.H = Hin; xa.W = Win; xa.K1 = pb.cexp; xa.N1 = pb.cout; xa.NT1 = (pb.cout + 15) / 16; xa.Cexp = b.cexp; xa.NT2 = b.cexp / 16;
    xa.Ho = Ho; xa.Wo = Wo; xa.k = b.k; xa.s = b.stride; xa.pad_t = pt; xa.pad_l = pl; xa.bf16 = s->dtype;
    xa.se_rows = defer.se.rows; xa.sq = defer.se.sq; xa.sqp = defer.se.sqp; xa.inv_hw = defer.se.inv_hw; xa.sq2 = b.se; xa.sqp2 = sqp2;
    xa.generic = kn.xbf_generic == 2 ? 2 : (kn.xbf_generic != 0);
    xa.has_res = pb.skip ? 1 : 0;
    if (xbf_layout(&xa) == 0) return false;
    xa.tiles_x = (Wo + xa.tow - 1) / xa.tow; xa.tiles = xa.tiles_x * ((Ho + xa.toh - 1) / xa.toh);
    // weights: project of the deferred block (BN2 folded), expand of this block (BN0 folded), depthwise (BN1 folded, by the caller)
    char pb_[96]; snprintf(pb_, sizeof pb_, "backbone_net.model._blocks.%d", i);
    const std::string p = pb_;
    const PackTensor* w1 = get(defer.p + "._project_conv.conv.weight", {pb.cout, pb.cexp, 1, 1});
    const PackTensor* w2 = get(p + "._expand_conv.conv.weight", {b.cexp, b.cin, 1, 1});
    BnFold bn2, bn0;
    if (!fold_bn(pk, defer.p + "._bn2", pb.cout, &bn2, err) || !fold_bn(pk, p + "._bn0", b.cexp, &bn0, err)) ok = false;
    if (!ok) return true;
    const size_t pad = s->dtype ? 8 : 4;
    std::vector<unsigned char> blob((size_t)xa.blob_bytes, 0);
    // rows of a folded [N][K] matrix in the session dtype, row pitch `pitch` elements, from byte_off on
    auto put_rows = [&](size_t byte_off, const FoldedPw& fw, int N, int K, size_t pitch) {
      for (int n = 0; n < N; n++)
        for (int k = 0; k < K; k++) {
          const float v = fw.w[(size_t)n * K + k];
          const size_t idx = (size_t)n * pitch + k;
          if (s->dtype) { const uint16_t h = f32_to_bf16(v); memcpy(blob.data() + byte_off + idx * 2, &h, 2); }
          else memcpy(blob.data() + byte_off + idx * 4, &v, 4);
        }
    };
    const FoldedPw f1 = fold_pw(w1, pb.cexp, nullptr, &bn2, 0, pb.cout, pb.cout), f2 = fold_pw(w2, b.cin, nullptr, &bn0, 0, b.cexp, b.cexp);
    const size_t W1P = xa.K1 + pad, K2P = (size_t)xa.NT1 * 16, W2P = K2P + pad;
    put_rows(0, f1, pb.cout, pb.cexp, W1P);
    put_rows((size_t)(xa.off_w2 - xa.off_w1), f2, b.cexp, b.cin, W2P);
    float* f = reinterpret_cast<float*>(blob.data() + (xa.off_f - xa.off_w1));
    memcpy(f, wdw.data(), wdw.size() * 4); f += wdw.size();                  // [k*k][Cexp]
    memcpy(f, bdw.data(), (size_t)b.cexp * 4); f += b.cexp;                   // depthwise bias
    memcpy(f, f2.b.data(), (size_t)b.cexp * 4); f += (size_t)xa.NT2 * 16;     // expand bias
    memcpy(f, f1.b.data(), (size_t)pb.cout * 4);                              // project bias (padded with zeros)
    const size_t boff = wb.put_bytes(blob);
    char nm[64];
    snprintf(nm, sizeof nm, "b%d.se_hpart", i);
    // tiles per workgroup (alt build: HEP_XBF_TPW, A/B runs).  Measured at phi 0 b16: 2 tiles per workgroup on the 128x128 map (one
    // round of 512 workgroups instead of two) 31.0 us against 32.7 - the blob / squeeze-excite prologue it amortises is not
    // what a tile costs; 4 tiles per workgroup 35.2 us.  Default 1.
    {
      // default: two tiles per workgroup where one tile per workgroup would need more than the 512 workgroups the GPU holds at
      // once (two per CU) - the second round then runs in the same workgroups, without their blob / squeeze-excite prologue
      const int tpw_env = kn.xbf_tpw;
      const int tpw = tpw_env > 0 ? tpw_env : ((int64_t)xa.tiles * s->lane_batch > 512 ? 2 : 1);
      xa.tpw = std::max(1, std::min(tpw, xa.tiles));
    }
    *nblk = (xa.tiles + xa.tpw - 1) / xa.tpw;
    *part_t = tensor(nm, 1, *nblk, sqp2, true);
    snprintf(nm, sizeof nm, "b%d.project+b%d.front", defer.i, i);
    const int op = new_op(OP_XBF, nm);
    Op& o = s->ops[op];
    o.xbf = xa;
    wref(op, SLOT(xbf.blob), boff); wref(op, SLOT(xbf.se_br), defer.se.br); wref(op, SLOT(xbf.se_we), defer.se.we); wref(op, SLOT(xbf.se_be), defer.se.be); wref(op, SLOT(xbf.se_wr), wr_off);
    tref(op, SLOT(xbf.in), defer.dw_t, false); tref(op, SLOT(xbf.hpart), defer.se.hpart_t, false);
    if (xa.has_res) tref(op, SLOT(xbf.res), defer.inp, false);
    if (mid_needed) tref(op, SLOT(xbf.mid), defer.out_t, true);
    tref(op, SLOT(xbf.out), dw_t, true); tref(op, SLOT(xbf.hpart_out), *part_t, true);
    const double HWin = (double)Hin * Win;
    o.act_bytes_per_image = (HWin * pb.cexp + (double)Ho * Wo * b.cexp + HWin * pb.cout * ((pb.skip ? 1 : 0) + (mid_needed ? 1 : 0))) * es() +
                            ((double)defer.se.rows * defer.se.sqp + (double)*nblk * sqp2) * 4;
    o.weight_bytes = (double)blob.size() + (double)pb.cexp * defer.se.sq * es();
    o.flops_per_image = 2.0 * HWin * pb.cexp * pb.cout + 2.0 * HWin * b.cin * b.cexp + 2.0 * b.k * b.k * Ho * Wo * b.cexp;
    defer.active = false;
    return true;
  }
  std::vector<int> tap_blocks;     // blocks whose outputs feed the BiFPN (their outputs must reach HBM)
  // stem conv fused into block 0's depthwise launch (k_sbf.hip): set by add_stem instead of emitting a stem launch (alt build: HEP_SBF=1)
  struct FusedStem { bool on = false; size_t w_off = 0, b_off = 0; int S = 0, pad_t = 0, pad_l = 0, stem_t = -1; } fstem;
  int add_mbconv(int i, const MBConv& b, int x, int* H, int* W) {
    char pb[96]; snprintf(pb, sizeof pb, "backbone_net.model._blocks.%d", i);
    const std::string p = pb;
    char nm[64];
    const int inp = x;
    const int Hin = *H, Win = *W;
    // depthwise geometry
    int pt, pbm, pl, pr; same_pad(Hin, b.k, b.stride, &pt, &pbm); same_pad(Win, b.k, b.stride, &pl, &pr);
    const int Ho = (Hin + b.stride - 1) / b.stride, Wo = (Win + b.stride - 1) / b.stride;
    const PackTensor* wd = get(p + "._depthwise_conv.conv.weight", {b.cexp, 1, b.k, b.k});
    BnFold bn1; if (!fold_bn(pk, p + "._bn1", b.cexp, &bn1, err)) ok = false;
    if (!ok) return -1;
    const std::vector<float> wdw = fold_dw(wd, b.cexp, b.k * b.k, bn1.scale.data());
    snprintf(nm, sizeof nm, "b%d.dw", i);
    const int dw_t = tensor(nm, Ho, Wo, (b.cexp + 31) & ~31);      // (room for the project GEMM's fragment order: K padded to whole k-steps)
    s->tensors[dw_t].C_logical = b.cexp;

    // fused front (expand -> LDS -> depthwise, k_mbf.hip) whenever its LDS tiles fit; the expanded
    // tensor then never reaches HBM.  (alt build: HEP_MBF=none forces the two-kernel path, A/B measurements.)
    // output tile side of the fused front: 16 on the stride-1 layers of 16x16 / 32x32 maps (the whole 16x16 map per
    // workgroup: no halo re-expansion, a quarter of the workgroups and of their fixed staging / drain latency), else 8.
    // (alt build: HEP_MBF_TS=8 forces the small tile - A/B measurements, parity test of the alternative plan.)
    const int ts16_maxh = kn.mbf_ts16_maxh;     // 32 (alt build: A/B knob)
    int ts = (b.stride == 1 && b.expand && Ho >= 16 && Ho <= ts16_maxh) ? 16 : 8;
    if (kn.mbf_ts8) ts = 8;
    int max_in = mbf_max_inside(Hin, Win, b.k, b.stride, pt, pl, ts);   // rows of the compact input tile in LDS
    if (ts == 16 && mbf_lds_layout(b.cin, 64, b.k, b.stride, s->dtype, b.expand, max_in, ts, nullptr) > 159 * 1024 &&
        mbf_lds_layout(b.cin, 32, b.k, b.stride, s->dtype, b.expand, max_in, ts, nullptr) > 159 * 1024) {
      ts = 8; max_in = mbf_max_inside(Hin, Win, b.k, b.stride, pt, pl, ts);
    }
    int CC = 0, npass = 1, kp = 0;
    // Measured on MI355X at bs16 (profiles/README.md): the fused kernel beats expand+depthwise on input
    // maps up to 32x32 (it expands only the tile pixels inside the image, so on the 8x8 maps the halo costs
    // nothing) and loses on the big early maps (bandwidth-bound, the two-kernel path already streams well;
    // stride-2 halos there cost up to 4.5x recompute).  (alt build: HEP_MBF=all|none overrides for A/B runs.)
    const int maxh = kn.mbf_maxh;     // largest input map that takes the fused front (32)
    const bool want = kn.mbf >= 0 ? kn.mbf == 1 : Hin <= maxh;
    if (want)
      for (int cand : {64, 32, 16})      // (128 would need an item loop in phase C: one (pixel quad, channel quad) item per lane covers 64 channels of an 8x8 / 16x16 tile)
        if ((kn.mbf_cc < 0 || cand <= kn.mbf_cc) && mbf_lds_layout(b.cin, std::min(cand, b.expand ? cand : b.cexp), b.k, b.stride, s->dtype, b.expand, max_in, ts, nullptr) <= 159 * 1024) { CC = cand; break; }
    if (kn.mbf_cc < 0 && CC == 64 && b.expand) {      // (alt build A/B: the narrower chunk where it fills one round of workgroups that the wide one leaves half empty)
      const long tiles = (long)((Ho + ts - 1) / ts) * ((Wo + ts - 1) / ts), wg64 = tiles * ((b.cexp + 63) / 64) * s->lane_batch, wg32 = tiles * ((b.cexp + 31) / 32) * s->lane_batch;
      if (wg64 <= -kn.mbf_cc && wg32 <= 256) CC = 32;
    }
    // The tile / channel chunk / K-slice plan with the fewest ROUNDS of workgroups (HEP_MBF_MP=0 disables, =2 lifts the bf16
    // restriction below, =force takes the multi-pass form wherever it exists).  With the whole K staged at once an fp32 front needs twice the LDS of the bf16 one: the 16x16 tile of blocks 9,
    // 10 fell back to 8x8 (704 workgroups on 256 CUs: three rounds, 37 us against 17 us in bf16), the 8x8 maps kept one workgroup
    // of 146 KB per CU where 288 want to be resident (two rounds).  The multi-pass expand (k_mbf.hip, MP) stages K in slices and
    // gives fp32 the workgroup counts of the bf16 plan.
    {
      const bool force = kn.mbf_mp == 3;                             // parity runs: the multi-pass form wherever it exists, whatever the rounds
      const bool mp_on = kn.mbf_mp != 0;
      // A pass costs ~1 us of phase changes and the wider chunk a longer depthwise phase, so one round saved out of three does not
      // pay (phi 3 blocks 9-12, bf16: 3 -> 2 rounds, 23.6 -> 26.4 us): the multi-pass plan must at least HALVE the rounds.  bf16
      // sessions additionally keep plans of up to two rounds (HEP_MBF_MP=2 lifts that): measured only where the gain is large -
      // phi 3 @ 512 b8 blocks 14-17 (7 -> 2 rounds) 47 -> 38 us, blocks 19-23 26.5 -> 18.9 us, 4.65k -> 4.87k frames/s.
      const long min_old_rounds = (s->dtype == 0 || kn.mbf_mp == 2) ? 2 : 3;
      if (CC && b.expand && mp_on && s->dtype != 2) {
        struct Cand { int ts, CC, npass, kp; long rounds; size_t lds; };
        const int kstep = s->dtype ? 32 : 16, ksteps = (b.cin + kstep - 1) / kstep;
        auto rounds_of = [&](int ts_, int cc_, size_t lds) {
          const long tiles = (long)((Ho + ts_ - 1) / ts_) * ((Wo + ts_ - 1) / ts_), wgs = tiles * ((b.cexp + cc_ - 1) / cc_) * s->lane_batch;
          const long per_cu = std::max<long>(1, std::min<long>((long)(160 * 1024 / lds), ts_ == 16 ? 2 : 4));
          return (wgs + 256 * per_cu - 1) / (256 * per_cu);
        };
        Cand best{ts, CC, 1, 0, rounds_of(ts, CC, mbf_lds_layout(b.cin, CC, b.k, b.stride, s->dtype, 1, max_in, ts, nullptr)), 0};
        const bool ts16_ok = b.stride == 1 && Ho >= 16 && Ho <= ts16_maxh && !kn.mbf_ts8;
        for (int ts_ : {16, 8}) {
          if (ts_ == 16 && !ts16_ok) continue;
          const int mi = mbf_max_inside(Hin, Win, b.k, b.stride, pt, pl, ts_);
          for (int cc_ : {64, 48, 32})                        // (48: three n-tiles - fewer passes where the 64-wide expanded tile leaves no room for a wider K slice)
            for (int kpp = 3; kpp >= 1; kpp--) {              // k-steps per pass
              const int kp_ = kpp * kstep, np_ = (b.cin + kp_ - 1) / kp_;
              if (np_ < 2 || kpp > ksteps || !mbf_mp_fits(cc_, kp_, s->dtype, mi, ts_)) continue;
              const size_t lds = mbf_lds_layout(b.cin, cc_, b.k, b.stride, s->dtype, 1, mi, ts_, nullptr, kp_);
              if (lds > 159 * 1024) continue;
              const Cand c{ts_, cc_, np_, kp_, rounds_of(ts_, cc_, lds), lds};
              // fewer rounds first; then fewer passes (two barriers each); then the wider chunk
              if ((best.npass == 1 && 2 * c.rounds <= best.rounds && best.rounds >= min_old_rounds) || (best.npass > 1 && c.rounds < best.rounds) || (force && best.npass == 1) ||
                  (c.rounds == best.rounds && best.npass > 1 && (c.npass < best.npass || (c.npass == best.npass && c.CC > best.CC)))) best = c;
            }
        }
        if (best.npass > 1) { ts = best.ts; CC = best.CC; npass = best.npass; kp = best.kp; max_in = mbf_max_inside(Hin, Win, b.k, b.stride, pt, pl, ts); }
        if (kn.plan_debug) fprintf(stderr, "libhep plan: block %d front: tile %d, %d channels per workgroup, %d pass(es) of %d input channels, %ld round(s)\n", i, ts, CC, npass, kp ? kp : b.cin, best.rounds);
      }
    }
    // squeeze-excite weights: reduce FC [sq][Cexp] (fp32) for the front kernel; bias, expand FC [Cexp][sqp] (session
    // dtype, rows padded with zeros) and its bias for the project GEMM's prologue
    const PackTensor *wr = get(p + "._se_reduce.conv.weight", {b.se, b.cexp, 1, 1}), *br = get(p + "._se_reduce.conv.bias", {b.se}),
                     *we = get(p + "._se_expand.conv.weight", {b.cexp, b.se, 1, 1}), *be = get(p + "._se_expand.conv.bias", {b.cexp});
    if (!ok) return -1;
    const int sqp = (b.se + 7) & ~7;          // one 16-byte vector of the expand-FC weights = 8 (bf16) / 4 (fp32) hidden units
    if (sqp > 256) { *err = "squeeze-excite width above 256 is not supported"; ok = false; return -1; }
    const size_t wr_off = wb.put_f32(wr);
    SeSpec se; se.sq = b.se; se.sqp = sqp; se.inv_hw = 1.0f / (float)(Ho * Wo);
    se.br = wb.put_f32(br);
    {
      std::vector<float> wep((size_t)b.cexp * sqp, 0.f);
      for (int c = 0; c < b.cexp; c++) for (int j = 0; j < b.se; j++) wep[(size_t)c * sqp + j] = we->data[(size_t)c * b.se + j];
      se.we = wb.put_typed(wep);              // session dtype: half the bytes of the project prologue in bf16 sessions
    }
    se.be = wb.put_f32(be);
    int part_t = -1, nblk = 0;
    bool boundary = false;
    if (defer.active) {
      const bool keep = s->flags & 1u;
      const bool mid_needed = keep || b.skip || std::find(tap_blocks.begin(), tap_blocks.end(), defer.i) != tap_blocks.end();
      boundary = try_xbf(i, b, dw_t, wdw, bn1.shift, wr_off, sqp, Hin, Win, Ho, Wo, pt, pl, mid_needed, &part_t, &nblk);
      if (!ok) return -1;
      if (!boundary) flush_project();
      if (!ok) return -1;
    }
    // What the depthwise launches share, whichever kernel runs them.  dw_op: the partial squeeze-excite rows (nblk of them, one
    // per workgroup) and the op.  dw_refs: depthwise weights (BN1 folded) and bias, the reduce FC, input / output / partial
    // rows, and the bytes and flops of a depthwise conv on its own.
    auto dw_op = [&](OpKind kind, const std::string& name) {
      snprintf(nm, sizeof nm, "b%d.se_hpart", i);
      part_t = tensor(nm, 1, nblk, sqp, true);
      return new_op(kind, name);
    };
    auto dw_refs = [&](int op, Slot w, Slot bias, Slot se_wr, Slot in, Slot out, Slot part) {
      wref(op, w, wb.put_f32(wdw)); wref(op, bias, wb.put_f32(bn1.shift)); wref(op, se_wr, wr_off);
      if (in) tref(op, in, x, false);
      tref(op, out, dw_t, true); tref(op, part, part_t, true);
      Op& o = s->ops[op];
      o.act_bytes_per_image = ((double)Hin * Win + (double)Ho * Wo) * b.cexp * es();
      o.weight_bytes = (double)b.k * b.k * b.cexp * 4;
      o.flops_per_image = 2.0 * b.k * b.k * Ho * Wo * b.cexp;
    };
    // k_mbf.hip, with its expand stage (the fused front) or without (depthwise through LDS)
    auto mbf_op = [&](const char* suffix, int cin, int cc, int ts_, int has_expand, int max_in_, int npass_, int kp_) {
      nblk = ((Ho + ts_ - 1) / ts_) * ((Wo + ts_ - 1) / ts_) * ((b.cexp + cc - 1) / cc);      // one row per workgroup
      const int op = dw_op(OP_MBF, "b" + std::to_string(i) + suffix);
      MbfArgs& m = s->ops[op].mbf;
      m.H = Hin; m.W = Win; m.Cin = cin; m.Cexp = b.cexp; m.Ho = Ho; m.Wo = Wo; m.k = b.k; m.s = b.stride;
      m.pad_t = pt; m.pad_l = pl; m.has_expand = has_expand; m.bf16 = s->dtype; m.CC = cc; m.sq = b.se; m.sqp = sqp; m.ts = ts_;
      m.npass = npass_; m.kp = kp_; m.generic = kn.mbf_generic != 0;
      mbf_lds_layout(cin, cc, b.k, b.stride, s->dtype, has_expand, max_in_, ts_, &m, kp_);
      front_of_out[dw_t] = op; front_of_part[part_t] = op;
      return op;
    };
    if (boundary) {
    } else if (CC) {
      if (!b.expand) CC = std::min(CC, b.cexp);
      const int op = mbf_op(".front", b.cin, CC, ts, b.expand, max_in, npass, kp);
      MbfArgs& m = s->ops[op].mbf;
      // (the register-resident form - the whole tile requested at kernel start, parked slice by slice - measured SLOWER than fetching
      //  slice by slice: 8x8 maps 24.1 us against 22.4 us per launch, blocks 9 / 10 31.4 against 29.6: a pass is not bound by its
      //  memory round trip but by its three phase changes, ~1 us per pass whatever feeds it; alt build: HEP_MBF_MP_RES=1 selects it)
      m.mp_resident = npass > 1 && mbf_mp_resident(b.cin, CC, max_in, ts) && kn.mbf_mp_res != 0;
      if (b.expand) {
        const PackTensor* w = get(p + "._expand_conv.conv.weight", {b.cexp, b.cin, 1, 1});
        BnFold bn0; if (!fold_bn(pk, p + "._bn0", b.cexp, &bn0, err)) ok = false;
        if (!ok) return -1;
        const int rows = (b.cexp + 15) / 16 * 16;
        const FoldedPw f = fold_pw(w, b.cin, nullptr, &bn0, 0, b.cexp, rows);
        if (s->dtype == 2) {
          std::vector<float> sc;
          wref(op, SLOT(mbf.we), wb.put_fp8(f.w, rows, b.cin, (b.cin + 15) & ~15, &sc)); wref(op, SLOT(mbf.we_scale), wb.put_f32(sc));
          m.fp8 = 1; m.a_scale = 1.f;
        } else wref(op, SLOT(mbf.we), wb.put_typed(f.w));
        wref(op, SLOT(mbf.be), wb.put_f32(bn0.shift));      // (no conv bias: the folded bias is BN0's shift, Cexp values without the row padding)
      }
      dw_refs(op, SLOT(mbf.wdw), SLOT(mbf.bdw), SLOT(mbf.se_wr), SLOT(mbf.in), SLOT(mbf.out), mbf_hpart_slot);
      if (b.expand) {
        Op& o = s->ops[op];
        o.act_bytes_per_image = ((double)Hin * Win * b.cin + (double)Ho * Wo * b.cexp) * es();
        o.weight_bytes += (double)b.cexp * b.cin * (m.fp8 ? 1.0 : es());
        o.flops_per_image += 2.0 * Hin * Win * b.cin * b.cexp;
      }
    } else {
      if (b.expand) {
        snprintf(nm, sizeof nm, "b%d.expand", i);
        x = add_pw(nm, x, Hin * Win, b.cin, b.cexp, p + "._expand_conv.conv.weight", "", p + "._bn0", ACT_SWISH, nullptr, -1,
                   std::string(nm), Hin, Win, true);
        if (!ok) return -1;
      }
      // depthwise on its own: from global memory for the big maps (bandwidth-bound, k_dw.hip), through
      // LDS (the fused kernel without its expand stage) on the 8x8 maps, where the global-memory
      // version is a chain of k*k dependent load latencies.  (alt build: HEP_DWLDS=0|1 overrides.)
      const int dl = kn.dwlds;
      // (measured at bs16: the 5x5 stride-2 layer on the 64x64 map takes 20.6 us through LDS against
      //  27.2 us from global memory - 25 taps per output re-read too much through L1)
      const bool lds_dw = dl >= 0 ? dl != 0 : (Hin <= 8 || (b.k == 5 && Hin <= 64));
      const int ccl = std::min(64, b.cexp);
      const int max_in8 = mbf_max_inside(Hin, Win, b.k, b.stride, pt, pl, 8);
      if (lds_dw && mbf_lds_layout(b.cexp, ccl, b.k, b.stride, s->dtype, 0, max_in8, 8, nullptr) <= 159 * 1024) {
        const int op = mbf_op(".dw", b.cexp, ccl, 8, 0, max_in8, 0, 0);
        dw_refs(op, SLOT(mbf.wdw), SLOT(mbf.bdw), SLOT(mbf.se_wr), SLOT(mbf.in), SLOT(mbf.out), mbf_hpart_slot);
#ifdef HEP_ALT
      } else if (i == 0 && fstem.on) {
        // stem conv + this depthwise conv as ONE launch (k_sbf.hip): the stem's output stays in LDS
        SbfArgs f{};
        f.H = fstem.S; f.W = fstem.S; f.Hs = Hin; f.Ws = Win; f.C = b.cexp; f.pad_t = fstem.pad_t; f.pad_l = fstem.pad_l; f.bf16 = s->dtype;
        f.sq = b.se; f.sqp = sqp;
        sbf_layout(&f);
        nblk = f.tiles;
        const int op = dw_op(OP_SBF, "stem+b0.dw");
        s->ops[op].sbf = f;
        wref(op, SLOT(sbf.w_stem), fstem.w_off); wref(op, SLOT(sbf.b_stem), fstem.b_off);
        if (s->flags & 1u) tref(op, SLOT(sbf.stem_out), fstem.stem_t, true);
        dw_refs(op, SLOT(sbf.wdw), SLOT(sbf.bdw), SLOT(sbf.se_wr), nullptr, SLOT(sbf.out), SLOT(sbf.hpart));
        Op& o = s->ops[op];
        o.act_bytes_per_image = 3.0 * fstem.S * fstem.S * 4 + (double)Ho * Wo * b.cexp * es() + (double)nblk * sqp * 4;
        o.weight_bytes = (27.0 + 10.0) * b.cexp * 4;
        o.flops_per_image = 2.0 * 27 * Hin * Win * b.cexp + 2.0 * 9 * Ho * Wo * b.cexp;
#endif
      } else {
        // strip width: 4 output pixels per lane on the big maps; the stride-2 layers read 2x the columns per
        // output, so 2 keeps their loads denser (measured 18.1 us against 19.8 us on 128x128 -> 64x64 x 96)
        const int TW = Wo >= 32 ? (b.stride == 2 ? 2 : 4) : (Wo >= 16 ? 2 : 1);
        nblk = dw_blocks_per_image(Ho, Wo, b.cexp, TW);
        const int op = dw_op(OP_DW, "b" + std::to_string(i) + ".dw");
        DwArgs& d = s->ops[op].dw;
        d.H = Hin; d.W = Win; d.C = b.cexp; d.Ho = Ho; d.Wo = Wo; d.k = b.k; d.s = b.stride;
        d.pad_t = pt; d.pad_l = pl; d.act = ACT_SWISH; d.bf16 = s->dtype; d.TW = TW; d.blocks_per_image = nblk;
        d.sq = b.se; d.sqp = sqp;
        dw_refs(op, SLOT(dw.w), SLOT(dw.bias), SLOT(dw.se_wr), SLOT(dw.in), SLOT(dw.out), SLOT(dw.hpart));
      }
    }
    se.hpart_t = part_t; se.rows = nblk;
    // project + bn2 (+ residual), SE scale applied on the GEMM's input side: deferred (see flush_project / try_xbf)
    defer.active = true; defer.i = i; defer.b = b; defer.dw_t = dw_t; defer.inp = inp; defer.Ho = Ho; defer.Wo = Wo; defer.se = se; defer.p = p;
    defer.out_t = tensor(std::string("block") + std::to_string(i), Ho, Wo, b.cout);
    *H = Ho; *W = Wo;
    return defer.out_t;
  }

#ifdef HEP_ALT
  // ---- image-resident run of late blocks (k_late.hip): blocks i0 .. i1 as ONE launch, one workgroup per image ----
  // how many blocks starting at i0 (input map H x W, bf16 sessions) the late kernel can take: 0 = none
  int late_run(const std::vector<MBConv>& blocks, int i0, int H, int W) const {
    // HEP_LATE: 0 = launch by launch (front / squeeze-excite / project per block), 1 = the image-resident kernel
    if (!kn.late || s->dtype != 1) return 0;
    int n = 0;
    for (size_t i = i0; i < blocks.size() && n < LATE_MAX_BLOCKS; i++, n++) {
      const MBConv& b = blocks[i];
      if (!b.expand || !late_block_supported(b.cin, b.cexp, b.cout, b.k, b.stride, H, W, b.se) || (n > 0 && b.cin != blocks[i - 1].cout)) break;
    }
    if (n < 2) return 0;
    LateArgs probe; memset(&probe, 0, sizeof probe);
    probe.nblk = n;
    for (int j = 0; j < n; j++) { const MBConv& b = blocks[i0 + j]; probe.blk[j].Cin = b.cin; probe.blk[j].Cexp = b.cexp; probe.blk[j].N = b.cout; probe.blk[j].k = b.k; }
    return late_layout(&probe) ? n : 0;
  }
  // returns the output tensors of the blocks
  std::vector<int> add_late(const std::vector<MBConv>& blocks, int i0, int n, int x) {
    std::vector<int> outs;
    flush_project();
    if (!ok) return outs;
    char nm[64]; snprintf(nm, sizeof nm, "b%d-b%d.blocks", i0, i0 + n - 1);
    const int op = new_op(OP_LATE, nm);
    LateArgs la; memset(&la, 0, sizeof la);
    la.nblk = n;
    std::vector<unsigned char> blob;
    auto reserve = [&](size_t bytes) { const size_t off = (blob.size() + 15) & ~(size_t)15; blob.resize(off + bytes, 0); return off; };
    auto put_bf16 = [&](size_t off, size_t idx, float v) { const uint16_t h = f32_to_bf16(v); memcpy(blob.data() + off + idx * 2, &h, 2); };
    auto put_f32v = [&](size_t off, size_t idx, float v) { memcpy(blob.data() + off + idx * 4, &v, 4); };
    int cexp_max = 0;
    double act = 0, flops = 0;
    for (int j = 0; j < n; j++) {
      const MBConv& b = blocks[i0 + j];
      LateBlock& L = la.blk[j];
      L.Cin = b.cin; L.Cexp = b.cexp; L.N = b.cout; L.k = b.k; L.skip = b.skip ? 1 : 0; L.nchunks = b.cexp / LATE_CC;
      L.sq = b.se; L.sqp = (b.se + 7) & ~7; L.inv_hw = 1.0f / 64.0f;
      cexp_max = std::max(cexp_max, b.cexp);
    }
    if (!late_layout(&la)) { *err = "late blocks do not fit LDS"; ok = false; return outs; }      // (fills ntw / ng)
    for (int j = 0; j < n; j++) {
      const MBConv& b = blocks[i0 + j];
      LateBlock& L = la.blk[j];
      char pb[96]; snprintf(pb, sizeof pb, "backbone_net.model._blocks.%d", i0 + j);
      const std::string p = pb;
      const PackTensor *we = get(p + "._expand_conv.conv.weight", {b.cexp, b.cin, 1, 1}), *wd = get(p + "._depthwise_conv.conv.weight", {b.cexp, 1, b.k, b.k}),
                       *wr = get(p + "._se_reduce.conv.weight", {b.se, b.cexp, 1, 1}), *br = get(p + "._se_reduce.conv.bias", {b.se}),
                       *w2 = get(p + "._se_expand.conv.weight", {b.cexp, b.se, 1, 1}), *b2 = get(p + "._se_expand.conv.bias", {b.cexp}),
                       *wp = get(p + "._project_conv.conv.weight", {b.cout, b.cexp, 1, 1});
      BnFold bn0, bn1, bn2;
      if (!fold_bn(pk, p + "._bn0", b.cexp, &bn0, err) || !fold_bn(pk, p + "._bn1", b.cexp, &bn1, err) || !fold_bn(pk, p + "._bn2", b.cout, &bn2, err)) ok = false;
      if (!ok) return outs;
      const int kse = b.cin / 32, ksp = b.cexp / 32, kk = b.k * b.k, NC = L.nchunks, sqp = L.sqp;
      const FoldedPw fe = fold_pw(we, b.cin, nullptr, &bn0, 0, b.cexp, b.cexp), fp = fold_pw(wp, b.cexp, nullptr, &bn2, 0, b.cout, b.cout);
      const std::vector<float> fdw = fold_dw(wd, b.cexp, kk, bn1.scale.data());
      // expand weights in MFMA fragment order: [chunk][n-tile][k-step][lane = (r, g)][8]: W[n = c*128 + t*16 + r][k = ks*32 + 8g + e]
      L.off_we = (uint32_t)reserve((size_t)b.cexp * b.cin * 2);
      for (int c = 0; c < NC; c++) for (int t = 0; t < 8; t++) for (int ks = 0; ks < kse; ks++) for (int lane = 0; lane < 64; lane++) for (int e = 0; e < 8; e++) {
        const int nn = c * LATE_CC + t * 16 + (lane & 15), k = ks * 32 + 8 * (lane >> 4) + e;
        put_bf16(L.off_we, ((size_t)((c * 8 + t) * kse + ks) * 64 + lane) * 8 + e, fe.w[(size_t)nn * b.cin + k]);
      }
      L.off_be = (uint32_t)reserve((size_t)b.cexp * 4);
      for (int c = 0; c < b.cexp; c++) put_f32v(L.off_be, c, fe.b[c]);
      L.off_wdw = (uint32_t)reserve((size_t)kk * b.cexp * 4);
      for (int c = 0; c < NC; c++) for (int t = 0; t < kk; t++) for (int i = 0; i < LATE_CC; i++) {
        put_f32v(L.off_wdw, ((size_t)c * kk + t) * LATE_CC + i, fdw[(size_t)t * b.cexp + c * LATE_CC + i]);
      }
      L.off_bdw = (uint32_t)reserve((size_t)b.cexp * 4);
      for (int c = 0; c < b.cexp; c++) put_f32v(L.off_bdw, c, bn1.shift[c]);
      L.off_w1 = (uint32_t)reserve((size_t)NC * sqp * LATE_CC * 4);
      for (int c = 0; c < NC; c++) for (int jj = 0; jj < b.se; jj++) for (int i = 0; i < LATE_CC; i++)
        put_f32v(L.off_w1, ((size_t)c * sqp + jj) * LATE_CC + i, wr->data[(size_t)jj * b.cexp + c * LATE_CC + i]);
      L.off_b1 = (uint32_t)reserve(64 * 4);
      for (int jj = 0; jj < b.se; jj++) put_f32v(L.off_b1, jj, br->data[jj]);
      L.off_w2 = (uint32_t)reserve((size_t)b.cexp * sqp * 2);
      for (int c = 0; c < b.cexp; c++) for (int jj = 0; jj < b.se; jj++) put_bf16(L.off_w2, (size_t)c * sqp + jj, w2->data[(size_t)c * b.se + jj]);
      L.off_b2 = (uint32_t)reserve((size_t)b.cexp * 4);
      for (int c = 0; c < b.cexp; c++) put_f32v(L.off_b2, c, b2->data[c]);
      // project weights: [n-group][k-step][n-tile of the group][lane][8]: W[n = (ng*ntw + jt)*16 + r][k = ks*32 + 8g + e], rows >= N zero
      L.off_wp = (uint32_t)reserve((size_t)L.ng * ksp * L.ntw * 1024);
      for (int ng = 0; ng < L.ng; ng++) for (int ks = 0; ks < ksp; ks++) for (int jt = 0; jt < L.ntw; jt++) for (int lane = 0; lane < 64; lane++) {
        const int nn = (ng * L.ntw + jt) * 16 + (lane & 15);
        if (nn >= b.cout) continue;
        for (int e = 0; e < 8; e++) {
          const int k = ks * 32 + 8 * (lane >> 4) + e;
          put_bf16(L.off_wp, ((size_t)((ng * ksp + ks) * L.ntw + jt) * 64 + lane) * 8 + e, fp.w[(size_t)nn * b.cexp + k]);
        }
      }
      L.off_bp = (uint32_t)reserve((size_t)L.ng * L.ntw * 16 * 4);
      for (int c = 0; c < b.cout; c++) put_f32v(L.off_bp, c, fp.b[c]);
      const int out_t = tensor(std::string("block") + std::to_string(i0 + j), 8, 8, b.cout);
      outs.push_back(out_t);
      act += 64.0 * b.cout * es() * (b.skip ? 2 : 1);
      flops += 2.0 * 64 * b.cin * b.cexp + 2.0 * kk * 64 * b.cexp + 2.0 * 64 * b.cexp * b.cout + 4.0 * b.cexp * b.se;
    }
    const size_t boff = wb.put_bytes(blob);
    // workgroups per image (HEP_LATE_G; default 3 where every block's chunk count divides): each runs 1 / G of the chunk loop -
    // the part that is bound by ONE CU's vector ALU - and they meet once per block (k_late.hip)
    int G = kn.late_g;
    if (G < 1 || G > 8) G = 1;
    for (int j = 0; j < n; j++) if (la.blk[j].nchunks % G != 0) G = 1;
    // the members of a group spin-wait for each other: they must all be resident at once.  A workgroup of this kernel fills a CU (1024
    // threads, near-full LDS), so a launch of lane_batch * G workgroups is only safe while that is a small part of the chip - other
    // streams' workgroups hold CUs as well.  Beyond a quarter of the CUs: one workgroup per image, no meetings.
    if ((long)s->lane_batch * G > s->cu_count / 4) G = 1;
    la.G = G;
    la.cross_xcd = kn.late_xcd != 0;      // 1: a group on consecutive workgroup ids = across XCDs (tests: same bits)
    const int ds_t = tensor(std::string(nm) + ".dw", 1, 1, 64 * cexp_max * (G > 1 ? 2 : 1));
    la.dstride = 64 * cexp_max * 2 * (G > 1 ? 2 : 1);
    const int hp_t = tensor(std::string(nm) + ".se_part", 1, 1, 2 * 8 * 64, true);
    s->ops[op].late = la;
    wref(op, SLOT(late.blob), boff);
    tref(op, SLOT(late.in), x, false); tref(op, SLOT(late.dscratch), ds_t, true); tref(op, SLOT(late.hpart), hp_t, true);
    for (int j = 0; j < n; j++) {
      tref(op, SLOT(late.blk[seg].out), outs[j], true, j);
      if (blocks[i0 + j].skip) tref(op, SLOT(late.blk[seg].res), j == 0 ? x : outs[j - 1], false, j);
    }
    Op& o = s->ops[op];
    o.act_bytes_per_image = 64.0 * blocks[i0].cin * es() + act;      // (the depthwise outputs' round trip through L2 is the kernel's own business)
    o.weight_bytes = (double)blob.size();
    o.flops_per_image = flops;
    return outs;
  }

#endif   // HEP_ALT

  // ---- fused separable conv launch (1..n segments sharing C) ----
  struct SegSpec {
    int src[3] = {-1, -1, -1}, kind[3] = {SRC_SAME, SRC_SAME, SRC_SAME}; float fw[3] = {1.f, 1.f, 1.f}; int nsrc = 1, pre_act = 0;
    int level = 0;                   // pyramid level index 0..4 of the output
    std::string key;                 // state_dict prefix of the SeparableConvBlock
    std::string bn;                  // BN to fold (may be empty)
    int N = 0, act = ACT_NONE;
    int out_t = -1;                  // dtype tensor, or -1 for a head output
    int head_out = -1, col_kin = 1, col_kout = 1, col_off = 0, out_k = 0;   // head output index 0..4 and column mapping
  };
  int sep_tile_side() const {
    SepArgs probe; memset(&probe, 0, sizeof probe);
    sep_lds_layout(s->arch.fpn_w, s->dtype, 8, 96, s->arch.fpn_w, &probe);
    return probe.lds_bytes > 160 * 1024 ? 4 : 8;
  }
  void add_sep(const std::string& name, const std::vector<SegSpec>& specs, bool chain = false) {
    const int C = s->arch.fpn_w;
    const int op = new_op(OP_SEP, name);
    int tile_begin = 0, ts_max = 4, cols_f32 = 0, cols_map = 0;
    // tile side 8; 4 where the 8x8 tile of this width and dtype does not fit in LDS (fp32, width >= 288);
    // chains (one tile per image) then only cover levels <= 4x4
    const int ts_pick = sep_tile_side();
    double bytes = 0, flops = 0, wbytes = 0;
    // head layers (many independent single-source segments, all maps or all head outputs) run on the
    // wave-per-patch kernel of k_tower.hip (alt build: HEP_TOWER=0 keeps them on the tiled kernel of k_sep.hip)
    int direct = 0;
    {
      bool simple = specs.size() > 1 && !chain && tower_supports(C) && kn.tower != 0;
      bool maps = true, heads = true;
      for (const SegSpec& sp : specs) {
        simple = simple && sp.nsrc == 1 && sp.kind[0] == SRC_SAME && !sp.pre_act && sp.fw[0] == 1.f;
        maps = maps && sp.out_t >= 0 && sp.N == C; heads = heads && sp.out_t < 0;
      }
      if (simple && (maps || heads)) direct = maps ? 1 : 2;
    }
    // cooperative tower form (tower_coop_kernel) wherever it is instantiated and measured faster: bf16 map layers from width 160, where
    // the wave-private halos of tower_kernel no longer fit (phi 3 @ 512 b8: 5.02k -> 5.15k frames/s; the bf16 header launch there stays
    // on tower_kernel: 113 against 118 us - its segments have 1-10 n-tiles for five waves), fp32 at width 64 (24.7k -> 25.7k).
    // HEP_TOWER_COOP: 0 off, 1 on wherever instantiated, 2 map layers only, 3 headers only
    int coop = 0;
    if (direct && tower_coop_built(s->dtype != 0, C)) {      // (direct: C is a tower width)
      const int v = kn.tower_coop;
      // bf16 below width 160 stays on tower_kernel.  At width 64 (instantiated for the A/B, bit-identical): map layers 16 against 13.3 us, the
      // header launch - the hand head as one 36-tile segment on eight waves - 47.6 against 27.3 us; 49.0k against 49.7k frames/s with both:
      // tower_kernel's four wave-private halos fit at this width and it has no barrier per image
      if (v < 0) coop = s->dtype == 0 || (C >= 160 && direct == 1);
      else coop = v == 1 || (v == 2 && direct == 1) || (v == 3 && direct == 2);
    }
    const int chunk_cols_out = (direct ? (coop ? tower_coop_hdr_tiles(C, s->dtype != 0) : tower_hdr_tiles(C, s->dtype != 0)) : SEP_MAX_TILES_N) * 16;   // head outputs are split into column chunks, maps never
    int tiles_n_max = 0;
    for (size_t i = 0; i < specs.size(); i++) {
      const SegSpec& sp = specs[i];
      const int hw = s->levels[sp.level];
      const PackTensor* wd = get(sp.key + ".depthwise_conv.conv.weight", {C, 1, 3, 3});
      const PackTensor* wp = get(sp.key + ".pointwise_conv.conv.weight", {sp.N, C, 1, 1});
      const PackTensor* bp = get(sp.key + ".pointwise_conv.conv.bias", {sp.N});
      BnFold bn; if (!sp.bn.empty() && !fold_bn(pk, sp.bn, sp.N, &bn, err)) ok = false;
      if (!ok) return;
      const size_t wdw_off = wb.put_f32(fold_dw(wd, C, 9));
      for (int j = 0; j < sp.nsrc; j++) bytes += (double)s->tensors[sp.src[j]].H * s->tensors[sp.src[j]].W * C * es();
      bytes += (double)hw * hw * sp.N * (sp.out_t >= 0 ? es() : 4.0);
      flops += 2.0 * 9 * hw * hw * C + 2.0 * hw * hw * C * sp.N;
      wbytes += (double)sp.N * C * es() + 9.0 * C * 4;
      const int chunk_cols = sp.out_t >= 0 ? SEP_MAX_TILES_MAP * 16 : chunk_cols_out;
      for (int n0 = 0; n0 < sp.N; n0 += chunk_cols) {        // wide headers: one segment per chunk of columns
        const int Nc = std::min(chunk_cols, sp.N - n0);
        SepSeg sg; memset(&sg, 0, sizeof sg);
        sg.h = hw; sg.w = hw; sg.C = C; sg.nsrc = sp.nsrc; sg.pre_act = sp.pre_act;
        for (int j = 0; j < sp.nsrc; j++) {
          const TensorDesc& t = s->tensors[sp.src[j]];
          sg.kind[j] = sp.kind[j]; sg.fw[j] = sp.fw[j]; sg.sh[j] = t.H; sg.sw[j] = t.W;
          int pb, pa; same_pad(t.H, 3, 2, &pb, &pa); sg.pool_pad[j] = pb;
        }
        const int tilesN = direct == 1 ? tower_map_tiles(C) : (Nc + 15) / 16;
        tiles_n_max = std::max(tiles_n_max, tilesN);
        // k_tower.hip map layers: MFMA row (nt, i) holds channel (i/4)*RUN + 4*nt + i%4 (RUN = 4*tilesN),
        // so that a lane's results over the n-tiles are consecutive channels
        std::vector<int> row_of(direct == 1 ? Nc : 0);
        for (size_t n = 0; n < row_of.size(); n++) { const int run = 4 * tilesN, gq = (int)n / run, rem = (int)n % run; row_of[n] = (rem / 4) * 16 + gq * 4 + rem % 4; }
        const FoldedPw f = fold_pw(wp, C, bp, sp.bn.empty() ? nullptr : &bn, n0, Nc, tilesN * 16, direct == 1 ? &row_of : nullptr);
        sg.N = Nc; sg.tilesN = tilesN; sg.act = sp.act; sg.n_base = n0;
        sg.ts = ts_pick;   // 8; 16x16 tiles measured slower (3 dependent gather rounds per lane, 1 workgroup per CU)
        if (!direct && !chain && specs.size() == 1 && hw <= kn.sep_ts4_maxhw) sg.ts = 4;   // latency knob: 4x4 tiles on levels with few 8x8 tiles (one batch in flight +1-3 %, four in flight -1-4 %: DESIGN section 2)
        ts_max = std::max(ts_max, sg.ts);
        if (sp.out_t >= 0) cols_map = std::max(cols_map, Nc); else cols_f32 = std::max(cols_f32, Nc);
        sg.tiles_x = (hw + sg.ts - 1) / sg.ts; sg.tiles_y = sg.tiles_x; sg.tile_begin = tile_begin; sg.tiles_x_rcp = rcp_u32(sg.tiles_x);
        tile_begin += sg.tiles_x * sg.tiles_y;
        if (sp.out_t >= 0) {
          sg.out_f32 = 0; sg.out_bstride = (int64_t)hw * hw * sp.N; sg.out_off = n0; sg.out_rowstride = sp.N;
          sg.col_kin = 1; sg.col_kout = 1; sg.col_off = 0;
        } else {
          sg.out_f32 = 1; sg.out_bstride = (int64_t)s->num_anchors * sp.out_k; sg.out_off = (int64_t)s->level_off[sp.level] * sp.out_k;
          sg.out_rowstride = 9 * sp.out_k; sg.col_kin = sp.col_kin; sg.col_kout = sp.col_kout; sg.col_off = sp.col_off;
        }
        s->ops[op].segs.push_back(sg);
        const int si = (int)s->ops[op].segs.size() - 1;
        wref(op, SLOT(segs[seg].wdw), wdw_off, si); wref(op, SLOT(segs[seg].wpw), wb.put_typed(f.w), si); wref(op, SLOT(segs[seg].bias), wb.put_f32(f.b), si);
        for (int j = 0; j < sp.nsrc; j++) tref(op, SLOT(segs[seg].src[idx]), sp.src[j], false, si, j);
        if (sp.out_t >= 0) tref(op, SLOT(segs[seg].out), sp.out_t, true, si);
        else href(op, SLOT(segs[seg].out), sp.head_out, si);
      }
    }
    Op& o = s->ops[op];
    o.sep.nseg = (int)o.segs.size(); o.sep.total_tiles = tile_begin; o.sep.bf16 = s->dtype; o.sep.C = C;
    o.sep.chain = chain && o.segs.size() > 1;
    o.sep.direct = direct;
    o.sep.coop = coop;
    o.sep.generic = kn.neck_generic == 1 || kn.neck_generic == 2;
    o.sep.seg0 = o.segs[0];      // (its shape fields decide the kernel - sep_shape_id, also for a plan that is never realised; build_session copies it again with the addresses)
    bool all_maps = true;
    for (const SegSpec& sp : specs) all_maps = all_maps && sp.out_t >= 0 && sp.N == C;
    sep_lds_layout(C, s->dtype, ts_max, cols_f32, cols_map, &o.sep, (chain || specs.size() == 1) && all_maps && !direct && kn.sep_wlds != 0);
    if (direct) { o.sep.off_wdw = 0; o.sep.off_bias = (size_t)9 * C * 4; o.sep.lds_bytes = o.sep.off_bias + (size_t)tiles_n_max * 16 * 4; }
    if (o.sep.lds_bytes > 160 * 1024) { *err = "BiFPN width too large for the fused separable-conv tile"; ok = false; return; }
    o.act_bytes_per_image = bytes; o.flops_per_image = flops; o.weight_bytes = wbytes;
  }

#ifdef HEP_ALT
  // ---- the five head towers depth-first (k_heads.hip): ONE launch for the tower layers and headers of every net and level ----
  struct HeaderSpec { int net; std::string key; int kin, kout, off, out, act; };
  bool add_heads_fused(const std::vector<std::string>& nets, const std::vector<HeaderSpec>& hds, const int feat[5], int depth) {
    const int C = s->arch.fpn_w;
    if (!heads_fused_supported(C, depth, s->dtype)) return false;
    const int op = new_op(OP_HEADS, "heads.fused");
    HeadsArgs ha; memset(&ha, 0, sizeof ha);
    ha.D = depth; ha.num_anchors = s->num_anchors;
    for (int l = 0; l < 5; l++) ha.level_off[l] = s->level_off[l];
    ha.lds_bytes = heads_lds_bytes(depth, &ha.off_wdw);
    // items: 16x16 output tiles, sorted by decreasing work - pixels of the tile x (tower layers + the header's n-tiles): the hand net's
    // tiles of the big levels first (the grid is (images, items): item 0 of every image is dispatched before item 1 of any)
    std::vector<HeadItem> items;
    std::vector<double> work;
    for (int l = 0; l < 5; l++)
      for (int n = 0; n < (int)nets.size(); n++) {
        const int hw = s->levels[l];
        int ncols = 0;
        for (const HeaderSpec& h : hds) if (h.net == n) ncols += 9 * h.kin;
        for (int ty = 0; ty < hw; ty += 16) for (int tx = 0; tx < hw; tx += 16) {
          HeadItem it; memset(&it, 0, sizeof it);
          it.net = n; it.level = l; it.hw = hw; it.y0 = ty; it.x0 = tx;
          items.push_back(it);
          const double px = (double)std::min(16, hw - ty) * std::min(16, hw - tx);
          work.push_back(px * (depth * 1.6 * 64 + ncols) + 2000);
        }
      }
    {
      std::vector<int> order(items.size());
      for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
      std::stable_sort(order.begin(), order.end(), [&](int x_, int y_) { return work[x_] > work[y_]; });
      std::vector<HeadItem> sorted;
      for (int i : order) sorted.push_back(items[i]);
      items.swap(sorted);
    }
    std::vector<unsigned char> blob(items.size() * sizeof(HeadItem), 0);
    auto reserve = [&](size_t bytes) { const size_t off = (blob.size() + 15) & ~(size_t)15; blob.resize(off + bytes, 0); return off; };
    auto put_bf16 = [&](size_t off, size_t idx, float v) { const uint16_t h = f32_to_bf16(v); memcpy(blob.data() + off + idx * 2, &h, 2); };
    auto put_f32v = [&](size_t off, size_t idx, float v) { memcpy(blob.data() + off + idx * 4, &v, 4); };
    // depthwise table [9][C] fp32 with k_tower.hip's swizzle: channels (0,2,1,3 | 4,6,5,7) of every octet
    auto put_dw = [&](size_t off, const PackTensor* wd) {
      static const int perm[8] = {0, 2, 1, 3, 4, 6, 5, 7};
      const std::vector<float> dw = fold_dw(wd, C, 9);
      for (int t = 0; t < 9; t++) for (int c = 0; c < C; c++) put_f32v(off, (size_t)t * C + c, dw[(size_t)t * C + (c & ~7) + perm[c & 7]]);
    };
    // pointwise fragments [n-tile][k-step][lane = (r, g)][8]: W[n = nt*16 + r][k = ks*32 + 8g + e] (rows >= N zero)
    auto put_frags = [&](size_t off, const std::vector<float>& w, int N, int ntiles) {
      for (int nt = 0; nt < ntiles; nt++) for (int ks = 0; ks < C / 32; ks++) for (int lane = 0; lane < 64; lane++) {
        const int n = nt * 16 + (lane & 15);
        if (n >= N) continue;
        for (int e = 0; e < 8; e++) { const int k = ks * 32 + 8 * (lane >> 4) + e; put_bf16(off, ((size_t)(nt * (C / 32) + ks) * 64 + lane) * 8 + e, w[(size_t)n * C + k]); }
      }
    };
    double wbytes = 0, flops = 0, obytes = 0;
    std::vector<std::vector<size_t>> layer_off(nets.size(), std::vector<size_t>(5, 0));
    for (size_t n = 0; n < nets.size(); n++)
      for (int l = 0; l < 5; l++) {
        const size_t off = reserve((size_t)depth * (8192 + 256 + 2304));
        layer_off[n][l] = off;
        for (int i = 0; i < depth; i++) {
          const std::string key = nets[n] + ".conv_list." + std::to_string(i);
          const PackTensor* wd = get(key + ".depthwise_conv.conv.weight", {C, 1, 3, 3});
          const PackTensor* wp = get(key + ".pointwise_conv.conv.weight", {C, C, 1, 1});
          const PackTensor* bp = get(key + ".pointwise_conv.conv.bias", {C});
          BnFold bn; if (!fold_bn(pk, nets[n] + ".bn_list." + std::to_string(l) + "." + std::to_string(i), C, &bn, err)) ok = false;
          if (!ok) return true;
          const size_t lo = off + (size_t)i * (8192 + 256 + 2304);
          const FoldedPw f = fold_pw(wp, C, bp, &bn, 0, C, C);
          put_frags(lo, f.w, C, 4);
          for (int c = 0; c < C; c++) put_f32v(lo + 8192, c, f.b[c]);
          put_dw(lo + 8192 + 256, wd);
        }
        wbytes += depth * (8192.0 + 256 + 2304);
        flops += depth * (2.0 * 9 * s->levels[l] * s->levels[l] * C + 2.0 * s->levels[l] * s->levels[l] * C * C);
      }
    std::vector<size_t> hdr_off(hds.size(), 0);
    for (size_t h = 0; h < hds.size(); h++) {
      const HeaderSpec& hd = hds[h];
      const int N = 9 * hd.kin, ntiles = (N + 15) / 16;
      const PackTensor* wd = get(hd.key + ".depthwise_conv.conv.weight", {C, 1, 3, 3});
      const PackTensor* wp = get(hd.key + ".pointwise_conv.conv.weight", {N, C, 1, 1});
      const PackTensor* bp = get(hd.key + ".pointwise_conv.conv.bias", {N});
      if (!ok) return true;
      const size_t off = reserve(2304 + (size_t)ntiles * 64 + (size_t)ntiles * 2 * 1024);
      hdr_off[h] = off;
      put_dw(off, wd);
      const FoldedPw f = fold_pw(wp, C, bp, nullptr, 0, N, N);
      for (int c = 0; c < N; c++) put_f32v(off + 2304, c, f.b[c]);
      put_frags(off + 2304 + (size_t)ntiles * 64, f.w, N, ntiles);
      wbytes += 2304.0 + ntiles * (64.0 + 2048);
      for (int l = 0; l < 5; l++) { flops += 2.0 * 9 * s->levels[l] * s->levels[l] * C + 2.0 * s->levels[l] * s->levels[l] * C * N; obytes += (double)s->levels[l] * s->levels[l] * N * 4; }
    }
    for (HeadItem& it : items) {
      it.off_layers = (uint32_t)layer_off[it.net][it.level];
      for (size_t h = 0; h < hds.size(); h++)
        if (hds[h].net == it.net) {
          const int j = it.nhdr++;
          if (j >= 2) { *err = "more than two headers on one head net"; ok = false; return true; }
          it.off_hdr[j] = (uint32_t)hdr_off[h]; it.hdr_N[j] = 9 * hds[h].kin; it.hdr_ntiles[j] = (9 * hds[h].kin + 15) / 16;
          it.hdr_kin[j] = hds[h].kin; it.hdr_kout[j] = hds[h].kout; it.hdr_off[j] = hds[h].off; it.hdr_act[j] = hds[h].act; it.hdr_out[j] = hds[h].out;
        }
    }
    memcpy(blob.data(), items.data(), items.size() * sizeof(HeadItem));
    ha.nitems = (int)items.size();
    const size_t boff = wb.put_bytes(blob);
    s->ops[op].heads = ha;
    wref(op, SLOT(heads.blob), boff);
    double ibytes = 0;
    for (int l = 0; l < 5; l++) { tref(op, SLOT(heads.feat[seg]), feat[l], false, l); ibytes += (double)s->levels[l] * s->levels[l] * C * es() * nets.size(); }
    for (int k = 0; k < 5; k++) href(op, SLOT(heads.out[seg]), k, k);
    Op& o = s->ops[op];
    o.act_bytes_per_image = ibytes + obytes; o.weight_bytes = wbytes; o.flops_per_image = flops;
    return true;
  }

#endif   // HEP_ALT

  // ---- LDS-resident chain of small-level BiFPN nodes (k_chain.hip): [optional max-pools of cell 0] + nodes ----
  // pools: {source tensor, output tensor, output level} in order (cell 0: p6_in from p6_pre, p7_in from p6_in).
  // Returns false (nothing added) when the chain does not fit the kernel: the caller then emits the k_sep.hip path.
  struct PoolSpec { int src_t, out_t, level; };
  bool add_chain(const std::string& name, const std::vector<PoolSpec>& pools, const std::vector<SegSpec>& specs) {
    const int C = s->arch.fpn_w;
    if (C % 8 != 0 || specs.empty()) return false;
    if (s->dtype == 0 && kn.chain_f32 == 0) return false;      // (alt build A/B knob: fp32 chains back on k_sep.hip)
    // LDS map slots.  Every slot records who writes it (def: -1 = the prologue, else the node index) and the last node that
    // reads it; after the node list is complete the slots are packed by liveness (pack_slots below): the output of node n takes
    // the place of a map of the same size whose last reader is a node <= n.  fp32 sessions need it (maps of 16 KB), bf16
    // sessions just use less LDS.
    struct Slot { int off, h, w; };
    struct SlotLife { int off, elems, def, last; };
    std::map<std::pair<int, int>, Slot> slot;          // (tensor, 0 as stored / 1 pooled to half size) -> LDS slot
    std::vector<SlotLife> life;
    int top = 0;                                        // elements
    auto new_slot = [&](int t, int form, int h, int w, int def) {
      Slot sl{top, h, w}; const int elems = (h * w * C + 7) & ~7;
      life.push_back({top, elems, def, def}); top += elems; slot[{t, form}] = sl; return sl;
    };
    auto touch = [&](int off, int node) { for (SlotLife& l : life) if (l.off == off) l.last = std::max(l.last, node); };
    std::vector<ChainExt> exts; std::vector<int> ext_t, ext_store_t;
    std::vector<ChainNode> nodes; std::vector<int> node_out_t;
    auto pool_pad_of = [&](int n) { int pb, pa; same_pad(n, 3, 2, &pb, &pa); return pb; };
    auto add_ext = [&](int t, bool pooled, int store_t) {
      const TensorDesc& td = s->tensors[t];
      ChainExt x; memset(&x, 0, sizeof x);
      x.sh = td.H; x.sw = td.W; x.kind = pooled ? SRC_DOWN : SRC_SAME;
      x.h = pooled ? (td.H + 1) / 2 : td.H; x.w = pooled ? (td.W + 1) / 2 : td.W; x.pool_pad = pool_pad_of(td.H);
      x.has_store = store_t >= 0;
      x.off = new_slot(store_t >= 0 ? store_t : t, store_t >= 0 ? 0 : (pooled ? 1 : 0), x.h, x.w, -1).off;
      exts.push_back(x); ext_t.push_back(t); ext_store_t.push_back(store_t);
    };
    // pools of cell 0
    for (size_t i = 0; i < pools.size(); i++) {
      const PoolSpec& ps = pools[i];
      if (!slot.count({ps.src_t, 0})) {                 // first pool: its input comes from an earlier launch -> pooled while loaded
        add_ext(ps.src_t, true, ps.out_t);
      } else {                                          // pool of a map that lives in a slot
        const Slot in = slot[{ps.src_t, 0}];
        ChainNode nd; memset(&nd, 0, sizeof nd);
        nd.pool_only = 1; nd.nsrc = 1; nd.h = (in.h + 1) / 2; nd.w = (in.w + 1) / 2; nd.pool_pad = pool_pad_of(in.h);
        nd.src[0] = ChainSrc{in.off, SRC_DOWN, in.h, in.w, 1.f};
        touch(in.off, (int)nodes.size());
        nd.out_off = new_slot(ps.out_t, 0, nd.h, nd.w, (int)nodes.size()).off; nd.widx = -1;
        nodes.push_back(nd); node_out_t.push_back(ps.out_t);
      }
    }
    const size_t es2 = s->dtype ? 2 : 4, pad = s->dtype ? 8 : 4;
    const int wnode_bytes = (int)((((size_t)10 * C * 4 + (size_t)C * (C + pad) * es2) + 1023) & ~(size_t)1023);   // whole KB: streamed by LDS-DMA, 1 KB per wave instruction
    std::vector<unsigned char> blob;
    double bytes = 0, flops = 0, wbytes = 0;
    int nconv = 0, hw_max = 0;
    for (const SegSpec& sp : specs) {
      const int hw = s->levels[sp.level];
      if (sp.N != C || sp.out_t < 0 || sp.act != ACT_NONE || !sp.pre_act) return false;
      ChainNode nd; memset(&nd, 0, sizeof nd);
      nd.nsrc = sp.nsrc; nd.h = hw; nd.w = hw; nd.widx = nconv++;
      hw_max = std::max(hw_max, hw);
      const int me = (int)nodes.size();
      for (int j = 0; j < sp.nsrc; j++) {
        const int t = sp.src[j];
        const TensorDesc& td = s->tensors[t];
        bytes += (double)td.H * td.W * C * es();
        if (slot.count({t, 0})) {                       // a map of this chain (or an input already in a slot), at its own size
          const Slot sl = slot[{t, 0}];
          nd.src[j] = ChainSrc{sl.off, sp.kind[j], sl.h, sl.w, sp.fw[j]};
          if (sp.kind[j] == SRC_DOWN) nd.pool_pad = pool_pad_of(sl.h);
        } else if (sp.kind[j] == SRC_DOWN) {            // input from a bigger level: pooled while it is loaded
          if (!slot.count({t, 1})) add_ext(t, true, -1);
          const Slot sl = slot[{t, 1}];
          nd.src[j] = ChainSrc{sl.off, SRC_SAME, sl.h, sl.w, sp.fw[j]};
        } else {
          add_ext(t, false, -1);
          const Slot sl = slot[{t, 0}];
          nd.src[j] = ChainSrc{sl.off, sp.kind[j], sl.h, sl.w, sp.fw[j]};
        }
        touch(nd.src[j].off, me);
      }
      nd.out_off = new_slot(sp.out_t, 0, hw, hw, me).off;
      nodes.push_back(nd); node_out_t.push_back(sp.out_t);
      // weights in the kernel's LDS layout: [9][C] depthwise f32 | [C] bias f32 | [C][C + pad] pointwise rows in the session dtype
      const PackTensor* wd = get(sp.key + ".depthwise_conv.conv.weight", {C, 1, 3, 3});
      const PackTensor* wp = get(sp.key + ".pointwise_conv.conv.weight", {C, C, 1, 1});
      const PackTensor* bp = get(sp.key + ".pointwise_conv.conv.bias", {C});
      BnFold bn; if (!fold_bn(pk, sp.bn, C, &bn, err)) ok = false;
      if (!ok) return true;                             // (the error is reported by the caller through `ok`)
      const size_t base = blob.size();
      blob.resize(base + wnode_bytes, 0);
      const FoldedPw f = fold_pw(wp, C, bp, &bn, 0, C, C);
      const std::vector<float> dw = fold_dw(wd, C, 9);
      float* fdw = reinterpret_cast<float*>(blob.data() + base);
      memcpy(fdw, dw.data(), dw.size() * 4);
      float* fb = fdw + 9 * C;
      memcpy(fb, f.b.data(), (size_t)C * 4);
      uint16_t* fw16 = reinterpret_cast<uint16_t*>(fb + C);
      float* fw32 = fb + C;
      for (int n = 0; n < C; n++)
        for (int k = 0; k < C; k++) {
          const float v = f.w[(size_t)n * C + k];
          if (s->dtype) fw16[(size_t)n * (C + pad) + k] = f32_to_bf16(v); else fw32[(size_t)n * (C + pad) + k] = v;
        }
      bytes += (double)hw * hw * C * es(); flops += 2.0 * hw * hw * C * (9 + C); wbytes += (double)C * C * es() + 10.0 * C * 4;
    }
    if (nodes.size() > CH_MAX_NODES || exts.size() > CH_MAX_EXT) return false;
    // ---- pack the slots by liveness: exact-size reuse (the maps of a chain come in three sizes).  A convolution node reads its
    //      sources in its gather phase, two barriers before its MFMA phase writes the output, so its output may take the slot of
    //      one of its own sources; a pool-only node reads and writes in one phase and may not. ----
    {
      std::vector<int> order(life.size());
      for (size_t i = 0; i < life.size(); i++) order[i] = (int)i;
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return life[x].def < life[y].def; });
      struct Placed { int new_off, elems, last; };
      std::vector<Placed> placed; std::map<int, int> remap; int ntop = 0;
      for (int i : order) {
        const SlotLife& l = life[i];
        int pick = -1;
        // (a pool-only node writes its output in its only phase, with no barrier behind the previous node's copy-out: it never
        //  takes over a slot)
        if (l.def >= 0 && !nodes[l.def].pool_only)
          for (size_t q = 0; q < placed.size(); q++)
            if (placed[q].elems == l.elems && placed[q].last <= l.def) { pick = (int)q; break; }
        if (pick >= 0) { remap[l.off] = placed[pick].new_off; placed[pick].last = std::max(l.last, l.def); }
        else { remap[l.off] = ntop; placed.push_back({ntop, l.elems, std::max(l.last, l.def)}); ntop += l.elems; }
      }
      for (ChainExt& x : exts) x.off = remap[x.off];
      for (ChainNode& nd : nodes) { nd.out_off = remap[nd.out_off]; for (int j = 0; j < nd.nsrc; j++) nd.src[j].off = remap[nd.src[j].off]; }
      top = ntop;
    }
    ChainArgs ca; memset(&ca, 0, sizeof ca);
    ca.nnodes = (int)nodes.size(); ca.nconv = nconv; ca.next = (int)exts.size(); ca.C = C; ca.wnode_bytes = wnode_bytes; ca.bf16 = s->dtype ? 1 : 0; ca.generic = kn.neck_generic == 1 || kn.neck_generic == 3;
    const size_t halo_b = (((size_t)(hw_max + 2) * (hw_max + 2) * (C + pad) * es2 + 15) & ~(size_t)15);
    const size_t atile_b = (size_t)((hw_max * hw_max + 15) & ~15) * (C + pad) * es2;
    ca.off_w = ((size_t)top * es2 + 15) & ~(size_t)15;
    // all node weights resident when they fit; else two nodes' weights in LDS, the next node's streamed under the running one (fp32
    // at width 64); else only the depthwise weights + biases in LDS and the pointwise fragments straight from global memory (width 160)
    const size_t wsmall = (size_t)10 * C * 4;
    auto wlds = [&](int mode) { return mode == 2 ? (size_t)nconv * wsmall : (size_t)(mode == 1 ? std::min(2, nconv) : nconv) * wnode_bytes; };
    ca.stream_w = 0;
    while (ca.stream_w < 2 && ca.off_w + wlds(ca.stream_w) + halo_b + atile_b > 158 * 1024) ca.stream_w++;
    if (kn.chain_stream >= 0) ca.stream_w = std::min(2, kn.chain_stream);     // A/B knob, parity tests of the other forms in bf16
    if (ca.stream_w == 2 && (C + (s->dtype ? 31 : 15)) / (s->dtype ? 32 : 16) > 6) return false;         // six k-steps of fragments in registers
    if (ca.stream_w == 2 && kn.chain_wglobal == 0) return false;
    ca.off_halo = ca.off_w + wlds(ca.stream_w);
    ca.off_atile = ca.off_halo + halo_b;
    ca.lds_bytes = ca.off_atile + atile_b;
    if (ca.lds_bytes > 158 * 1024) return false;
    const int op = new_op(OP_CHAIN, name);
    Op& o = s->ops[op];
    for (size_t e = 0; e < exts.size(); e++) {
      ca.ext[e] = exts[e];
      tref(op, SLOT(chain.ext[seg].src), ext_t[e], false, (int)e);
      if (ext_store_t[e] >= 0) tref(op, SLOT(chain.ext[seg].store), ext_store_t[e], true, (int)e);
    }
    for (ChainNode& nd : nodes) { nd.w_rcp = (uint32_t)(0x100000000ull / (uint32_t)nd.w) + 1; nd.hs_rcp = (uint32_t)(0x100000000ull / (uint32_t)(nd.w + 2)) + 1; }
    for (size_t n = 0; n < nodes.size(); n++) tref(op, SLOT(cnodes[seg].out), node_out_t[n], true, (int)n);
    o.chain = ca; o.cnodes = nodes;
    const size_t boff = wb.put_bytes(blob);
    wref(op, SLOT(chain.wblob), boff);
    o.act_bytes_per_image = bytes; o.flops_per_image = flops; o.weight_bytes = wbytes;
    return true;
  }

  // ---- stem conv (BN0 folded); returns its output tensor, H x W its map ----
  int add_stem(int* H, int* W) {
    const Arch& A = s->arch;
    const int S = s->size;
    *H = (S + 1) / 2; *W = (S + 1) / 2;
    const PackTensor* w = get("backbone_net.model._conv_stem.conv.weight", {A.stem, 3, 3, 3});
    BnFold bn; if (!fold_bn(pk, "backbone_net.model._bn0", A.stem, &bn, err)) ok = false;
    if (!ok) return -1;
    std::vector<float> wf((size_t)27 * A.stem);
    for (int co = 0; co < A.stem; co++)
      for (int ci = 0; ci < 3; ci++)
        for (int t = 0; t < 9; t++) wf[((size_t)t * 3 + ci) * A.stem + co] = w->data[((size_t)co * 3 + ci) * 9 + t] * bn.scale[co];
    const int x = tensor("stem", *H, *W, A.stem);
    int pt, pb, pl, pr; same_pad(S, 3, 2, &pt, &pb); same_pad(S, 3, 2, &pl, &pr);
#ifdef HEP_ALT
    // stem + block 0's depthwise conv as one launch (k_sbf.hip), possible when block 0 has no expand conv (every
    // EfficientNet-B0..B7).  NOT the default: measured at phi 0 b16 bf16 the fused launch takes 42.8 us against 14.5 + 16.0 us
    // for the two kernels (workgroup life 14.8 us: 4 us input staging, 6.3 us for the stem phase - instruction-bound, not
    // matrix-pipe-bound: the split-bf16 MFMA form changed nothing - 2 us depthwise, 1.9 us channel sums; 14x14 tiles
    // recompute 1.56x the stem pixels).  HEP_SBF=1 selects it (parity-tested as an alternative plan).
    const MBConv& b0 = A.blocks[0];
    if (kn.sbf != 0 && s->dtype != 2 && !b0.expand && b0.k == 3 && b0.stride == 1 && A.stem % 8 == 0 && A.stem <= 64 && b0.cexp == A.stem &&
        b0.se <= 16) {
      fstem.on = true; fstem.w_off = wb.put_f32(wf); fstem.b_off = wb.put_f32(bn.shift); fstem.S = S; fstem.pad_t = pt; fstem.pad_l = pl; fstem.stem_t = x;
      return x;
    }
#endif
    const int op = new_op(OP_STEM, "stem");
    Op& o = s->ops[op];
    o.stem.H = S; o.stem.W = S; o.stem.Ho = *H; o.stem.Wo = *W; o.stem.Cout = A.stem; o.stem.pad_t = pt; o.stem.pad_l = pl; o.stem.bf16 = s->dtype; o.stem.mfma = stem_uses_mfma(A.stem, kn.stem_mfma);
    wref(op, SLOT(stem.w), wb.put_f32(wf)); wref(op, SLOT(stem.bias), wb.put_f32(bn.shift));
    tref(op, SLOT(stem.out), x, true);
    o.act_bytes_per_image = 3.0 * S * S * 4 + (double)*H * *W * A.stem * es();
    o.weight_bytes = 27.0 * A.stem * 4; o.flops_per_image = 2.0 * 27 * *H * *W * A.stem;
    return x;
  }

  // ---- backbone: the MBConv blocks behind the stem output x; taps[] receives the three outputs that feed the BiFPN ----
  void add_backbone(int x, int H, int W, int taps[3]) {
    const Arch& A = s->arch;
    for (int t = 0; t < 3; t++) { taps[t] = -1; tap_blocks.push_back(A.taps[t]); }
    for (size_t i = 0; i < A.blocks.size(); i++) {
#ifdef HEP_ALT
      if (const int nl = late_run(A.blocks, (int)i, H, W)) {        // blocks i .. i + nl - 1 as one image-resident launch (k_late.hip)
        const std::vector<int> outs = add_late(A.blocks, (int)i, nl, x);
        if ((int)outs.size() != nl) ok = false;
        if (!ok) return;
        for (int j = 0; j < nl; j++)
          for (int t = 0; t < 3; t++) if (A.taps[t] == (int)i + j) taps[t] = outs[j];
        x = outs.back();
        i += nl - 1;
        continue;
      }
#endif
      x = add_mbconv((int)i, A.blocks[i], x, &H, &W);
      if (!ok) return;
      for (int t = 0; t < 3; t++) if (A.taps[t] == (int)i) taps[t] = x;
    }
    flush_project();
  }

  // ---- BiFPN ----
  std::vector<SegSpec> pending; std::vector<std::string> pending_names;   // small-level BiFPN nodes awaiting a chain launch
  std::vector<PoolSpec> pending_pools;                                      // cell 0's two max-pools ride in the first chain
  void emit_pools() {
    const int Wf = s->arch.fpn_w;
    for (const PoolSpec& ps : pending_pools) {
      const int ph = s->tensors[ps.src_t].H, oh = s->levels[ps.level];
      const int op = new_op(OP_POOL, s->tensors[ps.out_t].name.substr(0, s->tensors[ps.out_t].name.size() - 3) + "_pool");
      Op& o = s->ops[op];
      int pb, pa; same_pad(ph, 3, 2, &pb, &pa);
      o.pool.H = ph; o.pool.W = ph; o.pool.C = Wf; o.pool.Ho = oh; o.pool.Wo = oh; o.pool.pad_t = pb; o.pool.pad_l = pb; o.pool.bf16 = s->dtype;
      tref(op, SLOT(pool.in), ps.src_t, false); tref(op, SLOT(pool.out), ps.out_t, true);
      o.act_bytes_per_image = ((double)ph * ph + (double)oh * oh) * Wf * es();
    }
    pending_pools.clear();
  }
  // the pending nodes as one launch: an LDS-resident chain (k_chain.hip, with the pending pools) where it fits, else k_sep.hip
  void flush_nodes() {
    if (pending.empty()) { emit_pools(); return; }
    std::string nm = pending_names.front();
    for (size_t i = 1; i < pending_names.size(); i++) nm += "+" + pending_names[i].substr(pending_names[i].find('.') + 1);
    if (kn.chain == 2 && add_chain(nm, pending_pools, pending)) pending_pools.clear();
    else { emit_pools(); if (ok) add_sep(nm, pending, pending.size() > 1); }
    pending.clear(); pending_names.clear();
  }
  void fusion_weights(const std::string& key, int n, float* out) {
    if (!s->arch.attention) { for (int i = 0; i < n; i++) out[i] = 1.f; return; }
    const PackTensor* t = get(key, {n});
    if (!t) return;
    float r[3], sum = 0.f;
    for (int i = 0; i < n; i++) { r[i] = std::max(t->data[i], 0.f); sum += r[i]; }
    for (int i = 0; i < n; i++) out[i] = r[i] / (sum + kFusionEps);   // efficientdet/model.py:212-213
  }
  // one fusion node of cell `p` (tensor names `tn`): sources {tensor, SRC_*}, weights `wkey`, separable conv `conv`
  int add_node(const std::string& p, const std::string& tn, const char* conv, const char* wkey, int level, const std::vector<std::pair<int, int>>& srcs, const char* oname) {
    const int Wf = s->arch.fpn_w;
    float w[3];
    fusion_weights(p + "." + wkey, (int)srcs.size(), w);
    SegSpec sp;
    sp.nsrc = (int)srcs.size(); sp.pre_act = 1; sp.level = level; sp.key = p + "." + conv; sp.bn = p + "." + conv + ".bn"; sp.N = Wf;
    for (int j = 0; j < sp.nsrc; j++) { sp.src[j] = srcs[j].first; sp.kind[j] = srcs[j].second; sp.fw[j] = w[j]; }
    sp.out_t = tensor(tn + oname, s->levels[level], s->levels[level], Wf);
    // Consecutive nodes on levels <= 8x8 (one tile per image) are launched as ONE chain: a workgroup
    // per image runs them back to back (k_sep.hip mode 2).  Measured at bs16: a 5-node chain takes
    // 29.8 us against 5 x 7 us as separate launches (a node is ~6 us of dependent global round trips
    // inside the kernel either way; the chain saves the launch boundaries).
    // (alt build) HEP_CHAIN: 0 = every node its own launch, 1 = chains inside k_sep.hip (mode 2), 2 (default) = LDS-resident chains
    // (k_chain.hip) wherever they fit - BiFPN width 64 in every session dtype (fp32: streamed node weights) - and k_sep.hip chains elsewhere
    if (kn.chain != 0 && s->levels[level] <= sep_tile_side() && Wf <= SEP_MAX_TILES_MAP * 16) { pending.push_back(sp); pending_names.push_back(tn + conv); }
    else { flush_nodes(); add_sep(tn + conv, {sp}); }
    return sp.out_t;
  }
  void add_bifpn(const int taps[3], int feat[5]) {
    const Arch& A = s->arch;
    const int Wf = A.fpn_w;
    for (int r = 0; r < A.fpn_cells; r++) {
      const std::string p = "bifpn." + std::to_string(r);
      const std::string tn = "c" + std::to_string(r) + ".";
      int in[5], in2[5];
      if (r == 0) {
        const int L3 = s->levels[0], L4 = s->levels[1], L5 = s->levels[2];
        // the six lateral 1x1 convs only depend on the backbone taps: one grouped launch (alt build: HEP_PWG=0, six launches)
        struct Lat { const char* nm; int tap, L; const char* key; const char* out; };
        const Lat lat[6] = {{"p3_down", 0, L3, ".p3_down_channel", "p3_in"}, {"p4_down", 1, L4, ".p4_down_channel", "p4_in"},
                            {"p5_down", 2, L5, ".p5_down_channel", "p5_in"}, {"p4_down2", 1, L4, ".p4_down_channel_2", "p4_in2"},
                            {"p5_down2", 2, L5, ".p5_down_channel_2", "p5_in2"}, {"p5_to_p6", 2, L5, ".p5_to_p6", "p6_pre"}};
        int lat_out[6];
        if (kn.pwg != 0) {
          std::vector<PwSpec> specs;
          for (const Lat& l : lat)
            specs.push_back({tn + l.nm, p + l.key + ".0.conv.weight", p + l.key + ".0.conv.bias", p + l.key + ".1", tn + l.out,
                             taps[l.tap], l.L * l.L, A.tap_channels[l.tap], l.L, l.L});
          const std::vector<int> outs = add_pw_group(tn + "laterals", specs, Wf);
          if (outs.size() != 6) ok = false;
          if (!ok) return;
          for (int i = 0; i < 6; i++) lat_out[i] = outs[i];
        } else {
          for (int i = 0; i < 6; i++)
            lat_out[i] = add_pw(tn + lat[i].nm, taps[lat[i].tap], lat[i].L * lat[i].L, A.tap_channels[lat[i].tap], Wf, p + lat[i].key + ".0.conv.weight",
                                p + lat[i].key + ".0.conv.bias", p + lat[i].key + ".1", ACT_NONE, nullptr, -1, tn + lat[i].out, lat[i].L, lat[i].L);
        }
        in[0] = lat_out[0]; in[1] = lat_out[1]; in[2] = lat_out[2]; in2[1] = lat_out[3]; in2[2] = lat_out[4];
        if (!ok) return;
        int prev = lat_out[5];           // p6_pre
        for (int l = 3; l < 5; l++) {      // p6_in = pool(p6_pre), p7_in = pool(p6_in): launched with the first chain, or on their own
          const int oh = s->levels[l];
          const int t = tensor(tn + (l == 3 ? "p6_in" : "p7_in"), oh, oh, Wf);
          pending_pools.push_back({prev, t, l});
          in[l] = t; prev = t;
        }
        in2[0] = in[0]; in2[3] = in[3]; in2[4] = in[4];
      } else {
        for (int l = 0; l < 5; l++) { in[l] = feat[l]; in2[l] = feat[l]; }
      }
      const int p6_up = add_node(p, tn, "conv6_up", "p6_w1", 3, {{in[3], SRC_SAME}, {in[4], SRC_UP}}, "p6_up"); if (!ok) return;
      const int p5_up = add_node(p, tn, "conv5_up", "p5_w1", 2, {{in[2], SRC_SAME}, {p6_up, SRC_UP}}, "p5_up"); if (!ok) return;
      const int p4_up = add_node(p, tn, "conv4_up", "p4_w1", 1, {{in[1], SRC_SAME}, {p5_up, SRC_UP}}, "p4_up"); if (!ok) return;
      const int p3_out = add_node(p, tn, "conv3_up", "p3_w1", 0, {{in[0], SRC_SAME}, {p4_up, SRC_UP}}, "p3_out"); if (!ok) return;
      const int p4_out = add_node(p, tn, "conv4_down", "p4_w2", 1, {{in2[1], SRC_SAME}, {p4_up, SRC_SAME}, {p3_out, SRC_DOWN}}, "p4_out"); if (!ok) return;
      const int p5_out = add_node(p, tn, "conv5_down", "p5_w2", 2, {{in2[2], SRC_SAME}, {p5_up, SRC_SAME}, {p4_out, SRC_DOWN}}, "p5_out"); if (!ok) return;
      const int p6_out = add_node(p, tn, "conv6_down", "p6_w2", 3, {{in[3], SRC_SAME}, {p6_up, SRC_SAME}, {p5_out, SRC_DOWN}}, "p6_out"); if (!ok) return;
      const int p7_out = add_node(p, tn, "conv7_down", "p7_w2", 4, {{in[4], SRC_SAME}, {p6_out, SRC_DOWN}}, "p7_out"); if (!ok) return;
      feat[0] = p3_out; feat[1] = p4_out; feat[2] = p5_out; feat[3] = p6_out; feat[4] = p7_out;
    }
    if (!pending.empty()) flush_nodes();      // (the pools of cell 0 left with that cell's first launch: level 0 never chains)
  }

  // ---- heads ----
  void add_heads(const int feat[5]) {
    const Arch& A = s->arch;
    const int Wf = A.fpn_w;
    static const char* nets[5] = {"regressor", "classifier", "rotation_net", "translation_net", "hand_net"};
    struct Hd { int net; const char* key; int kin, kout, off, out, act; };
    const int NC = s->num_classes;     // per anchor the classifier emits one column per class (efficientdet/model.py:406-408)
    const Hd hds[6] = {{0, "regressor.header", 4, 4, 0, 0, ACT_NONE}, {1, "classifier.header", NC, NC, 0, 1, ACT_SIGMOID},
                       {2, "rotation_net.initial_rotation", 3, 3, 0, 2, ACT_NONE},
                       {3, "translation_net.initial_translation_xy", 2, 3, 0, 3, ACT_NONE},
                       {3, "translation_net.initial_translation_z", 1, 3, 2, 3, ACT_NONE},
                       {4, "hand_net.initial_hand_coords", 63, 63, 0, 4, ACT_NONE}};
#ifdef HEP_ALT
    // HEP_HEADS_FUSED: 1 = the towers depth-first in ONE launch (k_heads.hip; bf16 at BiFPN width 64), 0 = launch by launch
    if (kn.heads_fused != 0) {
      std::vector<std::string> nv(nets, nets + 5);
      std::vector<HeaderSpec> hv;
      for (const Hd& h : hds) hv.push_back({h.net, h.key, h.kin, h.kout, h.off, h.out, h.act});
      if (add_heads_fused(nv, hv, feat, A.head_depth) || !ok) return;
    }
#endif
    // one launch per tower layer (all five nets x five levels) + one for all headers (k_tower.hip)
    int cur[5][5];
    for (int n = 0; n < 5; n++) for (int l = 0; l < 5; l++) cur[n][l] = feat[l];
    for (int i = 0; i < A.head_depth; i++) {
      std::vector<SegSpec> specs;
      for (int n = 0; n < 5; n++)
        for (int l = 0; l < 5; l++) {
          SegSpec sp;
          sp.src[0] = cur[n][l]; sp.level = l; sp.N = Wf; sp.act = ACT_SWISH;
          sp.key = std::string(nets[n]) + ".conv_list." + std::to_string(i);
          sp.bn = std::string(nets[n]) + ".bn_list." + std::to_string(l) + "." + std::to_string(i);   // per-level BN, shared conv
          sp.out_t = tensor(std::string(nets[n]) + ".t" + std::to_string(i) + ".p" + std::to_string(l + 3), s->levels[l], s->levels[l], Wf);
          specs.push_back(sp);
        }
      add_sep("heads.tower" + std::to_string(i), specs);
      if (!ok) return;
      for (int n = 0; n < 5; n++) for (int l = 0; l < 5; l++) cur[n][l] = specs[n * 5 + l].out_t;
    }
    std::vector<SegSpec> specs;
    for (const Hd& h : hds)
      for (int l = 0; l < 5; l++) {
        SegSpec sp;
        sp.src[0] = cur[h.net][l]; sp.level = l; sp.key = h.key; sp.N = 9 * h.kin; sp.act = h.act; sp.head_out = h.out;
        sp.col_kin = h.kin; sp.col_kout = h.kout; sp.col_off = h.off; sp.out_k = h.kout;
        specs.push_back(sp);
      }
    add_sep("heads.headers", specs);
  }
};

// ---- activation arena: first-fit with liveness-based reuse.  keep: every tensor a place of its own; guard: bytes left free
//      behind every tensor.  Fills TensorDesc::offset, returns the bytes one lane needs. ----
static size_t layout_arena(Session* s, bool keep, size_t guard) {
  struct Free { size_t off, size; };
  std::vector<Free> freelist; size_t top = 0;
  auto slot_bytes = [&](const TensorDesc& td) { return (((td.bytes_per_image * s->lane_batch) + 255) & ~(size_t)255) + guard; };
  const int nops = (int)s->ops.size();
  for (int i = 0; i < nops; i++) {
    for (int t : s->ops[i].writes) {
      TensorDesc& td = s->tensors[t];
      if (td.first_op != i) continue;
      const size_t need = slot_bytes(td);
      bool placed = false;
      if (!keep)
        for (size_t f = 0; f < freelist.size(); f++)
          if (freelist[f].size >= need) {
            td.offset = freelist[f].off;
            freelist[f].off += need; freelist[f].size -= need;
            if (freelist[f].size == 0) freelist.erase(freelist.begin() + f);
            placed = true; break;
          }
      if (!placed) { td.offset = top; top += need; }
    }
    if (!keep) {
      std::vector<int> touched = s->ops[i].reads; touched.insert(touched.end(), s->ops[i].writes.begin(), s->ops[i].writes.end());
      std::sort(touched.begin(), touched.end()); touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
      for (int t : touched) {
        TensorDesc& td = s->tensors[t];
        if (td.last_op != i) continue;
        freelist.push_back({td.offset, slot_bytes(td)});
        // coalesce neighbours
        std::sort(freelist.begin(), freelist.end(), [](const Free& a, const Free& b) { return a.off < b.off; });
        for (size_t f = 0; f + 1 < freelist.size();)
          if (freelist[f].off + freelist[f].size == freelist[f + 1].off) { freelist[f].size += freelist[f + 1].size; freelist.erase(freelist.begin() + f + 1); }
          else f++;
      }
    }
  }
  return (top + 255) & ~(size_t)255;
}

int plan_session(Session* s, const Pack& pack, Plan* plan, std::string* err) {
  const int S = s->size;
  int off = 0;
  for (int l = 0; l < 5; l++) { s->levels[l] = (S + (1 << (l + 3)) - 1) >> (l + 3); s->level_off[l] = off; off += s->levels[l] * s->levels[l] * 9; }
  s->num_anchors = off;
  {   // classes: whatever the classifier's header was trained with (num_anchors * num_classes channels, efficientdet/model.py:393)
    auto it = pack.tensors.find("classifier.header.pointwise_conv.conv.weight");
    if (it == pack.tensors.end() || it->second.dims.size() != 4) { *err = "weight pack: missing tensor 'classifier.header.pointwise_conv.conv.weight'"; return HEP_ERR_PACK; }
    const int64_t n = it->second.dims[0];
    if (n < 9 || n % 9 || n / 9 > 63) { *err = "weight pack: the classifier header must hold 9 * num_classes channels, num_classes in 1..63"; return HEP_ERR_PACK; }
    s->num_classes = (int)(n / 9);
  }
  Planner P(s, pack, plan, err);
  int H, W, taps[3], feat[5];
  const int x = P.add_stem(&H, &W);
  if (P.ok) P.add_backbone(x, H, W, taps);
  if (P.ok) P.add_bifpn(taps, feat);
  if (!P.ok) return HEP_ERR_PACK;
  for (int l = 0; l < 5; l++) s->feat_ids[l] = feat[l];
  P.add_heads(feat);
  if (!P.ok) return HEP_ERR_PACK;
  // every launch has a device function: a tower width that is not built, a cooperative form that is not, a shape id without a row
  for (const Op& o : s->ops)
    if (!op_pick(o).fn) { *err = "plan: no kernel instantiation is built for launch '" + o.name + "'"; return HEP_ERR_INTERNAL; }

  // ---- liveness, then the arena ----
  const int nops = (int)s->ops.size();
  for (int i = 0; i < nops; i++) {
    for (int t : s->ops[i].writes) { if (s->tensors[t].first_op < 0) s->tensors[t].first_op = i; s->tensors[t].last_op = std::max(s->tensors[t].last_op, i); }
    for (int t : s->ops[i].reads) s->tensors[t].last_op = std::max(s->tensors[t].last_op, i);
  }
  for (int l = 0; l < 5; l++) s->tensors[feat[l]].last_op = nops;   // exported after the last op
#ifdef HEP_POISON_LDS     // sanitizer build: every tensor keeps a place of its own, followed by a guard band that hep_destroy checks (hep_api.cpp)
  s->arena_bytes = layout_arena(s, true, 256);
#else
  s->arena_bytes = layout_arena(s, s->flags & 1u, 0);
#endif
  plan->weights = std::move(P.wb.host);
  return 0;
}

}  // namespace hep
