// hep_pack.cpp - HEPW weight pack reader and the weight builder: BatchNorm folding, the pointwise / depthwise
// fold helpers every planner site shares, conversion to the session dtype.  Host only.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "hep_plan.h"

namespace hep {

// ---- weight pack ----
bool Pack::parse(const void* blob, size_t n, std::string* err, bool borrow) {
  if (!borrow) storage.assign((const unsigned char*)blob, (const unsigned char*)blob + n);
  const unsigned char* p = borrow ? (const unsigned char*)blob : storage.data();
  auto fail = [&](const char* m) { *err = std::string("weight pack: ") + m; return false; };
  if (n < 12 || memcmp(p, "HEPW", 4) != 0) return fail("bad magic (expected HEPW)");
  uint32_t ver, count; memcpy(&ver, p + 4, 4); memcpy(&count, p + 8, 4);
  if (ver != 1) return fail("unsupported version");
  size_t q = 12;
  for (uint32_t i = 0; i < count; i++) {
    if (q + 2 > n) return fail("truncated table");
    uint16_t nl; memcpy(&nl, p + q, 2); q += 2;
    if (q + nl + 1 > n) return fail("truncated table");
    std::string name((const char*)p + q, nl); q += nl;
    int nd = p[q]; q += 1;
    if (nd > 8 || q + 4 * nd + 16 > n) return fail("truncated table");
    PackTensor t; size_t cnt = 1; bool big = false;
    for (int d = 0; d < nd; d++) {
      uint32_t v; memcpy(&v, p + q, 4); q += 4; t.dims.push_back(v);
      if (v != 0 && cnt > (n / 4) / v) big = true; else cnt *= v;      // checked product: a tensor cannot hold more floats than the file
    }
    uint64_t off, nb; memcpy(&off, p + q, 8); memcpy(&nb, p + q + 8, 8); q += 16;
    if (big || nb != (uint64_t)cnt * 4 || off > n || nb > n - off || (off & 3) || off < 12) return fail("tensor out of bounds");
    t.data = (const float*)(p + off); t.count = cnt;
    tensors[name] = t;
  }
  return true;
}

const PackTensor* Pack::get(const std::string& name, std::initializer_list<int64_t> dims, std::string* err) const {
  auto it = tensors.find(name);
  if (it == tensors.end()) { *err = "weight pack: missing tensor '" + name + "'"; return nullptr; }
  if (it->second.dims != std::vector<int64_t>(dims)) {
    *err = "weight pack: tensor '" + name + "' has the wrong shape for this phi";
    return nullptr;
  }
  return &it->second;
}

// ---- weight builder: folds BN, lays weights out, converts to the session dtype ----
uint16_t f32_to_bf16(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// fp32 -> OCP e4m3fn (bias 7, no infinities, max 448), round to nearest even, saturating
static uint8_t f32_to_e4m3(float f) {
  const uint8_t sign = std::signbit(f) ? 0x80 : 0;
  float a = fabsf(f);
  if (a != a) return sign | 0x7f;
  if (a >= 464.f) return sign | 0x7e;                                  // beyond the last rounding boundary: +-448
  if (a < 0.015625f) {                                                 // below 2^-6: subnormals, step 2^-9
    const int q = (int)nearbyintf(a * 512.f);
    return sign | (uint8_t)q;                                          // q == 8 is the smallest normal, 0x08
  }
  int e; const float m = frexpf(a, &e);                                // a = m * 2^e, m in [0.5, 1)
  int ee = e - 1, mant = (int)nearbyintf((m * 2.f - 1.f) * 8.f);
  if (mant == 8) { mant = 0; ee++; }
  if (ee > 8 || (ee == 8 && mant > 6)) return sign | 0x7e;
  return sign | (uint8_t)(((ee + 7) << 3) | mant);
}

size_t WBuilder::alloc(size_t bytes) {
  size_t off = (size + 255) & ~(size_t)255;
  size = off + bytes;
  if (!layout_only) host.resize(size, 0);
  return off;
}
size_t WBuilder::put_bytes(const std::vector<unsigned char>& v) {
  size_t off = alloc(v.size());
  if (!layout_only) memcpy(host.data() + off, v.data(), v.size());
  return off;
}
size_t WBuilder::put_f32(const std::vector<float>& v) {
  size_t off = alloc(v.size() * 4);
  if (!layout_only) memcpy(host.data() + off, v.data(), v.size() * 4);
  return off;
}
size_t WBuilder::put_fp8(const std::vector<float>& v, int rows, int K, int stride, std::vector<float>* scales) {
  const size_t off = alloc((size_t)rows * stride);
  scales->assign(rows, 1.f);
  if (layout_only) return off;
  for (int n = 0; n < rows; n++) {
    float amax = 0.f;
    for (int k = 0; k < K; k++) amax = std::max(amax, fabsf(v[(size_t)n * K + k]));
    const float sc = amax > 0.f ? amax / 448.f : 1.f;
    (*scales)[n] = sc;
    for (int k = 0; k < K; k++) host[off + (size_t)n * stride + k] = f32_to_e4m3(v[(size_t)n * K + k] / sc);
  }
  return off;
}
size_t WBuilder::put_typed(const std::vector<float>& v) {
  if (dtype == 0) return put_f32(v);
  size_t off = alloc(v.size() * 2);
  if (layout_only) return off;
  uint16_t* d = (uint16_t*)(host.data() + off);
  for (size_t i = 0; i < v.size(); i++) d[i] = f32_to_bf16(v[i]);
  return off;
}

static const float kBnEps = 1e-3f;      // efficientnet/utils.py:245, efficientdet/model.py:36
bool fold_bn(const Pack& pk, const std::string& p, int c, BnFold* out, std::string* err) {
  const PackTensor *g = pk.get(p + ".weight", {c}, err), *b = pk.get(p + ".bias", {c}, err),
                   *m = pk.get(p + ".running_mean", {c}, err), *v = pk.get(p + ".running_var", {c}, err);
  if (!g || !b || !m || !v) return false;
  out->scale.resize(c); out->shift.resize(c);
  for (int i = 0; i < c; i++) {
    const float s = g->data[i] / sqrtf(v->data[i] + kBnEps);
    out->scale[i] = s; out->shift[i] = b->data[i] - m->data[i] * s;
  }
  return true;
}

FoldedPw fold_pw(const PackTensor* w, int K, const PackTensor* conv_bias, const BnFold* bn, int n0, int Nc, int rows, const std::vector<int>* row_of) {
  FoldedPw f;
  f.w.assign((size_t)rows * K, 0.f); f.b.assign(rows, 0.f);
  for (int n = 0; n < Nc; n++) {
    const float sc = bn ? bn->scale[n0 + n] : 1.f, sh = bn ? bn->shift[n0 + n] : 0.f;
    const int row = row_of ? (*row_of)[n] : n;
    for (int k = 0; k < K; k++) f.w[(size_t)row * K + k] = w->data[(size_t)(n0 + n) * K + k] * sc;
    f.b[n] = (conv_bias ? conv_bias->data[n0 + n] : 0.f) * sc + sh;
  }
  return f;
}

std::vector<float> fold_dw(const PackTensor* wd, int C, int taps, const float* scale) {
  std::vector<float> out((size_t)taps * C);
  for (int c = 0; c < C; c++)
    for (int t = 0; t < taps; t++) out[(size_t)t * C + c] = scale ? wd->data[(size_t)c * taps + t] * scale[c] : wd->data[(size_t)c * taps + t];
  return out;
}

}  // namespace hep
