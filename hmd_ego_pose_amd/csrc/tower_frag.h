// tower_frag.h - the head towers' depthwise accumulation over one MFMA operand fragment (k_tower.hip, and k_heads.hip of the
// alternative build): Frag (hep_dev.h) plus the accumulator that becomes the fragment.
// bf16: the even channels of two packed words are unpacked with one shift each, the odd ones with one mask each, and every pair
// feeds one v_pk_fma_f32 - so the accumulators (and the depthwise weights in LDS, see `swz`) are kept in the order 0,2,1,3 | 4,6,5,7.
#pragma once
#include "hep_dev.h"

template <bool BF16> struct TowerFrag;
template <> struct TowerFrag<true> : Frag<true> {
  struct Acc { f32x2_t a[4]; };      // channels (0,2) (1,3) (4,6) (5,7)
  static __device__ __forceinline__ f32x4 swz(f32x4 w) { return (f32x4){w[0], w[2], w[1], w[3]}; }
  static __device__ __forceinline__ void zero(Acc& c) { for (int i = 0; i < 4; i++) c.a[i] = (f32x2_t){0.f, 0.f}; }
  static __device__ __forceinline__ void fma_tap_r(Acc& c, const raw& x, const f32x4& wa, const f32x4& wb) {   // weights in registers (swizzled)
    const f32x2_t e0 = {__uint_as_float(x[0] << 16), __uint_as_float(x[1] << 16)}, o0 = {__uint_as_float(x[0] & 0xffff0000u), __uint_as_float(x[1] & 0xffff0000u)};
    const f32x2_t e1 = {__uint_as_float(x[2] << 16), __uint_as_float(x[3] << 16)}, o1 = {__uint_as_float(x[2] & 0xffff0000u), __uint_as_float(x[3] & 0xffff0000u)};
    c.a[0] = __builtin_elementwise_fma(e0, (f32x2_t){wa[0], wa[1]}, c.a[0]);
    c.a[1] = __builtin_elementwise_fma(o0, (f32x2_t){wa[2], wa[3]}, c.a[1]);
    c.a[2] = __builtin_elementwise_fma(e1, (f32x2_t){wb[0], wb[1]}, c.a[2]);
    c.a[3] = __builtin_elementwise_fma(o1, (f32x2_t){wb[2], wb[3]}, c.a[3]);
  }
  static __device__ __forceinline__ void fma_tap(Acc& c, const raw& x, const float* w /* 8 swizzled weights in LDS */) {
    fma_tap_r(c, x, reinterpret_cast<const f32x4*>(w)[0], reinterpret_cast<const f32x4*>(w)[1]);
  }
  static __device__ __forceinline__ raw pack(const Acc& c) {
    return (raw){pack_bf16x2(c.a[0][0], c.a[1][0]), pack_bf16x2(c.a[0][1], c.a[1][1]), pack_bf16x2(c.a[2][0], c.a[3][0]), pack_bf16x2(c.a[2][1], c.a[3][1])};
  }
};
template <> struct TowerFrag<false> : Frag<false> {
  struct Acc { f32x4 a; };
  static __device__ __forceinline__ f32x4 swz(f32x4 w) { return w; }
  static __device__ __forceinline__ void zero(Acc& c) { c.a = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ void fma_tap(Acc& c, const raw& x, const float* w) {
    c.a = __builtin_elementwise_fma(x, *reinterpret_cast<const f32x4*>(w), c.a);
  }
  static __device__ __forceinline__ void fma_tap_r(Acc& c, const raw& x, const f32x4& wa, const f32x4&) { c.a = __builtin_elementwise_fma(x, wa, c.a); }
  static __device__ __forceinline__ raw pack(const Acc& c) { return c.a; }
};
