// mifwt_mfma_elem.h — what the matrix-core kernels (mifwt_dwt2_fwd_mfma.h, mifwt_dwt2_inv_mfma.h) need to know of their 16-bit storage
// type H: the 8- and 4-wide vectors and the 32x32x16 MFMA with f32 accumulation.  Conversions are plain casts: (H)float rounds to nearest
// even in hardware for both types (v_cvt_f16_f32 / v_cvt_pk_bf16_f32), (float)H is exact.
//
// Taps enter as PAIRS t = t_hi + t_lo of H with t_hi = (H)t, t_lo = (H)(t - t_hi), two MFMAs per K-step:
//   _Float16 (11 significant bits): |t - t_hi - t_lo| <= 2^-24 absolutely (the low half of a small tap is a subnormal), DESIGN.md 4.9;
//   __bf16   ( 8 significant bits, unit roundoff 2^-8): r = t - t_hi is exact in f32 with |r| <= 2^-8 |t|, and |r - t_lo| <= 2^-8 |r|, so
//            |t - t_hi - t_lo| <= 2^-16 |t| (no subnormals in reach: bf16 has f32's exponent range) — 1/256 of the output's unit
//            roundoff, DESIGN.md 4.17.
// Products of two H values are exact in f32 (22 / 16 significant bits).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mifwt {

typedef float f16x __attribute__((ext_vector_type(16)));

template <typename H>
struct MfmaElem;
template <>
struct MfmaElem<_Float16> {
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  typedef _Float16 v4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ f16x mfma(v8 a, v8 b, f16x c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <>
struct MfmaElem<__bf16> {
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  typedef __bf16 v4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ f16x mfma(v8 a, v8 b, f16x c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

}  // namespace mifwt
