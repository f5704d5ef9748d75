// mifwt_bands.h — what the kernels that read coefficient BANDS share (mifwt_estim.hip, ids 50 .. 53; mifwt_select.hip, ids 54 / 55;
// mifwt_compact.hip, ids 56 .. 58).
//
// A BAND is one strided tensor in the collapsed form of mifwt_thresh.hip: extent[0] x extent[1] rows of extent[2] contiguous elements,
// the rows addressed through two element strides; `rows_per_index` consecutive rows form one IMAGE (one leading index).  A row is cut
// into SLOTS of 16 bytes: slot s covers columns [s VEC - a, s VEC - a + VEC) clipped to the row, a the misalignment of the row's first
// element, so every slot that lies inside its row is one aligned 16-byte load and the others are peeled element by element.  Nothing is
// read outside a row.
//
// The KEY of an element is its bit pattern with the sign cleared: for non-negative IEEE numbers unsigned order is value order, so a
// radix selection on the keys finds an exact order statistic of |x|, the bits a sort gives.
#pragma once
#include <vector>

#include "mifwt_common.h"

namespace mifwt {
namespace bands {

constexpr int kMaxSeg = 24;
constexpr int kThreads = 256;
constexpr int kLdsKeyBytes = 48 * 1024;  // keys of one image in LDS: with the histograms 50 KB, three workgroups per CU
constexpr int kLdsBins = 256;            // 8-bit digits in LDS
constexpr int kStreamBits = 11;          // widest digit of the streaming passes
constexpr int kStreamBins = 1 << kStreamBits;
constexpr uint32_t kSlotsPerWg = kThreads * 16;  // streaming: slots a workgroup takes at least
constexpr uint32_t kMaxWgs = 4096;               // streaming: workgroups per pass, about

template <typename C>
struct KeyOf;
template <>
struct KeyOf<float> {
  typedef uint32_t type;
  static constexpr int bits = 31;
};
template <>
struct KeyOf<double> {
  typedef uint64_t type;
  static constexpr int bits = 63;
};

template <typename C>
__device__ __forceinline__ typename KeyOf<C>::type key_of(C v) {
  typedef typename KeyOf<C>::type K;
  return __builtin_bit_cast(K, v) & ~(K(1) << KeyOf<C>::bits);
}

// the digit of streaming pass `pass`: T bits in P = ceil(T / 11) passes from the top, the first T % P passes one bit wider
__host__ __device__ __forceinline__ void stream_plan(int total_bits, int pass, int* shift, int* width) {
  const int passes = (total_bits + kStreamBits - 1) / kStreamBits;
  const int base = total_bits / passes, extra = total_bits % passes;
  int used = 0;
  for (int p = 0; p < pass; ++p) used += base + (p < extra ? 1 : 0);
  *width = base + (pass < extra ? 1 : 0);
  *shift = total_bits - used - *width;
}
__host__ __device__ __forceinline__ int stream_passes(int total_bits) { return (total_bits + kStreamBits - 1) / kStreamBits; }

struct Band {
  const char* x;
  int64_t s0, s1;  // element strides of the two outer extents
  uint32_t n;      // elements per row
  uint32_t e1;     // inner one of the two outer extents: row = i0 * e1 + i1
  uint32_t vpr;    // slots per row
  uint32_t rp;     // rows per image
};

template <typename C>
struct alignas(16) Vec16 {
  C c[16 / sizeof(C)];
};

// slot `sl` of row `row`: f(position of the element in its row, value) for every element of the slot
template <typename C, typename F>
__device__ __forceinline__ void visit_slot(const Band& b, uint32_t row, uint32_t sl, F&& f) {
  constexpr int VEC = 16 / sizeof(C);
  const int64_t i0 = b.e1 == 1 ? row : row / b.e1, i1 = b.e1 == 1 ? 0 : row - (row / b.e1) * b.e1;
  const C* px = reinterpret_cast<const C*>(b.x) + (i0 * b.s0 + i1 * b.s1);
  const int64_t a = (int64_t)(((uintptr_t)px & 15) / sizeof(C));
  const int64_t c0 = (int64_t)sl * VEC - a;  // (column c0 of the row is 16-byte aligned)
  if (c0 >= 0 && c0 + VEC <= (int64_t)b.n) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const Vec16<C> v = __builtin_bit_cast(Vec16<C>, *reinterpret_cast<const u4*>(px + c0));
#pragma unroll
    for (int j = 0; j < VEC; ++j) f((uint32_t)(c0 + j), v.c[j]);
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int64_t c = c0 + j;
      if (c >= 0 && c < (int64_t)b.n) f((uint32_t)c, px[c]);
    }
  }
}

// where a per-image count k comes from: the number itself, or device memory read when the kernel runs
struct KSource {
  int64_t k;
  const int64_t* dk;  // NULL: k
  int64_t stride;     // 0: dk[0] for every image
};

// k of image g, clipped to [0, n]
__device__ __forceinline__ uint32_t k_of(const KSource& s, uint32_t g, uint32_t n) {
  int64_t k = s.dk ? s.dk[(int64_t)g * s.stride] : s.k;
  k = k < 0 ? 0 : k;
  return k > (int64_t)n ? n : (uint32_t)k;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct Geo {
  Band b;
  uint64_t images, count;  // count: elements per image
};

inline int band_geometry(int dtype, const mifwt_estim_band& s, Geo* o) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return MIFWT_ERR_BADARG;
  const int64_t e0 = s.extent[0], e1 = s.extent[1], n = s.extent[2];
  if (e0 < 0 || e1 < 0 || n < 0 || s.rows_per_index < 0) return MIFWT_ERR_BADARG;
  if (n > 1 && s.stride[2] != 1) return MIFWT_ERR_BADARG;
  Geo g = {};
  if (e0 == 0 || e1 == 0 || n == 0) {
    *o = g;
    return MIFWT_OK;
  }
  if (n > (int64_t)1 << 30 || e1 > (int64_t)1 << 30 || (double)e0 * (double)e1 >= 2147483648.0) return MIFWT_ERR_UNSUPPORTED;
  const uint64_t rows = (uint64_t)e0 * (uint64_t)e1;
  const uint64_t rp = s.rows_per_index ? (uint64_t)s.rows_per_index : rows;
  if (rows % rp != 0) return MIFWT_ERR_BADARG;
  if ((double)rp * (double)n >= 2147483648.0) return MIFWT_ERR_UNSUPPORTED;  // fewer than 2^31 elements per image
  const int vec = dtype == MIFWT_F64 ? 2 : 4;
  g.b.x = static_cast<const char*>(s.x);
  g.b.s0 = s.stride[0], g.b.s1 = s.stride[1];
  g.b.n = (uint32_t)n, g.b.e1 = (uint32_t)e1, g.b.rp = (uint32_t)rp;
  g.b.vpr = (uint32_t)((n + 2 * (int64_t)vec - 2) / vec);  // (at most n: slots per image stay below 2^31)
  g.images = rows / rp;
  g.count = rp * (uint64_t)n;
  *o = g;
  return MIFWT_OK;
}

// the non-empty segments of a container whose bands share their images, one multiset per image
struct Pool {
  std::vector<Geo> segs;  // the non-empty segments
  uint64_t count = 0;     // pooled elements per image
};

// the non-empty segments of a container and their pooled count; MIFWT_OK or an error code
inline int pool_of(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, Pool* p) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return MIFWT_ERR_BADARG;
  if (nseg < 0 || (nseg > 0 && segs == nullptr) || images < 0 || images >= 2147483648ll) return MIFWT_ERR_BADARG;
  for (int i = 0; i < nseg; ++i) {
    Geo g;
    const int rc = band_geometry(dtype, segs[i], &g);
    if (rc != MIFWT_OK) return rc;
    if (g.count == 0) continue;
    if (g.images != (uint64_t)images) return MIFWT_ERR_BADARG;
    p->count += g.count;
    if (p->count >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;  // fewer than 2^31 pooled elements per image
    p->segs.push_back(g);
  }
  return MIFWT_OK;
}

// streaming: how a segment's slots are cut into units (chunks), one workgroup each: units per image, slots per unit
inline void unit_plan(const Geo& g, uint64_t images, uint64_t* slots, uint64_t* wpi, uint64_t* spw) {
  uint64_t per_image = kMaxWgs / images;
  if (per_image < 1) per_image = 1;
  *slots = (uint64_t)g.b.rp * g.b.vpr;
  uint64_t w = (*slots + kSlotsPerWg - 1) / kSlotsPerWg;
  if (w > per_image) w = per_image;
  *spw = (*slots + w - 1) / w;
  *wpi = (*slots + *spw - 1) / *spw;
}

inline int lds_capacity(int dtype) { return kLdsKeyBytes / (dtype == MIFWT_F64 ? 8 : 4); }

}  // namespace bands
}  // namespace mifwt
