// mifwt_level_tile.h — what the fused-level units share, once: mifwt_per.hip (periodization), mifwt_ext.hip (value-map extensions),
// mifwt_cplx.hip (interleaved complex) and mifwt_bwt.hip (boundary wavelets, with mifwt_bwt3.hip and mifwt_bwt_tree.hip through
// mifwt_bwt_rows.h).  Each of them is a fused level on an LDS tile with a run-time-tap axis pass as the fallback, and each has
//   device: 16-byte vectors of T, the row pass over an aligned window of a staged row, one tap of the column pass over two row-filtered
//           LDS planes and the four band stores of a 2-D analysis tile;
//   host:   the kernel arguments every family carries (LevelArgs, AxisArgsBase) and how a descriptor fills them, the tile cut, the
//           descriptor checks every family makes before and after its own extent rule, the filter-length dispatch, and the packing of
//           the extern "C" level entries.
// A family keeps what is its own: the index / value map of its extension, the staging of its window, its tile geometry, every synthesis /
// adjoint kernel, and the kernel launches.  Nothing here asks which family calls: the pieces take types, compile-time constants and
// plain values.
#pragma once
#include <type_traits>

#include "mifwt_common.h"

namespace mifwt {

namespace {

// ---- 16 bytes of T -----------------------------------------------------------------------------------------------------------------------------
template <typename T>
struct Vec16;
template <>
struct Vec16<float> {
  static constexpr int E = 4;
  typedef float type __attribute__((ext_vector_type(4)));
};
template <>
struct Vec16<double> {
  static constexpr int E = 2;
  typedef double type __attribute__((ext_vector_type(2)));
};

constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// E values from `valid` on: one 16-byte store, or element stores
template <typename T>
__device__ __forceinline__ void store_vec(T* p, const typename Vec16<T>::type& v, int valid, bool vec_ok) {
  constexpr int E = Vec16<T>::E;
  if (vec_ok && valid >= E) {
    *reinterpret_cast<typename Vec16<T>::type*>(p) = v;
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (e < valid) p[e] = v[e];
  }
}

// ---- kernel arguments of a fused level -----------------------------------------------------------------------------------------------------------
// A family derives its own struct from this one and adds only its own fields.  For complex data T is the component type and every
// stride and extent counts COMPLEX elements.
template <typename T, int L>
struct LevelArgs {
  const void* in[4];  // analysis: in[0] = x;  synthesis / adjoint: the 2^ndim bands
  void* out[4];       // analysis: the bands;  synthesis / adjoint: out[0] = y
  int64_t sig_bs, sig_rs;          // signal side: batch / row stride (elements; samples contiguous).  1-D: rows = batch, sig_rs unused
  int64_t a_bs, a_rs, d_bs, d_rs;  // band 0 / bands 1..: batch / row strides
  int n_r, n_c;                    // signal extents (1-D: n_r = 1)
  int m_r, m_c;                    // coefficient extents
  int sig_vec, coef_vec;           // 16-byte accesses allowed on the signal / coefficient side
  int tiles_c, tiles_r;
  T lo[L], hi[L];                  // the two filters, PyWavelets order, as the family's kernels take them
};

// The common part from a descriptor.  `e` = elements per 16 bytes: a side takes 16-byte accesses when its base pointers are 16-byte
// aligned and its batch / row strides are multiples of `e`.
template <typename T, int L>
void fill_level_args(LevelArgs<T, L>& a, const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo,
                     const double* hi, int e) {
  const int nd = d->ndim, nb = 1 << nd;
  for (int s = 0; s < 4; ++s) {
    a.in[s] = nullptr;
    a.out[s] = nullptr;
  }
  for (int s = 0; s < (inverse ? nb : 1); ++s) a.in[s] = in[s];
  for (int s = 0; s < (inverse ? 1 : nb); ++s) a.out[s] = out[s];
  a.sig_bs = d->sig_stride[0];
  a.a_bs = d->approx_stride[0];
  a.d_bs = d->detail_stride[0];
  a.sig_rs = nd == 2 ? d->sig_stride[1] : 0;
  a.a_rs = nd == 2 ? d->approx_stride[1] : 0;
  a.d_rs = nd == 2 ? d->detail_stride[1] : 0;
  a.n_r = nd == 2 ? (int)d->sig_extent[0] : 1;
  a.m_r = nd == 2 ? (int)d->coef_extent[0] : 1;
  a.n_c = (int)d->sig_extent[nd - 1];
  a.m_c = (int)d->coef_extent[nd - 1];
  const void* sig = inverse ? out[0] : in[0];
  a.sig_vec = aligned16(sig) && a.sig_bs % e == 0 && a.sig_rs % e == 0;
  a.coef_vec = a.a_bs % e == 0 && a.d_bs % e == 0 && a.a_rs % e == 0 && a.d_rs % e == 0;
  for (int s = 0; s < nb; ++s) a.coef_vec = a.coef_vec && aligned16(inverse ? in[s] : (const void*)out[s]);
  for (int t = 0; t < L; ++t) {
    a.lo[t] = (T)lo[t];
    a.hi[t] = (T)hi[t];
  }
}

// Tiles of tile_w x tile_h over ext_c x ext_r outputs (a 1-D level has ext_r = 1: one row of tiles): the grid, or -1 beyond INT32_MAX
template <typename T, int L>
int64_t cut_tiles(LevelArgs<T, L>& a, int ext_c, int ext_r, int tile_w, int tile_h, int64_t batch) {
  a.tiles_c = (ext_c + tile_w - 1) / tile_w;
  a.tiles_r = (ext_r + tile_h - 1) / tile_h;
  const int64_t grid = (int64_t)a.tiles_c * a.tiles_r * batch;
  return grid > INT32_MAX ? -1 : grid;
}

// ---- the row pass over an aligned window ---------------------------------------------------------------------------------------------------------
// Output k of a row reads the L samples 2 k - H .. 2 k - H + L - 1 (H = the left reach of the family's window).  A staged row keeps PAD
// samples left of sample 2 * (first output of the tile), so that the window of E outputs starts OFF samples into a 16-byte aligned run
// of NV 16-byte pieces.
template <typename T, int L, int H>
struct RowWindow {
  static constexpr int E = Vec16<T>::E;
  static constexpr int PAD = round_up(H, E);          // staged columns left of sample 2 mc0 (keeps the staged vectors aligned)
  static constexpr int OFF = PAD - H;                 // window of output 0 starts at staged column OFF
  static constexpr int NV = (OFF + 2 * E + L - 2 + E - 1) / E;  // 16-byte pieces of the window of E outputs
};

// E consecutive outputs of both filters from a staged row; `p` = 16-byte aligned LDS address PAD samples left of sample 2 * (first output)
template <typename T, int L, int H>
__device__ __forceinline__ void window_run(const T* p, const T (&flo)[L], const T (&fhi)[L], typename Vec16<T>::type& lo,
                                           typename Vec16<T>::type& hi) {
  typedef RowWindow<T, L, H> W;
  typedef typename Vec16<T>::type V;
  constexpr int E = W::E, OFF = W::OFF, NV = W::NV;
  T w[NV * E];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const V v = *reinterpret_cast<const V*>(p + i * E);
#pragma unroll
    for (int e = 0; e < E; ++e) w[i * E + e] = v[e];
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    T sl = T(0), sh = T(0);
#pragma unroll
    for (int k = 0; k < L; ++k) {
      sl = fma(flo[L - 1 - k], w[OFF + 2 * e + k], sl);
      sh = fma(fhi[L - 1 - k], w[OFF + 2 * e + k], sh);
    }
    lo[e] = sl;
    hi[e] = sh;
  }
}

// ---- the column pass of a 2-D analysis tile --------------------------------------------------------------------------------------------------------
// One tap of the column pass: E columns of one window row of the two row-filtered planes into the four bands.  The loop over the L window
// rows stays in the kernel: as part of a device function it is unrolled before that function is inlined, every access to the kernel's
// arguments then has a constant offset before the kernel is optimised, the compiler loads all of them at kernel entry instead of at
// their uses, and the 2-D analysis kernels of the long filters spill scalar registers (EXPERIMENTS).
template <typename T>
__device__ __forceinline__ void column_tap(const T* lo_row, const T* hi_row, const T& tap_lo, const T& tap_hi, typename Vec16<T>::type& ll,
                                           typename Vec16<T>::type& lh, typename Vec16<T>::type& hl, typename Vec16<T>::type& hh) {
  typedef typename Vec16<T>::type V;
  const V vl = *reinterpret_cast<const V*>(lo_row);
  const V vh = *reinterpret_cast<const V*>(hi_row);
  const T cl = tap_lo, ch = tap_hi;  // (read after the rows, as the kernels always did: the instruction streams stay as they were)
  ll += cl * vl;
  lh += cl * vh;
  hl += ch * vl;
  hh += ch * vh;
}

// E columns of the four bands of coefficient row m, from column mc on, of image b
template <typename T, int L>
__device__ __forceinline__ void store_bands(const LevelArgs<T, L>& a, int b, int m, int mc, const typename Vec16<T>::type& ll,
                                            const typename Vec16<T>::type& lh, const typename Vec16<T>::type& hl,
                                            const typename Vec16<T>::type& hh) {
  const int valid = a.m_c - mc;
  const int64_t oa = (int64_t)b * a.a_bs + (int64_t)m * a.a_rs + mc;
  const int64_t od = (int64_t)b * a.d_bs + (int64_t)m * a.d_rs + mc;
  store_vec<T>(static_cast<T*>(a.out[0]) + oa, ll, valid, a.coef_vec);
  store_vec<T>(static_cast<T*>(a.out[1]) + od, lh, valid, a.coef_vec);
  store_vec<T>(static_cast<T*>(a.out[2]) + od, hl, valid, a.coef_vec);
  store_vec<T>(static_cast<T*>(a.out[3]) + od, hh, valid, a.coef_vec);
}

// ---- descriptor checks -------------------------------------------------------------------------------------------------------------------------
// What every family refuses as inconsistent before it looks at its own extent rule: 0 = go on, MIFWT_ERR_BADARG.  The 16-bit storage
// types pass: a family answers for them itself (outside the fused envelope, or unsupported).
int desc_prelude(const mifwt_level_desc* d) {
  if (!d) return MIFWT_ERR_BADARG;
  if (d->ndim < 1 || d->ndim > MIFWT_MAX_NDIM || d->filt_len < 2 || d->filt_len > MIFWT_MAX_FILT || (d->filt_len & 1) || d->batch < 0)
    return MIFWT_ERR_BADARG;
  if (d->dtype != MIFWT_F32 && d->dtype != MIFWT_F64 && !is_storage16(d->dtype)) return MIFWT_ERR_BADARG;
  return 0;
}

// The envelope of the fused kernels for a consistent descriptor: 1 = served, 0 = not served (the axis passes take it)
int fused_envelope(const mifwt_level_desc* d) {
  if (d->ndim > 2 || d->filt_len > 20 || (d->dtype != MIFWT_F32 && d->dtype != MIFWT_F64)) return 0;
  const int last = d->ndim;
  if (d->sig_stride[last] != 1 || d->approx_stride[last] != 1 || d->detail_stride[last] != 1) return 0;
  int64_t tiles = d->batch;
  for (int ax = 0; ax < d->ndim; ++ax) {
    if (d->coef_extent[ax] > (1 << 29)) return 0;
    tiles *= (d->coef_extent[ax] + 7) / 8;  // (more tiles than any family cuts in either direction)
  }
  if (tiles > INT32_MAX) return 0;
  return 1;
}

// The pointers of a level call whose descriptor passed the family's check (`ok` >= 0): taps, every band, the signal
int level_pointers(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi) {
  if (!lo || !hi) return MIFWT_ERR_BADARG;
  for (int s = 0; s < (1 << (d->ndim > 2 ? 0 : d->ndim)); ++s)
    if (!(inverse ? in[s] : (const void*)out[s])) return MIFWT_ERR_BADARG;
  if (!(inverse ? (const void*)out[0] : in[0])) return MIFWT_ERR_BADARG;
  return 0;
}

// ---- one instantiation per even filter length 2 .. 20 ------------------------------------------------------------------------------------------
// f(std::integral_constant<int, LEN>()) for the length at hand; any other length is not served
template <typename F>
int for_even_len(int filt_len, F&& f) {
  switch (filt_len) {
#define MIFWT_LEN_CASE(LEN) \
  case LEN: return f(std::integral_constant<int, LEN>());
    MIFWT_LEN_CASE(2)
    MIFWT_LEN_CASE(4)
    MIFWT_LEN_CASE(6)
    MIFWT_LEN_CASE(8)
    MIFWT_LEN_CASE(10)
    MIFWT_LEN_CASE(12)
    MIFWT_LEN_CASE(14)
    MIFWT_LEN_CASE(16)
    MIFWT_LEN_CASE(18)
    MIFWT_LEN_CASE(20)
#undef MIFWT_LEN_CASE
    default: return MIFWT_ERR_UNSUPPORTED;
  }
}

// ---- the extern "C" level entries -----------------------------------------------------------------------------------------------------------------
// The band side of an entry, (first, rest[]) -> slots[4]: P = void* (analysis writes the bands) or const void* (synthesis reads them).
// A level of more than two axes has no fused kernel and carries no details here.
template <typename P>
int pack_bands(const mifwt_level_desc* desc, P first, const P* rest, P (&slots)[4]) {
  if (!desc || desc->ndim < 1 || desc->ndim > MIFWT_MAX_NDIM) return MIFWT_ERR_BADARG;
  if (desc->ndim <= 2 && !rest) return MIFWT_ERR_BADARG;
  slots[0] = first;
  slots[1] = slots[2] = slots[3] = nullptr;
  if (desc->ndim <= 2)
    for (int s = 1; s < (1 << desc->ndim); ++s) slots[s] = rest[s - 1];
  return 0;
}

// *_kernel_id from the answer of *_supported
int kernel_id_answer(int supported, int direction, int fwd_id, int inv_id) {
  if (supported < 0) return supported;
  return supported ? (direction ? inv_id : fwd_id) : MIFWT_ERR_UNSUPPORTED;
}

// ---- one axis of [outer, n, inner] arrays: any even L <= MIFWT_MAX_FILT, any strides -----------------------------------------------------------
struct AxisArgsBase {
  const void* in0;  // analysis: x       synthesis / adjoint: lo
  const void* in1;  //                   synthesis / adjoint: hi
  void* out0;       // analysis: lo      synthesis / adjoint: y
  void* out1;       // analysis: hi
  int64_t sig_s[3], lo_s[3], hi_s[3];  // (outer, axis, inner) strides in elements
  int64_t outer, inner;
  int n, m, filt_len;
  double lo[MIFWT_MAX_FILT], hi[MIFWT_MAX_FILT];
};

// The arguments of an axis entry: MIFWT_ERR_BADARG (a null pointer, a length or extent out of range), then the answer for the data type
// (the 16-bit storage types are not served), 0 = go on
int axis_check(int inverse, int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* in0, const void* in1,
               const void* out0, const void* out1, const int64_t* sig_s, const int64_t* lo_s, const int64_t* hi_s, const double* lo,
               const double* hi) {
  if (!in0 || !out0 || (inverse ? !in1 : !out1) || !sig_s || !lo_s || !hi_s || !lo || !hi) return MIFWT_ERR_BADARG;
  if (filt_len < 2 || (filt_len & 1) || filt_len > MIFWT_MAX_FILT || outer < 0 || inner < 0 || n < 1) return MIFWT_ERR_BADARG;
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return is_storage16(dtype) ? MIFWT_ERR_UNSUPPORTED : MIFWT_ERR_BADARG;
  return 0;
}

// Fills the common part for an axis of n samples and m coefficients (the family's rule); `lo` / `hi` as its kernel takes them.
// MIFWT_ERR_UNSUPPORTED for an axis beyond the int index arithmetic of the kernels.
int fill_axis_args(AxisArgsBase& a, int filt_len, int64_t outer, int64_t n, int64_t m, int64_t inner, const void* in0, const void* in1,
                   void* out0, void* out1, const int64_t* sig_s, const int64_t* lo_s, const int64_t* hi_s, const double* lo,
                   const double* hi) {
  if (n > INT32_MAX / 4) return MIFWT_ERR_UNSUPPORTED;
  a.in0 = in0;
  a.in1 = in1;
  a.out0 = out0;
  a.out1 = out1;
  for (int i = 0; i < 3; ++i) {
    a.sig_s[i] = sig_s[i];
    a.lo_s[i] = lo_s[i];
    a.hi_s[i] = hi_s[i];
  }
  a.outer = outer;
  a.inner = inner;
  a.n = (int)n;
  a.m = (int)m;
  a.filt_len = filt_len;
  for (int t = 0; t < MIFWT_MAX_FILT; ++t) {
    a.lo[t] = t < filt_len ? lo[t] : 0.0;
    a.hi[t] = t < filt_len ? hi[t] : 0.0;
  }
  return 0;
}

// One thread per output, at most `grid_cap` workgroups of 256 (the kernels stride over the rest): the kernel of (dtype, direction)
template <typename Args>
int launch_axis(int dtype, int inverse, int64_t total, int grid_cap, void* stream, const Args& a, void (*f32_fwd)(const Args),
                void (*f32_inv)(const Args), void (*f64_fwd)(const Args), void (*f64_inv)(const Args)) {
  const int64_t blocks = (total + 255) / 256;
  const dim3 g((unsigned)(blocks < grid_cap ? blocks : grid_cap)), blk(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  void (*kernel)(const Args) = dtype == MIFWT_F32 ? (inverse ? f32_inv : f32_fwd) : (inverse ? f64_inv : f64_fwd);
  hipLaunchKernelGGL(kernel, g, blk, 0, st, a);
  return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
}

}  // namespace

}  // namespace mifwt
