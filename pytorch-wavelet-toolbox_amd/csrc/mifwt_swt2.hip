// mifwt_swt2.hip — fused 2-D stationary (undecimated, "a trous") wavelet levels for gfx950: kernel ids 34 (analysis) / 35 (synthesis).
//
// A 2-D level is the 1-D level of mifwt_swt.hip along both axes of a plane (periodic, dilation D, any number of wraps):
//   analysis   p_lo/hi[r][n] = sum_t row_lo/hi[t] x[r][(n + D (L/2 - t)) mod W]                            (axis -1)
//              cA = s sum_m col_lo[m] p_lo[(r + D (L/2 - m)) mod H][n]     cH = s sum_m col_hi[m] p_lo[..][n]      (axis -2)
//              cV = s sum_m col_lo[m] p_hi[..][n]                          cD = s sum_m col_hi[m] p_hi[..][n]
//   synthesis  U[r][n] = sum_t row_lo[t] cA[r][(n + D (L/2 - 1 - t)) mod W] + row_hi[t] cV[r][..]          (axis -1)
//              V[r][n] = sum_t row_lo[t] cH[r][..]                         + row_hi[t] cD[r][..]
//              y[r][n] = s sum_m col_lo[m] U[(r + D (L/2 - 1 - m)) mod H][n] + col_hi[m] V[..][n]           (axis -2)
// (cH: high-pass along axis -2, low-pass along axis -1, as wavedec2 names its bands; s = 1 resp. 1/4 in the transform; with all four
// filters reversed and the same s each kernel is the other's adjoint).
//
// Bound: HBM — 1 plane in and 4 out (analysis), 4 in and 1 out (synthesis); one launch per level, no intermediate plane, no transpose.
// An LDS tile would need a halo of (L - 1) D samples on every side (112 for 8 taps at D = 16), so the kernel walks the a-trous LATTICE
// instead: output row r only needs the input rows (r + D k) mod H.  A wave owns one image, one row residue rho < min(D, H), a segment of
// the lattice rows rho + i D < H and a strip of 64 E columns (a lane: E consecutive columns).  For every new lattice row it does the
// axis -1 pass straight from global memory, as swt_kernel does (one vector load of the lane's run per tap, shifted by a multiple of D;
// the L-fold re-reads are served by the vector L1 / L2; lanes whose window wraps walk a wrapped index instead), and pushes the pair
// (p_lo, p_hi) resp. (U, V) into a ring of L row pairs held in REGISTERS.  The axis -2 pass combines the ring into one row of each
// output plane, stored with full-width vector stores.  Consecutive lattice rows share L - 1 ring rows, so a row is filtered along
// axis -1 once per strip and segment; a segment's warm-up reads the L - 1 (wrapped) lattice rows before its first one again, which
// costs (L - 1) / segment rows of extra reads — the host cuts segments only as far as the chip needs waves (swt2_plan).  Waves never
// talk to each other: no LDS, no barrier.  Row indices wrap with mod H for every H (H not a multiple of D, D >= H, H = 1): the lattice
// index j of a row is just an integer, the row is (rho + j D) mod H.
//
// LIMIT (mifwt_swt2_supported): the ring lives in registers with compile-time indices, so only the compile-time lengths exist — even
// L in 2 .. 20, float32 and float64.  Longer filters (db11+, sym11+, coif4+, dmey) and float16 answer 0 / MIFWT_ERR_UNSUPPORTED and the
// caller composes the level from mifwt_swt_fwd / mifwt_swt_inv.  A lane's run is E = 4 (f32) / 2 (f64) columns up to 10 taps and half
// of that above, which keeps the ring at 80 registers.
#include "mifwt_axis_stream.h"

namespace mifwt {

namespace {

constexpr int kSwt2MaxFused = 20;

template <typename T, int L>
struct Swt2Run {
  static constexpr int E = L <= 10 ? ElemTraits<T>::EO : ElemTraits<T>::EO / 2;
};

template <typename A, int L>
struct Swt2Args {
  const void* in[4];   // analysis: x, -, -, -          synthesis: cA, cH, cV, cD
  void* out[4];        // analysis: cA, cH, cV, cD      synthesis: y, -, -, -
  int64_t in_is[4], in_rs[4], out_is[4], out_rs[4];  // image / row strides (elements); samples are contiguous
  int H, W, D, nres, nsegs, nstrips, seglen;
  int64_t ntasks;
  A scale;
  A rlo[L], rhi[L], clo[L], chi[L];
};

// one tap of the axis -1 pass for element e: analysis (one plane) p_lo += lo x, p_hi += hi x; synthesis (planes cA, cH, cV, cD)
// U += lo cA + hi cV, V += lo cH + hi cD
template <typename A, int NIN, int E>
__device__ __forceinline__ void row_tap(A lo, A hi, const A (&v)[NIN][E], int e, A& p0, A& p1) {
  if constexpr (NIN == 4) {
    p0 = fma(lo, v[0][e], p0);
    p0 = fma(hi, v[2][e], p0);
    p1 = fma(lo, v[1][e], p1);
    p1 = fma(hi, v[3][e], p1);
  } else {
    p0 = fma(lo, v[0][e], p0);
    p1 = fma(hi, v[0][e], p1);
  }
}

template <typename T, int L, bool INVERSE>
__global__ void __launch_bounds__(256) swt2_kernel(const Swt2Args<typename ElemTraits<T>::Acc, L> a) {
  using A = typename ElemTraits<T>::Acc;
  constexpr int E = Swt2Run<T, L>::E;
  constexpr int NIN = INVERSE ? 4 : 1;
  constexpr int NOUT = INVERSE ? 1 : 4;
  constexpr int OFF = L / 2 - (INVERSE ? 1 : 0);  // newest lattice row of output row i: i + OFF (tap 0)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int64_t task = (int64_t)blockIdx.x * 4 + wave;
  if (task >= a.ntasks) return;
  const int strip = (int)(task % a.nstrips);
  task /= a.nstrips;
  const int seg = (int)(task % a.nsegs);
  task /= a.nsegs;
  const int res = (int)(task % a.nres);
  const int64_t img = task / a.nres;
  const int H = a.H, W = a.W, D = a.D;
  const int cnt = (H - res + D - 1) / D;  // rows res + i D < H
  const int i0 = seg * a.seglen;
  const int i1 = min(i0 + a.seglen, cnt);
  if (i0 >= i1) return;
  const int n0 = (strip * 64 + lane) * E;
  if (n0 >= W) return;  // (waves never synchronise: a lane may leave)

  // columns: tap t reads the run starting at n0 + off_max - D t
  const int off_max = D * OFF;
  const int off_min = off_max - D * (L - 1);
  const bool interior = n0 + off_min >= 0 && n0 + off_max + E <= W;
  const int Dw = D % W;
  int b0 = (n0 + off_max) % W;  // wrapped start of tap 0's run (n0 + off_max >= 0)
  const bool narrow = W < E;    // b + e may pass W more than once

  const T* __restrict__ pin[NIN];
#pragma unroll
  for (int q = 0; q < NIN; ++q) pin[q] = static_cast<const T*>(a.in[q]) + img * a.in_is[q];
  T* pout[NOUT];
#pragma unroll
  for (int q = 0; q < NOUT; ++q) pout[q] = static_cast<T*>(a.out[q]) + img * a.out_is[q] + n0;

  // rows: lattice index j -> row (res + j D) mod H, stepped without a division
  const int Dh = D % H;
  const int j0 = i0 + OFF - (L - 1);
  int64_t r64 = ((int64_t)res + (int64_t)j0 * D) % H;
  int row = (int)(r64 < 0 ? r64 + H : r64);

  A ring0[L][E], ring1[L][E];
#pragma unroll
  for (int k = 0; k < L; ++k)
#pragma unroll
    for (int e = 0; e < E; ++e) ring0[k][e] = ring1[k][e] = A(0);

  // ---- axis -2 pass of output row res + i D: tap m takes lattice row i + OFF - m = ring slot L - 1 - m (newest row: i + OFF)
  auto emit = [&](int i) {
    A o[NOUT][E];
#pragma unroll
    for (int q = 0; q < NOUT; ++q)
#pragma unroll
      for (int e = 0; e < E; ++e) o[q][e] = A(0);
#pragma unroll
    for (int m = 0; m < L; ++m)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (INVERSE) {
          o[0][e] = fma(a.clo[m], ring0[L - 1 - m][e], o[0][e]);
          o[0][e] = fma(a.chi[m], ring1[L - 1 - m][e], o[0][e]);
        } else {
          o[0][e] = fma(a.clo[m], ring0[L - 1 - m][e], o[0][e]);
          o[NOUT > 1 ? 1 : 0][e] = fma(a.chi[m], ring0[L - 1 - m][e], o[NOUT > 1 ? 1 : 0][e]);
          o[NOUT > 2 ? 2 : 0][e] = fma(a.clo[m], ring1[L - 1 - m][e], o[NOUT > 2 ? 2 : 0][e]);
          o[NOUT - 1][e] = fma(a.chi[m], ring1[L - 1 - m][e], o[NOUT - 1][e]);
        }
      }
    const int64_t orow = (int64_t)res + (int64_t)i * D;  // < H
#pragma unroll
    for (int q = 0; q < NOUT; ++q) {
#pragma unroll
      for (int e = 0; e < E; ++e) o[q][e] *= a.scale;
      T* op = pout[q] + orow * a.out_rs[q];
      if (n0 + E <= W) {
        store_run<T, A, E>(op, o[q]);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (n0 + e < W) op[e] = (T)o[q][e];
      }
    }
  };

  // Analysis is software-pipelined: the L loads of lattice row j are issued BEFORE the axis -2 pass and the four stores of the output
  // row that lattice row j - 1 completed, and consumed after them, so a wave's memory latency overlaps its own arithmetic (waves are
  // few: a ring of L row pairs per lane leaves three to four per SIMD).  Synthesis would have to hold 4 L runs; it keeps the plain order.
  constexpr bool PIPE = !INVERSE;
  const int jend = i1 - 1 + OFF;
  for (int j = j0; j <= jend; ++j) {
    int64_t roff[NIN];
#pragma unroll
    for (int q = 0; q < NIN; ++q) roff[q] = (int64_t)row * a.in_rs[q];
    A raw[PIPE ? L : 1][E];
    if (PIPE && interior) {
#pragma unroll
      for (int t = 0; t < L; ++t) load_run<T, A, E>(pin[0] + roff[0] + (n0 + off_max - D * t), raw[PIPE ? t : 0]);
    }
    if (PIPE && j - 1 - OFF >= i0) emit(j - 1 - OFF);
    // ---- axis -1 pass of lattice row j
    A p0[E], p1[E];
#pragma unroll
    for (int e = 0; e < E; ++e) p0[e] = p1[e] = A(0);
    if (interior) {
#pragma unroll
      for (int t = 0; t < L; ++t) {
        if (PIPE) {
#pragma unroll
          for (int e = 0; e < E; ++e) {
            p0[e] = fma(a.rlo[t], raw[PIPE ? t : 0][e], p0[e]);
            p1[e] = fma(a.rhi[t], raw[PIPE ? t : 0][e], p1[e]);
          }
        } else {
          const int s = n0 + off_max - D * t;
          A v[NIN][E];
#pragma unroll
          for (int q = 0; q < NIN; ++q) load_run<T, A, E>(pin[q] + roff[q] + s, v[q]);
#pragma unroll
          for (int e = 0; e < E; ++e) row_tap<A, NIN, E>(a.rlo[t], a.rhi[t], v, e, p0[e], p1[e]);
          // four planes per tap: left alone, the scheduler hoists all 4 L loads of a row (4 L E registers); a fence after every second
          // tap keeps 8 loads in flight per lane
          if (t & 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else {
      // the window wraps (or the run hangs over the row end): element by element along a wrapped index, taps in a run-time loop (few
      // lanes take this path; unrolled it would set the kernel's register count)
      int b = b0;
#pragma unroll 1
      for (int t = 0; t < L; ++t) {
        const A tl = a.rlo[t], th = a.rhi[t];
        A v[NIN][E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          int i = b + e;
          if (narrow)
            i %= W;
          else
            i -= i >= W ? W : 0;
#pragma unroll
          for (int q = 0; q < NIN; ++q) v[q][e] = (A)pin[q][roff[q] + i];
        }
#pragma unroll
        for (int e = 0; e < E; ++e) row_tap<A, NIN, E>(tl, th, v, e, p0[e], p1[e]);
        b -= Dw;
        b += b < 0 ? W : 0;
      }
    }
    // ---- push into the ring (compile-time slots: the ring is shifted, not indexed)
#pragma unroll
    for (int k = 0; k + 1 < L; ++k)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        ring0[k][e] = ring0[k + 1][e];
        ring1[k][e] = ring1[k + 1][e];
      }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      ring0[L - 1][e] = p0[e];
      ring1[L - 1][e] = p1[e];
    }
    row += Dh;
    row -= row >= H ? H : 0;
    if (!PIPE && j - OFF >= i0) emit(j - OFF);
  }
  if (PIPE) emit(jend - OFF);
}

struct Swt2Call {
  int inverse, filt_len;
  int64_t images, H, W, dilation;
  const void* in[4];
  void* out[4];
  int64_t in_is[4], in_rs[4], out_is[4], out_rs[4];
  const double* taps[4];  // row_lo, row_hi, col_lo, col_hi
  double scale;
  hipStream_t stream;
};

// Work split of a launch: a wave per (image, row residue, lattice segment, column strip).  Segments are cut only until the launch has
// about 16 waves per CU, and never shorter than 4 L lattice rows (warm-up re-reads <= 25 %); MIFWT_OPT_ROWS_PER_CHUNK overrides.
template <typename T, int L>
void swt2_plan(const Swt2Call& c, int& nres, int& nsegs, int& nstrips, int& seglen) {
  constexpr int E = Swt2Run<T, L>::E;
  const int64_t H = c.H, D = c.dilation;
  nres = (int)(D < H ? D : H);
  const int64_t maxcnt = (H + D - 1) / D;
  nstrips = (int)((c.W + 64 * E - 1) / (64 * E));
  const int64_t base = c.images * nres * nstrips;
  const int64_t want = (4096 + base - 1) / (base > 0 ? base : 1);
  int64_t len = (maxcnt + want - 1) / (want > 0 ? want : 1);
  if (len < 4 * L) len = 4 * L;
  if (g_options[MIFWT_OPT_ROWS_PER_CHUNK] > 0) len = g_options[MIFWT_OPT_ROWS_PER_CHUNK];
  if (len > maxcnt) len = maxcnt;
  seglen = (int)len;
  nsegs = (int)((maxcnt + len - 1) / len);
}

template <typename T, int L>
int swt2_launch(const Swt2Call& c) {
  using A = typename ElemTraits<T>::Acc;
  Swt2Args<A, L> a;
  for (int q = 0; q < 4; ++q) {
    a.in[q] = c.in[q];
    a.out[q] = c.out[q];
    a.in_is[q] = c.in_is[q];
    a.in_rs[q] = c.in_rs[q];
    a.out_is[q] = c.out_is[q];
    a.out_rs[q] = c.out_rs[q];
  }
  a.H = (int)c.H;
  a.W = (int)c.W;
  a.D = (int)c.dilation;
  swt2_plan<T, L>(c, a.nres, a.nsegs, a.nstrips, a.seglen);
  a.ntasks = c.images * a.nres * a.nsegs * a.nstrips;
  a.scale = (A)c.scale;
  for (int t = 0; t < L; ++t) {
    a.rlo[t] = (A)c.taps[0][t];
    a.rhi[t] = (A)c.taps[1][t];
    a.clo[t] = (A)c.taps[2][t];
    a.chi[t] = (A)c.taps[3][t];
  }
  if (a.ntasks == 0) return MIFWT_OK;
  const int64_t nblk = (a.ntasks + 3) / 4;
  if (nblk > INT32_MAX) return MIFWT_ERR_UNSUPPORTED;
  if (c.inverse)
    hipLaunchKernelGGL((swt2_kernel<T, L, true>), dim3((unsigned)nblk), dim3(256), 0, c.stream, a);
  else
    hipLaunchKernelGGL((swt2_kernel<T, L, false>), dim3((unsigned)nblk), dim3(256), 0, c.stream, a);
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  count_launch(c.inverse ? MIFWT_KERNEL_SWT2_INV : MIFWT_KERNEL_SWT2_FWD);
  return MIFWT_OK;
}

template <typename T>
int swt2_dispatch(const Swt2Call& c) {
  switch (c.filt_len) {
    case 2: return swt2_launch<T, 2>(c);
    case 4: return swt2_launch<T, 4>(c);
    case 6: return swt2_launch<T, 6>(c);
    case 8: return swt2_launch<T, 8>(c);
    case 10: return swt2_launch<T, 10>(c);
    case 12: return swt2_launch<T, 12>(c);
    case 14: return swt2_launch<T, 14>(c);
    case 16: return swt2_launch<T, 16>(c);
    case 18: return swt2_launch<T, 18>(c);
    case 20: return swt2_launch<T, 20>(c);
    default: return MIFWT_ERR_UNSUPPORTED;
  }
}

bool swt2_extents_ok(int64_t images, int64_t H, int64_t W, int64_t dilation, int filt_len) {
  return images <= INT32_MAX / 8 && H <= INT32_MAX / 8 && W <= INT32_MAX / 8 && dilation * filt_len <= INT32_MAX / 8;
}

int swt2_level(Swt2Call& c, int dtype) {
  const int nin = c.inverse ? 4 : 1, nout = c.inverse ? 1 : 4;
  for (int q = 0; q < nin; ++q)
    if (!c.in[q]) return MIFWT_ERR_BADARG;
  for (int q = 0; q < nout; ++q)
    if (!c.out[q]) return MIFWT_ERR_BADARG;
  for (int q = 0; q < 4; ++q)
    if (!c.taps[q]) return MIFWT_ERR_BADARG;
  if (c.filt_len < 2 || (c.filt_len & 1) || c.filt_len > MIFWT_MAX_FILT || c.images < 0 || c.H < 1 || c.W < 1 || c.dilation < 1)
    return MIFWT_ERR_BADARG;
  if (!mifwt_swt2_supported(dtype, c.filt_len, c.images, c.H, c.W, c.dilation)) return MIFWT_ERR_UNSUPPORTED;
  return dtype == MIFWT_F32 ? swt2_dispatch<float>(c) : swt2_dispatch<double>(c);
}

}  // namespace

}  // namespace mifwt

extern "C" {

int mifwt_swt2_supported(int dtype, int filt_len, int64_t images, int64_t H, int64_t W, int64_t dilation) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return 0;
  if (filt_len < 2 || (filt_len & 1) || filt_len > mifwt::kSwt2MaxFused) return 0;
  if (images < 0 || H < 1 || W < 1 || dilation < 1) return 0;
  return mifwt::swt2_extents_ok(images, H, W, dilation, filt_len) ? 1 : 0;
}

int mifwt_swt2_fwd(int dtype, int filt_len, int64_t images, int64_t H, int64_t W, int64_t dilation, const void* x,
                   int64_t x_image_stride, int64_t x_row_stride, void* const* bands, const int64_t* band_image_strides,
                   const int64_t* band_row_strides, const double* row_lo, const double* row_hi, const double* col_lo,
                   const double* col_hi, double scale, void* stream) {
  if (!bands || !band_image_strides || !band_row_strides) return MIFWT_ERR_BADARG;
  mifwt::Swt2Call c = {};
  c.inverse = 0;
  c.filt_len = filt_len;
  c.images = images;
  c.H = H;
  c.W = W;
  c.dilation = dilation;
  c.in[0] = x;
  c.in_is[0] = x_image_stride;
  c.in_rs[0] = x_row_stride;
  for (int q = 0; q < 4; ++q) {
    c.out[q] = bands[q];
    c.out_is[q] = band_image_strides[q];
    c.out_rs[q] = band_row_strides[q];
  }
  c.taps[0] = row_lo;
  c.taps[1] = row_hi;
  c.taps[2] = col_lo;
  c.taps[3] = col_hi;
  c.scale = scale;
  c.stream = static_cast<hipStream_t>(stream);
  return mifwt::swt2_level(c, dtype);
}

int mifwt_swt2_inv(int dtype, int filt_len, int64_t images, int64_t H, int64_t W, int64_t dilation, const void* const* bands,
                   const int64_t* band_image_strides, const int64_t* band_row_strides, void* y, int64_t y_image_stride,
                   int64_t y_row_stride, const double* row_lo, const double* row_hi, const double* col_lo, const double* col_hi,
                   double scale, void* stream) {
  if (!bands || !band_image_strides || !band_row_strides) return MIFWT_ERR_BADARG;
  mifwt::Swt2Call c = {};
  c.inverse = 1;
  c.filt_len = filt_len;
  c.images = images;
  c.H = H;
  c.W = W;
  c.dilation = dilation;
  for (int q = 0; q < 4; ++q) {
    c.in[q] = bands[q];
    c.in_is[q] = band_image_strides[q];
    c.in_rs[q] = band_row_strides[q];
  }
  c.out[0] = y;
  c.out_is[0] = y_image_stride;
  c.out_rs[0] = y_row_stride;
  c.taps[0] = row_lo;
  c.taps[1] = row_hi;
  c.taps[2] = col_lo;
  c.taps[3] = col_hi;
  c.scale = scale;
  c.stream = static_cast<hipStream_t>(stream);
  return mifwt::swt2_level(c, dtype);
}

}  // extern "C"
