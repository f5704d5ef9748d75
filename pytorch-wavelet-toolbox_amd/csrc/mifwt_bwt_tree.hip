// mifwt_bwt_tree.hip — a SUBTREE of a boundary-wavelet packet tree per launch for gfx950 (kernel ids 32 / 33).
//
// A packet node of h samples splits into two nodes of exactly h / 2 (the padding-free transform of mifwt_bwt.hip), so every level of
// the tree below a row of n samples is again n numbers and one contiguous span: level s = [2^s nodes][n / 2^s].  ptwt.WaveletPacket
// with mode="boundary" expands one node per MatrixWavedec(level=1) call (reference src/ptwt/packets.py:240-271, :312-316); per-level
// launches of kernel 26 run on ever shorter rows.  Here ONE workgroup owns a row (a node of the tree folded into the batch), keeps it
// in LDS together with its next level and computes k >= 2 levels: HBM is read once, every level is written once.
//
//   analysis (id 32), level with node length h, pair index p in [0, n/2): parent node q = p / (h/2), row m = p % (h/2); the lane
//     computes both children's sample m,  o = (2q + band) * (h/2) + m  — i.e. child c = o / (h/2), q = c >> 1, band = c & 1 —
//       interior rows:   y = sum_t f_band[t] x[q h + 2m + L/2 - t]
//       top rows    m <  nt = ceil((L-2)/4):   table row m        over samples q h + 0 .. L-1
//       bottom rows m >= h/2 - nb, nb = L/4:   table row nt + ..  over samples q h + h-L .. h-1          (layout: mifwt_bwt_rows.h)
//   synthesis (id 33), output position o in [0, n): node q = o / h, sample i = o % h, bands at q h (+ h/2):
//       y = sum_band sum_{k<L/2} g[p+2k] c[m0+k] (interior rows) + column i of the table rows,  p = (L/2-i)&1, m0 = (i+p-L/2)/2
//     with the synthesis bank (reversed rec_* filters and ITS tables: S != A^T for biorthogonal banks).
//
// The result of a level goes to the second LDS image; after the barrier the image is copied to that level's dense [rows, n] buffer
// with 16-byte stores while it is the input of the next level.  The table sits in LDS, converted like the taps; only lanes that own a
// boundary row read it.  Envelope (host): f32 / f64, even L <= 20, every fused level's input node even and >= 2 (L-1), two images of
// n samples <= 64 KB.
#include "mifwt_bwt_rows.h"

namespace mifwt {

namespace {

constexpr int TREE_MAX_LEVELS = 16;
constexpr int TREE_IMAGE_BYTES = 32768;  // one LDS image: n <= 8192 f32 / 4096 f64

template <typename T, int L>
struct TreeArgs {
  const T* in;                  // analysis: x (row stride in_rs);  synthesis: the leaves' span, dense [rows, n]
  T* lev[TREE_MAX_LEVELS];      // analysis: lev[i] = level i + 1;  synthesis: lev[i] = level i (lev[0] = the rows);  dense [rows, n]
  int64_t in_rs;
  int n, nlev;
  int in_vec, out_vec;          // 16-byte accesses allowed on the input / on every level buffer
  const double* tab;            // DEVICE [2][max(nt + nb, 1)][L]
  T lo[L], hi[L];               // row filters f_lo, f_hi
};

extern __shared__ __attribute__((aligned(16))) unsigned char bwt_tree_lds[];

template <typename T>
__device__ __forceinline__ void tree_stage(T* img, const T* __restrict__ src, int n, bool vec) {
  typedef typename Vec16<T>::type V;
  constexpr int E = Vec16<T>::E;
  if (vec) {
    for (int i = threadIdx.x; i < n / E; i += blockDim.x) reinterpret_cast<V*>(img)[i] = reinterpret_cast<const V*>(src)[i];
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) img[i] = src[i];
  }
}

template <typename T>
__device__ __forceinline__ void tree_flush(T* __restrict__ dst, const T* img, int n, bool vec) {
  typedef typename Vec16<T>::type V;
  constexpr int E = Vec16<T>::E;
  if (vec) {
    for (int i = threadIdx.x; i < n / E; i += blockDim.x) reinterpret_cast<V*>(dst)[i] = reinterpret_cast<const V*>(img)[i];
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = img[i];
  }
}

// ---- analysis ------------------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_tree_fwd_kernel(const TreeArgs<T, L> a) {
  constexpr int NT = Rows<L>::NT, NB = Rows<L>::NB, NR = Rows<L>::NR;
  const int n = a.n;
  T* cur = reinterpret_cast<T*>(bwt_tree_lds);
  T* nxt = cur + n;
  T* tl = cur + 2 * n;
  const int64_t row = blockIdx.x;
  load_table<T, L>(tl, a);
  tree_stage<T>(cur, a.in + row * a.in_rs, n, a.in_vec);
  __syncthreads();
  for (int lev = 0; lev < a.nlev; ++lev) {
    if (lev > 0) tree_flush<T>(a.lev[lev - 1] + row * n, cur, n, a.out_vec);
    const int h = n >> lev, half = h >> 1;
    for (int p = threadIdx.x; p < (n >> 1); p += 256) {
      const int q = p / half, m = p - q * half;
      const T* x = cur + q * h;
      T sl = T(0), sh = T(0);
      if (NR == 0 || (m >= NT && m < half - NB)) {
        const T* w = x + 2 * m - (L / 2 - 1);
#pragma unroll
        for (int k = 0; k < L; ++k) {
          const T v = w[k];
          sl = fma(a.lo[L - 1 - k], v, sl);
          sh = fma(a.hi[L - 1 - k], v, sh);
        }
      } else {
        const int r = m < NT ? m : NT + m - (half - NB);
        const T* w = x + (m < NT ? 0 : h - L);
        const T* cl = tl + r * L;
        const T* ch = tl + (NR + 1 + r) * L;
#pragma unroll
        for (int k = 0; k < L; ++k) {
          const T v = w[k];
          sl = fma(cl[k], v, sl);
          sh = fma(ch[k], v, sh);
        }
      }
      nxt[q * h + m] = sl;
      nxt[q * h + half + m] = sh;
    }
    __syncthreads();
    T* t = cur;
    cur = nxt;
    nxt = t;
  }
  tree_flush<T>(a.lev[a.nlev - 1] + row * n, cur, n, a.out_vec);
}

// ---- synthesis -----------------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_tree_inv_kernel(const TreeArgs<T, L> a) {
  constexpr int NT = Rows<L>::NT, NB = Rows<L>::NB, NR = Rows<L>::NR;
  const int n = a.n;
  T* cur = reinterpret_cast<T*>(bwt_tree_lds);
  T* nxt = cur + n;
  T* tl = cur + 2 * n;
  const int64_t row = blockIdx.x;
  load_table<T, L>(tl, a);
  tree_stage<T>(cur, a.in + row * a.in_rs, n, a.in_vec);
  __syncthreads();
  for (int lev = a.nlev - 1; lev >= 0; --lev) {
    if (lev < a.nlev - 1) tree_flush<T>(a.lev[lev + 1] + row * n, cur, n, a.out_vec);
    const int h = n >> lev, half = h >> 1;
    for (int o = threadIdx.x; o < n; o += 256) {
      const int q = o / h, i = o - q * h;
      const T* cl = cur + q * h;
      const T* ch = cl + half;
      const int p = (L / 2 - i) & 1;
      const int m0 = (i + p - L / 2) >> 1;  // (even numerator: exact)
      T acc = T(0);
      if (NR == 0 || (m0 >= NT && m0 + L / 2 <= half - NB && i >= L - 1 && i <= h - L)) {
        if (p) {
#pragma unroll
          for (int k = 0; k < L / 2; ++k) acc = fma(a.lo[2 * k + 1], cl[m0 + k], fma(a.hi[2 * k + 1], ch[m0 + k], acc));
        } else {
#pragma unroll
          for (int k = 0; k < L / 2; ++k) acc = fma(a.lo[2 * k], cl[m0 + k], fma(a.hi[2 * k], ch[m0 + k], acc));
        }
      } else {
#pragma unroll
        for (int k = 0; k < L / 2; ++k) {
          const int m = m0 + k;
          if (m >= NT && m < half - NB) {
            const T fl = tl[NR * L + (L - 1 - (p + 2 * k))], fh = tl[(NR + 1 + NR) * L + (L - 1 - (p + 2 * k))];
            acc = fma(fl, cl[m], fma(fh, ch[m], acc));
          }
        }
        if (i < L - 1) {
          for (int m = 0; m < NT; ++m) acc = fma(tl[m * L + i], cl[m], fma(tl[(NR + 1 + m) * L + i], ch[m], acc));
        }
        const int jb = i - (h - L);
        if (jb >= 1 && jb < L) {
          for (int r = 0; r < NB; ++r) {
            const int m = half - NB + r;
            acc = fma(tl[(NT + r) * L + jb], cl[m], fma(tl[(NR + 1 + NT + r) * L + jb], ch[m], acc));
          }
        }
      }
      nxt[o] = acc;
    }
    __syncthreads();
    T* t = cur;
    cur = nxt;
    nxt = t;
  }
  tree_flush<T>(a.lev[0] + row * n, cur, n, a.out_vec);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
int tree_elem_bytes(int dtype) { return dtype == MIFWT_F32 ? 4 : dtype == MIFWT_F64 ? 8 : 0; }

// number of consecutive levels one launch takes from a node of n samples (0: none)
int tree_levels(int dtype, int filt_len, int64_t n, int max_levels) {
  const int eb = tree_elem_bytes(dtype);
  if (!eb || filt_len < 2 || filt_len > 20 || (filt_len & 1) || n < 2 || n * eb > TREE_IMAGE_BYTES) return 0;
  int k = 0;
  int64_t h = n;
  while (k < max_levels && k < TREE_MAX_LEVELS && !(h & 1) && h >= 2 * (int64_t)(filt_len - 1)) {
    ++k;
    h >>= 1;
  }
  return k >= 2 ? k : 0;
}

template <typename T, int L>
int tree_launch(int inverse, int64_t rows, int n, int64_t in_rs, int nlevels, const void* in, void* const* levels, const double* flo,
                const double* fhi, const mifwt_bwt_tables* tb, hipStream_t stream) {
  constexpr int E = Vec16<T>::E;
  TreeArgs<T, L> a;
  a.in = static_cast<const T*>(in);
  a.in_rs = in_rs;
  a.n = n;
  a.nlev = nlevels;
  a.in_vec = aligned16(in) && in_rs % E == 0 && n % E == 0;
  a.out_vec = n % E == 0;
  for (int i = 0; i < TREE_MAX_LEVELS; ++i) {
    a.lev[i] = i < nlevels ? static_cast<T*>(levels[i]) : nullptr;
    if (i < nlevels) a.out_vec = a.out_vec && aligned16(levels[i]);
  }
  a.tab = tb->rows;
  for (int t = 0; t < L; ++t) {
    a.lo[t] = (T)flo[t];
    a.hi[t] = (T)fhi[t];
  }
  if (rows == 0) return MIFWT_OK;
  const int lds = (2 * n + Rows<L>::TL) * (int)sizeof(T);
  const dim3 g((unsigned)rows), blk(256);
  if (inverse) {
    static DynLdsOnce once;
    if (lds > 65536 && !once.ensure(reinterpret_cast<const void*>(&bwt_tree_inv_kernel<T, L>), 2 * TREE_IMAGE_BYTES + Rows<L>::TL * (int)sizeof(T)))
      return MIFWT_ERR_LAUNCH;
    hipLaunchKernelGGL((bwt_tree_inv_kernel<T, L>), g, blk, lds, stream, a);
  } else {
    static DynLdsOnce once;
    if (lds > 65536 && !once.ensure(reinterpret_cast<const void*>(&bwt_tree_fwd_kernel<T, L>), 2 * TREE_IMAGE_BYTES + Rows<L>::TL * (int)sizeof(T)))
      return MIFWT_ERR_LAUNCH;
    hipLaunchKernelGGL((bwt_tree_fwd_kernel<T, L>), g, blk, lds, stream, a);
  }
  return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
}

template <typename T>
int tree_dispatch(int filt_len, int inverse, int64_t rows, int n, int64_t in_rs, int nlevels, const void* in, void* const* levels,
                  const double* flo, const double* fhi, const mifwt_bwt_tables* tb, hipStream_t stream) {
  return for_even_len(filt_len, [&](auto len) {
    return tree_launch<T, decltype(len)::value>(inverse, rows, n, in_rs, nlevels, in, levels, flo, fhi, tb, stream);
  });
}

int tree_call(int inverse, int dtype, int filt_len, int64_t rows, int64_t n, int64_t in_rs, int nlevels, const void* in,
              void* const* levels, const double* lo, const double* hi, const mifwt_bwt_tables* tb, void* stream) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return is_storage16(dtype) ? MIFWT_ERR_UNSUPPORTED : MIFWT_ERR_BADARG;
  if (filt_len < 2 || filt_len > MIFWT_MAX_FILT || rows < 0 || n < 1) return MIFWT_ERR_BADARG;
  if (!in || !levels || !lo || !hi || !tb || !tb->rows) return MIFWT_ERR_BADARG;
  if (nlevels < 2 || (filt_len & 1) || filt_len > 20 || tree_levels(dtype, filt_len, n, nlevels) != nlevels) return MIFWT_ERR_UNSUPPORTED;
  if (rows > INT32_MAX || (inverse ? in_rs != n : in_rs < n)) return MIFWT_ERR_UNSUPPORTED;
  if (!table_fits(tb, filt_len)) return MIFWT_ERR_BADARG;
  for (int i = 0; i < nlevels; ++i)
    if (!levels[i]) return MIFWT_ERR_BADARG;
  double flo[MIFWT_MAX_FILT], fhi[MIFWT_MAX_FILT];
  bank_taps(inverse, filt_len, lo, hi, flo, fhi);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == MIFWT_F32 ? tree_dispatch<float>(filt_len, inverse, rows, (int)n, in_rs, nlevels, in, levels, flo, fhi, tb, st)
                            : tree_dispatch<double>(filt_len, inverse, rows, (int)n, in_rs, nlevels, in, levels, flo, fhi, tb, st);
}

}  // namespace

}  // namespace mifwt

extern "C" {

int mifwt_bwt_tree_levels(int dtype, int filt_len, int64_t n, int max_levels) { return mifwt::tree_levels(dtype, filt_len, n, max_levels); }

int mifwt_bwt_tree_fwd(int dtype, int filt_len, int64_t rows, int64_t n, int64_t x_row_stride, int nlevels, const void* x,
                       void* const* levels, const double* lo, const double* hi, const mifwt_bwt_tables* tables, void* stream) {
  return mifwt::tree_call(0, dtype, filt_len, rows, n, x_row_stride, nlevels, x, levels, lo, hi, tables, stream);
}

int mifwt_bwt_tree_inv(int dtype, int filt_len, int64_t rows, int64_t n, int nlevels, const void* leaves, void* const* levels,
                       const double* lo, const double* hi, const mifwt_bwt_tables* tables, void* stream) {
  return mifwt::tree_call(1, dtype, filt_len, rows, n, n, nlevels, leaves, levels, lo, hi, tables, stream);
}

}  // extern "C"
