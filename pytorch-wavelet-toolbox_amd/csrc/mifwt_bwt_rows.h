// mifwt_bwt_rows.h — the ROW BANK of the boundary-wavelet kernels (mifwt_bwt.hip, mifwt_bwt3.hip, mifwt_bwt_tree.hip), once.
//
// A level operator A (N x N, N = 2 M) is a banded matrix of plain filter taps except for a few rows at each end of each band
// (csrc comments use "row bank" for: the two filters f_lo / f_hi and their boundary table):
//   interior row m of a band :  B[m, j] = f[2 m + L/2 - j]                     (j = 2m - L/2 + 1 .. 2m + L/2)
//   top row      m <  nt     :  B[m, j] = tab[band][m][j]                      (j = 0 .. L-1; nt = ceil((L-2)/4))
//   bottom row   m >= M - nb :  B[m, j] = tab[band][nt + m - (M-nb)][j-(N-L)]  (j = N-L .. N-1; nb = floor(L/4))
// so every analysis output is L multiply-adds over a contiguous window, and a synthesis output n is
//   y[n] = sum_{band} ( sum_{k < L/2} f[p + 2k] c[m0 + k]  [rows nt <= m < M-nb only]  +  the table column n of the top / bottom rows ),
//   p = (L/2 - n) & 1,  m0 = (n + p - L/2) / 2.
// Analysis applies the rows of a bank, synthesis the transposed bank; the adjoint of either is the other kernel with the same bank.
// An odd signal extent has one virtual sample at its end (index map, `mode`); synthesis simply does not store it.
// The 16-byte vectors, the stores and the row pass of an interior window come from mifwt_level_tile.h, which the fused levels of the
// other modes share; only what is about the row bank is here.
#pragma once
#include "mifwt_level_tile.h"

namespace mifwt {

namespace {

template <int L>
struct Rows {
  static constexpr int NT = (L - 2 + 3) / 4, NB = L / 4, NR = NT + NB, NTAB = NR > 0 ? NR : 1;
  static constexpr int TL = 2 * (NR + 1) * L;  // LDS table entries: per band the boundary rows, then the plain taps in window order
};

// Table -> LDS: rows 0 .. nt+nb-1 the boundary rows, row nt+nb the plain taps in window order (c[k] = f[L-1-k]).
// Args: any argument struct with `tab` (DEVICE [2][NTAB][L]) and the filters `lo`, `hi`.
template <typename T, int L, typename Args>
__device__ __forceinline__ void load_table(T* tl, const Args& a) {
  constexpr int NR = Rows<L>::NR;
  for (int i = threadIdx.x; i < 2 * (NR + 1) * L; i += blockDim.x) {
    const int band = i / ((NR + 1) * L), r = (i / L) % (NR + 1), k = i % L;
    T v;
    if (r < NR)
      v = (T)a.tab[(band * Rows<L>::NTAB + r) * L + k];
    else
      v = band ? a.hi[L - 1 - k] : a.lo[L - 1 - k];
    tl[i] = v;
  }
}

// One staged vector of a row: LDS <- samples g0 .. g0 + E - 1 of a row with `n` real samples (padded extent n_pad); outside: 0, the
// virtual sample: row[src].  `row` == nullptr: zeros.
template <typename T, int E>
__device__ __forceinline__ void stage_vec(T* dst, const T* __restrict__ row, int g0, int n, int n_pad, int src, bool vec_ok) {
  typedef typename Vec16<T>::type V;
  V v;
  if (row && vec_ok && g0 >= 0 && g0 + E <= n) {
    v = *reinterpret_cast<const V*>(row + g0);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int g = g0 + e;
      T s = T(0);
      if (row && g >= 0 && g < n_pad) {
        if (g < n)
          s = row[g];
        else if (src >= 0)
          s = row[src];
      }
      v[e] = s;
    }
  }
  *reinterpret_cast<V*>(dst) = v;
}

// E consecutive analysis outputs (both bands) from a staged row.  xr: LDS row, `pad` = staged samples left of sample 2 * m_first_of_tile.
template <typename T, int L, bool EDGE>
__device__ __forceinline__ void analysis_run(const T* xr, int pad, int ml, int m_glob, int m_ext, const T* tl, const T (&flo)[L],
                                             const T (&fhi)[L], typename Vec16<T>::type& lo, typename Vec16<T>::type& hi) {
  constexpr int E = Vec16<T>::E, NT = Rows<L>::NT, NB = Rows<L>::NB, NR = NT + NB;
  if (!EDGE) {
    // the window starts OFF samples into a 16-byte aligned run of the staged row (2 ml, pad and the window's PAD are multiples of E)
    typedef RowWindow<T, L, L / 2 - 1> W;
    window_run<T, L, L / 2 - 1>(xr + 2 * ml + pad - W::PAD, flo, fhi, lo, hi);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int m = m_glob + e;
      int r = NR, w0 = 2 * (ml + e) + pad - (L / 2 - 1);
      if (m < NT) {
        r = m;
        w0 = pad - 2 * (m_glob - ml);  // sample 0
      } else if (m >= m_ext - NB) {
        r = NT + m - (m_ext - NB);
        w0 = 2 * m_ext - L - 2 * (m_glob - ml) + pad;  // sample N - L
      }
      T sl = T(0), sh = T(0);
      if (m < m_ext) {
        const T* cl = tl + r * L;
        const T* ch = tl + (NR + 1 + r) * L;
#pragma unroll
        for (int k = 0; k < L; ++k) {
          const T v = xr[w0 + k];
          sl = fma(cl[k], v, sl);
          sh = fma(ch[k], v, sh);
        }
      }
      lo[e] = sl;
      hi[e] = sh;
    }
  }
}

// One synthesis output (sample n of an axis with M coefficients per band) from windows of the two bands.  get(band, i): window entry
// i (scalar or vector), window entry 0 = coefficient m_org.
template <int L>
__device__ __forceinline__ bool synthesis_plain(int n, int m_ext) {
  const int p = (L / 2 - n) & 1, m0 = (n + p - L / 2) >> 1;
  return m0 >= Rows<L>::NT && m0 + L / 2 <= m_ext - Rows<L>::NB && n >= L - 1 && n <= 2 * m_ext - L;
}

template <typename T, int L, bool EDGE, typename V, typename Get>
__device__ __forceinline__ V synthesis_point(int n, int m_org, int m_ext, const T* tl, const T (&flo)[L], const T (&fhi)[L], Get get) {
  constexpr int NT = Rows<L>::NT, NB = Rows<L>::NB, NR = NT + NB;
  const int p = (L / 2 - n) & 1;
  const int m0 = (n + p - L / 2) >> 1;  // (even numerator: exact)
  V acc = V(0);
  if (!EDGE) {
    if (p) {
#pragma unroll
      for (int k = 0; k < L / 2; ++k) acc += flo[2 * k + 1] * get(0, m0 - m_org + k) + fhi[2 * k + 1] * get(1, m0 - m_org + k);
    } else {
#pragma unroll
      for (int k = 0; k < L / 2; ++k) acc += flo[2 * k] * get(0, m0 - m_org + k) + fhi[2 * k] * get(1, m0 - m_org + k);
    }
  } else {
#pragma unroll
    for (int k = 0; k < L / 2; ++k) {
      const int m = m0 + k;
      if (m >= NT && m < m_ext - NB) {
        // (the plain taps in window order sit in table row NR: c[j] = f[L-1-j])
        const T cl = tl[NR * L + (L - 1 - (p + 2 * k))], ch = tl[(NR + 1 + NR) * L + (L - 1 - (p + 2 * k))];
        acc += cl * get(0, m - m_org) + ch * get(1, m - m_org);
      }
    }
    if (n < L - 1) {
      for (int m = 0; m < NT; ++m) acc += tl[m * L + n] * get(0, m - m_org) + tl[(NR + 1 + m) * L + n] * get(1, m - m_org);
    }
    const int jb = n - (2 * m_ext - L);
    if (jb >= 1 && jb < L) {
      for (int i = 0; i < NB; ++i) {
        const int m = m_ext - NB + i;
        acc += tl[(NT + i) * L + jb] * get(0, m - m_org) + tl[(NR + 1 + NT + i) * L + jb] * get(1, m - m_org);
      }
    }
  }
  return acc;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
// the table of a bank of L taps has ceil((L-2)/4) top and floor(L/4) bottom rows
bool table_fits(const mifwt_bwt_tables* tb, int L) { return tb->n_top == (L - 2 + 3) / 4 && tb->n_bot == L / 4; }

// the taps as the kernels take them: synthesis builds the rows of S^T from the reversed rec_* filters
void bank_taps(int inverse, int L, const double* lo, const double* hi, double* flo, double* fhi) {
  for (int t = 0; t < L; ++t) {
    flo[t] = inverse ? lo[L - 1 - t] : lo[t];
    fhi[t] = inverse ? hi[L - 1 - t] : hi[t];
  }
}

}  // namespace

}  // namespace mifwt
