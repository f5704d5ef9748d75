// mifwt_bwt.hip — levels of the padding-free BOUNDARY-WAVELET transform for gfx950 (kernel ids 26 / 27, generic passes 28 / 29).
//
// Replaces, per level of ptwt.MatrixWavedec / MatrixWaverec / MatrixWavedec2 / MatrixWaverec2 (reference
// src/ptwt/matmul_transform.py:409-430 and :679-703, src/ptwt/matmul_transform_2.py:514-529 and :799-840):
//   analysis : pad one sample if the extent is odd + torch.sparse.mm(A, x) (2-D: A_rows X A_cols^T, two transposes) + split
//   synthesis: cat + torch.sparse.mm(S, c) (2-D likewise) + drop the pad sample
// The matrix a level stands for (interior, top and bottom rows, p, m0) and the device pieces that apply it are in mifwt_bwt_rows.h.
//
// Bound: HBM (N in, N out per axis).  Fused kernels (unit innermost stride, f32 / f64, even L <= 20, N >= 2 (L-1) per axis):
//   2-D: one launch per level.  A workgroup stages the input window of a TR x TC tile of coefficients in LDS (16-byte loads where
//        the rows allow), filters it along the rows into LDS and along the columns into registers, and stores the four bands with
//        16-byte stores.  Synthesis mirrors it: the windows of the four bands -> columns -> rows -> y.
//   1-D: the horizontal half of the same code, a piece of one row per workgroup.
// Workgroups whose tile touches an end of an axis load the table into LDS, and their lanes whose outputs involve a boundary row take
// the EDGE instantiation of the filter step (per-output window start and coefficient row from the table); everything else runs the
// plain taps from registers, its window read from LDS in 16-byte pieces, without a per-element branch.
// Everything else (20 < L <= 128, any strides) runs bwt_axis_generic: one thread per output, run-time tap loop, one axis per launch.
// Shared with the fused levels of the other modes, from mifwt_level_tile.h (through mifwt_bwt_rows.h): the 16-byte vectors, the row pass
// of an interior window, the tap step of the plain column pass and the band stores, the common kernel arguments and their fill, the
// tile cut, the descriptor prelude and envelope, the length dispatch, the packing of the level entries and the axis-pass arguments and
// launcher.  The column pass over boundary rows reads its taps from the LDS table at every use and stays here.
#include "mifwt_bwt_rows.h"

namespace mifwt {

namespace {

// ---- tile geometry (compile time; LDS stays below the 64 KB a kernel gets without opting in) ---------------------------------------------
template <typename T, int L>
struct FwdTile {
  static constexpr int E = Vec16<T>::E;
  static constexpr int TC = 16 * E;                 // coefficient columns per tile (64 f32 / 32 f64): 16 lanes x one 16-byte store
  static constexpr int TR = 8;                      // coefficient rows per tile
  static constexpr int PADI = round_up(L / 2 - 1, E);  // staged columns left of sample 2 mc0: interior tiles
  static constexpr int PADE = round_up(L - 2, E);      // ... tiles at an end (a bottom row's window reaches back L - 1 samples)
  static constexpr int WC = round_up(PADE + 2 * TC + L / 2 - 1, E);
  static constexpr int WR = 2 * TR + (L - 2) + L / 2 - 1;
  static constexpr int TC1 = 256 * E;               // 1-D: coefficients per workgroup
  static constexpr int WC1 = round_up(PADE + 2 * TC1 + L / 2 - 1, E);
  static constexpr int LDS2 = (WR * WC + 2 * WR * TC + 2 * (L / 2 + 1) * L) * (int)sizeof(T);
};

template <typename T, int L>
struct InvTile {
  static constexpr int E = Vec16<T>::E;
  static constexpr int TQ = 16;                                            // coefficient rows per tile (32 output rows)
  static constexpr int TQC = (L <= 12 ? 16 : 8) * E;                      // coefficient columns per tile
  static constexpr int PMC = round_up(L / 2, E);                           // staged coefficients either side
  static constexpr int PMR = L / 2;
  static constexpr int WCM = TQC + 2 * PMC;
  static constexpr int WRM = TQ + 2 * PMR;
  static constexpr int TQ1 = 128 * E;                                      // 1-D: coefficient columns per workgroup
  static constexpr int WCM1 = TQ1 + 2 * PMC;
  static constexpr int LDS2 = (4 * WRM * WCM + 2 * 2 * TQ * WCM + 2 * (L / 2 + 1) * L) * (int)sizeof(T);
};

// real signal extents, coefficient extents = ceil(n / 2); the filters f_lo, f_hi of the bank
template <typename T, int L>
struct BwtArgs : LevelArgs<T, L> {
  int batch;
  int src_r, src_c;   // source index of the virtual sample of an odd extent (-1: zero)
  const double* tab;  // DEVICE [2][max(nt + nb, 1)][L]
};

// ---- analysis, 2-D -----------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_fwd2_kernel(const BwtArgs<T, L> a) {
  typedef FwdTile<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TC = G::TC, TR = G::TR, NT = Rows<L>::NT, NB = Rows<L>::NB, NR = NT + NB;
  __shared__ __attribute__((aligned(16))) T xs[G::WR * G::WC];
  __shared__ __attribute__((aligned(16))) T hs[2 * G::WR * TC];
  __shared__ T tl[2 * (NR + 1) * L];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tc = bid % a.tiles_c;
  bid /= a.tiles_c;
  const int tr = bid % a.tiles_r;
  const int b = bid / a.tiles_r;
  const int mc0 = tc * TC, mr0 = tr * TR;
  const bool edge_c = NR > 0 && (mc0 < NT || mc0 + TC > a.m_c - NB);
  const bool edge_r = NR > 0 && (mr0 < NT || mr0 + TR > a.m_r - NB);
  const int padc = edge_c ? G::PADE : G::PADI;
  const int padr = edge_r ? L - 2 : L / 2 - 1;
  const int wc = round_up(padc + 2 * TC + L / 2 - 1, E);  // staged columns (<= WC)
  const int wr = padr + 2 * TR + L / 2 - 1;               // staged rows (<= WR)
  const int ws_c = 2 * mc0 - padc, ws_r = 2 * mr0 - padr;
  const T* __restrict__ x = static_cast<const T*>(a.in[0]) + (int64_t)b * a.sig_bs;
  if (edge_c || edge_r) load_table<T, L>(tl, a);
  const int vpr = wc / E;
  for (int i = tid; i < wr * vpr; i += 256) {
    const int r = i / vpr, cv = i - r * vpr;
    int gr = ws_r + r;
    const T* row = nullptr;
    if (gr >= 0 && gr < 2 * a.m_r) {
      if (gr >= a.n_r) gr = a.src_r;
      if (gr >= 0) row = x + (int64_t)gr * a.sig_rs;
    }
    stage_vec<T, E>(xs + r * G::WC + cv * E, row, ws_c + cv * E, a.n_c, 2 * a.m_c, a.src_c, a.sig_vec);
  }
  __syncthreads();
  // along the rows of the window: (lo, hi) of every staged row
  for (int i = tid; i < wr * (TC / E); i += 256) {
    const int r = i / (TC / E), cg = i - r * (TC / E);
    V lo, hi;
    if (edge_c && (mc0 + cg * E < NT || mc0 + cg * E + E > a.m_c - NB))  // (only the lanes whose outputs include a boundary row)
      analysis_run<T, L, true>(xs + r * G::WC, padc, cg * E, mc0 + cg * E, a.m_c, tl, a.lo, a.hi, lo, hi);
    else
      analysis_run<T, L, false>(xs + r * G::WC, padc, cg * E, mc0 + cg * E, a.m_c, tl, a.lo, a.hi, lo, hi);
    *reinterpret_cast<V*>(hs + r * TC + cg * E) = lo;
    *reinterpret_cast<V*>(hs + (G::WR + r) * TC + cg * E) = hi;
  }
  __syncthreads();
  // along the columns: four bands, E columns per lane
  for (int i = tid; i < TR * (TC / E); i += 256) {
    const int ro = i / (TC / E), cg = i - ro * (TC / E);
    const int m = mr0 + ro, mc = mc0 + cg * E;
    if (m >= a.m_r || mc >= a.m_c) continue;
    V ll = V(0), lh = V(0), hl = V(0), hh = V(0);
    const T* hl0 = hs + cg * E;
    const T* hh0 = hs + G::WR * TC + cg * E;
    if (!edge_r || (m >= NT && m < a.m_r - NB)) {
      const int w0 = 2 * ro + padr - (L / 2 - 1);
#pragma unroll
      for (int k = 0; k < L; ++k) column_tap<T>(hl0 + (w0 + k) * TC, hh0 + (w0 + k) * TC, a.lo[L - 1 - k], a.hi[L - 1 - k], ll, lh, hl, hh);
    } else {
      int r = NR, w0 = 2 * ro + padr - (L / 2 - 1);
      if (m < NT) {
        r = m;
        w0 = -ws_r;
      } else if (m >= a.m_r - NB) {
        r = NT + m - (a.m_r - NB);
        w0 = 2 * a.m_r - L - ws_r;
      }
      const T* cl = tl + r * L;
      const T* ch = tl + (NR + 1 + r) * L;
#pragma unroll
      for (int k = 0; k < L; ++k) {
        const V vl = *reinterpret_cast<const V*>(hl0 + (w0 + k) * TC);
        const V vh = *reinterpret_cast<const V*>(hh0 + (w0 + k) * TC);
        ll += cl[k] * vl;
        lh += cl[k] * vh;
        hl += ch[k] * vl;
        hh += ch[k] * vh;
      }
    }
    store_bands<T, L>(a, b, m, mc, ll, lh, hl, hh);
  }
}

// ---- analysis, 1-D: a piece of one row per workgroup -----------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_fwd1_kernel(const BwtArgs<T, L> a) {
  typedef FwdTile<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TC = G::TC1, NT = Rows<L>::NT, NB = Rows<L>::NB, NR = NT + NB;
  __shared__ __attribute__((aligned(16))) T xs[G::WC1];
  __shared__ T tl[2 * (NR + 1) * L];
  const int tid = threadIdx.x;
  const int tc = blockIdx.x % a.tiles_c;
  const int b = blockIdx.x / a.tiles_c;
  const int mc0 = tc * TC;
  const bool edge_c = NR > 0 && (mc0 < NT || mc0 + TC > a.m_c - NB);
  const int padc = edge_c ? G::PADE : G::PADI;
  const int wc = round_up(padc + 2 * TC + L / 2 - 1, E);
  const int ws_c = 2 * mc0 - padc;
  const T* __restrict__ x = static_cast<const T*>(a.in[0]) + (int64_t)b * a.sig_bs;
  if (edge_c) load_table<T, L>(tl, a);
  for (int i = tid; i < wc / E; i += 256) stage_vec<T, E>(xs + i * E, x, ws_c + i * E, a.n_c, 2 * a.m_c, a.src_c, a.sig_vec);
  __syncthreads();
  const int mc = mc0 + tid * E;
  if (mc >= a.m_c) return;
  V lo, hi;
  if (edge_c && (mc < NT || mc + E > a.m_c - NB))
    analysis_run<T, L, true>(xs, padc, tid * E, mc, a.m_c, tl, a.lo, a.hi, lo, hi);
  else
    analysis_run<T, L, false>(xs, padc, tid * E, mc, a.m_c, tl, a.lo, a.hi, lo, hi);
  store_vec<T>(static_cast<T*>(a.out[0]) + (int64_t)b * a.a_bs + mc, lo, a.m_c - mc, a.coef_vec);
  store_vec<T>(static_cast<T*>(a.out[1]) + (int64_t)b * a.d_bs + mc, hi, a.m_c - mc, a.coef_vec);
}

// ---- synthesis ---------------------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_inv2_kernel(const BwtArgs<T, L> a) {
  typedef InvTile<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TQ = G::TQ, TQC = G::TQC, WCM = G::WCM, WRM = G::WRM, NT = Rows<L>::NT, NB = Rows<L>::NB, NR = NT + NB;
  __shared__ __attribute__((aligned(16))) T bs[4 * WRM * WCM];
  __shared__ __attribute__((aligned(16))) T ts[2 * 2 * TQ * WCM];
  __shared__ T tl[2 * (NR + 1) * L];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tc = bid % a.tiles_c;
  bid /= a.tiles_c;
  const int tr = bid % a.tiles_r;
  const int b = bid / a.tiles_r;
  const int qc0 = tc * TQC, qr0 = tr * TQ;
  const bool edge_c = NR > 0 && (qc0 == 0 || 2 * (qc0 + TQC) + L + 2 >= 2 * a.m_c);
  const bool edge_r = NR > 0 && (qr0 == 0 || 2 * (qr0 + TQ) + L + 2 >= 2 * a.m_r);
  const int mo_c = qc0 - G::PMC, mo_r = qr0 - G::PMR;
  if (edge_c || edge_r) load_table<T, L>(tl, a);
  // the windows of the four bands
  for (int i = tid; i < 4 * WRM * (WCM / E); i += 256) {
    const int cv = i % (WCM / E), r = (i / (WCM / E)) % WRM, s = i / ((WCM / E) * WRM);
    const int mr = mo_r + r;
    const T* row = nullptr;
    if (mr >= 0 && mr < a.m_r)
      row = static_cast<const T*>(a.in[s]) + (s ? (int64_t)b * a.d_bs + (int64_t)mr * a.d_rs : (int64_t)b * a.a_bs + (int64_t)mr * a.a_rs);
    stage_vec<T, E>(bs + (s * WRM + r) * WCM + cv * E, row, mo_c + cv * E, a.m_c, a.m_c, -1, a.coef_vec);
  }
  __syncthreads();
  // along the columns (axis 0): ts[cb][output row][window column], cb = band along axis 1
  for (int i = tid; i < 2 * 2 * TQ * (WCM / E); i += 256) {
    const int cv = i % (WCM / E), nl = (i / (WCM / E)) % (2 * TQ), cb = i / ((WCM / E) * 2 * TQ);
    const int n = 2 * qr0 + nl;
    auto get = [&](int rb, int idx) -> V { return *reinterpret_cast<const V*>(bs + ((rb * 2 + cb) * WRM + idx) * WCM + cv * E); };
    V v = V(0);
    if (n < 2 * a.m_r)
      v = edge_r && !synthesis_plain<L>(n, a.m_r) ? synthesis_point<T, L, true, V>(n, mo_r, a.m_r, tl, a.lo, a.hi, get)
                 : synthesis_point<T, L, false, V>(n, mo_r, a.m_r, tl, a.lo, a.hi, get);
    *reinterpret_cast<V*>(ts + (cb * 2 * TQ + nl) * WCM + cv * E) = v;
  }
  __syncthreads();
  // along the rows (axis 1): E consecutive samples per lane
  T* __restrict__ y = static_cast<T*>(a.out[0]) + (int64_t)b * a.sig_bs;
  for (int i = tid; i < 2 * TQ * (2 * TQC / E); i += 256) {
    const int cg = i % (2 * TQC / E), nl = i / (2 * TQC / E);
    const int nr = 2 * qr0 + nl, nc = 2 * qc0 + cg * E;
    if (nr >= a.n_r || nc >= a.n_c) continue;
    auto get = [&](int cb, int idx) -> T { return ts[(cb * 2 * TQ + nl) * WCM + idx]; };
    V v;
#pragma unroll
    for (int e = 0; e < E; ++e)
      v[e] = (nc + e >= 2 * a.m_c) ? T(0)
             : edge_c && !synthesis_plain<L>(nc + e, a.m_c) ? synthesis_point<T, L, true, T>(nc + e, mo_c, a.m_c, tl, a.lo, a.hi, get)
                                   : synthesis_point<T, L, false, T>(nc + e, mo_c, a.m_c, tl, a.lo, a.hi, get);
    store_vec<T>(y + (int64_t)nr * a.sig_rs + nc, v, a.n_c - nc, a.sig_vec);
  }
}

template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_inv1_kernel(const BwtArgs<T, L> a) {
  typedef InvTile<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TQ1 = G::TQ1, WCM = G::WCM1, NT = Rows<L>::NT, NB = Rows<L>::NB, NR = NT + NB;
  __shared__ __attribute__((aligned(16))) T bs[2 * WCM];
  __shared__ T tl[2 * (NR + 1) * L];
  const int tid = threadIdx.x;
  const int tc = blockIdx.x % a.tiles_c;
  const int b = blockIdx.x / a.tiles_c;
  const int qc0 = tc * TQ1;
  const bool edge_c = NR > 0 && (qc0 == 0 || 2 * (qc0 + TQ1) + L + 2 >= 2 * a.m_c);
  const int mo_c = qc0 - G::PMC;
  if (edge_c) load_table<T, L>(tl, a);
  for (int i = tid; i < 2 * (WCM / E); i += 256) {
    const int cv = i % (WCM / E), s = i / (WCM / E);
    const T* row = static_cast<const T*>(a.in[s]) + (int64_t)b * (s ? a.d_bs : a.a_bs);
    stage_vec<T, E>(bs + s * WCM + cv * E, row, mo_c + cv * E, a.m_c, a.m_c, -1, a.coef_vec);
  }
  __syncthreads();
  T* __restrict__ y = static_cast<T*>(a.out[0]) + (int64_t)b * a.sig_bs;
  auto get = [&](int cb, int idx) -> T { return bs[cb * WCM + idx]; };
  for (int i = tid; i < 2 * TQ1 / E; i += 256) {
    const int nc = 2 * qc0 + i * E;
    if (nc >= a.n_c) continue;
    V v;
#pragma unroll
    for (int e = 0; e < E; ++e)
      v[e] = (nc + e >= 2 * a.m_c) ? T(0)
             : edge_c && !synthesis_plain<L>(nc + e, a.m_c) ? synthesis_point<T, L, true, T>(nc + e, mo_c, a.m_c, tl, a.lo, a.hi, get)
                                   : synthesis_point<T, L, false, T>(nc + e, mo_c, a.m_c, tl, a.lo, a.hi, get);
    store_vec<T>(y + nc, v, a.n_c - nc, a.sig_vec);
  }
}

// ---- generic per-axis passes: any even L <= MIFWT_MAX_FILT, any strides ------------------------------------------------------------------------
struct BwtAxisArgs : AxisArgsBase {
  int src, nt, nb, ntab;
  const double* tab;
};

template <typename T, bool INVERSE>
__global__ void __launch_bounds__(256) bwt_axis_generic(const BwtAxisArgs a) {
  const int L = a.filt_len, NT = a.nt, NB = a.nb, M = a.m;
  const int64_t len = INVERSE ? a.n : M;
  const int64_t total = a.outer * len * a.inner;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t in = idx % a.inner, o = idx / (a.inner * len);
    const int pos = (int)((idx / a.inner) % len);
    if (!INVERSE) {
      const T* x = static_cast<const T*>(a.in0) + o * a.sig_s[0] + in * a.sig_s[2];
      int w0 = 2 * pos - (L / 2 - 1), r = -1;
      if (pos < NT) {
        r = pos;
        w0 = 0;
      } else if (pos >= M - NB) {
        r = NT + pos - (M - NB);
        w0 = 2 * M - L;
      }
      double sl = 0, sh = 0;
      for (int k = 0; k < L; ++k) {
        int j = w0 + k;
        if (j >= a.n) j = a.src;
        const double v = j >= 0 ? (double)x[(int64_t)j * a.sig_s[1]] : 0.0;
        const double cl = r < 0 ? a.lo[L - 1 - k] : a.tab[(int64_t)r * L + k];
        const double ch = r < 0 ? a.hi[L - 1 - k] : a.tab[((int64_t)a.ntab + r) * L + k];
        sl = fma(cl, v, sl);
        sh = fma(ch, v, sh);
      }
      static_cast<T*>(a.out0)[o * a.lo_s[0] + (int64_t)pos * a.lo_s[1] + in * a.lo_s[2]] = (T)sl;
      static_cast<T*>(a.out1)[o * a.hi_s[0] + (int64_t)pos * a.hi_s[1] + in * a.hi_s[2]] = (T)sh;
    } else {
      const T* cl = static_cast<const T*>(a.in0) + o * a.lo_s[0] + in * a.lo_s[2];
      const T* ch = static_cast<const T*>(a.in1) + o * a.hi_s[0] + in * a.hi_s[2];
      const int n = pos;
      const int p = (L / 2 - n) & 1, m0 = (n + p - L / 2) >> 1;
      double acc = 0;
      for (int k = 0; k < L / 2; ++k) {
        const int m = m0 + k;
        if (m >= NT && m < M - NB)
          acc += a.lo[p + 2 * k] * (double)cl[(int64_t)m * a.lo_s[1]] + a.hi[p + 2 * k] * (double)ch[(int64_t)m * a.hi_s[1]];
      }
      if (n < L - 1)
        for (int m = 0; m < NT; ++m)
          acc += a.tab[(int64_t)m * L + n] * (double)cl[(int64_t)m * a.lo_s[1]] +
                 a.tab[((int64_t)a.ntab + m) * L + n] * (double)ch[(int64_t)m * a.hi_s[1]];
      const int jb = n - (2 * M - L);
      if (jb >= 1 && jb < L)
        for (int i = 0; i < NB; ++i) {
          const int m = M - NB + i;
          acc += a.tab[(int64_t)(NT + i) * L + jb] * (double)cl[(int64_t)m * a.lo_s[1]] +
                 a.tab[((int64_t)a.ntab + NT + i) * L + jb] * (double)ch[(int64_t)m * a.hi_s[1]];
        }
      static_cast<T*>(a.out0)[o * a.sig_s[0] + (int64_t)n * a.sig_s[1] + in * a.sig_s[2]] = (T)acc;
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
// 0 = not served by the fused kernels, MIFWT_ERR_BADARG = inconsistent, 1 = served
int fused_check(const mifwt_level_desc* d, int inverse) {
  if (const int bad = desc_prelude(d)) return bad;
  if (d->mode < MIFWT_MODE_ZERO || d->mode > MIFWT_MODE_SYMMETRIC) return MIFWT_ERR_BADARG;
  for (int ax = 0; ax < d->ndim; ++ax) {
    const int64_t n = d->sig_extent[ax], m = d->coef_extent[ax];
    if (n < 1 || m < 1 || (n != 2 * m && n != 2 * m - 1)) return MIFWT_ERR_BADARG;
    if (2 * m < d->filt_len) return MIFWT_ERR_BADARG;  // a level needs L <= N
  }
  (void)inverse;
  for (int ax = 0; ax < d->ndim; ++ax)
    if (2 * d->coef_extent[ax] < 2 * (d->filt_len - 1)) return 0;  // the two ends overlap: no compact table
  return fused_envelope(d);
}

template <typename T, int L>
int launch_fused(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* flo, const double* fhi,
                 const mifwt_bwt_tables* tb, hipStream_t stream) {
  static_assert(FwdTile<T, L>::LDS2 <= 65536 && InvTile<T, L>::LDS2 <= 65536, "tile does not fit the default LDS allowance");
  BwtArgs<T, L> a;
  fill_level_args(a, d, inverse, in, out, flo, fhi, Vec16<T>::E);
  const int nd = d->ndim;
  a.batch = (int)d->batch;
  a.src_r = nd == 2 ? ext_index(a.n_r, a.n_r, d->mode) : -1;
  a.src_c = ext_index(a.n_c, a.n_c, d->mode);
  a.tab = tb->rows;
  if (d->batch == 0) return MIFWT_OK;
  const int tcw = nd == 2 ? (inverse ? InvTile<T, L>::TQC : FwdTile<T, L>::TC) : (inverse ? InvTile<T, L>::TQ1 : FwdTile<T, L>::TC1);
  const int64_t grid = cut_tiles(a, a.m_c, a.m_r, tcw, inverse ? InvTile<T, L>::TQ : FwdTile<T, L>::TR, d->batch);
  if (grid < 0) return MIFWT_ERR_UNSUPPORTED;
  const dim3 g((unsigned)grid), blk(256);
  if (nd == 2) {
    if (inverse)
      hipLaunchKernelGGL((bwt_inv2_kernel<T, L>), g, blk, 0, stream, a);
    else
      hipLaunchKernelGGL((bwt_fwd2_kernel<T, L>), g, blk, 0, stream, a);
  } else {
    if (inverse)
      hipLaunchKernelGGL((bwt_inv1_kernel<T, L>), g, blk, 0, stream, a);
    else
      hipLaunchKernelGGL((bwt_fwd1_kernel<T, L>), g, blk, 0, stream, a);
  }
  return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
}

template <typename T>
int dispatch_len(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* flo, const double* fhi,
                 const mifwt_bwt_tables* tb, hipStream_t stream) {
  return for_even_len(d->filt_len,
                      [&](auto len) { return launch_fused<T, decltype(len)::value>(d, inverse, in, out, flo, fhi, tb, stream); });
}

int bwt_level(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi,
              const mifwt_bwt_tables* tb, void* stream) {
  const int ok = fused_check(d, inverse);
  if (ok < 0) return ok;
  if (!tb || !tb->rows) return MIFWT_ERR_BADARG;
  const int L = d->filt_len;
  if (!table_fits(tb, L)) return MIFWT_ERR_BADARG;
  if (const int bad = level_pointers(d, inverse, in, out, lo, hi)) return bad;
  if (!ok) return MIFWT_ERR_UNSUPPORTED;
  double flo[MIFWT_MAX_FILT], fhi[MIFWT_MAX_FILT];
  bank_taps(inverse, L, lo, hi, flo, fhi);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return d->dtype == MIFWT_F32 ? dispatch_len<float>(d, inverse, in, out, flo, fhi, tb, st)
                               : dispatch_len<double>(d, inverse, in, out, flo, fhi, tb, st);
}

int bwt_axis(int inverse, int dtype, int filt_len, int mode, int64_t outer, int64_t n, int64_t inner, const void* in0, const void* in1,
             void* out0, void* out1, const int64_t* sig_s, const int64_t* lo_s, const int64_t* hi_s, const double* lo, const double* hi,
             const mifwt_bwt_tables* tb, void* stream) {
  if (!tb || !tb->rows) return MIFWT_ERR_BADARG;
  if (mode < MIFWT_MODE_ZERO || mode > MIFWT_MODE_SYMMETRIC) return MIFWT_ERR_BADARG;
  if (const int bad = axis_check(inverse, dtype, filt_len, outer, n, inner, in0, in1, out0, out1, sig_s, lo_s, hi_s, lo, hi)) return bad;
  const int64_t m = (n + 1) / 2;
  if (2 * m < 2 * (int64_t)(filt_len - 1)) return filt_len <= 2 * m ? MIFWT_ERR_UNSUPPORTED : MIFWT_ERR_BADARG;
  if (!table_fits(tb, filt_len)) return MIFWT_ERR_BADARG;
  double flo[MIFWT_MAX_FILT], fhi[MIFWT_MAX_FILT];
  bank_taps(inverse, filt_len, lo, hi, flo, fhi);
  BwtAxisArgs a;
  if (const int bad = fill_axis_args(a, filt_len, outer, n, m, inner, in0, in1, out0, out1, sig_s, lo_s, hi_s, flo, fhi)) return bad;
  a.src = ext_index((int)n, (int)n, mode);
  a.nt = tb->n_top;
  a.nb = tb->n_bot;
  a.ntab = a.nt + a.nb > 0 ? a.nt + a.nb : 1;
  a.tab = tb->rows;
  const int64_t total = outer * (inverse ? n : m) * inner;
  if (total == 0) return MIFWT_OK;
  return launch_axis(dtype, inverse, total, 8192, stream, a, bwt_axis_generic<float, false>, bwt_axis_generic<float, true>,
                     bwt_axis_generic<double, false>, bwt_axis_generic<double, true>);
}

}  // namespace

}  // namespace mifwt

extern "C" {

int mifwt_bwt_supported(const mifwt_level_desc* desc, int direction) {
  if (direction != 0 && direction != 1) return MIFWT_ERR_BADARG;
  return mifwt::fused_check(desc, direction);
}

int mifwt_bwt_kernel_id(const mifwt_level_desc* desc, int direction) {
  return mifwt::kernel_id_answer(mifwt_bwt_supported(desc, direction), direction, MIFWT_KID_BWT_FWD, MIFWT_KID_BWT_INV);
}

int mifwt_bwt_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* lo, const double* hi,
                  const mifwt_bwt_tables* tables, void* stream) {
  const void* in[4] = {x, nullptr, nullptr, nullptr};
  void* out[4];
  if (const int bad = mifwt::pack_bands<void*>(desc, approx, details, out)) return bad;
  return mifwt::bwt_level(desc, 0, in, out, lo, hi, tables, stream);
}

int mifwt_bwt_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* lo, const double* hi,
                  const mifwt_bwt_tables* tables, void* stream) {
  const void* in[4];
  void* out[4] = {y, nullptr, nullptr, nullptr};
  if (const int bad = mifwt::pack_bands<const void*>(desc, approx, details, in)) return bad;
  return mifwt::bwt_level(desc, 1, in, out, lo, hi, tables, stream);
}

int mifwt_bwt_axis_fwd(int dtype, int filt_len, int mode, int64_t outer, int64_t n, int64_t inner, const void* x, const int64_t* x_strides,
                       void* lo_out, const int64_t* lo_strides, void* hi_out, const int64_t* hi_strides, const double* lo, const double* hi,
                       const mifwt_bwt_tables* tables, void* stream) {
  return mifwt::bwt_axis(0, dtype, filt_len, mode, outer, n, inner, x, nullptr, lo_out, hi_out, x_strides, lo_strides, hi_strides, lo, hi,
                         tables, stream);
}

int mifwt_bwt_axis_inv(int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* lo_in, const int64_t* lo_strides,
                       const void* hi_in, const int64_t* hi_strides, void* y, const int64_t* y_strides, const double* lo, const double* hi,
                       const mifwt_bwt_tables* tables, void* stream) {
  return mifwt::bwt_axis(1, dtype, filt_len, MIFWT_MODE_ZERO, outer, n, inner, lo_in, hi_in, y, nullptr, y_strides, lo_strides, hi_strides,
                         lo, hi, tables, stream);
}

}  // extern "C"
