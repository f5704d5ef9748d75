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
#include "mifwt_bwt_rows.h"

namespace mifwt {

namespace {

// ---- tile geometry (compile time; LDS stays below the 64 KB a kernel gets without opting in) ---------------------------------------------
template <typename T, int L>
struct FwdTile {
  static constexpr int E = BwtVec<T>::E;
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
  static constexpr int E = BwtVec<T>::E;
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

template <typename T, int L>
struct BwtArgs {
  const void* in[4];   // analysis: in[0] = x;  synthesis: the 2^ndim bands
  void* out[4];        // analysis: the bands;  synthesis: out[0] = y
  int64_t sig_bs, sig_rs;   // signal side: batch / row stride (elements; samples contiguous).  1-D: rows = batch, sig_rs unused
  int64_t a_bs, a_rs, d_bs, d_rs;  // band 0 / bands 1..: batch / row strides
  int batch, n_r, n_c;      // real signal extents (1-D: n_r = 1)
  int m_r, m_c;             // coefficient extents = ceil(n / 2)
  int src_r, src_c;         // source index of the virtual sample of an odd extent (-1: zero)
  int sig_vec, coef_vec;    // 16-byte accesses allowed on the signal / coefficient side
  int tiles_c, tiles_r;
  const double* tab;        // DEVICE [2][max(nt + nb, 1)][L]
  T lo[L], hi[L];           // f_lo, f_hi
};

// ---- analysis, 2-D -----------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_fwd2_kernel(const BwtArgs<T, L> a) {
  typedef FwdTile<T, L> G;
  typedef typename BwtVec<T>::type V;
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
      for (int k = 0; k < L; ++k) {
        const V vl = *reinterpret_cast<const V*>(hl0 + (w0 + k) * TC);
        const V vh = *reinterpret_cast<const V*>(hh0 + (w0 + k) * TC);
        const T cl = a.lo[L - 1 - k], ch = a.hi[L - 1 - k];
        ll += cl * vl;
        lh += cl * vh;
        hl += ch * vl;
        hh += ch * vh;
      }
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
    const int valid = a.m_c - mc;
    const int64_t oa = (int64_t)b * a.a_bs + (int64_t)m * a.a_rs + mc;
    const int64_t od = (int64_t)b * a.d_bs + (int64_t)m * a.d_rs + mc;
    store_vec<T>(static_cast<T*>(a.out[0]) + oa, ll, valid, a.coef_vec);
    store_vec<T>(static_cast<T*>(a.out[1]) + od, lh, valid, a.coef_vec);
    store_vec<T>(static_cast<T*>(a.out[2]) + od, hl, valid, a.coef_vec);
    store_vec<T>(static_cast<T*>(a.out[3]) + od, hh, valid, a.coef_vec);
  }
}

// ---- analysis, 1-D: a piece of one row per workgroup -----------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_fwd1_kernel(const BwtArgs<T, L> a) {
  typedef FwdTile<T, L> G;
  typedef typename BwtVec<T>::type V;
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
  typedef typename BwtVec<T>::type V;
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
  typedef typename BwtVec<T>::type V;
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
struct AxisArgs {
  const void* in0;  // analysis: x       synthesis: lo
  const void* in1;  //                   synthesis: hi
  void* out0;       // analysis: lo      synthesis: y
  void* out1;       // analysis: hi
  int64_t sig_s[3], lo_s[3], hi_s[3];  // (outer, axis, inner) strides in elements
  int64_t outer, inner;
  int n, m, src, filt_len, nt, nb, ntab;
  const double* tab;
  double lo[MIFWT_MAX_FILT], hi[MIFWT_MAX_FILT];
};

template <typename T, bool INVERSE>
__global__ void __launch_bounds__(256) bwt_axis_generic(const AxisArgs a) {
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
  if (!d) return MIFWT_ERR_BADARG;
  if (d->ndim < 1 || d->ndim > MIFWT_MAX_NDIM || d->filt_len < 2 || d->filt_len > MIFWT_MAX_FILT || (d->filt_len & 1) || d->batch < 0)
    return MIFWT_ERR_BADARG;
  if (d->dtype != MIFWT_F32 && d->dtype != MIFWT_F64 && !is_storage16(d->dtype)) return MIFWT_ERR_BADARG;
  if (d->mode < MIFWT_MODE_ZERO || d->mode > MIFWT_MODE_SYMMETRIC) return MIFWT_ERR_BADARG;
  for (int ax = 0; ax < d->ndim; ++ax) {
    const int64_t n = d->sig_extent[ax], m = d->coef_extent[ax];
    if (n < 1 || m < 1 || (n != 2 * m && n != 2 * m - 1)) return MIFWT_ERR_BADARG;
    if (2 * m < d->filt_len) return MIFWT_ERR_BADARG;  // a level needs L <= N
  }
  (void)inverse;
  if (d->ndim > 2 || d->filt_len > 20 || (d->dtype != MIFWT_F32 && d->dtype != MIFWT_F64)) return 0;
  const int last = d->ndim;
  if (d->sig_stride[last] != 1 || d->approx_stride[last] != 1 || d->detail_stride[last] != 1) return 0;
  int64_t tiles = d->batch;
  for (int ax = 0; ax < d->ndim; ++ax) {
    if (2 * d->coef_extent[ax] < 2 * (d->filt_len - 1)) return 0;  // the two ends overlap: no compact table
    if (d->coef_extent[ax] > (1 << 29)) return 0;
    tiles *= (d->coef_extent[ax] + 7) / 8;
  }
  if (tiles > INT32_MAX) return 0;
  return 1;
}

template <typename T, int L>
int launch_fused(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* flo, const double* fhi,
                 const mifwt_bwt_tables* tb, hipStream_t stream) {
  constexpr int E = BwtVec<T>::E;
  static_assert(FwdTile<T, L>::LDS2 <= 65536 && InvTile<T, L>::LDS2 <= 65536, "tile does not fit the default LDS allowance");
  BwtArgs<T, L> a;
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
  a.batch = (int)d->batch;
  a.n_r = nd == 2 ? (int)d->sig_extent[0] : 1;
  a.m_r = nd == 2 ? (int)d->coef_extent[0] : 1;
  a.n_c = (int)d->sig_extent[nd - 1];
  a.m_c = (int)d->coef_extent[nd - 1];
  a.src_r = nd == 2 ? ext_index(a.n_r, a.n_r, d->mode) : -1;
  a.src_c = ext_index(a.n_c, a.n_c, d->mode);
  const void* sig = inverse ? out[0] : in[0];
  a.sig_vec = aligned16(sig) && a.sig_bs % E == 0 && a.sig_rs % E == 0;
  a.coef_vec = a.a_bs % E == 0 && a.d_bs % E == 0 && a.a_rs % E == 0 && a.d_rs % E == 0;
  for (int s = 0; s < nb; ++s) a.coef_vec = a.coef_vec && aligned16(inverse ? in[s] : (const void*)out[s]);
  a.tab = tb->rows;
  for (int t = 0; t < L; ++t) {
    a.lo[t] = (T)flo[t];
    a.hi[t] = (T)fhi[t];
  }
  if (d->batch == 0) return MIFWT_OK;
  int64_t grid;
  if (nd == 2) {
    const int tcw = inverse ? InvTile<T, L>::TQC : FwdTile<T, L>::TC, trw = inverse ? InvTile<T, L>::TQ : FwdTile<T, L>::TR;
    a.tiles_c = (a.m_c + tcw - 1) / tcw;
    a.tiles_r = (a.m_r + trw - 1) / trw;
    grid = (int64_t)a.tiles_c * a.tiles_r * d->batch;
  } else {
    const int tcw = inverse ? InvTile<T, L>::TQ1 : FwdTile<T, L>::TC1;
    a.tiles_c = (a.m_c + tcw - 1) / tcw;
    a.tiles_r = 1;
    grid = (int64_t)a.tiles_c * d->batch;
  }
  if (grid > INT32_MAX) return MIFWT_ERR_UNSUPPORTED;
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
  switch (d->filt_len) {
#define MIFWT_BWT_CASE(LEN) \
  case LEN: return launch_fused<T, LEN>(d, inverse, in, out, flo, fhi, tb, stream);
    MIFWT_BWT_CASE(2)
    MIFWT_BWT_CASE(4)
    MIFWT_BWT_CASE(6)
    MIFWT_BWT_CASE(8)
    MIFWT_BWT_CASE(10)
    MIFWT_BWT_CASE(12)
    MIFWT_BWT_CASE(14)
    MIFWT_BWT_CASE(16)
    MIFWT_BWT_CASE(18)
    MIFWT_BWT_CASE(20)
#undef MIFWT_BWT_CASE
    default: return MIFWT_ERR_UNSUPPORTED;
  }
}

int bwt_level(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi,
              const mifwt_bwt_tables* tb, void* stream) {
  const int ok = fused_check(d, inverse);
  if (ok < 0) return ok;
  if (!lo || !hi || !tb || !tb->rows) return MIFWT_ERR_BADARG;
  const int L = d->filt_len;
  if (!table_fits(tb, L)) return MIFWT_ERR_BADARG;
  for (int s = 0; s < (1 << (d->ndim > 2 ? 0 : d->ndim)); ++s)
    if (!(inverse ? in[s] : (const void*)out[s])) return MIFWT_ERR_BADARG;
  if (!(inverse ? (const void*)out[0] : in[0])) return MIFWT_ERR_BADARG;
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
  if (!in0 || !out0 || (inverse ? !in1 : !out1) || !sig_s || !lo_s || !hi_s || !lo || !hi || !tb || !tb->rows) return MIFWT_ERR_BADARG;
  if (filt_len < 2 || (filt_len & 1) || filt_len > MIFWT_MAX_FILT || outer < 0 || inner < 0 || n < 1) return MIFWT_ERR_BADARG;
  if (mode < MIFWT_MODE_ZERO || mode > MIFWT_MODE_SYMMETRIC) return MIFWT_ERR_BADARG;
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return is_storage16(dtype) ? MIFWT_ERR_UNSUPPORTED : MIFWT_ERR_BADARG;
  const int64_t m = (n + 1) / 2;
  if (2 * m < 2 * (int64_t)(filt_len - 1)) return filt_len <= 2 * m ? MIFWT_ERR_UNSUPPORTED : MIFWT_ERR_BADARG;
  if (!table_fits(tb, filt_len)) return MIFWT_ERR_BADARG;
  if (n > INT32_MAX / 4) return MIFWT_ERR_UNSUPPORTED;
  AxisArgs a;
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
  a.src = ext_index((int)n, (int)n, mode);
  a.filt_len = filt_len;
  a.nt = tb->n_top;
  a.nb = tb->n_bot;
  a.ntab = a.nt + a.nb > 0 ? a.nt + a.nb : 1;
  a.tab = tb->rows;
  bank_taps(inverse, filt_len, lo, hi, a.lo, a.hi);
  const int64_t total = outer * (inverse ? n : m) * inner;
  if (total == 0) return MIFWT_OK;
  const int64_t blocks = (total + 255) / 256;
  const dim3 g((unsigned)(blocks < 8192 ? blocks : 8192)), blk(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MIFWT_F32) {
    if (inverse)
      hipLaunchKernelGGL((bwt_axis_generic<float, true>), g, blk, 0, st, a);
    else
      hipLaunchKernelGGL((bwt_axis_generic<float, false>), g, blk, 0, st, a);
  } else {
    if (inverse)
      hipLaunchKernelGGL((bwt_axis_generic<double, true>), g, blk, 0, st, a);
    else
      hipLaunchKernelGGL((bwt_axis_generic<double, false>), g, blk, 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
}

}  // namespace

}  // namespace mifwt

extern "C" {

int mifwt_bwt_supported(const mifwt_level_desc* desc, int direction) {
  if (direction != 0 && direction != 1) return MIFWT_ERR_BADARG;
  return mifwt::fused_check(desc, direction);
}

int mifwt_bwt_kernel_id(const mifwt_level_desc* desc, int direction) {
  const int ok = mifwt_bwt_supported(desc, direction);
  if (ok < 0) return ok;
  return ok ? (direction ? MIFWT_KID_BWT_INV : MIFWT_KID_BWT_FWD) : MIFWT_ERR_UNSUPPORTED;
}

int mifwt_bwt_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* lo, const double* hi,
                  const mifwt_bwt_tables* tables, void* stream) {
  if (!desc || desc->ndim < 1 || desc->ndim > MIFWT_MAX_NDIM) return MIFWT_ERR_BADARG;
  if (desc->ndim <= 2 && !details) return MIFWT_ERR_BADARG;
  const void* in[4] = {x, nullptr, nullptr, nullptr};
  void* out[4] = {approx, nullptr, nullptr, nullptr};
  if (desc->ndim <= 2)
    for (int s = 1; s < (1 << desc->ndim); ++s) out[s] = details[s - 1];
  return mifwt::bwt_level(desc, 0, in, out, lo, hi, tables, stream);
}

int mifwt_bwt_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* lo, const double* hi,
                  const mifwt_bwt_tables* tables, void* stream) {
  if (!desc || desc->ndim < 1 || desc->ndim > MIFWT_MAX_NDIM) return MIFWT_ERR_BADARG;
  if (desc->ndim <= 2 && !details) return MIFWT_ERR_BADARG;
  const void* in[4] = {approx, nullptr, nullptr, nullptr};
  void* out[4] = {y, nullptr, nullptr, nullptr};
  if (desc->ndim <= 2)
    for (int s = 1; s < (1 << desc->ndim); ++s) in[s] = details[s - 1];
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
