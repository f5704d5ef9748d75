// mifwt_ext.hip — padded levels whose extension is a VALUE map (PyWavelets modes "smooth", "antisymmetric", "antireflect") for gfx950:
// kernel ids 42 / 43 (fused analysis level and its adjoint, one or two transformed axes) and 44 / 45 (one axis, any strides, run-time tap
// loop).  The contract is in include/mifwt.h:
//   extension  xe[i] = sum of at most three source samples with small integer weights (ext_terms below), any integer i
//   analysis   c[k] = sum_j f[j] xe[2 k + 1 - j],  0 <= k < M = floor((N + L - 1) / 2)      (the padded level of mode "zero" with xe for the zeros)
//   adjoint    T[i] = sum_k f_lo[2 k + 1 - i] g_a[k] + f_hi[2 k + 1 - i] g_d[k]  over the padded extent -(L-2) <= i < N + L - 2 + (N mod 2),
//              g_x[s] = sum_i E[i, s] T[i],  E[i, s] = weight of x[s] in xe[i]
// so an output k of the analysis reads the window 2 k - (L - 2) .. 2 k + 1.
//
// Bound: HBM (a level reads N samples and writes about N per axis).  Fused analysis (unit innermost strides, f32 / f64, even L <= 20):
//   2-D: a workgroup of 256 threads owns TR x TC coefficients.  It stages the (2 TR + L - 2) x (2 TC + L - 2) window of xe in LDS (16-byte
//        loads where the window lies inside the plane; elsewhere every staged sample is the weighted sum of its terms: a row outside the
//        plane is the weighted sum of at most three column-extended source rows, which also gives the corners), filters it along the rows
//        into LDS, along the columns into registers and stores the four bands with 16-byte stores.
//   1-D: the row half of the same code, a chunk of one row per workgroup.
// Fused adjoint: a gather.  A sample away from the edges is not met by any padded sample, so g_x[s] = T[s]: L / 2 taps of each band.  A
//   sample within L of an edge adds E[i, s] T[i] over the pad of that edge (left pad only for s <= L - 1, right pad only for s >= N - 1 - L:
//   where the extension wraps more than once, N <= L, both hold for every s).  T is formed on the fly, in registers: no padded-extent
//   tensor exists.  2-D: a workgroup owns TSR x TSC samples; it applies the column adjoint to the coefficient rows behind its sample rows
//   (global -> LDS, two planes: low / high band along the rows), then the row adjoint from LDS, and stores 16 bytes per lane.
// Everything else (L > 20, any strides, the depth axis of a 3-D level) runs ext_axis_kernel: one thread per output, run-time tap loop,
// double accumulators.
// Shared with the other fused-level units, from mifwt_level_tile.h: the 16-byte vectors, the row pass over the aligned window (left
// reach H = L - 2), the tap step of the column pass and the band stores, the common kernel arguments and their fill, the tile cut, the
// descriptor prelude and envelope, the length dispatch, the packing of the level entries and the axis-pass arguments and launcher.
// Here: the value map, the staging with its partial windows, the geometry, the adjoint kernels and the launches.
#include "mifwt_level_tile.h"

namespace mifwt {

namespace {

// ---- the extension: xe[i] = w[0] x[idx[0]] + w[1] x[idx[1]] + w[2] x[idx[2]] (a weight 0 marks an unused term) -----------------------------
struct Terms {
  int idx[3];
  int w[3];
};

// floor division
__device__ __forceinline__ void fdivmod(int i, int m, int& q, int& r) {
  q = i / m;
  r = i - q * m;
  if (r < 0) {
    r += m;
    --q;
  }
}

__device__ __forceinline__ Terms ext_terms(int i, int n, int mode) {
  Terms t;
  t.idx[0] = t.idx[1] = t.idx[2] = 0;
  t.w[0] = 1;
  t.w[1] = t.w[2] = 0;
  if (i >= 0 && i < n) {
    t.idx[0] = i;
    return t;
  }
  if (mode == MIFWT_EXT_ANTISYMMETRIC) {  // ... -x[1] -x[0] | x | -x[n-1] -x[n-2] ...
    int q, r;
    fdivmod(i, n, q, r);
    if (q & 1) {
      t.idx[0] = n - 1 - r;
      t.w[0] = -1;
    } else {
      t.idx[0] = r;
    }
    return t;
  }
  if (n == 1) return t;  // smooth / antireflect of one sample: that sample
  if (mode == MIFWT_EXT_ANTIREFLECT) {  // point reflection about the edge samples, period 2 (n - 1) up to a linear drift
    int q, r;
    fdivmod(i, n - 1, q, r);
    t.idx[1] = n - 1;
    t.idx[2] = 0;
    if (q & 1) {
      t.idx[0] = n - 1 - r;
      t.w[0] = -1;
      t.w[1] = q + 1;
      t.w[2] = -(q - 1);
    } else {
      t.idx[0] = r;
      t.w[1] = q;
      t.w[2] = -q;
    }
    return t;
  }
  if (i < 0) {  // smooth: the line through the two edge samples
    t.idx[0] = 0;
    t.w[0] = 1 - i;
    t.idx[1] = 1;
    t.w[1] = i;
  } else {
    const int k = i - n + 1;
    t.idx[0] = n - 1;
    t.w[0] = 1 + k;
    t.idx[1] = n - 2;
    t.w[1] = -k;
  }
  return t;
}

// E[i, s]: weight of x[s] in xe[i]
__device__ __forceinline__ int ext_weight(int i, int s, int n, int mode) {
  const Terms t = ext_terms(i, n, mode);
  int w = 0;
#pragma unroll
  for (int q = 0; q < 3; ++q) w += t.idx[q] == s ? t.w[q] : 0;
  return w;
}

// xe[i] of a line of n samples with stride `st`
template <typename A, typename T>
__device__ __forceinline__ A ext_value(const T* __restrict__ line, int64_t st, int i, int n, int mode) {
  const Terms t = ext_terms(i, n, mode);
  A v = (A)t.w[0] * (A)line[(int64_t)t.idx[0] * st];
#pragma unroll
  for (int q = 1; q < 3; ++q)
    if (t.w[q] != 0) v += (A)t.w[q] * (A)line[(int64_t)t.idx[q] * st];
  return v;
}

// ---- the adjoint of one axis at sample s -----------------------------------------------------------------------------------------------------
// acc += w T[i]; g(k, cl, ch, acc) adds cl g_a[k] + ch g_d[k].  Tap j of coefficient k meets position i = 2 k + 1 - j.
template <typename C, typename Acc, typename F>
__device__ __forceinline__ void tconv_add(int i, int m, int L, const C* lo, const C* hi, C w, Acc& acc, F&& g) {
  const int j0 = (i + 1) & 1;
  int k = (i + j0 - 1) >> 1;  // (an even number: the shift is exact, also below zero)
  for (int j = j0; j < L; j += 2, ++k)
    if (k >= 0 && k < m) g(k, w * lo[j], w * hi[j], acc);
}

template <typename C, typename Acc, typename F>
__device__ __forceinline__ void adjoint_at(int s, int n, int m, int L, int mode, const C* lo, const C* hi, Acc& acc, F&& g) {
  tconv_add(s, m, L, lo, hi, C(1), acc, g);
  if (s <= L - 1)
    for (int i = -(L - 2); i < 0; ++i) {
      const int w = ext_weight(i, s, n, mode);
      if (w != 0) tconv_add(i, m, L, lo, hi, C(w), acc, g);
    }
  if (s >= n - 1 - L)
    for (int i = n; i < n + L - 2 + (n & 1); ++i) {
      const int w = ext_weight(i, s, n, mode);
      if (w != 0) tconv_add(i, m, L, lo, hi, C(w), acc, g);
    }
}

// ---- tile geometry (compile time; static LDS below 64 KB, at least two workgroups per CU) ----------------------------------------------
template <typename T, int L>
struct FwdGeo {
  static constexpr int E = Vec16<T>::E;
  static constexpr int H = L - 2;                     // samples of the window left of sample 2 k
  static constexpr int TC = 16 * E;                   // coefficient columns per tile: 16 lanes x one 16-byte store
  static constexpr int TR = 16;                       // coefficient rows per tile: one column-pass item per thread
  static constexpr int PAD = RowWindow<T, L, H>::PAD;  // staged columns left of sample 2 mc0 (keeps the staged vectors aligned)
  static constexpr int WC = round_up(PAD + 2 * TC, E);
  static constexpr int XP = WC + E;                   // pitch of the staged window (a lane's last piece may end inside the pad)
  static constexpr int WR = 2 * TR + L - 2;
  static constexpr int HP = TC + E;                   // pitch of the row-filtered planes: one access width against bank conflicts
  static constexpr int TC1 = 256 * E;                 // 1-D: coefficients per workgroup
  static constexpr int WC1 = round_up(PAD + 2 * TC1, E);
  static constexpr int LDS2 = (WR * XP + 2 * WR * HP) * (int)sizeof(T);
};

template <typename T, int L>
struct AdjGeo {
  static constexpr int E = Vec16<T>::E;
  static constexpr int TSC = 16 * E;                  // sample columns per tile
  static constexpr int TSR = 16;                      // sample rows per tile
  static constexpr int KWR = TSR / 2 + 3 * L / 2;     // coefficient rows behind a tile's rows: both pads where the axis is short
  static constexpr int TS1 = 256 * E;                 // 1-D: samples per workgroup
  static constexpr int LDS2 = 2 * KWR * TSC * (int)sizeof(T);
};

// analysis and adjoint take dec_lo / dec_hi;  coefficient extents = floor((n + L - 1) / 2)
template <typename T, int L>
struct ExtArgs : LevelArgs<T, L> {
  int mode;  // MIFWT_EXT_*
};

// E staged samples of extended row `gr` from extended column g0 (a multiple of E).  `mapped` = the tile's window leaves the plane.
template <typename T>
__device__ __forceinline__ void stage_ext(T* dst, const T* __restrict__ plane, int64_t rs, int gr, int g0, int n_r, int n_c, int mode,
                                          bool vec_ok, bool mapped) {
  constexpr int E = Vec16<T>::E;
  typedef typename Vec16<T>::type V;
  const bool row_in = !mapped || (gr >= 0 && gr < n_r);
  const bool col_in = !mapped || (g0 >= 0 && g0 + E <= n_c);
  if (row_in && col_in) {
    const T* row = plane + (int64_t)gr * rs;
    if (vec_ok) {
      *reinterpret_cast<V*>(dst) = *reinterpret_cast<const V*>(row + g0);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) dst[e] = row[g0 + e];
    }
    return;
  }
  // The weighted sum of up to nine samples in double, rounded once: the weights grow with the distance from the edge (up to L - 1 per
  // axis, their product in a corner), and a float32 sum of such terms would round at the size of its largest term several times.
  const Terms tr = ext_terms(gr, n_r, mode);  // (a 1-D level has n_r = 1 and gr = 0: the identity)
#pragma unroll
  for (int e = 0; e < E; ++e) {
    double v = (double)tr.w[0] * ext_value<double, T>(plane + (int64_t)tr.idx[0] * rs, 1, g0 + e, n_c, mode);
#pragma unroll
    for (int q = 1; q < 3; ++q)
      if (tr.w[q] != 0) v += (double)tr.w[q] * ext_value<double, T>(plane + (int64_t)tr.idx[q] * rs, 1, g0 + e, n_c, mode);
    dst[e] = (T)v;
  }
}

// ---- analysis, 2-D ---------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) ext_fwd2_kernel(const ExtArgs<T, L> a) {
  typedef FwdGeo<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TC = G::TC, TR = G::TR, H = G::H, WC = G::WC, WR = G::WR, XP = G::XP, HP = G::HP;
  __shared__ __attribute__((aligned(16))) T xs[WR * XP];
  __shared__ __attribute__((aligned(16))) T hs[2 * WR * HP];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tc = bid % a.tiles_c;
  bid /= a.tiles_c;
  const int tr = bid % a.tiles_r;
  const int b = bid / a.tiles_r;
  const int mc0 = tc * TC, mr0 = tr * TR;
  const int cs = 2 * mc0 - G::PAD, rs = 2 * mr0 - H;  // extended sample behind staged column / row 0
  const bool mapped = !(rs >= 0 && rs + WR <= a.n_r && cs >= 0 && cs + WC <= a.n_c);
  const T* __restrict__ x = static_cast<const T*>(a.in[0]) + (int64_t)b * a.sig_bs;
  // A tile that overhangs the plane (the padded coefficient count is rarely a multiple of the tile: 129 for 256 samples under db2) works
  // on the part of its window that feeds an output: the last coefficient of an axis reads up to extended sample 2 m - 1, so `wr` staged
  // rows and `tcg` groups of E coefficient columns.  What a lane's last 16-byte piece reads beyond the staged columns feeds no output.
  const int wr = min(WR, 2 * a.m_r - rs);
  const int tcg = min(TC / E, (a.m_c - mc0 + E - 1) / E);
  const int vpr = min(WC / E, G::PAD / E + 2 * tcg);
  for (int i = tid; i < wr * vpr; i += 256) {
    const int r = i / vpr, cv = i - r * vpr;
    if (cs + cv * E > 2 * a.m_c - 1)  // (a piece of the last group beyond the last window: extending it would cost up to nine loads a sample)
      *reinterpret_cast<V*>(xs + r * XP + cv * E) = V(0);
    else
      stage_ext<T>(xs + r * XP + cv * E, x, a.sig_rs, rs + r, cs + cv * E, a.n_r, a.n_c, a.mode, a.sig_vec, mapped);
  }
  __syncthreads();
  // along the rows of the window: (lo, hi) of every staged row
  for (int i = tid; i < wr * tcg; i += 256) {
    const int r = i / tcg, cg = i - r * tcg;
    V lo, hi;
    window_run<T, L, H>(xs + r * XP + 2 * cg * E, a.lo, a.hi, lo, hi);
    *reinterpret_cast<V*>(hs + r * HP + cg * E) = lo;
    *reinterpret_cast<V*>(hs + (WR + r) * HP + cg * E) = hi;
  }
  __syncthreads();
  // along the columns: four bands, E columns per lane
  for (int i = tid; i < TR * (TC / E); i += 256) {
    const int ro = i / (TC / E), cg = i - ro * (TC / E);
    const int m = mr0 + ro, mc = mc0 + cg * E;
    if (m >= a.m_r || mc >= a.m_c) continue;
    V ll = V(0), lh = V(0), hl = V(0), hh = V(0);
    const T* hl0 = hs + (2 * ro) * HP + cg * E;
    const T* hh0 = hl0 + WR * HP;
#pragma unroll
    for (int k = 0; k < L; ++k) column_tap<T>(hl0 + k * HP, hh0 + k * HP, a.lo[L - 1 - k], a.hi[L - 1 - k], ll, lh, hl, hh);
    store_bands<T, L>(a, b, m, mc, ll, lh, hl, hh);
  }
}

// ---- analysis, 1-D: a chunk of one row per workgroup -------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) ext_fwd1_kernel(const ExtArgs<T, L> a) {
  typedef FwdGeo<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TC = G::TC1, WC = G::WC1;
  __shared__ __attribute__((aligned(16))) T xs[WC + E];
  const int tid = threadIdx.x;
  const int tc = blockIdx.x % a.tiles_c;
  const int b = blockIdx.x / a.tiles_c;
  const int mc0 = tc * TC;
  const int cs = 2 * mc0 - G::PAD;
  const bool mapped = !(cs >= 0 && cs + WC <= a.n_c);
  const T* __restrict__ x = static_cast<const T*>(a.in[0]) + (int64_t)b * a.sig_bs;
  for (int i = tid; i < WC / E; i += 256) {
    if (cs + i * E > 2 * a.m_c - 1)  // (beyond the window of the last coefficient: feeds no output)
      *reinterpret_cast<V*>(xs + i * E) = V(0);
    else
      stage_ext<T>(xs + i * E, x, 0, 0, cs + i * E, 1, a.n_c, a.mode, a.sig_vec, mapped);
  }
  __syncthreads();
  const int mc = mc0 + tid * E;
  if (mc >= a.m_c) return;
  V lo, hi;
  window_run<T, L, G::H>(xs + 2 * tid * E, a.lo, a.hi, lo, hi);
  store_vec<T>(static_cast<T*>(a.out[0]) + (int64_t)b * a.a_bs + mc, lo, a.m_c - mc, a.coef_vec);
  store_vec<T>(static_cast<T*>(a.out[1]) + (int64_t)b * a.d_bs + mc, hi, a.m_c - mc, a.coef_vec);
}

// ---- adjoint, 2-D ----------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) ext_adj2_kernel(const ExtArgs<T, L> a) {
  typedef AdjGeo<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TSC = G::TSC, TSR = G::TSR, KWR = G::KWR;
  __shared__ __attribute__((aligned(16))) T us[2 * KWR * TSC];  // [band along the rows][coefficient row - k_lo][sample column]
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tc = bid % a.tiles_c;
  bid /= a.tiles_c;
  const int tr = bid % a.tiles_r;
  const int b = bid / a.tiles_r;
  const int sc0 = tc * TSC, sr0 = tr * TSR;
  const int sr1 = min(sr0 + TSR, a.n_r) - 1;  // last sample row of the tile
  // coefficient rows behind the positions of T that the tile's rows collect: their own and, near an edge, that edge's pad
  const int i_lo = sr0 <= L - 1 ? -(L - 2) : sr0;
  const int i_hi = sr1 >= a.n_r - 1 - L ? a.n_r + L - 3 + (a.n_r & 1) : sr1;
  const int k_lo = max(i_lo >> 1, 0);
  const int k_hi = min(min((i_hi + L - 2) >> 1, a.m_r - 1), k_lo + KWR - 1);
  const int kr = k_hi - k_lo + 1;
  // along the columns: both row bands of every coefficient row of the window, E sample columns per lane
  for (int i = tid; i < 2 * kr * (TSC / E); i += 256) {
    const int cg = i % (TSC / E), r = (i / (TSC / E)) % kr, br = i / ((TSC / E) * kr);
    const int k = k_lo + r;
    const T* ga = static_cast<const T*>(a.in[2 * br]) + (br ? (int64_t)b * a.d_bs + (int64_t)k * a.d_rs : (int64_t)b * a.a_bs + (int64_t)k * a.a_rs);
    const T* gd = static_cast<const T*>(a.in[2 * br + 1]) + (int64_t)b * a.d_bs + (int64_t)k * a.d_rs;
    V v = V(0);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int s = sc0 + cg * E + e;
      T acc = T(0);
      if (s < a.n_c)
        adjoint_at<T>(s, a.n_c, a.m_c, L, a.mode, a.lo, a.hi, acc,
                      [&](int kc, T cl, T ch, T& o) { o = fma(cl, ga[kc], fma(ch, gd[kc], o)); });
      v[e] = acc;
    }
    *reinterpret_cast<V*>(us + (br * KWR + r) * TSC + cg * E) = v;
  }
  __syncthreads();
  // along the rows
  T* __restrict__ y = static_cast<T*>(a.out[0]) + (int64_t)b * a.sig_bs;
  for (int i = tid; i < TSR * (TSC / E); i += 256) {
    const int cg = i % (TSC / E), rl = i / (TSC / E);
    const int s = sr0 + rl, sc = sc0 + cg * E;
    if (s >= a.n_r || sc >= a.n_c) continue;
    const T* u0 = us + cg * E;
    const T* u1 = u0 + KWR * TSC;
    V acc = V(0);
    adjoint_at<T>(s, a.n_r, a.m_r, L, a.mode, a.lo, a.hi, acc, [&](int k, T cl, T ch, V& o) {
      if (k >= k_lo && k <= k_hi)
        o += cl * *reinterpret_cast<const V*>(u0 + (k - k_lo) * TSC) + ch * *reinterpret_cast<const V*>(u1 + (k - k_lo) * TSC);
    });
    store_vec<T>(y + (int64_t)s * a.sig_rs + sc, acc, a.n_c - sc, a.sig_vec);
  }
}

// ---- adjoint, 1-D: E samples per lane ------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) ext_adj1_kernel(const ExtArgs<T, L> a) {
  typedef AdjGeo<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TS1 = G::TS1;
  const int tc = blockIdx.x % a.tiles_c;
  const int b = blockIdx.x / a.tiles_c;
  const int sc = tc * TS1 + threadIdx.x * E;
  if (sc >= a.n_c) return;
  const T* ga = static_cast<const T*>(a.in[0]) + (int64_t)b * a.a_bs;
  const T* gd = static_cast<const T*>(a.in[1]) + (int64_t)b * a.d_bs;
  V v = V(0);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    T acc = T(0);
    if (sc + e < a.n_c)
      adjoint_at<T>(sc + e, a.n_c, a.m_c, L, a.mode, a.lo, a.hi, acc,
                    [&](int k, T cl, T ch, T& o) { o = fma(cl, ga[k], fma(ch, gd[k], o)); });
    v[e] = acc;
  }
  store_vec<T>(static_cast<T*>(a.out[0]) + (int64_t)b * a.sig_bs + sc, v, a.n_c - sc, a.sig_vec);
}

// ---- one axis of [outer, n, inner] arrays: any even L <= MIFWT_MAX_FILT, any strides -----------------------------------------------------------
struct ExtAxisArgs : AxisArgsBase {
  int mode;  // MIFWT_EXT_*
};

template <typename T, bool ADJOINT>
__global__ void __launch_bounds__(256) ext_axis_kernel(const ExtAxisArgs a) {
  const int L = a.filt_len;
  const int64_t len = ADJOINT ? a.n : a.m;
  const int64_t total = a.outer * len * a.inner;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t in = idx % a.inner, o = idx / (a.inner * len);
    const int pos = (int)((idx / a.inner) % len);
    if (!ADJOINT) {
      const T* x = static_cast<const T*>(a.in0) + o * a.sig_s[0] + in * a.sig_s[2];
      const int top = 2 * pos + 1;  // position of tap 0; tap j reads j samples further back
      const bool inside = top < a.n && top - (L - 1) >= 0;
      double sl = 0, sh = 0;
      for (int j = 0; j < L; ++j) {
        const double v = inside ? (double)x[(int64_t)(top - j) * a.sig_s[1]] : ext_value<double, T>(x, a.sig_s[1], top - j, a.n, a.mode);
        sl = fma(a.lo[j], v, sl);
        sh = fma(a.hi[j], v, sh);
      }
      static_cast<T*>(a.out0)[o * a.lo_s[0] + (int64_t)pos * a.lo_s[1] + in * a.lo_s[2]] = (T)sl;
      static_cast<T*>(a.out1)[o * a.hi_s[0] + (int64_t)pos * a.hi_s[1] + in * a.hi_s[2]] = (T)sh;
    } else {
      const T* gl = static_cast<const T*>(a.in0) + o * a.lo_s[0] + in * a.lo_s[2];
      const T* gh = static_cast<const T*>(a.in1) + o * a.hi_s[0] + in * a.hi_s[2];
      const int64_t sl = a.lo_s[1], sh = a.hi_s[1];
      double acc = 0;
      adjoint_at<double>(pos, a.n, a.m, L, a.mode, a.lo, a.hi, acc, [&](int k, double cl, double ch, double& r) {
        r = fma(cl, (double)gl[(int64_t)k * sl], fma(ch, (double)gh[(int64_t)k * sh], r));
      });
      static_cast<T*>(a.out0)[o * a.sig_s[0] + (int64_t)pos * a.sig_s[1] + in * a.sig_s[2]] = (T)acc;
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
bool mode_ok(int ext_mode) {
  return ext_mode == MIFWT_EXT_SMOOTH || ext_mode == MIFWT_EXT_ANTISYMMETRIC || ext_mode == MIFWT_EXT_ANTIREFLECT;
}

// 0 = not served by the fused kernels, MIFWT_ERR_BADARG = inconsistent, 1 = served
int fused_check(const mifwt_level_desc* d, int ext_mode) {
  if (const int bad = desc_prelude(d)) return bad;
  if (!mode_ok(ext_mode)) return MIFWT_ERR_BADARG;
  for (int ax = 0; ax < d->ndim; ++ax) {
    const int64_t n = d->sig_extent[ax], m = d->coef_extent[ax];
    if (n < 1 || m != (n + d->filt_len - 1) / 2) return MIFWT_ERR_BADARG;
  }
  return fused_envelope(d);
}

template <typename T, int L>
int launch_fused(const mifwt_level_desc* d, int ext_mode, int adjoint, const void* const* in, void* const* out, const double* lo,
                 const double* hi, hipStream_t stream) {
  typedef FwdGeo<T, L> FG;
  typedef AdjGeo<T, L> AG;
  static_assert(FG::LDS2 <= 65536 && AG::LDS2 <= 65536, "tile does not fit the default LDS allowance");
  ExtArgs<T, L> a;
  fill_level_args(a, d, adjoint, in, out, lo, hi, Vec16<T>::E);
  a.mode = ext_mode;
  if (d->batch == 0) return MIFWT_OK;
  const int nd = d->ndim;
  // analysis cuts the coefficients, the adjoint the samples
  const int tcw = nd == 2 ? (adjoint ? AG::TSC : FG::TC) : (adjoint ? AG::TS1 : FG::TC1);
  const int64_t grid = adjoint ? cut_tiles(a, a.n_c, a.n_r, tcw, AG::TSR, d->batch) : cut_tiles(a, a.m_c, a.m_r, tcw, FG::TR, d->batch);
  if (grid < 0) return MIFWT_ERR_UNSUPPORTED;
  const dim3 g((unsigned)grid), blk(256);
  if (nd == 2) {
    if (adjoint)
      hipLaunchKernelGGL((ext_adj2_kernel<T, L>), g, blk, 0, stream, a);
    else
      hipLaunchKernelGGL((ext_fwd2_kernel<T, L>), g, blk, 0, stream, a);
  } else {
    if (adjoint)
      hipLaunchKernelGGL((ext_adj1_kernel<T, L>), g, blk, 0, stream, a);
    else
      hipLaunchKernelGGL((ext_fwd1_kernel<T, L>), g, blk, 0, stream, a);
  }
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  count_launch(adjoint ? MIFWT_KID_EXT_ADJ : MIFWT_KID_EXT_FWD);
  return MIFWT_OK;
}

template <typename T>
int dispatch_len(const mifwt_level_desc* d, int ext_mode, int adjoint, const void* const* in, void* const* out, const double* lo,
                 const double* hi, hipStream_t stream) {
  return for_even_len(d->filt_len,
                      [&](auto len) { return launch_fused<T, decltype(len)::value>(d, ext_mode, adjoint, in, out, lo, hi, stream); });
}

int ext_level(const mifwt_level_desc* d, int ext_mode, int adjoint, const void* const* in, void* const* out, const double* lo,
              const double* hi, void* stream) {
  const int ok = fused_check(d, ext_mode);
  if (ok < 0) return ok;
  if (const int bad = level_pointers(d, adjoint, in, out, lo, hi)) return bad;
  if (!ok) return MIFWT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return d->dtype == MIFWT_F32 ? dispatch_len<float>(d, ext_mode, adjoint, in, out, lo, hi, st)
                               : dispatch_len<double>(d, ext_mode, adjoint, in, out, lo, hi, st);
}

int ext_axis(int adjoint, int ext_mode, int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* in0, const void* in1,
             void* out0, void* out1, const int64_t* sig_s, const int64_t* lo_s, const int64_t* hi_s, const double* lo, const double* hi,
             void* stream) {
  if (!mode_ok(ext_mode)) return MIFWT_ERR_BADARG;
  if (const int bad = axis_check(adjoint, dtype, filt_len, outer, n, inner, in0, in1, out0, out1, sig_s, lo_s, hi_s, lo, hi)) return bad;
  ExtAxisArgs a;
  if (const int bad = fill_axis_args(a, filt_len, outer, n, (n + filt_len - 1) / 2, inner, in0, in1, out0, out1, sig_s, lo_s, hi_s, lo, hi))
    return bad;
  a.mode = ext_mode;
  const int64_t total = outer * (adjoint ? n : (int64_t)a.m) * inner;
  if (total == 0) return MIFWT_OK;
  const int rc = launch_axis(dtype, adjoint, total, 65536, stream, a, ext_axis_kernel<float, false>, ext_axis_kernel<float, true>,
                             ext_axis_kernel<double, false>, ext_axis_kernel<double, true>);
  if (rc != MIFWT_OK) return rc;
  count_launch(adjoint ? MIFWT_KID_EXT_AXIS_ADJ : MIFWT_KID_EXT_AXIS_FWD);
  return MIFWT_OK;
}

}  // namespace

}  // namespace mifwt

extern "C" {

int mifwt_ext_supported(const mifwt_level_desc* desc, int ext_mode, int direction) {
  if (direction != 0 && direction != 1) return MIFWT_ERR_BADARG;
  return mifwt::fused_check(desc, ext_mode);
}

int mifwt_ext_kernel_id(const mifwt_level_desc* desc, int ext_mode, int direction) {
  return mifwt::kernel_id_answer(mifwt_ext_supported(desc, ext_mode, direction), direction, MIFWT_KID_EXT_FWD, MIFWT_KID_EXT_ADJ);
}

int mifwt_ext_fwd(const mifwt_level_desc* desc, int ext_mode, const void* x, void* approx, void* const* details, const double* lo,
                  const double* hi, void* stream) {
  const void* in[4] = {x, nullptr, nullptr, nullptr};
  void* out[4];
  if (const int bad = mifwt::pack_bands<void*>(desc, approx, details, out)) return bad;
  return mifwt::ext_level(desc, ext_mode, 0, in, out, lo, hi, stream);
}

int mifwt_ext_adj(const mifwt_level_desc* desc, int ext_mode, const void* g_approx, const void* const* g_details, void* g_x, const double* lo,
                  const double* hi, void* stream) {
  const void* in[4];
  void* out[4] = {g_x, nullptr, nullptr, nullptr};
  if (const int bad = mifwt::pack_bands<const void*>(desc, g_approx, g_details, in)) return bad;
  return mifwt::ext_level(desc, ext_mode, 1, in, out, lo, hi, stream);
}

int mifwt_ext_axis_fwd(int ext_mode, int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* x, const int64_t* x_strides,
                       void* lo_out, const int64_t* lo_strides, void* hi_out, const int64_t* hi_strides, const double* lo, const double* hi,
                       void* stream) {
  return mifwt::ext_axis(0, ext_mode, dtype, filt_len, outer, n, inner, x, nullptr, lo_out, hi_out, x_strides, lo_strides, hi_strides, lo, hi,
                         stream);
}

int mifwt_ext_axis_adj(int ext_mode, int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* g_lo, const int64_t* lo_strides,
                       const void* g_hi, const int64_t* hi_strides, void* g_x, const int64_t* x_strides, const double* lo, const double* hi,
                       void* stream) {
  return mifwt::ext_axis(1, ext_mode, dtype, filt_len, outer, n, inner, g_lo, g_hi, g_x, nullptr, x_strides, lo_strides, hi_strides, lo, hi,
                         stream);
}

}  // extern "C"
