// mifwt_per.hip — levels of the PERIODIZED transform (PyWavelets mode="periodization") for gfx950: kernel ids 38 / 39 (fused level,
// one or two transformed axes) and 40 / 41 (one axis, any strides, run-time tap loop).  The contract is in include/mifwt.h:
//   extension  N~ = N + (N mod 2), x~[i] = x[min(i mod N~, N - 1)]                      (an odd extent repeats its last sample)
//   analysis   c[k] = sum_j f[j] x~[(2 k + L/2 - j) mod N~],  0 <= k < M = N~ / 2
//   synthesis  y[(2 k + t - L/2 + 1) mod 2 M] += r_lo[t] a[k] + r_hi[t] d[k]
// so an output k of the analysis reads the window 2 k - H .. 2 k + L/2 (H = L/2 - 1) and a sample n of the synthesis the coefficients
// k0 - q, q < L/2, with the taps p + 2 q, where p = (n + H) & 1 and k0 = (n + H - p) / 2.
//
// Bound: HBM (a level reads N samples and writes N per axis).  Fused kernels (unit innermost strides, f32 / f64, even L <= 20):
//   2-D: one launch per level.  A workgroup of 256 threads owns TR x TC coefficients.  It stages the (2 TR + L - 2) x (2 TC + L - 2)
//        input window in LDS through the index map (16-byte loads where a row allows), filters it along the rows into LDS (both
//        filters of every staged row), along the columns into registers, and stores the four bands with 16-byte stores.  A tile whose
//        window lies inside the plane stages without the map; the others take a real modulo per element: a window may wrap many times.
//        Synthesis mirrors it: the tiles of the four bands with L/2 - 1 coefficients of halo -> columns -> rows -> y.
//   1-D: the row half of the same code, a chunk of one row per workgroup.
// The parity p of a synthesis sample selects the taps, so every lane computes whole pairs (columns) or whole vectors (rows) of samples
// and all tap indices are compile-time: the taps stay in registers.
// Everything else (L > 20, any strides, the depth axis of a 3-D level) runs per_axis_kernel: one thread per output, run-time tap loop.
// Shared with the other fused-level units, from mifwt_level_tile.h: the 16-byte vectors, the row pass over the aligned window (left
// reach H), the tap step of the column pass and the band stores, the common kernel arguments and their fill, the tile cut, the
// descriptor prelude and envelope, the length dispatch, the packing of the level entries and the axis-pass arguments and launcher.
// Here: the index map, the staging, the geometry, the synthesis kernels and the launches.
#include "mifwt_level_tile.h"

namespace mifwt {

namespace {

// index i of the periodic extension of `m` entries (any i)
__device__ __forceinline__ int wrap(int i, int m) {
  int p = i % m;
  return p < 0 ? p + m : p;
}

// source sample of x~[i]: period n2 = 2 ceil(n / 2), the virtual sample n2 - 1 of an odd extent is sample n - 1
__device__ __forceinline__ int per_map(int i, int n, int n2) {
  const int p = wrap(i, n2);
  return p < n ? p : n - 1;
}

// ---- tile geometry (compile time; static LDS below 64 KB, at least two workgroups per CU) ----------------------------------------------
template <typename T, int L>
struct FwdGeo {
  static constexpr int E = Vec16<T>::E;
  static constexpr int H = L / 2 - 1;
  static constexpr int TC = 16 * E;                   // coefficient columns per tile: 16 lanes x one 16-byte store
  static constexpr int TR = 16;                       // coefficient rows per tile: one column-pass item per thread
  static constexpr int PAD = RowWindow<T, L, H>::PAD;  // staged columns left of sample 2 mc0 (keeps the staged vectors aligned)
  static constexpr int WC = round_up(PAD + 2 * TC + L / 2 - 1, E);
  static constexpr int XP = WC + E;                   // pitch of the staged window (a lane's last piece may end inside the pad)
  static constexpr int WR = 2 * TR + L - 2;
  static constexpr int HP = TC + E;                   // pitch of the row-filtered planes: one access width against bank conflicts
  static constexpr int TC1 = 256 * E;                 // 1-D: coefficients per workgroup
  static constexpr int WC1 = round_up(PAD + 2 * TC1 + L / 2 - 1, E);
  static constexpr int LDS2 = (WR * XP + 2 * WR * HP) * (int)sizeof(T);
};

template <typename T, int L>
struct InvGeo {
  static constexpr int E = Vec16<T>::E;
  static constexpr int H = L / 2 - 1;
  static constexpr int TQC = 16 * E;                  // coefficient columns per tile (2 TQC samples)
  static constexpr int TQ = L <= 12 ? 16 : 8;         // coefficient rows per tile (2 TQ sample rows)
  static constexpr int PMC = round_up(H, E);          // staged coefficients left of column qc0
  static constexpr int WCM = round_up(PMC + TQC + H, E);
  static constexpr int WRM = TQ + 2 * H;
  static constexpr int WL = H + (E + L / 2 - 2) / 2 + 1;  // coefficients per band behind E consecutive samples
  static constexpr int TQ1 = 128 * E;                 // 1-D: coefficients per workgroup
  static constexpr int WCM1 = round_up(PMC + TQ1 + H, E);
  static constexpr int LDS2 = (4 * WRM * WCM + 2 * 2 * TQ * WCM) * (int)sizeof(T);
};

// analysis: dec_* taps and the real signal extents;  synthesis: rec_* taps;  coefficient extents = ceil(n / 2)
template <typename T, int L>
struct PerArgs : LevelArgs<T, L> {};

// E staged samples of one row from global column g0 (a multiple of E): `mapped` = through the index map
template <typename T>
__device__ __forceinline__ void stage_sig(T* dst, const T* __restrict__ row, int g0, int n, int n2, bool vec_ok, bool mapped) {
  constexpr int E = Vec16<T>::E;
  typedef typename Vec16<T>::type V;
  if (vec_ok && (!mapped || (g0 >= 0 && g0 + E <= n))) {
    *reinterpret_cast<V*>(dst) = *reinterpret_cast<const V*>(row + g0);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) dst[e] = row[mapped ? per_map(g0 + e, n, n2) : g0 + e];
  }
}

// E staged coefficients of one band row from column g0 (a multiple of E), periodic with period m
template <typename T>
__device__ __forceinline__ void stage_coef(T* dst, const T* __restrict__ row, int g0, int m, bool vec_ok, bool mapped) {
  constexpr int E = Vec16<T>::E;
  typedef typename Vec16<T>::type V;
  if (vec_ok && (!mapped || (g0 >= 0 && g0 + E <= m))) {
    *reinterpret_cast<V*>(dst) = *reinterpret_cast<const V*>(row + g0);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) dst[e] = row[mapped ? wrap(g0 + e, m) : g0 + e];
  }
}

// E consecutive samples (first one even) from the staged rows of the two bands; r0 / r1 point at the coefficient k0(first sample) - H
template <typename T, int L>
__device__ __forceinline__ typename Vec16<T>::type synthesis_run(const T* r0, const T* r1, const T (&rlo)[L], const T (&rhi)[L]) {
  typedef InvGeo<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, H = G::H, WL = G::WL;
  T w0[WL], w1[WL];
#pragma unroll
  for (int i = 0; i < WL; ++i) {
    w0[i] = r0[i];
    w1[i] = r1[i];
  }
  V v;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int p = (e + H) & 1, c = H + (e + H - p) / 2;
    T s = T(0);
#pragma unroll
    for (int q = 0; q < L / 2; ++q) {
      s = fma(rlo[p + 2 * q], w0[c - q], s);
      s = fma(rhi[p + 2 * q], w1[c - q], s);
    }
    v[e] = s;
  }
  return v;
}

// ---- analysis, 2-D ---------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) per_fwd2_kernel(const PerArgs<T, L> a) {
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
  const int cs = 2 * mc0 - G::PAD, rs = 2 * mr0 - H;  // sample behind staged column / row 0
  const bool mapped = !(rs >= 0 && rs + WR <= a.n_r && cs >= 0 && cs + WC <= a.n_c);
  const T* __restrict__ x = static_cast<const T*>(a.in[0]) + (int64_t)b * a.sig_bs;
  constexpr int VPR = WC / E;
  for (int i = tid; i < WR * VPR; i += 256) {
    const int r = i / VPR, cv = i - r * VPR;
    const int gr = mapped ? per_map(rs + r, a.n_r, 2 * a.m_r) : rs + r;
    stage_sig<T>(xs + r * XP + cv * E, x + (int64_t)gr * a.sig_rs, cs + cv * E, a.n_c, 2 * a.m_c, a.sig_vec, mapped);
  }
  __syncthreads();
  // along the rows of the window: (lo, hi) of every staged row
  for (int i = tid; i < WR * (TC / E); i += 256) {
    const int r = i / (TC / E), cg = i - r * (TC / E);
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
__global__ void __launch_bounds__(256) per_fwd1_kernel(const PerArgs<T, L> a) {
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
  for (int i = tid; i < WC / E; i += 256) stage_sig<T>(xs + i * E, x, cs + i * E, a.n_c, 2 * a.m_c, a.sig_vec, mapped);
  __syncthreads();
  const int mc = mc0 + tid * E;
  if (mc >= a.m_c) return;
  V lo, hi;
  window_run<T, L, G::H>(xs + 2 * tid * E, a.lo, a.hi, lo, hi);
  store_vec<T>(static_cast<T*>(a.out[0]) + (int64_t)b * a.a_bs + mc, lo, a.m_c - mc, a.coef_vec);
  store_vec<T>(static_cast<T*>(a.out[1]) + (int64_t)b * a.d_bs + mc, hi, a.m_c - mc, a.coef_vec);
}

// ---- synthesis, 2-D ------------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) per_inv2_kernel(const PerArgs<T, L> a) {
  typedef InvGeo<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, H = G::H, TQ = G::TQ, TQC = G::TQC, WCM = G::WCM, WRM = G::WRM, PMC = G::PMC;
  __shared__ __attribute__((aligned(16))) T bs[4 * WRM * WCM];
  __shared__ __attribute__((aligned(16))) T ts[2 * 2 * TQ * WCM];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tc = bid % a.tiles_c;
  bid /= a.tiles_c;
  const int tr = bid % a.tiles_r;
  const int b = bid / a.tiles_r;
  const int qc0 = tc * TQC, qr0 = tr * TQ;
  const int mo_c = qc0 - PMC, mo_r = qr0 - H;  // coefficient behind staged column / row 0
  const bool mapped = !(mo_r >= 0 && mo_r + WRM <= a.m_r && mo_c >= 0 && mo_c + WCM <= a.m_c);
  // the windows of the four bands
  for (int i = tid; i < 4 * WRM * (WCM / E); i += 256) {
    const int cv = i % (WCM / E), r = (i / (WCM / E)) % WRM, s = i / ((WCM / E) * WRM);
    const int mr = mapped ? wrap(mo_r + r, a.m_r) : mo_r + r;
    const T* row = static_cast<const T*>(a.in[s]) + (s ? (int64_t)b * a.d_bs + (int64_t)mr * a.d_rs : (int64_t)b * a.a_bs + (int64_t)mr * a.a_rs);
    stage_coef<T>(bs + (s * WRM + r) * WCM + cv * E, row, mo_c + cv * E, a.m_c, a.coef_vec, mapped);
  }
  __syncthreads();
  // along the columns (axis 0): ts[cb][sample row][window column], cb = band along axis 1; a lane makes the two rows of a coefficient row
  for (int i = tid; i < 2 * TQ * (WCM / E); i += 256) {
    const int cv = i % (WCM / E), u = (i / (WCM / E)) % TQ, cb = i / ((WCM / E) * TQ);
    const T* lo0 = bs + (cb * WRM + u) * WCM + cv * E;  // band (0, cb), staged row u = coefficient row qr0 + u - H
    const T* hi0 = lo0 + 2 * WRM * WCM;                 // band (1, cb)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      const int p = (par + H) & 1, c = H + (par + H - p) / 2;
      V v = V(0);
#pragma unroll
      for (int q = 0; q < L / 2; ++q) {
        v += a.lo[p + 2 * q] * *reinterpret_cast<const V*>(lo0 + (c - q) * WCM);
        v += a.hi[p + 2 * q] * *reinterpret_cast<const V*>(hi0 + (c - q) * WCM);
      }
      *reinterpret_cast<V*>(ts + (cb * 2 * TQ + 2 * u + par) * WCM + cv * E) = v;
    }
  }
  __syncthreads();
  // along the rows (axis 1): E consecutive samples per lane
  T* __restrict__ y = static_cast<T*>(a.out[0]) + (int64_t)b * a.sig_bs;
  for (int i = tid; i < 2 * TQ * (2 * TQC / E); i += 256) {
    const int cg = i % (2 * TQC / E), nl = i / (2 * TQC / E);
    const int nr = 2 * qr0 + nl, nc = 2 * qc0 + cg * E;
    if (nr >= a.n_r || nc >= a.n_c) continue;
    const T* r0 = ts + nl * WCM + PMC + cg * (E / 2) - H;
    const V v = synthesis_run<T, L>(r0, r0 + 2 * TQ * WCM, a.lo, a.hi);
    store_vec<T>(y + (int64_t)nr * a.sig_rs + nc, v, a.n_c - nc, a.sig_vec);
  }
}

template <typename T, int L>
__global__ void __launch_bounds__(256) per_inv1_kernel(const PerArgs<T, L> a) {
  typedef InvGeo<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, H = G::H, TQ1 = G::TQ1, WCM = G::WCM1, PMC = G::PMC;
  __shared__ __attribute__((aligned(16))) T bs[2 * WCM];
  const int tid = threadIdx.x;
  const int tc = blockIdx.x % a.tiles_c;
  const int b = blockIdx.x / a.tiles_c;
  const int qc0 = tc * TQ1;
  const int mo_c = qc0 - PMC;
  const bool mapped = !(mo_c >= 0 && mo_c + WCM <= a.m_c);
  for (int i = tid; i < 2 * (WCM / E); i += 256) {
    const int cv = i % (WCM / E), s = i / (WCM / E);
    const T* row = static_cast<const T*>(a.in[s]) + (int64_t)b * (s ? a.d_bs : a.a_bs);
    stage_coef<T>(bs + s * WCM + cv * E, row, mo_c + cv * E, a.m_c, a.coef_vec, mapped);
  }
  __syncthreads();
  const int nc = 2 * qc0 + tid * E;
  if (nc >= a.n_c) return;
  const T* r0 = bs + PMC + tid * (E / 2) - H;
  const V v = synthesis_run<T, L>(r0, r0 + WCM, a.lo, a.hi);
  store_vec<T>(static_cast<T*>(a.out[0]) + (int64_t)b * a.sig_bs + nc, v, a.n_c - nc, a.sig_vec);
}

// ---- one axis of [outer, n, inner] arrays: any even L <= MIFWT_MAX_FILT, any strides -----------------------------------------------------------
template <typename T, bool INVERSE>
__global__ void __launch_bounds__(256) per_axis_kernel(const AxisArgsBase a) {
  const int L = a.filt_len, M = a.m, N2 = 2 * a.m;
  const int64_t len = INVERSE ? a.n : M;
  const int64_t total = a.outer * len * a.inner;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t in = idx % a.inner, o = idx / (a.inner * len);
    const int pos = (int)((idx / a.inner) % len);
    if (!INVERSE) {
      const T* x = static_cast<const T*>(a.in0) + o * a.sig_s[0] + in * a.sig_s[2];
      int p = wrap(2 * pos + L / 2, N2);  // index of tap 0; tap j reads one sample further back
      double sl = 0, sh = 0;
      for (int j = 0; j < L; ++j) {
        const double v = (double)x[(int64_t)(p < a.n ? p : a.n - 1) * a.sig_s[1]];
        sl = fma(a.lo[j], v, sl);
        sh = fma(a.hi[j], v, sh);
        p = p == 0 ? N2 - 1 : p - 1;
      }
      static_cast<T*>(a.out0)[o * a.lo_s[0] + (int64_t)pos * a.lo_s[1] + in * a.lo_s[2]] = (T)sl;
      static_cast<T*>(a.out1)[o * a.hi_s[0] + (int64_t)pos * a.hi_s[1] + in * a.hi_s[2]] = (T)sh;
    } else {
      const T* cl = static_cast<const T*>(a.in0) + o * a.lo_s[0] + in * a.lo_s[2];
      const T* ch = static_cast<const T*>(a.in1) + o * a.hi_s[0] + in * a.hi_s[2];
      const int par = (pos + L / 2 - 1) & 1;
      int k = wrap((pos + L / 2 - 1 - par) / 2, M);  // coefficient of tap `par`; tap par + 2 q takes the one q further back
      double acc = 0;
      for (int q = 0; q < L / 2; ++q) {
        acc = fma(a.lo[par + 2 * q], (double)cl[(int64_t)k * a.lo_s[1]], acc);
        acc = fma(a.hi[par + 2 * q], (double)ch[(int64_t)k * a.hi_s[1]], acc);
        k = k == 0 ? M - 1 : k - 1;
      }
      static_cast<T*>(a.out0)[o * a.sig_s[0] + (int64_t)pos * a.sig_s[1] + in * a.sig_s[2]] = (T)acc;
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
// 0 = not served by the fused kernels, MIFWT_ERR_BADARG = inconsistent, 1 = served
int fused_check(const mifwt_level_desc* d) {
  if (const int bad = desc_prelude(d)) return bad;
  for (int ax = 0; ax < d->ndim; ++ax) {
    const int64_t n = d->sig_extent[ax], m = d->coef_extent[ax];
    if (n < 1 || m != (n + 1) / 2) return MIFWT_ERR_BADARG;
  }
  return fused_envelope(d);
}

template <typename T, int L>
int launch_fused(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi,
                 hipStream_t stream) {
  static_assert(FwdGeo<T, L>::LDS2 <= 65536 && InvGeo<T, L>::LDS2 <= 65536, "tile does not fit the default LDS allowance");
  PerArgs<T, L> a;
  fill_level_args(a, d, inverse, in, out, lo, hi, Vec16<T>::E);
  if (d->batch == 0) return MIFWT_OK;
  const int nd = d->ndim;
  const int tcw = nd == 2 ? (inverse ? InvGeo<T, L>::TQC : FwdGeo<T, L>::TC) : (inverse ? InvGeo<T, L>::TQ1 : FwdGeo<T, L>::TC1);
  const int64_t grid = cut_tiles(a, a.m_c, a.m_r, tcw, inverse ? InvGeo<T, L>::TQ : FwdGeo<T, L>::TR, d->batch);
  if (grid < 0) return MIFWT_ERR_UNSUPPORTED;
  const dim3 g((unsigned)grid), blk(256);
  if (nd == 2) {
    if (inverse)
      hipLaunchKernelGGL((per_inv2_kernel<T, L>), g, blk, 0, stream, a);
    else
      hipLaunchKernelGGL((per_fwd2_kernel<T, L>), g, blk, 0, stream, a);
  } else {
    if (inverse)
      hipLaunchKernelGGL((per_inv1_kernel<T, L>), g, blk, 0, stream, a);
    else
      hipLaunchKernelGGL((per_fwd1_kernel<T, L>), g, blk, 0, stream, a);
  }
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  count_launch(inverse ? MIFWT_KID_PER_INV : MIFWT_KID_PER_FWD);
  return MIFWT_OK;
}

template <typename T>
int dispatch_len(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi,
                 hipStream_t stream) {
  return for_even_len(d->filt_len, [&](auto len) { return launch_fused<T, decltype(len)::value>(d, inverse, in, out, lo, hi, stream); });
}

int per_level(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi,
              void* stream) {
  const int ok = fused_check(d);
  if (ok < 0) return ok;
  if (const int bad = level_pointers(d, inverse, in, out, lo, hi)) return bad;
  if (!ok) return MIFWT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return d->dtype == MIFWT_F32 ? dispatch_len<float>(d, inverse, in, out, lo, hi, st) : dispatch_len<double>(d, inverse, in, out, lo, hi, st);
}

int per_axis(int inverse, int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* in0, const void* in1, void* out0,
             void* out1, const int64_t* sig_s, const int64_t* lo_s, const int64_t* hi_s, const double* lo, const double* hi, void* stream) {
  if (const int bad = axis_check(inverse, dtype, filt_len, outer, n, inner, in0, in1, out0, out1, sig_s, lo_s, hi_s, lo, hi)) return bad;
  AxisArgsBase a;
  if (const int bad = fill_axis_args(a, filt_len, outer, n, (n + 1) / 2, inner, in0, in1, out0, out1, sig_s, lo_s, hi_s, lo, hi)) return bad;
  const int64_t total = outer * (inverse ? n : (int64_t)a.m) * inner;
  if (total == 0) return MIFWT_OK;
  const int rc = launch_axis(dtype, inverse, total, 65536, stream, a, per_axis_kernel<float, false>, per_axis_kernel<float, true>,
                             per_axis_kernel<double, false>, per_axis_kernel<double, true>);
  if (rc != MIFWT_OK) return rc;
  count_launch(inverse ? MIFWT_KID_PER_AXIS_INV : MIFWT_KID_PER_AXIS_FWD);
  return MIFWT_OK;
}

}  // namespace

}  // namespace mifwt

extern "C" {

int mifwt_per_supported(const mifwt_level_desc* desc, int direction) {
  if (direction != 0 && direction != 1) return MIFWT_ERR_BADARG;
  return mifwt::fused_check(desc);
}

int mifwt_per_kernel_id(const mifwt_level_desc* desc, int direction) {
  return mifwt::kernel_id_answer(mifwt_per_supported(desc, direction), direction, MIFWT_KID_PER_FWD, MIFWT_KID_PER_INV);
}

int mifwt_per_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* lo, const double* hi,
                  void* stream) {
  const void* in[4] = {x, nullptr, nullptr, nullptr};
  void* out[4];
  if (const int bad = mifwt::pack_bands<void*>(desc, approx, details, out)) return bad;
  return mifwt::per_level(desc, 0, in, out, lo, hi, stream);
}

int mifwt_per_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* lo, const double* hi,
                  void* stream) {
  const void* in[4];
  void* out[4] = {y, nullptr, nullptr, nullptr};
  if (const int bad = mifwt::pack_bands<const void*>(desc, approx, details, in)) return bad;
  return mifwt::per_level(desc, 1, in, out, lo, hi, stream);
}

int mifwt_per_axis_fwd(int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* x, const int64_t* x_strides, void* lo_out,
                       const int64_t* lo_strides, void* hi_out, const int64_t* hi_strides, const double* lo, const double* hi, void* stream) {
  return mifwt::per_axis(0, dtype, filt_len, outer, n, inner, x, nullptr, lo_out, hi_out, x_strides, lo_strides, hi_strides, lo, hi, stream);
}

int mifwt_per_axis_inv(int dtype, int filt_len, int64_t outer, int64_t n_out, int64_t inner, const void* lo_in, const int64_t* lo_strides,
                       const void* hi_in, const int64_t* hi_strides, void* y, const int64_t* y_strides, const double* lo, const double* hi,
                       void* stream) {
  return mifwt::per_axis(1, dtype, filt_len, outer, n_out, inner, lo_in, hi_in, y, nullptr, y_strides, lo_strides, hi_strides, lo, hi, stream);
}

}  // extern "C"
