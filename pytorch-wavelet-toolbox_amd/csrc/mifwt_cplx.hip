// mifwt_cplx.hip — padded levels of INTERLEAVED COMPLEX data (complex64 / complex128: pairs (re, im) of float / double) for gfx950: kernel
// ids 46 / 47, the fused analysis level and the fused padded synthesis level with its crop, one or two transformed axes.  The taps are
// real, so a level filters the two components separately: T(a + i b) = T(a) + i T(b).  The contract is in include/mifwt.h; every index
// below counts COMPLEX elements:
//   extension  xe[i] = x[ext_index(i, N, mode)] (mifwt_common.h; zero mode: 0), the map applied to the complex index — on the float index
//              a mirror would swap the components inside the pad
//   analysis   c[k] = sum_j f[j] xe[2 k + 1 - j],  0 <= k < M = floor((N + L - 1) / 2): output k reads the window 2 k - (L - 2) .. 2 k + 1
//   synthesis  y[n] = sum_k rec_lo[n + L - 2 - 2 k] a[k] + rec_hi[n + L - 2 - 2 k] d[k],  0 <= n < N_out in {2 M - L + 2, 2 M - L + 1}:
//              samples 2 p and 2 p + 1 read coefficients p .. p + L/2 - 1, all inside [0, M) — the crop is simply what is never computed
//
// Bound: HBM (a level reads N complex samples and writes about N per axis).  Only the pass along the innermost axis knows about the
// channels: along the rows of a plane complex data is real data of doubled width, and that pass works on 16-byte vectors of components.
//   analysis 2-D: a workgroup of 256 threads owns TR x TC coefficients, TC x sizeof(complex) = 256 bytes per tile row.  It stages the
//        (2 TR + L - 2) x (2 TC + L - 2) window of xe in LDS (16-byte loads where the row is 16-byte aligned, else one complex element
//        — 8 bytes of complex64 — per load), filters it along the rows into two LDS planes (one complex output per item: L reads of one
//        element, ds_read_b64 / ds_read_b128), along the columns into registers (16 bytes of components per lane) and stores the four
//        bands with 16-byte stores (element stores where a band row is not 16-byte aligned or the tile overhangs).
//        LDS lane map of the row pass: lane c of 16 consecutive lanes reads element 2 c + k, a stride of two elements, so 16 lanes cover a
//        whole 256-byte bank row (complex64: half of the 64 banks of ds_read_b64 twice over 32 lanes).  The next 16 lanes take the NEXT
//        staged row, and the pitch of the staged window is an ODD number of elements: their addresses fall into the other half of each
//        16-byte (complex128) / the other 8 bytes of each 16-byte slot (complex64), which makes both reads conflict-free.
//   analysis 1-D: the row half of the same code, 256 x (16 / sizeof(complex)) coefficients of one row per workgroup.
//   synthesis 2-D: a polyphase gather.  A workgroup owns TSR x TSC samples; it synthesises the coefficient rows behind its sample rows
//        along the columns (global -> LDS, two planes: low / high band along the rows; one pair of samples 2 p, 2 p + 1 per item), then
//        along the rows from LDS, 16 bytes of components per lane.  1-D: one pair of samples per thread.
// Both components run the same instructions in the same order (component-wise fma chains), no atomics: the real plane of every output is
// a function of the real plane of the input alone, bit for bit.  Batch, plane and row offsets are int64.
// Shared with the other fused-level units, from mifwt_level_tile.h: the common kernel arguments and their fill (with EC for the elements
// per 16 bytes, strides in complex elements), the tile cut, the descriptor prelude and envelope, the length dispatch and the packing of
// the level entries.  Every kernel body is this unit's own: its row pass is channel-aware and its window has an odd pitch.
#include "mifwt_level_tile.h"

namespace mifwt {

namespace {

template <typename T>
struct Cplx;
template <>
struct Cplx<float> {
  static constexpr int EC = 2;                               // complex elements per 16 bytes
  typedef float elem __attribute__((ext_vector_type(2)));    // one complex element
  typedef float vec __attribute__((ext_vector_type(4)));     // 16 bytes of components
};
template <>
struct Cplx<double> {
  static constexpr int EC = 1;
  typedef double elem __attribute__((ext_vector_type(2)));
  typedef double vec __attribute__((ext_vector_type(2)));
};

// acc + f * w per component: the same fma on the real and on the imaginary part
template <typename T>
__device__ __forceinline__ typename Cplx<T>::elem cfma(T f, const typename Cplx<T>::elem& w, const typename Cplx<T>::elem& acc) {
  typename Cplx<T>::elem r;
  r.x = fma(f, w.x, acc.x);
  r.y = fma(f, w.y, acc.y);
  return r;
}

template <typename T>
__device__ __forceinline__ typename Cplx<T>::vec vfma(T f, const typename Cplx<T>::vec& w, const typename Cplx<T>::vec& acc) {
  typename Cplx<T>::vec r;
#pragma unroll
  for (int e = 0; e < 16 / (int)sizeof(T); ++e) r[e] = fma(f, w[e], acc[e]);
  return r;
}

// ---- tile geometry (compile time; static LDS below 64 KB) -------------------------------------------------------------------------------
template <typename T, int L>
struct CFwdGeo {
  static constexpr int EC = Cplx<T>::EC;
  static constexpr int H = L - 2;                          // elements of the window left of element 2 k
  static constexpr int TC = 16 * EC;                       // coefficient columns per tile: a 256-byte row
  static constexpr int TR = sizeof(T) == 4 ? 16 : 8;       // coefficient rows per tile (complex128 at L = 20 fits with 8)
  static constexpr int WC = 2 * TC + H;                    // staged columns (even)
  static constexpr int XP = WC + 1;                        // ODD pitch of the staged window: see the lane map above
  static constexpr int WR = 2 * TR + H;                    // staged rows
  static constexpr int TC1 = 256 * EC;                     // 1-D: coefficients per workgroup
  static constexpr int WC1 = 2 * TC1 + H;
  static constexpr int LDS2 = (WR * XP + 2 * WR * TC) * 2 * (int)sizeof(T);
};

template <typename T, int L>
struct CInvGeo {
  static constexpr int EC = Cplx<T>::EC;
  static constexpr int TSC = 16 * EC;                      // sample columns per tile: a 256-byte row
  static constexpr int TSR = 16;                           // sample rows per tile
  static constexpr int KR = TSR / 2 + L / 2 - 1;           // coefficient rows behind a tile's rows
  static constexpr int TS1 = 512;                          // 1-D: samples per workgroup, a pair per thread
  static constexpr int LDS2 = 2 * KR * TSC * 2 * (int)sizeof(T);
};

// Strides and extents in COMPLEX elements; synthesis: n_r / n_c are the cropped output extents.  dec_lo / dec_hi (analysis), rec_lo /
// rec_hi (synthesis)
template <typename T, int L>
struct CplxArgs : LevelArgs<T, L> {
  int mode;  // enum mifwt_mode (analysis)
};

// EC complex elements from `valid` on: one 16-byte store, or element stores
template <typename T>
__device__ __forceinline__ void store_cvec(typename Cplx<T>::elem* p, const typename Cplx<T>::vec& v, int valid, bool vec_ok) {
  constexpr int EC = Cplx<T>::EC;
  typedef typename Cplx<T>::elem C;
  if (vec_ok && valid >= EC) {
    *reinterpret_cast<typename Cplx<T>::vec*>(p) = v;
  } else {
#pragma unroll
    for (int e = 0; e < EC; ++e)
      if (e < valid) {
        C c;
        c.x = v[2 * e];
        c.y = v[2 * e + 1];
        p[e] = c;
      }
  }
}

// EC staged elements of extended row `gr` from extended column g0 (complex indices; g0 a multiple of EC away from an even start)
template <typename T>
__device__ __forceinline__ void stage_cplx(typename Cplx<T>::elem* dst, const typename Cplx<T>::elem* __restrict__ plane, int64_t rs, int gr,
                                           int g0, int n_r, int n_c, int mode, bool vec_ok) {
  constexpr int EC = Cplx<T>::EC;
  typedef typename Cplx<T>::elem C;
  typedef typename Cplx<T>::vec V;
  const int sr = ext_index_near(gr, n_r, mode);  // (a 1-D level has n_r = 1 and gr = 0)
  const C zero = {T(0), T(0)};
  if (sr < 0) {
#pragma unroll
    for (int e = 0; e < EC; ++e) dst[e] = zero;
    return;
  }
  const C* row = plane + (int64_t)sr * rs;
  if (EC == 2 && vec_ok && g0 >= 0 && g0 + EC <= n_c) {  // (the staged window has an odd pitch: two 8-byte LDS stores)
    const V v = *reinterpret_cast<const V*>(row + g0);
    C c0, c1;
    c0.x = v[0];
    c0.y = v[1];
    c1.x = v[EC == 2 ? 2 : 0];
    c1.y = v[EC == 2 ? 3 : 1];
    dst[0] = c0;
    dst[EC - 1] = c1;
    return;
  }
#pragma unroll
  for (int e = 0; e < EC; ++e) {
    const int sc = ext_index_near(g0 + e, n_c, mode);
    dst[e] = sc < 0 ? zero : row[sc];
  }
}

// ---- analysis, 2-D -------------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) cplx_fwd2_kernel(const CplxArgs<T, L> a) {
  typedef CFwdGeo<T, L> G;
  typedef typename Cplx<T>::elem C;
  typedef typename Cplx<T>::vec V;
  constexpr int EC = G::EC, TC = G::TC, TR = G::TR, H = G::H, WC = G::WC, WR = G::WR, XP = G::XP;
  __shared__ __attribute__((aligned(16))) C xs[WR * XP];
  __shared__ __attribute__((aligned(16))) C hs[2 * WR * TC];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tc = bid % a.tiles_c;
  bid /= a.tiles_c;
  const int tr = bid % a.tiles_r;
  const int b = bid / a.tiles_r;
  const int mc0 = tc * TC, mr0 = tr * TR;
  const int cs = 2 * mc0 - H, rs = 2 * mr0 - H;  // extended element behind staged column / row 0
  const C* __restrict__ x = static_cast<const C*>(a.in[0]) + (int64_t)b * a.sig_bs;
  // a tile that overhangs the plane works on the part of its window that feeds an output: the last coefficient of an axis reads up to
  // extended element 2 m - 1
  const int wr = min(WR, 2 * a.m_r - rs);
  const int wc = min(WC, 2 * a.m_c - cs);  // (even)
  const int tcn = min(TC, a.m_c - mc0);    // coefficient columns of this tile
  const int vpr = (wc + EC - 1) / EC;
  for (int i = tid; i < wr * vpr; i += 256) {
    const int r = i / vpr, cv = i - r * vpr;
    stage_cplx<T>(xs + r * XP + cv * EC, x, a.sig_rs, rs + r, cs + cv * EC, a.n_r, a.n_c, a.mode, a.sig_vec);
  }
  __syncthreads();
  // along the rows of the window, the channel-aware pass: (lo, hi) of every staged row; 16 consecutive lanes = 16 columns of one row
  const int tcg = (tcn + 15) / 16;
  for (int i = tid; i < wr * tcg * 16; i += 256) {
    const int c16 = i & 15, q = i >> 4;
    const int r = q % wr, c = (q / wr) * 16 + c16;
    if (c >= tcn) continue;
    const C* w = xs + r * XP + 2 * c;
    C lo = {T(0), T(0)}, hi = {T(0), T(0)};
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const C v = w[k];
      lo = cfma<T>(a.lo[L - 1 - k], v, lo);
      hi = cfma<T>(a.hi[L - 1 - k], v, hi);
    }
    hs[r * TC + c] = lo;
    hs[(WR + r) * TC + c] = hi;
  }
  __syncthreads();
  // along the columns, real data of doubled width: four bands, 16 bytes of components per lane
  for (int i = tid; i < TR * 16; i += 256) {
    const int slot = i & 15, ro = i >> 4;
    const int m = mr0 + ro, c0 = slot * EC;
    if (m >= a.m_r || c0 >= tcn) continue;
    V ll = V(0), lh = V(0), hl = V(0), hh = V(0);
    const C* hl0 = hs + (2 * ro) * TC + c0;
    const C* hh0 = hl0 + WR * TC;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const V vl = *reinterpret_cast<const V*>(hl0 + k * TC);
      const V vh = *reinterpret_cast<const V*>(hh0 + k * TC);
      const T cl = a.lo[L - 1 - k], ch = a.hi[L - 1 - k];
      ll = vfma<T>(cl, vl, ll);
      lh = vfma<T>(cl, vh, lh);
      hl = vfma<T>(ch, vl, hl);
      hh = vfma<T>(ch, vh, hh);
    }
    // (a column of the second element that lies beyond the tile's coefficients was filtered from unstaged LDS: `valid` keeps it out)
    const int valid = tcn - c0;
    const int64_t oa = (int64_t)b * a.a_bs + (int64_t)m * a.a_rs + mc0 + c0;
    const int64_t od = (int64_t)b * a.d_bs + (int64_t)m * a.d_rs + mc0 + c0;
    store_cvec<T>(static_cast<C*>(a.out[0]) + oa, ll, valid, a.coef_vec);
    store_cvec<T>(static_cast<C*>(a.out[1]) + od, lh, valid, a.coef_vec);
    store_cvec<T>(static_cast<C*>(a.out[2]) + od, hl, valid, a.coef_vec);
    store_cvec<T>(static_cast<C*>(a.out[3]) + od, hh, valid, a.coef_vec);
  }
}

// ---- analysis, 1-D: a chunk of one row per workgroup, EC consecutive coefficients per thread ------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) cplx_fwd1_kernel(const CplxArgs<T, L> a) {
  typedef CFwdGeo<T, L> G;
  typedef typename Cplx<T>::elem C;
  typedef typename Cplx<T>::vec V;
  constexpr int EC = G::EC, TC = G::TC1, WC = G::WC1, H = G::H;
  __shared__ __attribute__((aligned(16))) C xs[WC];
  const int tid = threadIdx.x;
  const int tc = blockIdx.x % a.tiles_c;
  const int b = blockIdx.x / a.tiles_c;
  const int mc0 = tc * TC;
  const int cs = 2 * mc0 - H;
  const C* __restrict__ x = static_cast<const C*>(a.in[0]) + (int64_t)b * a.sig_bs;
  const int wc = min(WC, 2 * a.m_c - cs);  // (even: beyond it nothing feeds an output)
  for (int i = tid; i < (wc + EC - 1) / EC; i += 256) stage_cplx<T>(xs + i * EC, x, 0, 0, cs + i * EC, 1, a.n_c, a.mode, a.sig_vec);
  __syncthreads();
  const int mc = mc0 + tid * EC;
  if (mc >= a.m_c) return;
  const int valid = a.m_c - mc;
  C w[2 * EC + H];  // (what lies beyond the staged part of the window feeds only a coefficient that `valid` keeps out)
#pragma unroll
  for (int i = 0; i < 2 * EC + H; ++i) w[i] = xs[2 * tid * EC + i];
  V lo, hi;
#pragma unroll
  for (int e = 0; e < EC; ++e) {
    C sl = {T(0), T(0)}, sh = {T(0), T(0)};
#pragma unroll
    for (int k = 0; k < L; ++k) {
      sl = cfma<T>(a.lo[L - 1 - k], w[2 * e + k], sl);
      sh = cfma<T>(a.hi[L - 1 - k], w[2 * e + k], sh);
    }
    lo[2 * e] = sl.x;
    lo[2 * e + 1] = sl.y;
    hi[2 * e] = sh.x;
    hi[2 * e + 1] = sh.y;
  }
  store_cvec<T>(static_cast<C*>(a.out[0]) + (int64_t)b * a.a_bs + mc, lo, valid, a.coef_vec);
  store_cvec<T>(static_cast<C*>(a.out[1]) + (int64_t)b * a.d_bs + mc, hi, valid, a.coef_vec);
}

// Samples 2 p and 2 p + 1 of one synthesised line: coefficients p .. p + L/2 - 1 of its low / high band (all inside the band for a sample
// that exists, see the contract)
template <typename T, int L>
__device__ __forceinline__ void synth_pair(const typename Cplx<T>::elem* __restrict__ ga, const typename Cplx<T>::elem* __restrict__ gd,
                                           const T (&flo)[L], const T (&fhi)[L], typename Cplx<T>::elem& even, typename Cplx<T>::elem& odd) {
  typedef typename Cplx<T>::elem C;
  C e = {T(0), T(0)}, o = {T(0), T(0)};
#pragma unroll
  for (int i = 0; i < L / 2; ++i) {
    const C va = ga[i], vd = gd[i];
    e = cfma<T>(flo[L - 2 - 2 * i], va, e);
    e = cfma<T>(fhi[L - 2 - 2 * i], vd, e);
    o = cfma<T>(flo[L - 1 - 2 * i], va, o);
    o = cfma<T>(fhi[L - 1 - 2 * i], vd, o);
  }
  even = e;
  odd = o;
}

// ---- synthesis, 2-D ------------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) cplx_inv2_kernel(const CplxArgs<T, L> a) {
  typedef CInvGeo<T, L> G;
  typedef typename Cplx<T>::elem C;
  typedef typename Cplx<T>::vec V;
  constexpr int EC = G::EC, TSC = G::TSC, TSR = G::TSR, KR = G::KR;
  __shared__ __attribute__((aligned(16))) C us[2 * KR * TSC];  // [band along the rows][coefficient row - k_lo][sample column]
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tc = bid % a.tiles_c;
  bid /= a.tiles_c;
  const int tr = bid % a.tiles_r;
  const int b = bid / a.tiles_r;
  const int sc0 = tc * TSC, sr0 = tr * TSR;  // (both even)
  const int k_lo = sr0 >> 1;
  const int kr = min(KR, a.m_r - k_lo);  // coefficient rows behind the tile's rows that exist
  // along the columns, the channel-aware pass: both row bands of every coefficient row, a pair of samples per item
  for (int i = tid; i < 2 * kr * (TSC / 2); i += 256) {
    const int pl = i % (TSC / 2), r = (i / (TSC / 2)) % kr, br = i / ((TSC / 2) * kr);
    const int k = k_lo + r, p = (sc0 >> 1) + pl;
    C even = {T(0), T(0)}, odd = {T(0), T(0)};
    if (2 * p < a.n_c) {
      const C* ga = static_cast<const C*>(a.in[2 * br]) + (br ? (int64_t)b * a.d_bs + (int64_t)k * a.d_rs : (int64_t)b * a.a_bs + (int64_t)k * a.a_rs) + p;
      const C* gd = static_cast<const C*>(a.in[2 * br + 1]) + (int64_t)b * a.d_bs + (int64_t)k * a.d_rs + p;
      synth_pair<T, L>(ga, gd, a.lo, a.hi, even, odd);
    }
    C* dst = us + (br * KR + r) * TSC + 2 * pl;
    dst[0] = even;
    dst[1] = odd;
  }
  __syncthreads();
  // along the rows, real data of doubled width: 16 bytes of components per lane
  C* __restrict__ y = static_cast<C*>(a.out[0]) + (int64_t)b * a.sig_bs;
  for (int i = tid; i < TSR * 16; i += 256) {
    const int slot = i & 15, rl = i >> 4;
    const int s = sr0 + rl, c0 = slot * EC;
    if (s >= a.n_r || sc0 + c0 >= a.n_c) continue;
    const int p = rl >> 1;
    const bool par = rl & 1;
    const C* u0 = us + p * TSC + c0;
    const C* u1 = u0 + KR * TSC;
    V acc = V(0);
#pragma unroll
    for (int j = 0; j < L / 2; ++j) {
      const T cl = par ? a.lo[L - 1 - 2 * j] : a.lo[L - 2 - 2 * j];
      const T ch = par ? a.hi[L - 1 - 2 * j] : a.hi[L - 2 - 2 * j];
      acc = vfma<T>(cl, *reinterpret_cast<const V*>(u0 + j * TSC), acc);
      acc = vfma<T>(ch, *reinterpret_cast<const V*>(u1 + j * TSC), acc);
    }
    store_cvec<T>(y + (int64_t)s * a.sig_rs + sc0 + c0, acc, a.n_c - sc0 - c0, a.sig_vec);
  }
}

// ---- synthesis, 1-D: a pair of samples per thread ----------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) cplx_inv1_kernel(const CplxArgs<T, L> a) {
  typedef CInvGeo<T, L> G;
  typedef typename Cplx<T>::elem C;
  constexpr int TS1 = G::TS1;
  const int tc = blockIdx.x % a.tiles_c;
  const int b = blockIdx.x / a.tiles_c;
  const int p = tc * (TS1 / 2) + threadIdx.x;
  if (2 * p >= a.n_c) return;
  const C* ga = static_cast<const C*>(a.in[0]) + (int64_t)b * a.a_bs + p;
  const C* gd = static_cast<const C*>(a.in[1]) + (int64_t)b * a.d_bs + p;
  C even, odd;
  synth_pair<T, L>(ga, gd, a.lo, a.hi, even, odd);
  C* y = static_cast<C*>(a.out[0]) + (int64_t)b * a.sig_bs + 2 * p;
  if (2 * p + 1 < a.n_c) {
    if (sizeof(T) == 4 && a.sig_vec) {
      typename Cplx<T>::vec v;
      v[0] = even.x;
      v[1] = even.y;
      v[sizeof(T) == 4 ? 2 : 0] = odd.x;
      v[sizeof(T) == 4 ? 3 : 1] = odd.y;
      *reinterpret_cast<typename Cplx<T>::vec*>(y) = v;
    } else {
      y[0] = even;
      y[1] = odd;
    }
  } else {
    y[0] = even;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
// 0 = not served by the fused kernels, MIFWT_ERR_BADARG = inconsistent, MIFWT_ERR_UNSUPPORTED = a component type without kernels, 1 = served
int cplx_check(const mifwt_level_desc* d, int direction) {
  if (const int bad = desc_prelude(d)) return bad;
  if (direction != 0 && direction != 1) return MIFWT_ERR_BADARG;
  if (is_storage16(d->dtype)) return MIFWT_ERR_UNSUPPORTED;
  if (direction == 0 && (d->mode < MIFWT_MODE_ZERO || d->mode > MIFWT_MODE_SYMMETRIC)) return MIFWT_ERR_BADARG;
  for (int ax = 0; ax < d->ndim; ++ax) {
    const int64_t n = d->sig_extent[ax], m = d->coef_extent[ax];
    if (direction == 0) {
      if (n < 1 || m != (n + d->filt_len - 1) / 2) return MIFWT_ERR_BADARG;
    } else {  // the cropped output of the padded synthesis
      const int64_t full = 2 * m - d->filt_len + 2;
      if (m < 1 || n < 1 || (n != full && n != full - 1)) return MIFWT_ERR_BADARG;
    }
  }
  return fused_envelope(d);
}

template <typename T, int L>
int cplx_launch(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi,
                hipStream_t stream) {
  typedef CFwdGeo<T, L> FG;
  typedef CInvGeo<T, L> IG;
  static_assert(FG::LDS2 <= 65536 && IG::LDS2 <= 65536, "tile does not fit the default LDS allowance");
  CplxArgs<T, L> a;
  fill_level_args(a, d, inverse, in, out, lo, hi, Cplx<T>::EC);
  a.mode = d->mode;
  if (d->batch == 0) return MIFWT_OK;
  const int nd = d->ndim;
  // analysis cuts the coefficients, synthesis the samples
  const int tcw = nd == 2 ? (inverse ? IG::TSC : FG::TC) : (inverse ? IG::TS1 : FG::TC1);
  const int64_t grid = inverse ? cut_tiles(a, a.n_c, a.n_r, tcw, IG::TSR, d->batch) : cut_tiles(a, a.m_c, a.m_r, tcw, FG::TR, d->batch);
  if (grid < 0) return MIFWT_ERR_UNSUPPORTED;
  const dim3 g((unsigned)grid), blk(256);
  if (nd == 2) {
    if (inverse)
      hipLaunchKernelGGL((cplx_inv2_kernel<T, L>), g, blk, 0, stream, a);
    else
      hipLaunchKernelGGL((cplx_fwd2_kernel<T, L>), g, blk, 0, stream, a);
  } else {
    if (inverse)
      hipLaunchKernelGGL((cplx_inv1_kernel<T, L>), g, blk, 0, stream, a);
    else
      hipLaunchKernelGGL((cplx_fwd1_kernel<T, L>), g, blk, 0, stream, a);
  }
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  count_launch(inverse ? MIFWT_KID_CPLX_INV : MIFWT_KID_CPLX_FWD);
  return MIFWT_OK;
}

template <typename T>
int cplx_dispatch_len(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi,
                      hipStream_t stream) {
  return for_even_len(d->filt_len, [&](auto len) { return cplx_launch<T, decltype(len)::value>(d, inverse, in, out, lo, hi, stream); });
}

int cplx_level(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi,
               void* stream) {
  const int ok = cplx_check(d, inverse);
  if (ok < 0) return ok;
  if (const int bad = level_pointers(d, inverse, in, out, lo, hi)) return bad;
  if (!ok) return MIFWT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return d->dtype == MIFWT_F32 ? cplx_dispatch_len<float>(d, inverse, in, out, lo, hi, st)
                               : cplx_dispatch_len<double>(d, inverse, in, out, lo, hi, st);
}

}  // namespace

}  // namespace mifwt

extern "C" {

int mifwt_cplx_supported(const mifwt_level_desc* desc, int direction) { return mifwt::cplx_check(desc, direction); }

int mifwt_cplx_kernel_id(const mifwt_level_desc* desc, int direction) {
  return mifwt::kernel_id_answer(mifwt_cplx_supported(desc, direction), direction, MIFWT_KID_CPLX_FWD, MIFWT_KID_CPLX_INV);
}

int mifwt_cplx_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* dec_lo,
                   const double* dec_hi, void* stream) {
  const void* in[4] = {x, nullptr, nullptr, nullptr};
  void* out[4];
  if (const int bad = mifwt::pack_bands<void*>(desc, approx, details, out)) return bad;
  return mifwt::cplx_level(desc, 0, in, out, dec_lo, dec_hi, stream);
}

int mifwt_cplx_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* rec_lo,
                   const double* rec_hi, void* stream) {
  const void* in[4];
  void* out[4] = {y, nullptr, nullptr, nullptr};
  if (const int bad = mifwt::pack_bands<const void*>(desc, approx, details, in)) return bad;
  return mifwt::cplx_level(desc, 1, in, out, rec_lo, rec_hi, stream);
}

}  // extern "C"
