// mifwt_bwt3.hip — 3-D levels of the padding-free BOUNDARY-WAVELET transform for gfx950 (kernel ids 30 / 31).
//
// Replaces, per level of ptwt.MatrixWavedec3 / MatrixWaverec3 (reference src/ptwt/matmul_transform_3.py): three batched sparse products
// with the level operator of each axis and the transposes between them, i.e. three trips of the volume through memory.  Here a level is
// ONE launch that reads the volume once and writes the eight bands once (synthesis: reads the eight bands, writes the volume).  The row
// bank (two filters + boundary table, see mifwt_bwt_rows.h for the matrix it stands for) is the same for every axis and every level.
//
// ENVELOPE: float32 / float64, even L <= 8 (haar, db2, db3, db4, bior2.2, rbio2.4 ...), unit innermost stride, every axis with
// 2 ceil(n / 2) >= 2 (L - 1).  Longer filters do not fit a brick with a useful interior into 80 KB of LDS (the window of a brick grows by
// (L - 2) + (L/2 - 1) samples per axis); they run the per-axis passes 28 / 29 of mifwt_bwt.hip, composed on the host.
//
// Analysis (30): a workgroup owns a brick of TD x TR x TC coefficients of all eight bands.  It stages the input window of the brick in LDS
// (16-byte loads where the rows allow; the virtual sample of an odd extent and the zeros outside are index maps), then filters along the
// width, the height and the depth.  The first two passes work IN PLACE: every lane keeps its outputs in registers until all lanes have
// read (a barrier), then the image of the pass replaces the window, so that one buffer of WD x WR x WC samples is all the LDS a brick
// needs.  The depth pass goes to registers and from there to the eight bands, 16-byte stores where the alignment allows.
// Synthesis (31) mirrors it: the windows of the eight bands -> depth -> height (both in place) -> width -> y, storing only the
// sig_extent samples of each axis.
// Workgroups whose brick touches an end of an axis load the table into LDS; only their lanes whose outputs involve a boundary row take
// the EDGE form of a step (per-output window start + table row), everything else runs the plain taps from the kernel arguments.
//
// LDS (bytes per workgroup, dynamic; above 64 KB the kernels opt in per (kernel, device)) and workgroups per CU of 160 KB:
//   analysis  f32: L=2 32 K (4), L=4 59 K (2), L=6 71 K (2), L=8 76 K (2)     f64: 32 K, 59 K, 75 K, 74 K (2 each from L=4)
//   synthesis f32: L=2 32 K (4), L=4 60 K (2), L=6 100 K (1), L=8 150 K (1)   f64: 32 K, 60 K, 120 K, 150 K
// (synthesis stages eight windows with L/2 coefficients of halo on either side of every axis, so its bricks for L >= 6 are small and
// occupy a CU alone: the host layer routes synthesis levels of 6 / 8 taps to the composed passes and keeps these instances for
// measurement and tests; whether a (direction, dtype, L) cell is routed here is decided on the host, _bwt.COMPOSED3_CELLS.)
#include "mifwt_bwt_rows.h"

namespace mifwt {

namespace {

// ---- brick geometry (compile time) -------------------------------------------------------------------------------------------------------
template <typename T, int L>
struct Fwd3Tile {
  static constexpr int E = Vec16<T>::E;
  static constexpr int TC = 8 * E;                             // coefficient columns per brick: 8 lanes x one 16-byte store
  static constexpr int TD = L <= 6 ? 4 : 3;                    // coefficient slices per brick
  static constexpr int TR = L <= 4 ? 8 : (L == 6 ? 6 : (E == 4 ? 4 : 3));  // coefficient rows per brick
  static constexpr int PADI = round_up(L / 2 - 1, E);         // staged columns left of sample 2 mc0: interior bricks
  static constexpr int PADE = round_up(L - 2, E);             // ... bricks at an end (a bottom row's window reaches back L - 1 samples)
  static constexpr int WC = round_up(PADE + 2 * TC + L / 2 - 1, E);
  static constexpr int WR = 2 * TR + (L - 2) + L / 2 - 1;
  static constexpr int WD = 2 * TD + (L - 2) + L / 2 - 1;
  static constexpr int NTL = 2 * (L / 2 + 1) * L;              // table entries kept in LDS (>= 2 (nt + nb + 1) L)
  static constexpr int LDS3 = (WD * WR * WC + NTL) * (int)sizeof(T);
};

template <typename T, int L>
struct Inv3Tile {
  static constexpr int E = Vec16<T>::E;
  static constexpr int TQC = 8 * E;                            // coefficient columns per brick (2 TQC output samples)
  static constexpr int TQD = L <= 2 ? 4 : 2;                   // coefficient slices per brick
  static constexpr int TQR = L <= 2 ? 8 : (L == 8 && E == 2 ? 2 : 4);  // coefficient rows per brick
  static constexpr int PM = L <= 2 ? 0 : L / 2;                // staged coefficients either side (haar has no overlap)
  static constexpr int PMC = round_up(PM, E);
  static constexpr int WCM = TQC + 2 * PMC;
  static constexpr int WRM = TQR + 2 * PM;
  static constexpr int WDM = TQD + 2 * PM;
  static constexpr int NTL = 2 * (L / 2 + 1) * L;
  static constexpr int LDS3 = (8 * WDM * WRM * WCM + NTL) * (int)sizeof(T);
};

template <typename T, int L>
struct Bwt3Args {
  const void* in[8];   // analysis: in[0] = x;  synthesis: the eight bands (plane s: bit 2 depth, bit 1 height, bit 0 width high-pass)
  void* out[8];        // analysis: the bands;  synthesis: out[0] = y
  int64_t sig_bs, sig_ds, sig_rs;                     // signal side: batch / slice / row stride (elements; samples contiguous)
  int64_t a_bs, a_ds, a_rs, d_bs, d_ds, d_rs;         // band 0 / bands 1..7
  int n_d, n_r, n_c;         // real signal extents
  int m_d, m_r, m_c;         // coefficient extents = ceil(n / 2)
  int src_d, src_r, src_c;   // source index of the virtual sample of an odd extent (-1: zero)
  int sig_vec, coef_vec;     // 16-byte accesses allowed on the signal / coefficient side
  int tiles_c, tiles_r, tiles_d;
  const double* tab;         // DEVICE [2][max(nt + nb, 1)][L]
  T lo[L], hi[L];            // f_lo, f_hi
};

// One analysis output pair ACROSS rows / slices: coefficient m (brick-local index ml) of an axis whose window entries are `pitch` elements
// apart in LDS, E columns at a time.  ws = first staged sample of the axis, pad = 2 * (first coefficient of the brick) - ws.
template <typename T, int L>
__device__ __forceinline__ void analysis_across3(const T* col, int pitch, bool edge, int ml, int m, int m_ext, int pad, int ws, const T* tl,
                                                 const T (&flo)[L], const T (&fhi)[L], typename Vec16<T>::type& lo,
                                                 typename Vec16<T>::type& hi) {
  typedef typename Vec16<T>::type V;
  constexpr int NT = Rows<L>::NT, NB = Rows<L>::NB, NR = NT + NB;
  V sl = V(0), sh = V(0);
  if (!edge || (m >= NT && m < m_ext - NB)) {
    const int w0 = 2 * ml + pad - (L / 2 - 1);
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const V v = *reinterpret_cast<const V*>(col + (w0 + k) * pitch);
      sl += flo[L - 1 - k] * v;
      sh += fhi[L - 1 - k] * v;
    }
  } else if (m < m_ext) {
    int r, w0;
    if (m < NT) {
      r = m;
      w0 = -ws;
    } else {
      r = NT + m - (m_ext - NB);
      w0 = 2 * m_ext - L - ws;
    }
    const T* cl = tl + r * L;
    const T* ch = tl + (NR + 1 + r) * L;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const V v = *reinterpret_cast<const V*>(col + (w0 + k) * pitch);
      sl += cl[k] * v;
      sh += ch[k] * v;
    }
  }
  lo = sl;
  hi = sh;
}

extern __shared__ __attribute__((aligned(16))) unsigned char bwt3_lds[];

// ---- analysis ----------------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_fwd3_kernel(const Bwt3Args<T, L> a) {
  typedef Fwd3Tile<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TC = G::TC, TR = G::TR, TD = G::TD, WC = G::WC, WR = G::WR, WD = G::WD, CG = TC / E;
  constexpr int NT = Rows<L>::NT, NB = Rows<L>::NB, NR = NT + NB;
  static_assert(WC >= 2 * TC, "the width image of a row must fit into the row it replaces");
  static_assert(2 * TD + L / 2 - 1 >= L && 2 * TR + L / 2 - 1 >= L, "the window of the first brick must hold the L samples of a top row");
  static_assert(WR * WC >= TR * 4 * TC, "the (height, width) image of a slice must fit into the slice it replaces");
  T* const xs = reinterpret_cast<T*>(bwt3_lds);  // [WD][WR][WC]
  T* const tl = xs + WD * WR * WC;
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tc = bid % a.tiles_c;
  bid /= a.tiles_c;
  const int tr = bid % a.tiles_r;
  bid /= a.tiles_r;
  const int td = bid % a.tiles_d;
  const int b = bid / a.tiles_d;
  const int mc0 = tc * TC, mr0 = tr * TR, md0 = td * TD;
  const bool edge_c = NR > 0 && (mc0 < NT || mc0 + TC > a.m_c - NB);
  const bool edge_r = NR > 0 && (mr0 < NT || mr0 + TR > a.m_r - NB);
  const bool edge_d = NR > 0 && (md0 < NT || md0 + TD > a.m_d - NB);
  const int padc = edge_c ? G::PADE : G::PADI;
  const int padr = edge_r ? L - 2 : L / 2 - 1;
  const int padd = edge_d ? L - 2 : L / 2 - 1;
  const int wc = round_up(padc + 2 * TC + L / 2 - 1, E);  // staged columns (<= WC)
  const int wr = padr + 2 * TR + L / 2 - 1;                // staged rows (<= WR)
  const int wd = padd + 2 * TD + L / 2 - 1;                // staged slices (<= WD)
  const int ws_c = 2 * mc0 - padc, ws_r = 2 * mr0 - padr, ws_d = 2 * md0 - padd;
  const T* __restrict__ x = static_cast<const T*>(a.in[0]) + (int64_t)b * a.sig_bs;
  if (edge_c || edge_r || edge_d) load_table<T, L>(tl, a);
  const int vpr = wc / E;
  for (int i = tid; i < wd * wr * vpr; i += 256) {
    const int cv = i % vpr, r = (i / vpr) % wr, d = i / (vpr * wr);
    int gd = ws_d + d, gr = ws_r + r;
    const T* row = nullptr;
    if (gd >= 0 && gd < 2 * a.m_d && gr >= 0 && gr < 2 * a.m_r) {
      if (gd >= a.n_d) gd = a.src_d;
      if (gr >= a.n_r) gr = a.src_r;
      if (gd >= 0 && gr >= 0) row = x + (int64_t)gd * a.sig_ds + (int64_t)gr * a.sig_rs;
    }
    stage_vec<T, E>(xs + (d * WR + r) * WC + cv * E, row, ws_c + cv * E, a.n_c, 2 * a.m_c, a.src_c, a.sig_vec);
  }
  __syncthreads();
  // along the width, in place: row [wc samples] -> [TC low | TC high]
  {
    constexpr int IT = (WD * WR * CG + 255) / 256;
    const int n1 = wd * wr * CG;
    V lo[IT], hi[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * 256;
      if (i < n1) {
        const int cg = i % CG, r = (i / CG) % wr, d = i / (CG * wr);
        const T* xr = xs + (d * WR + r) * WC;
        if (edge_c && (mc0 + cg * E < NT || mc0 + cg * E + E > a.m_c - NB))  // (only the lanes whose outputs include a boundary row)
          analysis_run<T, L, true>(xr, padc, cg * E, mc0 + cg * E, a.m_c, tl, a.lo, a.hi, lo[it], hi[it]);
        else
          analysis_run<T, L, false>(xr, padc, cg * E, mc0 + cg * E, a.m_c, tl, a.lo, a.hi, lo[it], hi[it]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * 256;
      if (i < n1) {
        const int cg = i % CG, r = (i / CG) % wr, d = i / (CG * wr);
        T* xr = xs + (d * WR + r) * WC;
        *reinterpret_cast<V*>(xr + cg * E) = lo[it];
        *reinterpret_cast<V*>(xr + TC + cg * E) = hi[it];
      }
    }
    __syncthreads();
  }
  // along the height, in place: slice [wr rows][2 TC] -> [TR][4 planes (bit 1 height, bit 0 width)][TC]
  {
    constexpr int IT = (WD * TR * 2 * CG + 255) / 256;
    const int n2 = wd * TR * 2 * CG;
    V lo[IT], hi[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * 256;
      if (i < n2) {
        const int cg = i % CG, wb = (i / CG) & 1, ro = (i / (2 * CG)) % TR, d = i / (2 * CG * TR);
        analysis_across3<T, L>(xs + d * WR * WC + wb * TC + cg * E, WC, edge_r, ro, mr0 + ro, a.m_r, padr, ws_r, tl, a.lo, a.hi, lo[it],
                               hi[it]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * 256;
      if (i < n2) {
        const int cg = i % CG, wb = (i / CG) & 1, ro = (i / (2 * CG)) % TR, d = i / (2 * CG * TR);
        T* o = xs + d * WR * WC + ro * 4 * TC + cg * E;
        *reinterpret_cast<V*>(o + wb * TC) = lo[it];
        *reinterpret_cast<V*>(o + (2 + wb) * TC) = hi[it];
      }
    }
    __syncthreads();
  }
  // along the depth: eight bands, E columns per lane
  for (int i = tid; i < TD * TR * 4 * CG; i += 256) {
    const int cg = i % CG, pl = (i / CG) & 3, ro = (i / (4 * CG)) % TR, dq = i / (4 * CG * TR);
    const int md = md0 + dq, mr = mr0 + ro, mc = mc0 + cg * E;
    if (md >= a.m_d || mr >= a.m_r || mc >= a.m_c) continue;
    V lo, hi;
    analysis_across3<T, L>(xs + ro * 4 * TC + pl * TC + cg * E, WR * WC, edge_d, dq, md, a.m_d, padd, ws_d, tl, a.lo, a.hi, lo, hi);
    const int valid = a.m_c - mc;
    const int64_t oa = (int64_t)b * a.a_bs + (int64_t)md * a.a_ds + (int64_t)mr * a.a_rs + mc;
    const int64_t od = (int64_t)b * a.d_bs + (int64_t)md * a.d_ds + (int64_t)mr * a.d_rs + mc;
    store_vec<T>(static_cast<T*>(a.out[pl]) + (pl ? od : oa), lo, valid, a.coef_vec);
    store_vec<T>(static_cast<T*>(a.out[4 + pl]) + od, hi, valid, a.coef_vec);
  }
}

// ---- synthesis ---------------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(256) bwt_inv3_kernel(const Bwt3Args<T, L> a) {
  typedef Inv3Tile<T, L> G;
  typedef typename Vec16<T>::type V;
  constexpr int E = G::E, TQC = G::TQC, TQR = G::TQR, TQD = G::TQD, WCM = G::WCM, WRM = G::WRM, WDM = G::WDM, CV = WCM / E;
  constexpr int NR = Rows<L>::NR;
  T* const bs = reinterpret_cast<T*>(bwt3_lds);  // [8][WDM][WRM][WCM], then the images of the depth and the height pass
  T* const tl = bs + 8 * WDM * WRM * WCM;
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tc = bid % a.tiles_c;
  bid /= a.tiles_c;
  const int tr = bid % a.tiles_r;
  bid /= a.tiles_r;
  const int td = bid % a.tiles_d;
  const int b = bid / a.tiles_d;
  const int qc0 = tc * TQC, qr0 = tr * TQR, qd0 = td * TQD;
  const bool edge_c = NR > 0 && (2 * qc0 < L + 2 || 2 * (qc0 + TQC) + L + 2 >= 2 * a.m_c);
  const bool edge_r = NR > 0 && (2 * qr0 < L + 2 || 2 * (qr0 + TQR) + L + 2 >= 2 * a.m_r);
  const bool edge_d = NR > 0 && (2 * qd0 < L + 2 || 2 * (qd0 + TQD) + L + 2 >= 2 * a.m_d);
  // (a brick needs the table where one of its outputs is not a plain one: a superset of !synthesis_plain over its samples)
  const int mo_c = qc0 - G::PMC, mo_r = qr0 - G::PM, mo_d = qd0 - G::PM;
  if (edge_c || edge_r || edge_d) load_table<T, L>(tl, a);
  // the windows of the eight bands
  for (int i = tid; i < 8 * WDM * WRM * CV; i += 256) {
    const int cv = i % CV, r = (i / CV) % WRM, d = (i / (CV * WRM)) % WDM, s = i / (CV * WRM * WDM);
    const int md = mo_d + d, mr = mo_r + r;
    const T* row = nullptr;
    if (md >= 0 && md < a.m_d && mr >= 0 && mr < a.m_r)
      row = static_cast<const T*>(a.in[s]) + (s ? (int64_t)b * a.d_bs + (int64_t)md * a.d_ds + (int64_t)mr * a.d_rs
                                                : (int64_t)b * a.a_bs + (int64_t)md * a.a_ds + (int64_t)mr * a.a_rs);
    stage_vec<T, E>(bs + ((s * WDM + d) * WRM + r) * WCM + cv * E, row, mo_c + cv * E, a.m_c, a.m_c, -1, a.coef_vec);
  }
  __syncthreads();
  // along the depth, in place: [8][WDM] -> [4 planes (bit 1 height, bit 0 width)][2 TQD output slices]
  {
    constexpr int N1 = 4 * 2 * TQD * WRM * CV, IT = (N1 + 255) / 256;
    V v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * 256;
      if (i < N1) {
        const int cv = i % CV, r = (i / CV) % WRM, nl = (i / (CV * WRM)) % (2 * TQD), pl = i / (CV * WRM * 2 * TQD);
        const int n = 2 * qd0 + nl;
        auto get = [&](int db, int idx) -> V { return *reinterpret_cast<const V*>(bs + (((db * 4 + pl) * WDM + idx) * WRM + r) * WCM + cv * E); };
        V o = V(0);
        if (n < 2 * a.m_d)
          o = edge_d && !synthesis_plain<L>(n, a.m_d) ? synthesis_point<T, L, true, V>(n, mo_d, a.m_d, tl, a.lo, a.hi, get)
                                                        : synthesis_point<T, L, false, V>(n, mo_d, a.m_d, tl, a.lo, a.hi, get);
        v[it] = o;
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * 256;
      if (i < N1) *reinterpret_cast<V*>(bs + (i / CV) * WCM + (i % CV) * E) = v[it];  // [pl][nl][r][WCM]
    }
    __syncthreads();
  }
  // along the height, in place: [4][2 TQD][WRM] -> [2 (width band)][2 TQD][2 TQR output rows]
  {
    constexpr int N2 = 2 * 2 * TQD * 2 * TQR * CV, IT = (N2 + 255) / 256;
    V v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * 256;
      if (i < N2) {
        const int cv = i % CV, nl = (i / CV) % (2 * TQR), nd = (i / (CV * 2 * TQR)) % (2 * TQD), wb = i / (CV * 2 * TQR * 2 * TQD);
        const int n = 2 * qr0 + nl;
        auto get = [&](int hb, int idx) -> V {
          return *reinterpret_cast<const V*>(bs + ((((hb * 2 + wb) * 2 * TQD + nd) * WRM) + idx) * WCM + cv * E);
        };
        V o = V(0);
        if (n < 2 * a.m_r)
          o = edge_r && !synthesis_plain<L>(n, a.m_r) ? synthesis_point<T, L, true, V>(n, mo_r, a.m_r, tl, a.lo, a.hi, get)
                                                        : synthesis_point<T, L, false, V>(n, mo_r, a.m_r, tl, a.lo, a.hi, get);
        v[it] = o;
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * 256;
      if (i < N2) *reinterpret_cast<V*>(bs + (i / CV) * WCM + (i % CV) * E) = v[it];  // [wb][nd][nl][WCM]
    }
    __syncthreads();
  }
  // along the width: E consecutive samples per lane
  T* __restrict__ y = static_cast<T*>(a.out[0]) + (int64_t)b * a.sig_bs;
  constexpr int SG = 2 * TQC / E;
  for (int i = tid; i < 2 * TQD * 2 * TQR * SG; i += 256) {
    const int cg = i % SG, nl = (i / SG) % (2 * TQR), nd = i / (SG * 2 * TQR);
    const int gd = 2 * qd0 + nd, gr = 2 * qr0 + nl, nc = 2 * qc0 + cg * E;
    if (gd >= a.n_d || gr >= a.n_r || nc >= a.n_c) continue;
    auto get = [&](int wb, int idx) -> T { return bs[((wb * 2 * TQD + nd) * 2 * TQR + nl) * WCM + idx]; };
    V v;
#pragma unroll
    for (int e = 0; e < E; ++e)
      v[e] = (nc + e >= 2 * a.m_c) ? T(0)
             : edge_c && !synthesis_plain<L>(nc + e, a.m_c) ? synthesis_point<T, L, true, T>(nc + e, mo_c, a.m_c, tl, a.lo, a.hi, get)
                                                             : synthesis_point<T, L, false, T>(nc + e, mo_c, a.m_c, tl, a.lo, a.hi, get);
    store_vec<T>(y + (int64_t)gd * a.sig_ds + (int64_t)gr * a.sig_rs + nc, v, a.n_c - nc, a.sig_vec);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
constexpr int kMaxFused3 = 8;  // longest filter of the fused 3-D kernels

// 0 = not served by the fused kernels, MIFWT_ERR_BADARG = inconsistent, 1 = served
int fused3_check(const mifwt_level_desc* d) {
  if (!d) return MIFWT_ERR_BADARG;
  if (d->ndim != 3 || d->filt_len < 2 || d->filt_len > MIFWT_MAX_FILT || (d->filt_len & 1) || d->batch < 0) return MIFWT_ERR_BADARG;
  if (d->dtype != MIFWT_F32 && d->dtype != MIFWT_F64 && !is_storage16(d->dtype)) return MIFWT_ERR_BADARG;
  if (d->mode < MIFWT_MODE_ZERO || d->mode > MIFWT_MODE_SYMMETRIC) return MIFWT_ERR_BADARG;
  for (int ax = 0; ax < 3; ++ax) {
    const int64_t n = d->sig_extent[ax], m = d->coef_extent[ax];
    if (n < 1 || m < 1 || (n != 2 * m && n != 2 * m - 1)) return MIFWT_ERR_BADARG;
    if (2 * m < d->filt_len) return MIFWT_ERR_BADARG;  // a level needs L <= N
  }
  if (d->filt_len > kMaxFused3 || (d->dtype != MIFWT_F32 && d->dtype != MIFWT_F64)) return 0;
  if (d->sig_stride[3] != 1 || d->approx_stride[3] != 1 || d->detail_stride[3] != 1) return 0;
  int64_t tiles = d->batch;
  for (int ax = 0; ax < 3; ++ax) {
    if (2 * d->coef_extent[ax] < 2 * (d->filt_len - 1)) return 0;  // the two ends overlap: no compact table
    if (d->coef_extent[ax] > (1 << 29)) return 0;
    tiles *= (d->coef_extent[ax] + 1) / 2;  // (no brick is smaller than 2 coefficients along an axis)
    if (tiles > INT32_MAX) return 0;
  }
  return 1;
}

template <typename T, int L>
int launch_fused3(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* flo, const double* fhi,
                  const mifwt_bwt_tables* tb, hipStream_t stream) {
  constexpr int E = Vec16<T>::E;
  typedef Fwd3Tile<T, L> GF;
  typedef Inv3Tile<T, L> GI;
  static_assert(GF::LDS3 <= 80 * 1024, "analysis brick: two workgroups per CU");
  // (the synthesis bricks for 6 / 8 taps hold a CU alone; the host layer keeps those cells on the axis passes, _bwt.COMPOSED3_CELLS)
  static_assert(GI::LDS3 <= 80 * 1024 || L >= 6, "synthesis brick up to 4 taps: two workgroups per CU");
  static_assert(GF::LDS3 <= 160 * 1024 && GI::LDS3 <= 160 * 1024, "brick does not fit the LDS of a CU");
  Bwt3Args<T, L> a;
  for (int s = 0; s < 8; ++s) {
    a.in[s] = inverse ? in[s] : nullptr;
    a.out[s] = inverse ? nullptr : out[s];
  }
  if (inverse)
    a.out[0] = out[0];
  else
    a.in[0] = in[0];
  a.sig_bs = d->sig_stride[0], a.sig_ds = d->sig_stride[1], a.sig_rs = d->sig_stride[2];
  a.a_bs = d->approx_stride[0], a.a_ds = d->approx_stride[1], a.a_rs = d->approx_stride[2];
  a.d_bs = d->detail_stride[0], a.d_ds = d->detail_stride[1], a.d_rs = d->detail_stride[2];
  a.n_d = (int)d->sig_extent[0], a.n_r = (int)d->sig_extent[1], a.n_c = (int)d->sig_extent[2];
  a.m_d = (int)d->coef_extent[0], a.m_r = (int)d->coef_extent[1], a.m_c = (int)d->coef_extent[2];
  a.src_d = ext_index(a.n_d, a.n_d, d->mode);
  a.src_r = ext_index(a.n_r, a.n_r, d->mode);
  a.src_c = ext_index(a.n_c, a.n_c, d->mode);
  const void* sig = inverse ? (const void*)out[0] : in[0];
  a.sig_vec = aligned16(sig) && a.sig_bs % E == 0 && a.sig_ds % E == 0 && a.sig_rs % E == 0;
  a.coef_vec = a.a_bs % E == 0 && a.a_ds % E == 0 && a.a_rs % E == 0 && a.d_bs % E == 0 && a.d_ds % E == 0 && a.d_rs % E == 0;
  for (int s = 0; s < 8; ++s) a.coef_vec = a.coef_vec && aligned16(inverse ? in[s] : (const void*)out[s]);
  a.tab = tb->rows;
  for (int t = 0; t < L; ++t) {
    a.lo[t] = (T)flo[t];
    a.hi[t] = (T)fhi[t];
  }
  if (d->batch == 0) return MIFWT_OK;
  const int tcw = inverse ? GI::TQC : GF::TC, trw = inverse ? GI::TQR : GF::TR, tdw = inverse ? GI::TQD : GF::TD;
  a.tiles_c = (a.m_c + tcw - 1) / tcw;
  a.tiles_r = (a.m_r + trw - 1) / trw;
  a.tiles_d = (a.m_d + tdw - 1) / tdw;
  const int64_t grid = (int64_t)a.tiles_c * a.tiles_r * a.tiles_d * d->batch;
  if (grid > INT32_MAX) return MIFWT_ERR_UNSUPPORTED;
  const dim3 g((unsigned)grid), blk(256);
  if (inverse) {
    static DynLdsOnce once;
    if (GI::LDS3 > 65536 && !once.ensure(reinterpret_cast<const void*>(&bwt_inv3_kernel<T, L>), GI::LDS3)) return MIFWT_ERR_LAUNCH;
    hipLaunchKernelGGL((bwt_inv3_kernel<T, L>), g, blk, GI::LDS3, stream, a);
  } else {
    static DynLdsOnce once;
    if (GF::LDS3 > 65536 && !once.ensure(reinterpret_cast<const void*>(&bwt_fwd3_kernel<T, L>), GF::LDS3)) return MIFWT_ERR_LAUNCH;
    hipLaunchKernelGGL((bwt_fwd3_kernel<T, L>), g, blk, GF::LDS3, stream, a);
  }
  return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
}

template <typename T>
int dispatch_len3(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* flo, const double* fhi,
                  const mifwt_bwt_tables* tb, hipStream_t stream) {
  switch (d->filt_len) {
#define MIFWT_BWT3_CASE(LEN) \
  case LEN: return launch_fused3<T, LEN>(d, inverse, in, out, flo, fhi, tb, stream);
    MIFWT_BWT3_CASE(2)
    MIFWT_BWT3_CASE(4)
    MIFWT_BWT3_CASE(6)
    MIFWT_BWT3_CASE(8)
#undef MIFWT_BWT3_CASE
    default: return MIFWT_ERR_UNSUPPORTED;
  }
}

int bwt3_level(const mifwt_level_desc* d, int inverse, const void* const* in, void* const* out, const double* lo, const double* hi,
               const mifwt_bwt_tables* tb, void* stream) {
  const int ok = fused3_check(d);
  if (ok < 0) return ok;
  if (!lo || !hi || !tb || !tb->rows) return MIFWT_ERR_BADARG;
  const int L = d->filt_len;
  if (!table_fits(tb, L)) return MIFWT_ERR_BADARG;
  for (int s = 0; s < 8; ++s)
    if (!(inverse ? in[s] : (const void*)out[s])) return MIFWT_ERR_BADARG;
  if (!(inverse ? (const void*)out[0] : in[0])) return MIFWT_ERR_BADARG;
  if (!ok) return MIFWT_ERR_UNSUPPORTED;
  double flo[MIFWT_MAX_FILT], fhi[MIFWT_MAX_FILT];
  bank_taps(inverse, L, lo, hi, flo, fhi);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return d->dtype == MIFWT_F32 ? dispatch_len3<float>(d, inverse, in, out, flo, fhi, tb, st)
                               : dispatch_len3<double>(d, inverse, in, out, flo, fhi, tb, st);
}

}  // namespace

}  // namespace mifwt

extern "C" {

int mifwt_bwt3_supported(const mifwt_level_desc* desc, int direction) {
  if (direction != 0 && direction != 1) return MIFWT_ERR_BADARG;
  return mifwt::fused3_check(desc);
}

int mifwt_bwt3_kernel_id(const mifwt_level_desc* desc, int direction) {
  const int ok = mifwt_bwt3_supported(desc, direction);
  if (ok < 0) return ok;
  return ok ? (direction ? MIFWT_KID_BWT3_INV : MIFWT_KID_BWT3_FWD) : MIFWT_ERR_UNSUPPORTED;
}

int mifwt_bwt3_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* lo, const double* hi,
                   const mifwt_bwt_tables* tables, void* stream) {
  if (!desc || !details) return MIFWT_ERR_BADARG;
  const void* in[8] = {x, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  void* out[8] = {approx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int s = 1; s < 8; ++s) out[s] = details[s - 1];
  return mifwt::bwt3_level(desc, 0, in, out, lo, hi, tables, stream);
}

int mifwt_bwt3_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* lo, const double* hi,
                   const mifwt_bwt_tables* tables, void* stream) {
  if (!desc || !details) return MIFWT_ERR_BADARG;
  const void* in[8] = {approx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  void* out[8] = {y, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int s = 1; s < 8; ++s) in[s] = details[s - 1];
  return mifwt::bwt3_level(desc, 1, in, out, lo, hi, tables, stream);
}

}  // extern "C"
