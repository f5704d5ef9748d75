// mifwt_swt3.hip — fused 3-D stationary (undecimated, "a trous") wavelet levels for gfx950: kernel ids 36 (analysis) / 37 (synthesis).
//
// A 3-D level is the 1-D level of mifwt_swt.hip along the three axes of a volume (periodic, dilation D, any number of wraps), with
// SIX filters (w_* along axis -1, h_* along axis -2, z_* along axis -3):
//   analysis   p_b[s][r][n]    = sum_t w_b[t] x[s][r][(n + D (L/2 - t)) mod W]                                  b in {lo, hi}   (axis -1)
//              q_cb[s][r][n]   = sum_m h_c[m] p_b[s][(r + D (L/2 - m)) mod H][n]                                                (axis -2)
//              band_dcb[s][r][n] = scale sum_k z_d[k] q_cb[(s + D (L/2 - k)) mod Dz][r][n]                                      (axis -3)
//              band index 4 [d = hi] + 2 [c = hi] + [b = hi]: aaa, aad, ada, add, daa, dad, dda, ddd (first letter: axis -3)
//   synthesis  U_dc[s][r][n]   = sum_t w_lo[t] band_dc,lo[s][r][(n + D (L/2 - 1 - t)) mod W] + w_hi[t] band_dc,hi[s][r][..]    (axis -1)
//              V_d[s][r][n]    = sum_m h_lo[m] U_d,lo[s][(r + D (L/2 - 1 - m)) mod H][n] + h_hi[m] U_d,hi[s][..][n]             (axis -2)
//              y[s][r][n]      = scale sum_k z_lo[k] V_lo[(s + D (L/2 - 1 - k)) mod Dz][r][n] + z_hi[k] V_hi[..][r][n]          (axis -3)
// (scale = 1 resp. 1/8 in the transform; with all six filters reversed and the same scale each kernel is the other's adjoint).
//
// Bound: HBM — 1 volume in and 8 out (analysis), 8 in and 1 out (synthesis); one launch per level, no intermediate volume, every output
// written once.  As in mifwt_swt2.hip the kernel walks the a-trous LATTICE: output slice s only needs the slices (s + D k) mod Dz and
// output row r the rows (r + D m) mod H.  A WORKGROUP of four waves owns one volume, one slice residue rho_z < min(D, Dz), one row
// residue rho_r < min(D, H), a tile of RT lattice rows rho_r + i D, a strip of 64 E columns and a segment of the lattice slices
// rho_z + j D, and walks down the slices.  Per lattice slice:
//   1. axis -1 from GLOBAL memory for the RT + L - 1 lattice rows of the tile and its halo (wave w: halo rows w, w + 4, ..; a lane: E
//      columns; one vector load of the lane's run per tap, as swt2_kernel; lanes whose window wraps, or whose run hangs over the row
//      end, walk a wrapped index element by element).  The two (synthesis: four) results per point go to an LDS tile.
//   2. axis -2 from LDS: a lane owns RW tile rows x E columns, reads its RW + L - 1 LDS rows once and forms the four (synthesis: two)
//      values of each of its points.
//   3. axis -3 in REGISTERS: the values are pushed into a depth ring [L][4 resp. 2][RW][E] with compile-time slots (shifted, not
//      indexed); the slice that the newest lattice slice completes is combined, scaled and stored with full-width stores.
// The row halo re-reads the input (RT + L - 1) / RT times (one volume of nine in analysis; the re-reads of neighbouring tiles meet in
// L2), a segment's warm-up (L - 1) / segment of it.  The analysis tile is double-buffered: one __syncthreads() per slice; the
// synthesis tile (four planes, a taller tile) is single and takes two.  No wave leaves before a barrier: a workgroup without work
// returns as a whole, lanes beyond W and rows beyond the lattice are masked.  Indices wrap with mod for every extent (an extent that
// is no multiple of D, D >= an extent, an extent of 1): a lattice index is just an integer.
//
// LIMIT (mifwt_swt3_supported): compile-time lengths only — even L in 2 .. 10, float32 and float64.  The row halo makes long filters
// unattractive (the axis -1 pass runs (RT + L - 1) / RT times), so 12 .. 20 taps have no instance; they, longer filters and float16
// answer 0 / MIFWT_ERR_UNSUPPORTED and the caller composes the level from the 2-D and 1-D stationary levels.
#include "mifwt_axis_stream.h"

namespace mifwt {

namespace {

constexpr int kSwt3MaxFused = 10;

// compile-time geometry of an instance: a lane's run E, tile rows per lane RW, tile rows RT (four waves x RW), LDS planes and buffers
template <typename T, int L, bool INVERSE>
struct Swt3Geom {
  using A = typename ElemTraits<T>::Acc;
  static constexpr int E = (sizeof(T) == 4 && L <= 4) ? 2 : 1;
  // the synthesis ring is half as deep: a taller tile (less halo) where the registers allow it (float32 up to 6 taps)
  static constexpr int RW = (INVERSE && sizeof(T) == 4 && L <= 6) ? 4 : 2;
  static constexpr int RT = 4 * RW;
  static constexpr int NR = RT + L - 1;      // tile rows plus halo
  static constexpr int NP = INVERSE ? 4 : 2;  // LDS planes: (p_lo, p_hi) resp. U_dc
  static constexpr int NC = INVERSE ? 2 : 4;  // values per point in the depth ring: q_cb resp. V_d
  static constexpr int NBUF = INVERSE ? 1 : 2;
  static constexpr int COLS = 64 * E;
  static constexpr int LDS_BYTES = (NBUF * NP * NR * COLS + 2 * L) * (int)sizeof(A);  // the tile and the wrapped path's taps
};

template <typename A, int L>
struct Swt3Args {
  const void* in[8];  // analysis: x, -..            synthesis: the eight bands
  void* out[8];       // analysis: the eight bands   synthesis: y, -..
  int64_t in_vs[8], in_ss[8], in_rs[8], out_vs[8], out_ss[8], out_rs[8];  // volume / slice / row strides (elements)
  int Dz, H, W, D;
  int nresz, nresr, nsegs, ntiles, nstrips, seglen;
  A scale;
  A taps[6][L];  // w_lo, w_hi, h_lo, h_hi, z_lo, z_hi
};

// one tap of the axis -1 pass for element e: analysis p_lo += lo x, p_hi += hi x; synthesis U_p += lo band[2 p] + hi band[2 p + 1]
template <typename A, int NIN, int NP, int E>
__device__ __forceinline__ void swt3_row_tap(A lo, A hi, const A (&v)[NIN][E], int e, A (&acc)[NP][E]) {
  if constexpr (NIN == 8) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      acc[p][e] = fma(lo, v[2 * p][e], acc[p][e]);
      acc[p][e] = fma(hi, v[2 * p + 1][e], acc[p][e]);
    }
  } else {
    acc[0][e] = fma(lo, v[0][e], acc[0][e]);
    acc[1][e] = fma(hi, v[0][e], acc[1][e]);
  }
}

template <typename T, int L, bool INVERSE>
__global__ void __launch_bounds__(256) swt3_kernel(const Swt3Args<typename ElemTraits<T>::Acc, L> a) {
  using A = typename ElemTraits<T>::Acc;
  using G = Swt3Geom<T, L, INVERSE>;
  constexpr int E = G::E, RW = G::RW, RT = G::RT, NR = G::NR, NP = G::NP, NC = G::NC, NBUF = G::NBUF;
  constexpr int NIN = INVERSE ? 8 : 1;
  constexpr int NOUT = INVERSE ? 1 : 8;
  constexpr int OFF = L / 2 - (INVERSE ? 1 : 0);  // newest lattice index of output index i: i + OFF (tap 0), on every axis
  __shared__ A tile[NBUF][NP][NR][G::COLS];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int64_t task = blockIdx.x;
  const int strip = (int)(task % a.nstrips);
  task /= a.nstrips;
  const int rtile = (int)(task % a.ntiles);
  task /= a.ntiles;
  const int seg = (int)(task % a.nsegs);
  task /= a.nsegs;
  const int resr = (int)(task % a.nresr);
  task /= a.nresr;
  const int resz = (int)(task % a.nresz);
  const int64_t vol = task / a.nresz;
  const int Dz = a.Dz, H = a.H, W = a.W, D = a.D;
  const int cntz = (Dz - resz + D - 1) / D;  // slices resz + i D < Dz
  const int cntr = (H - resr + D - 1) / D;   // rows resr + i D < H
  const int i0 = seg * a.seglen;
  const int i1 = min(i0 + a.seglen, cntz);
  const int t0 = rtile * RT;
  if (i0 >= i1 || t0 >= cntr) return;  // the whole workgroup: nobody waits at a barrier
  // the wrapped path of the axis -1 pass takes its taps in a run-time loop: from LDS (a run-time index into the kernel arguments can
  // cost a scratch copy of them)
  __shared__ A wtaps[2][L];
#pragma unroll
  for (int t = 0; t < L; ++t)
    if (threadIdx.x == t) {
      wtaps[0][t] = a.taps[0][t];
      wtaps[1][t] = a.taps[1][t];
    }
  __syncthreads();
  const int n0 = (strip * 64 + lane) * E;
  const bool active = n0 < W;  // (a lane beyond the row end stays for the barriers)

  // columns: tap t reads the run starting at n0 + off_max - D t
  const int off_max = D * OFF;
  const int off_min = off_max - D * (L - 1);
  const bool interior = active && n0 + off_min >= 0 && n0 + off_max + E <= W;
  const int Dw = D % W;
  const int b0 = active ? (n0 + off_max) % W : 0;  // wrapped start of tap 0's run
  const bool narrow = W < E;                       // b + e may pass W more than once

  const T* __restrict__ pin[NIN];
#pragma unroll
  for (int q = 0; q < NIN; ++q) pin[q] = static_cast<const T*>(a.in[q]) + vol * a.in_vs[q];
  T* pout[NOUT];
#pragma unroll
  for (int q = 0; q < NOUT; ++q) pout[q] = static_cast<T*>(a.out[q]) + vol * a.out_vs[q] + n0;

  // rows of the axis -1 pass: this wave takes the halo rows k = wave, wave + 4, ..; halo row k is lattice row t0 + OFF - (L - 1) + k,
  // i.e. row (resr + that D) mod H — the same rows for every slice, stepped without a division
  const int D4h = (int)((4 * (int64_t)D) % H);
  int64_t r64 = ((int64_t)resr + (int64_t)(t0 + OFF - (L - 1) + wave) * D) % H;
  const int row0 = (int)(r64 < 0 ? r64 + H : r64);
  // slices: lattice index j -> slice (resz + j D) mod Dz
  const int Dzh = D % Dz;
  const int j0 = i0 + OFF - (L - 1);
  int64_t s64 = ((int64_t)resz + (int64_t)j0 * D) % Dz;
  int slice = (int)(s64 < 0 ? s64 + Dz : s64);

  A ring[L][NC][RW][E];
#pragma unroll
  for (int k = 0; k < L; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) ring[k][c][r][e] = A(0);

  const int rbase = wave * RW;  // this lane's tile rows in the axis -2 / -3 passes: rbase .. rbase + RW - 1
  const int jend = i1 - 1 + OFF;
  int buf = 0;
  for (int j = j0; j <= jend; ++j) {
    // ---- 1. axis -1 pass of lattice slice j, from global memory into the LDS tile
    {
      int row = row0;
#pragma unroll 1
      for (int k = wave; k < NR; k += 4) {
        if (active) {
          int64_t base[NIN];
#pragma unroll
          for (int q = 0; q < NIN; ++q) base[q] = (int64_t)slice * a.in_ss[q] + (int64_t)row * a.in_rs[q];
          A acc[NP][E];
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int e = 0; e < E; ++e) acc[p][e] = A(0);
          if (interior) {
#pragma unroll
            for (int t = 0; t < L; ++t) {
              const int s = n0 + off_max - D * t;
              A v[NIN][E];
#pragma unroll
              for (int q = 0; q < NIN; ++q) load_run<T, A, E>(pin[q] + base[q] + s, v[q]);
#pragma unroll
              for (int e = 0; e < E; ++e) swt3_row_tap<A, NIN, NP, E>(a.taps[0][t], a.taps[1][t], v, e, acc);
              // eight volumes per tap: a fence after every tap keeps eight loads in flight per lane instead of 8 L
              if (INVERSE) __builtin_amdgcn_sched_barrier(0);
            }
          } else {
            // the window wraps (or the run hangs over the row end): element by element along a wrapped index, taps in a run-time loop
            int b = b0;
#pragma unroll 1
            for (int t = 0; t < L; ++t) {
              const A tl = wtaps[0][t], th = wtaps[1][t];
              A v[NIN][E];
#pragma unroll
              for (int e = 0; e < E; ++e) {
                int i = b + e;
                if (narrow)
                  i %= W;
                else
                  i -= i >= W ? W : 0;
#pragma unroll
                for (int q = 0; q < NIN; ++q) v[q][e] = (A)pin[q][base[q] + i];
              }
#pragma unroll
              for (int e = 0; e < E; ++e) swt3_row_tap<A, NIN, NP, E>(tl, th, v, e, acc);
              b -= Dw;
              b += b < 0 ? W : 0;
            }
          }
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int e = 0; e < E; ++e) tile[buf][p][k][lane * E + e] = acc[p][e];
        }
        row += D4h;
        row -= row >= H ? H : 0;
      }
    }
    __syncthreads();
    // ---- 2. axis -2 pass from LDS: tile row rbase + r, tap m takes halo row rbase + r + (L - 1) - m
    A tmp[NP][RW + L - 1][E];
    if (active) {
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int kk = 0; kk < RW + L - 1; ++kk)
#pragma unroll
          for (int e = 0; e < E; ++e) tmp[p][kk][e] = tile[buf][p][rbase + kk][lane * E + e];
    }
    if (NBUF == 1)
      __syncthreads();  // the single tile is free for the next slice
    else
      buf ^= 1;  // the other tile: a wave that runs ahead writes it while the slow ones still read this one
    if (active) {
      // the ring is shifted (compile-time slots) and the newest slot filled
#pragma unroll
      for (int k = 0; k + 1 < L; ++k)
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int e = 0; e < E; ++e) ring[k][c][r][e] = ring[k + 1][c][r][e];
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) {
          A val[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c) val[c] = A(0);
#pragma unroll
          for (int m = 0; m < L; ++m) {
            const int kk = r + (L - 1) - m;
            if constexpr (INVERSE) {
#pragma unroll
              for (int c = 0; c < NC; ++c) {
                val[c] = fma(a.taps[2][m], tmp[2 * c][kk][e], val[c]);
                val[c] = fma(a.taps[3][m], tmp[2 * c + 1][kk][e], val[c]);
              }
            } else {
              // value 2 [axis -2 high] + [axis -1 high]
              val[0] = fma(a.taps[2][m], tmp[0][kk][e], val[0]);
              val[1] = fma(a.taps[2][m], tmp[1][kk][e], val[1]);
              val[2] = fma(a.taps[3][m], tmp[0][kk][e], val[2]);
              val[3] = fma(a.taps[3][m], tmp[1][kk][e], val[3]);
            }
          }
#pragma unroll
          for (int c = 0; c < NC; ++c) ring[L - 1][c][r][e] = val[c];
        }
      // ---- 3. axis -3 pass of output slice resz + i D, i = j - OFF: tap m takes lattice slice i + OFF - m = ring slot L - 1 - m
      const int i = j - OFF;
      if (i >= i0) {
        const int64_t oslice = (int64_t)resz + (int64_t)i * D;  // < Dz
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          const int li = t0 + rbase + r;
          if (li < cntr) {
            const int64_t orow = (int64_t)resr + (int64_t)li * D;  // < H
#pragma unroll
            for (int q = 0; q < NOUT; ++q) {
              A o[E];
#pragma unroll
              for (int e = 0; e < E; ++e) o[e] = A(0);
#pragma unroll
              for (int m = 0; m < L; ++m)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                  if constexpr (INVERSE) {
                    o[e] = fma(a.taps[4][m], ring[L - 1 - m][0][r][e], o[e]);
                    o[e] = fma(a.taps[5][m], ring[L - 1 - m][1][r][e], o[e]);
                  } else {
                    o[e] = fma(a.taps[4 + (q >> 2)][m], ring[L - 1 - m][q & 3][r][e], o[e]);
                  }
                }
#pragma unroll
              for (int e = 0; e < E; ++e) o[e] *= a.scale;
              T* op = pout[q] + oslice * a.out_ss[q] + orow * a.out_rs[q];
              if (n0 + E <= W) {
                store_run<T, A, E>(op, o);
              } else {
#pragma unroll
                for (int e = 0; e < E; ++e)
                  if (n0 + e < W) op[e] = (T)o[e];
              }
            }
          }
        }
      }
    }
    slice += Dzh;
    slice -= slice >= Dz ? Dz : 0;
  }
}

struct Swt3Call {
  int inverse, filt_len;
  int64_t volumes, Dz, H, W, dilation;
  const void* in[8];
  void* out[8];
  int64_t in_vs[8], in_ss[8], in_rs[8], out_vs[8], out_ss[8], out_rs[8];
  const double* taps[6];  // w_lo, w_hi, h_lo, h_hi, z_lo, z_hi
  double scale;
  hipStream_t stream;
};

struct Swt3Plan {
  int nresz, nresr, ntiles, nstrips, nsegs, seglen, RT, RW, E, lds_bytes, threads;
};

// Work split of a launch: a workgroup per (volume, slice residue, row residue, lattice segment, row tile, column strip).  Segments are
// cut only until the launch has about eight workgroups per CU, and never shorter than 4 L lattice slices (warm-up <= 25 % of the
// input passes); MIFWT_OPT_ROWS_PER_CHUNK overrides the lattice slices per segment.
template <typename T, int L, bool INVERSE>
Swt3Plan swt3_plan(int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t D) {
  using G = Swt3Geom<T, L, INVERSE>;
  Swt3Plan p;
  p.RT = G::RT;
  p.RW = G::RW;
  p.E = G::E;
  p.lds_bytes = G::LDS_BYTES;
  p.threads = 256;
  p.nresz = (int)(D < Dz ? D : Dz);
  p.nresr = (int)(D < H ? D : H);
  const int64_t maxcz = (Dz + D - 1) / D, maxcr = (H + D - 1) / D;
  p.ntiles = (int)((maxcr + G::RT - 1) / G::RT);
  p.nstrips = (int)((W + G::COLS - 1) / G::COLS);
  const int64_t base = volumes * p.nresz * p.nresr * p.ntiles * p.nstrips;
  const int64_t want = (2048 + base - 1) / (base > 0 ? base : 1);
  int64_t len = (maxcz + want - 1) / (want > 0 ? want : 1);
  if (len < 4 * L) len = 4 * L;
  if (g_options[MIFWT_OPT_ROWS_PER_CHUNK] > 0) len = g_options[MIFWT_OPT_ROWS_PER_CHUNK];
  if (len > maxcz) len = maxcz;
  p.seglen = (int)len;
  p.nsegs = (int)((maxcz + len - 1) / len);
  return p;
}

template <typename T, int L, bool INVERSE>
int swt3_launch(const Swt3Call& c) {
  using A = typename ElemTraits<T>::Acc;
  Swt3Args<A, L> a;
  for (int q = 0; q < 8; ++q) {
    a.in[q] = c.in[q];
    a.out[q] = c.out[q];
    a.in_vs[q] = c.in_vs[q];
    a.in_ss[q] = c.in_ss[q];
    a.in_rs[q] = c.in_rs[q];
    a.out_vs[q] = c.out_vs[q];
    a.out_ss[q] = c.out_ss[q];
    a.out_rs[q] = c.out_rs[q];
  }
  a.Dz = (int)c.Dz;
  a.H = (int)c.H;
  a.W = (int)c.W;
  a.D = (int)c.dilation;
  const Swt3Plan p = swt3_plan<T, L, INVERSE>(c.volumes, c.Dz, c.H, c.W, c.dilation);
  a.nresz = p.nresz;
  a.nresr = p.nresr;
  a.nsegs = p.nsegs;
  a.ntiles = p.ntiles;
  a.nstrips = p.nstrips;
  a.seglen = p.seglen;
  a.scale = (A)c.scale;
  for (int f = 0; f < 6; ++f)
    for (int t = 0; t < L; ++t) a.taps[f][t] = (A)c.taps[f][t];
  const int64_t nblk = c.volumes * p.nresz * p.nresr * p.nsegs * p.ntiles * p.nstrips;
  if (nblk == 0) return MIFWT_OK;
  if (nblk > INT32_MAX) return MIFWT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((swt3_kernel<T, L, INVERSE>), dim3((unsigned)nblk), dim3(256), 0, c.stream, a);
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  count_launch(INVERSE ? MIFWT_KERNEL_SWT3_INV : MIFWT_KERNEL_SWT3_FWD);
  return MIFWT_OK;
}

template <typename T, int L, bool INVERSE>
struct Swt3Tag {
  using Elem = T;
  static constexpr int kL = L;
  static constexpr bool kInverse = INVERSE;
};

// calls f(Swt3Tag<T, L, INVERSE>{}) for the instance of (dtype, filt_len, inverse); MIFWT_ERR_UNSUPPORTED where there is none
template <typename F>
int swt3_visit(int dtype, int filt_len, int inverse, F&& f) {
#define MIFWT_SWT3_CASE(LL)                                                                       \
  case LL:                                                                                        \
    if (dtype == MIFWT_F32) return inverse ? f(Swt3Tag<float, LL, true>{}) : f(Swt3Tag<float, LL, false>{}); \
    return inverse ? f(Swt3Tag<double, LL, true>{}) : f(Swt3Tag<double, LL, false>{});
  switch (filt_len) {
    MIFWT_SWT3_CASE(2)
    MIFWT_SWT3_CASE(4)
    MIFWT_SWT3_CASE(6)
    MIFWT_SWT3_CASE(8)
    MIFWT_SWT3_CASE(10)
    default: return MIFWT_ERR_UNSUPPORTED;
  }
#undef MIFWT_SWT3_CASE
}

// the limits of swt2_extents_ok, per axis
bool swt3_extents_ok(int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t dilation, int filt_len) {
  const int64_t lim = INT32_MAX / 8;
  return volumes <= lim && Dz <= lim && H <= lim && W <= lim && dilation * filt_len <= lim;
}

int swt3_level(Swt3Call& c, int dtype) {
  const int nin = c.inverse ? 8 : 1, nout = c.inverse ? 1 : 8;
  for (int q = 0; q < nin; ++q)
    if (!c.in[q]) return MIFWT_ERR_BADARG;
  for (int q = 0; q < nout; ++q)
    if (!c.out[q]) return MIFWT_ERR_BADARG;
  for (int q = 0; q < 6; ++q)
    if (!c.taps[q]) return MIFWT_ERR_BADARG;
  if (c.filt_len < 2 || (c.filt_len & 1) || c.filt_len > MIFWT_MAX_FILT || c.volumes < 0 || c.Dz < 1 || c.H < 1 || c.W < 1 ||
      c.dilation < 1)
    return MIFWT_ERR_BADARG;
  if (!mifwt_swt3_supported(dtype, c.filt_len, c.volumes, c.Dz, c.H, c.W, c.dilation)) return MIFWT_ERR_UNSUPPORTED;
  return swt3_visit(dtype, c.filt_len, c.inverse, [&](auto tag) {
    using Tag = decltype(tag);
    return swt3_launch<typename Tag::Elem, Tag::kL, Tag::kInverse>(c);
  });
}

}  // namespace

}  // namespace mifwt

extern "C" {

int mifwt_swt3_supported(int dtype, int filt_len, int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t dilation) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return 0;
  if (filt_len < 2 || (filt_len & 1) || filt_len > mifwt::kSwt3MaxFused) return 0;
  if (volumes < 0 || Dz < 1 || H < 1 || W < 1 || dilation < 1) return 0;
  return mifwt::swt3_extents_ok(volumes, Dz, H, W, dilation, filt_len) ? 1 : 0;
}

int mifwt_swt3_fwd(int dtype, int filt_len, int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t dilation, const void* x,
                   int64_t x_volume_stride, int64_t x_slice_stride, int64_t x_row_stride, void* const* bands,
                   const int64_t* band_volume_strides, const int64_t* band_slice_strides, const int64_t* band_row_strides,
                   const double* const* taps, double scale, void* stream) {
  if (!bands || !band_volume_strides || !band_slice_strides || !band_row_strides || !taps) return MIFWT_ERR_BADARG;
  mifwt::Swt3Call c = {};
  c.inverse = 0;
  c.filt_len = filt_len;
  c.volumes = volumes;
  c.Dz = Dz;
  c.H = H;
  c.W = W;
  c.dilation = dilation;
  c.in[0] = x;
  c.in_vs[0] = x_volume_stride;
  c.in_ss[0] = x_slice_stride;
  c.in_rs[0] = x_row_stride;
  for (int q = 0; q < 8; ++q) {
    c.out[q] = bands[q];
    c.out_vs[q] = band_volume_strides[q];
    c.out_ss[q] = band_slice_strides[q];
    c.out_rs[q] = band_row_strides[q];
  }
  for (int q = 0; q < 6; ++q) c.taps[q] = taps[q];
  c.scale = scale;
  c.stream = static_cast<hipStream_t>(stream);
  return mifwt::swt3_level(c, dtype);
}

int mifwt_swt3_inv(int dtype, int filt_len, int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t dilation,
                   const void* const* bands, const int64_t* band_volume_strides, const int64_t* band_slice_strides,
                   const int64_t* band_row_strides, void* y, int64_t y_volume_stride, int64_t y_slice_stride, int64_t y_row_stride,
                   const double* const* taps, double scale, void* stream) {
  if (!bands || !band_volume_strides || !band_slice_strides || !band_row_strides || !taps) return MIFWT_ERR_BADARG;
  mifwt::Swt3Call c = {};
  c.inverse = 1;
  c.filt_len = filt_len;
  c.volumes = volumes;
  c.Dz = Dz;
  c.H = H;
  c.W = W;
  c.dilation = dilation;
  for (int q = 0; q < 8; ++q) {
    c.in[q] = bands[q];
    c.in_vs[q] = band_volume_strides[q];
    c.in_ss[q] = band_slice_strides[q];
    c.in_rs[q] = band_row_strides[q];
  }
  c.out[0] = y;
  c.out_vs[0] = y_volume_stride;
  c.out_ss[0] = y_slice_stride;
  c.out_rs[0] = y_row_stride;
  for (int q = 0; q < 6; ++q) c.taps[q] = taps[q];
  c.scale = scale;
  c.stream = static_cast<hipStream_t>(stream);
  return mifwt::swt3_level(c, dtype);
}

int mifwt_swt3_plan(int dtype, int filt_len, int inverse, int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t dilation, int* out,
                    int capacity) {
  if (!out || capacity < MIFWT_SWT3_PLAN_INTS) return MIFWT_ERR_BADARG;
  if (!mifwt_swt3_supported(dtype, filt_len, volumes, Dz, H, W, dilation)) return MIFWT_ERR_UNSUPPORTED;
  return mifwt::swt3_visit(dtype, filt_len, inverse ? 1 : 0, [&](auto tag) {
    using Tag = decltype(tag);
    const mifwt::Swt3Plan p = mifwt::swt3_plan<typename Tag::Elem, Tag::kL, Tag::kInverse>(volumes, Dz, H, W, dilation);
    const int v[MIFWT_SWT3_PLAN_INTS] = {p.nresz, p.nresr, p.nsegs, p.seglen, p.ntiles, p.nstrips, p.RT, p.RW, p.E, p.lds_bytes, p.threads};
    for (int i = 0; i < MIFWT_SWT3_PLAN_INTS; ++i) out[i] = v[i];
    return MIFWT_SWT3_PLAN_INTS;
  });
}

}  // extern "C"
