// mifwt_thresh.hip — coefficient thresholding (pywt.threshold / pywt.threshold_firm) over a whole coefficient container per launch
// (C ABI mifwt_thresh_fwd / mifwt_thresh_bwd / mifwt_thresh_plan, include/mifwt.h; kernel ids 48 / 49).
//
// A launch takes up to kMaxSeg SEGMENTS, one per tensor: rows of `n` contiguous elements, the rows addressed through two outer extents
// with element strides.  The segment table travels in the kernel arguments (no device-side table, no staged copy: capturable).
//
// THE MAP.  A row is cut into SLOTS of 16 bytes (VEC elements).  Slot s of a row covers columns [s VEC - a, s VEC - a + VEC) clipped to
// [0, n), where a is the misalignment (in elements) of the row's first element when input and output rows (and, backward, the upstream
// gradient's) are misaligned by the SAME amount, else 0; a row has vpr = ceil((n + VEC - 1) / VEC) slots whatever a is.  A slot that lies
// inside the row and whose rows agree in alignment moves as one 16-byte load and one 16-byte store; every other slot — the head and the
// tail of a row, every slot of a row whose operands disagree — is peeled element by element.  Nothing is ever rounded down to an
// aligned address.  Rows are grouped by threshold index (`rows_per_value`): a UNIT, the work of one block iteration, is part of one row
// (long rows: upr units of su slots per row) or up to rb whole rows of one group (short rows), so a unit has ONE threshold of each kind
// and its threshold-gradient partial has one destination.  Blocks walk the units of all segments in a grid-stride loop and find a unit's
// segment in the prefix table `ustart`.  tests/test_thresh_host.py holds the CPU model of this map.
//
// FORWARD (48): loads, the closed form in the arithmetic type (float for f32 / f16 / bf16, double for f64), plain vector stores.  No LDS,
// no atomics.  BACKWARD (49): reads x and g, writes g_x = g dT/dx, and sums g dT/dv per unit: per thread at most kSlotsPerThread * VEC
// terms in the arithmetic type, from there on float64 across the wave (shuffles) and the workgroup (LDS), one plain float64 store per
// unit and threshold into the workspace.  A second tiny launch sums, per destination, the units that share it in a fixed order: no
// atomics anywhere, the same inputs give the same bits.
#include "mifwt_common.h"

namespace mifwt {
namespace {

constexpr int kMaxSeg = 24;
constexpr int kThreads = 256;
constexpr int kSlotsPerThread = 4;
constexpr uint32_t kUnitSlots = kThreads * kSlotsPerThread;  // slots of a full unit
constexpr int kMaxGrid = 2048;                               // memory-bound: cap the grid and stride over the rest

struct f16_t {
  uint16_t b;
};
struct bf16_t {
  uint16_t b;
};

template <typename C>
struct Arith {
  typedef float type;
};
template <>
struct Arith<double> {
  typedef double type;
};

__device__ __forceinline__ float to_arith(float v) { return v; }
__device__ __forceinline__ double to_arith(double v) { return v; }
__device__ __forceinline__ float to_arith(f16_t v) { return (float)__builtin_bit_cast(_Float16, v.b); }
__device__ __forceinline__ float to_arith(bf16_t v) { return __builtin_bit_cast(float, (uint32_t)v.b << 16); }
__device__ __forceinline__ void from_arith(float& o, float v) { o = v; }
__device__ __forceinline__ void from_arith(double& o, double v) { o = v; }
__device__ __forceinline__ void from_arith(f16_t& o, float v) { o.b = __builtin_bit_cast(uint16_t, (_Float16)v); }  // round to nearest even
__device__ __forceinline__ void from_arith(bf16_t& o, float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  if ((u & 0x7fffffffu) > 0x7f800000u)
    o.b = (uint16_t)((u >> 16) | 0x40u);  // NaN stays NaN
  else
    o.b = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);  // round to nearest even
}

// 16 bytes of storage
template <typename C>
struct alignas(16) Vec16 {
  C c[16 / sizeof(C)];
};
template <typename C>
__device__ __forceinline__ Vec16<C> load16(const C* p) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  return __builtin_bit_cast(Vec16<C>, *reinterpret_cast<const u4*>(p));
}
template <typename C>
__device__ __forceinline__ void store16(C* p, const Vec16<C>& v) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  *reinterpret_cast<u4*>(p) = __builtin_bit_cast(u4, v);
}

struct KSeg {
  const char* x;
  char* y;
  const char* g;
  int64_t xs0, xs1, ys0, ys1, gs0, gs1;  // element strides of the two outer extents
  const double* dv[2];                   // device thresholds (null: v)
  double v[2];
  uint32_t n;        // elements per row
  uint32_t e1;       // inner one of the two outer extents: row = i0 * e1 + i1
  uint32_t vpr;      // slots per row
  uint32_t upr, su;  // long rows (rb == 0): units per row, slots per unit
  uint32_t rb;       // short rows: whole rows per unit
  uint32_t rg;       // rows per group (rows that share every threshold index)
  uint32_t upg;      // units per group
  uint32_t tdiv[2];  // groups per threshold index (0: one value for the segment)
  uint32_t pad_;
};

struct ThreshArgs {
  KSeg seg[kMaxSeg];
  uint32_t ustart[kMaxSeg + 1];
  int nseg;
  double sub;
  double* part;  // backward: [2][total units] float64 partials (null: no threshold gradient wanted)
};
static_assert(sizeof(ThreshArgs) <= 4096, "the segment table must fit the kernel-argument segment");

enum { kSoft = MIFWT_THRESH_SOFT, kHard = MIFWT_THRESH_HARD, kGarrote = MIFWT_THRESH_GARROTE, kGreater = MIFWT_THRESH_GREATER,
       kLess = MIFWT_THRESH_LESS, kFirm = MIFWT_THRESH_FIRM };

// ---- the closed forms ------------------------------------------------------------------------------------------------------------
// T(x) for real x.  v: the threshold (firm: the low one), hi: firm's high threshold, sub: the substitute, use_sub: sub != 0.
template <int MODE, typename A>
__device__ __forceinline__ A thr_real(A x, A v, A hi, A sub, bool use_sub) {
  const A m = x < A(0) ? -x : x;
  const A none = A(0);
  if (MODE == kSoft) return m > v ? (x < A(0) ? x + v : x - v) : (use_sub && m < v ? sub : none);
  if (MODE == kHard) return m >= v ? x : sub;
  if (MODE == kGarrote) return m > v ? x * (A(1) - (v * v) / (x * x)) : (use_sub && m < v ? sub : none);
  if (MODE == kGreater) return x >= v ? x : sub;
  if (MODE == kLess) return x <= v ? x : sub;
  // firm: (the quotient is at most one and no difference is amplified: hi (m - v) <= m (hi - v) for m <= hi)
  if (!(m > v)) return none;
  if (m > hi) return x;
  return x * ((hi * (m - v)) / (m * (hi - v)));
}

// T(re + i im), the magnitude of the complex number deciding (soft, hard, garrote, firm)
template <int MODE, typename A>
__device__ __forceinline__ void thr_cplx(A& re, A& im, A v, A hi, A sub, bool use_sub) {
  const A m2 = re * re + im * im;
  const A m = sizeof(A) == 8 ? (A)__builtin_sqrt((double)m2) : (A)__builtin_sqrtf((float)m2);
  A f = A(0);
  bool replaced = false;
  if (MODE == kSoft) {
    if (m > v)
      f = A(1) - v / m;
    else
      replaced = use_sub && m < v;
  } else if (MODE == kHard) {
    if (m >= v)
      f = A(1);
    else
      replaced = true;
  } else if (MODE == kGarrote) {
    if (m > v)
      f = A(1) - (v * v) / m2;
    else
      replaced = use_sub && m < v;
  } else {
    if (m > hi)
      f = A(1);
    else if (m > v)
      f = (hi * (m - v)) / (m * (hi - v));
  }
  if (replaced) {
    re = sub;
    im = A(0);
  } else if (f != A(1)) {
    re = f == A(0) ? A(0) : re * f;
    im = f == A(0) ? A(0) : im * f;
  }
}

// dT/dx and the products g dT/dv (firm: dT/dv_lo in t0, dT/dv_hi in t1) for real x
template <int MODE, typename A>
__device__ __forceinline__ A thr_grad(A x, A g, A v, A hi, A& t0, A& t1) {
  const A m = x < A(0) ? -x : x;
  if (MODE == kSoft) {
    if (!(m > v)) return A(0);
    t0 += x < A(0) ? g : -g;
    return g;
  }
  if (MODE == kGarrote) {
    if (!(m > v)) return A(0);
    t0 += (A(-2) * v / x) * g;
    return g * (A(1) + (v * v) / (x * x));
  }
  if (MODE == kHard) return m >= v ? g : A(0);
  if (MODE == kGreater) return x >= v ? g : A(0);
  if (MODE == kLess) return x <= v ? g : A(0);
  // firm: T = hi (x - v s) / (hi - v) in the middle zone, s = sign(x)
  if (!(m > v)) return A(0);
  if (m > hi) return g;
  const A d = hi - v, sg = x < A(0) ? -g : g;
  t0 += sg * (hi * (m - hi)) / (d * d);
  t1 -= sg * (v * (m - v)) / (d * d);
  return g * (hi / d);
}

template <typename C, bool CPLX, int MODE, bool BWD>
struct SlotCtx {
  typedef typename Arith<C>::type A;
  static constexpr int NC = 16 / sizeof(C), EC = CPLX ? 2 : 1, VEC = NC / EC;
  A v, hi, sub;
  bool use_sub;
  uint32_t n;
  A t0, t1;  // this thread's threshold-gradient partials

  __device__ __forceinline__ void element(const C* px, C* py, const C* pg) {
    if (CPLX) {
      A re = to_arith(px[0]), im = to_arith(px[1]);
      thr_cplx<MODE>(re, im, v, hi, sub, use_sub);
      from_arith(py[0], re);
      from_arith(py[1], im);
    } else if (BWD) {
      from_arith(py[0], thr_grad<MODE>(to_arith(px[0]), to_arith(pg[0]), v, hi, t0, t1));
    } else {
      from_arith(py[0], thr_real<MODE>(to_arith(px[0]), v, hi, sub, use_sub));
    }
  }

  // slot `sl` of the row that starts at px / py / pg
  __device__ __forceinline__ void slot(const C* px, C* py, const C* pg, uint32_t sl) {
    constexpr uintptr_t ESZ = sizeof(C) * EC;
    const uintptr_t mx = (uintptr_t)px & 15, my = (uintptr_t)py & 15, mg = BWD ? (uintptr_t)pg & 15 : mx;
    const bool agree = mx == my && mx == mg && mx % ESZ == 0;
    const int64_t c0 = (int64_t)sl * VEC - (agree ? (int64_t)(mx / ESZ) : 0);  // (column c0 of an agreeing row is 16-byte aligned)
    if (agree && c0 >= 0 && c0 + VEC <= (int64_t)n) {
      const Vec16<C> xv = load16(px + c0 * EC);
      Vec16<C> gv, yv;
      if (BWD) gv = load16(pg + c0 * EC);
#pragma unroll
      for (int j = 0; j < VEC; ++j) element(&xv.c[j * EC], &yv.c[j * EC], BWD ? &gv.c[j * EC] : nullptr);
      store16(py + c0 * EC, yv);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int64_t c = c0 + j;
        if (c >= 0 && c < (int64_t)n) element(px + c * EC, py + c * EC, BWD ? pg + c * EC : nullptr);
      }
    }
  }
};

template <typename C, bool CPLX, int MODE, bool BWD>
__global__ __launch_bounds__(kThreads) void thresh_kernel(const ThreshArgs a) {
  typedef SlotCtx<C, CPLX, MODE, BWD> Ctx;
  typedef typename Ctx::A A;
  constexpr int EC = Ctx::EC;
  __shared__ double red[BWD ? 2 * (kThreads / 64) : 1];
  const uint32_t total = a.ustart[a.nseg];
  for (uint32_t u = blockIdx.x; u < total; u += gridDim.x) {
    int si = 0;
    while (si + 1 < a.nseg && u >= a.ustart[si + 1]) ++si;
    const KSeg& s = a.seg[si];
    const uint32_t lu = u - a.ustart[si];
    const uint32_t grp = lu / s.upg, ug = lu - grp * s.upg;
    Ctx c;
    c.n = s.n;
    c.sub = (A)a.sub;
    c.use_sub = a.sub != 0.0;
    c.t0 = c.t1 = A(0);
    c.v = s.dv[0] ? (A)s.dv[0][s.tdiv[0] ? grp / s.tdiv[0] : 0] : (A)s.v[0];
    c.hi = MODE != kFirm ? A(0) : s.dv[1] ? (A)s.dv[1][s.tdiv[1] ? grp / s.tdiv[1] : 0] : (A)s.v[1];
    const C* x = reinterpret_cast<const C*>(s.x);
    C* y = reinterpret_cast<C*>(s.y);
    const C* g = reinterpret_cast<const C*>(s.g);
    if (s.rb == 0) {  // part of one row
      const uint32_t rr = ug / s.upr, part = ug - rr * s.upr;
      const uint32_t row = grp * s.rg + rr, s0 = part * s.su;
      const uint32_t cnt = min(s.su, s.vpr - s0);
      const int64_t i0 = row / s.e1, i1 = row - (row / s.e1) * s.e1;
      const C* px = x + (i0 * s.xs0 + i1 * s.xs1) * EC;
      C* py = y + (i0 * s.ys0 + i1 * s.ys1) * EC;
      const C* pg = BWD ? g + (i0 * s.gs0 + i1 * s.gs1) * EC : nullptr;
      for (uint32_t l = threadIdx.x; l < cnt; l += kThreads) c.slot(px, py, pg, s0 + l);
    } else {  // whole short rows of one group
      const uint32_t r0 = ug * s.rb;
      const uint32_t cnt = min(s.rb, s.rg - r0) * s.vpr;
      for (uint32_t l = threadIdx.x; l < cnt; l += kThreads) {
        const uint32_t rr = l / s.vpr, sl = l - rr * s.vpr;
        const uint32_t row = grp * s.rg + r0 + rr;
        const int64_t i0 = s.e1 == 1 ? row : row / s.e1, i1 = s.e1 == 1 ? 0 : row - (row / s.e1) * s.e1;
        c.slot(x + (i0 * s.xs0 + i1 * s.xs1) * EC, y + (i0 * s.ys0 + i1 * s.ys1) * EC,
               BWD ? g + (i0 * s.gs0 + i1 * s.gs1) * EC : nullptr, sl);
      }
    }
    if (BWD && a.part != nullptr) {  // (uniform: every thread of the block takes it or none)
      double d0 = (double)c.t0, d1 = (double)c.t1;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        d0 += __shfl_xor(d0, o, 64);
        d1 += __shfl_xor(d1, o, 64);
      }
      const int wave = threadIdx.x >> 6;
      if ((threadIdx.x & 63) == 0) {
        red[2 * wave] = d0;
        red[2 * wave + 1] = d1;
      }
      __syncthreads();
      if (threadIdx.x < 2) {  // lane k sums threshold k of the waves in a fixed order: one plain store each
        double t = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) t += red[2 * w + threadIdx.x];
        a.part[(size_t)threadIdx.x * total + u] = t;
      }
      __syncthreads();
    }
  }
}

// ---- second launch of the backward: per destination, the sum of the unit partials that share it -----------------------------------
struct RedArgs {
  const double* part[2 * kMaxSeg];  // first partial of entry e (a segment's units of threshold k)
  double* dst[2 * kMaxSeg];         // distinct destinations
  uint32_t upd[2 * kMaxSeg];        // units per destination element of entry e
  uint32_t dst_n[2 * kMaxSeg];      // elements of destination d
  uint32_t bstart[2 * kMaxSeg + 1];
  uint8_t dst_of[2 * kMaxSeg];      // destination of entry e
  int nent, ndst;
};

constexpr int kRedThreads = 1024;  // (one workgroup per destination element: a one-element threshold sums thousands of partials here)

__global__ __launch_bounds__(kRedThreads) void thresh_reduce_kernel(const RedArgs a) {
  __shared__ double red[kRedThreads];
  int d = 0;
  while (d + 1 < a.ndst && blockIdx.x >= a.bstart[d + 1]) ++d;
  const uint32_t t = blockIdx.x - a.bstart[d];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};  // (four loads in flight per thread; the order of the sum is fixed all the same)
  for (int e = 0; e < a.nent; ++e) {
    if (a.dst_of[e] != d) continue;
    const uint32_t n = a.upd[e];
    const double* p = a.part[e] + (size_t)t * n;
    uint32_t i = threadIdx.x;
    for (; i + 3 * kRedThreads < n; i += 4 * kRedThreads) {
      const double v0 = p[i], v1 = p[i + kRedThreads], v2 = p[i + 2 * kRedThreads], v3 = p[i + 3 * kRedThreads];
      acc[0] += v0, acc[1] += v1, acc[2] += v2, acc[3] += v3;
    }
    for (; i < n; i += kRedThreads) acc[0] += p[i];
  }
  red[threadIdx.x] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  for (int w = kRedThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.dst[d][t] = red[0];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct Geo {
  uint32_t n, e1, vpr, upr, su, rb, rg, upg, tdiv[2];
  uint64_t rows, groups, units;
};

int seg_geometry(int dtype, int is_complex, const mifwt_thresh_seg& s, Geo* o) {
  const int64_t e0 = s.extent[0], e1 = s.extent[1], n = s.extent[2];
  if (e0 < 0 || e1 < 0 || n < 0) return MIFWT_ERR_BADARG;
  if (n > 1 && (s.x_stride[2] != 1 || s.y_stride[2] != 1)) return MIFWT_ERR_BADARG;
  const int comp = dtype == MIFWT_F64 ? 8 : dtype == MIFWT_F32 ? 4 : 2;
  const int vec = 16 / (comp * (is_complex ? 2 : 1));
  Geo g = {};
  if (e0 == 0 || e1 == 0 || n == 0) {
    *o = g;
    return MIFWT_OK;
  }
  if (n > (int64_t)1 << 30 || e1 > (int64_t)1 << 30 || (double)e0 * (double)e1 >= 2147483648.0) return MIFWT_ERR_UNSUPPORTED;
  g.rows = (uint64_t)e0 * (uint64_t)e1;
  g.n = (uint32_t)n;
  g.e1 = (uint32_t)e1;
  g.vpr = (uint32_t)((n + 2 * (int64_t)vec - 2) / vec);
  // groups: rows that share both threshold indices (the finer of the two forms; the coarser one must nest)
  uint64_t rg = g.rows;
  for (int k = 0; k < 2; ++k) {
    const int64_t rp = s.dvalue[k] ? s.rows_per_value[k] : 0;
    if (rp < 0 || (rp > 0 && g.rows % (uint64_t)rp != 0)) return MIFWT_ERR_BADARG;
    if (rp > 0 && (uint64_t)rp < rg) rg = (uint64_t)rp;
  }
  for (int k = 0; k < 2; ++k) {
    const int64_t rp = s.dvalue[k] ? s.rows_per_value[k] : 0;
    if (rp > 0 && (uint64_t)rp % rg != 0) return MIFWT_ERR_BADARG;
    g.tdiv[k] = rp > 0 ? (uint32_t)((uint64_t)rp / rg) : 0;
  }
  g.rg = (uint32_t)rg;
  g.groups = g.rows / rg;
  if (g.vpr >= kUnitSlots) {
    g.rb = 0;
    g.upr = (g.vpr + kUnitSlots - 1) / kUnitSlots;
    g.su = (g.vpr + g.upr - 1) / g.upr;
    g.upr = (g.vpr + g.su - 1) / g.su;  // (no empty unit at the end of a row)
    const uint64_t upg = (uint64_t)g.rg * g.upr;
    if (upg >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;
    g.upg = (uint32_t)upg;
  } else {
    g.rb = kUnitSlots / g.vpr;
    g.upr = 1;
    g.su = 0;
    g.upg = (g.rg + g.rb - 1) / g.rb;
  }
  g.units = g.groups * g.upg;
  *o = g;
  return MIFWT_OK;
}

int check_call(int dtype, int is_complex, int mode, int nseg, const mifwt_thresh_seg* segs) {
  if (segs == nullptr || nseg < 1 || nseg > kMaxSeg) return MIFWT_ERR_BADARG;
  if (mode < MIFWT_THRESH_SOFT || mode > MIFWT_THRESH_FIRM) return MIFWT_ERR_BADARG;
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64 && dtype != MIFWT_F16 && dtype != MIFWT_BF16) return MIFWT_ERR_BADARG;
  if (is_complex && (mode == MIFWT_THRESH_GREATER || mode == MIFWT_THRESH_LESS)) return MIFWT_ERR_UNSUPPORTED;
  if (is_complex && is_storage16(dtype)) return MIFWT_ERR_UNSUPPORTED;
  return MIFWT_OK;
}

// fills the table; returns the number of units or an error code
int64_t build_args(int dtype, int is_complex, const mifwt_thresh_seg* segs, int nseg, bool bwd, ThreshArgs* a, int64_t* unit_start) {
  uint64_t total = 0;
  for (int i = 0; i < nseg; ++i) {
    Geo g;
    const int rc = seg_geometry(dtype, is_complex, segs[i], &g);
    if (rc != MIFWT_OK) return rc;
    const mifwt_thresh_seg& s = segs[i];
    if (g.units && (s.x == nullptr || s.y == nullptr) && a != nullptr) return MIFWT_ERR_BADARG;
    if (bwd && g.units && a != nullptr && (s.g == nullptr || (g.n > 1 && s.g_stride[2] != 1))) return MIFWT_ERR_BADARG;
    if (unit_start) unit_start[i] = (int64_t)total;
    if (a) {
      KSeg& k = a->seg[i];
      k.x = static_cast<const char*>(s.x);
      k.y = static_cast<char*>(s.y);
      k.g = static_cast<const char*>(s.g);
      k.xs0 = s.x_stride[0], k.xs1 = s.x_stride[1], k.ys0 = s.y_stride[0], k.ys1 = s.y_stride[1];
      k.gs0 = bwd ? s.g_stride[0] : 0, k.gs1 = bwd ? s.g_stride[1] : 0;
      for (int t = 0; t < 2; ++t) k.dv[t] = s.dvalue[t], k.v[t] = s.value[t], k.tdiv[t] = g.tdiv[t];
      k.n = g.n, k.e1 = g.e1 ? g.e1 : 1, k.vpr = g.vpr, k.upr = g.upr ? g.upr : 1, k.su = g.su, k.rb = g.rb, k.rg = g.rg;
      k.upg = g.upg ? g.upg : 1, k.pad_ = 0;
      a->ustart[i] = (uint32_t)total;
    }
    total += g.units;
    if (total >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;
  }
  if (unit_start) unit_start[nseg] = (int64_t)total;
  if (a) {
    a->ustart[nseg] = (uint32_t)total;
    a->nseg = nseg;
  }
  return (int64_t)total;
}

template <typename C, bool CPLX, bool BWD>
void launch_mode(int mode, dim3 grid, hipStream_t stream, const ThreshArgs& a) {
  const dim3 blk(kThreads);
  switch (mode) {
    case kSoft: hipLaunchKernelGGL((thresh_kernel<C, CPLX, kSoft, BWD>), grid, blk, 0, stream, a); break;
    case kHard: hipLaunchKernelGGL((thresh_kernel<C, CPLX, kHard, BWD>), grid, blk, 0, stream, a); break;
    case kGarrote: hipLaunchKernelGGL((thresh_kernel<C, CPLX, kGarrote, BWD>), grid, blk, 0, stream, a); break;
    case kFirm: hipLaunchKernelGGL((thresh_kernel<C, CPLX, kFirm, BWD>), grid, blk, 0, stream, a); break;
    default:
      if (!CPLX) {  // (refused for complex data before any launch)
        if (mode == kGreater)
          hipLaunchKernelGGL((thresh_kernel<C, false, kGreater, BWD>), grid, blk, 0, stream, a);
        else
          hipLaunchKernelGGL((thresh_kernel<C, false, kLess, BWD>), grid, blk, 0, stream, a);
      }
  }
}

template <bool BWD>
int launch_type(int dtype, int is_complex, int mode, int64_t units, hipStream_t stream, const ThreshArgs& a) {
  const dim3 grid((unsigned)(units < kMaxGrid ? units : kMaxGrid));
  if (is_complex) {
    if constexpr (BWD) {
      return MIFWT_ERR_UNSUPPORTED;
    } else {
      if (dtype == MIFWT_F32)
        launch_mode<float, true, false>(mode, grid, stream, a);
      else
        launch_mode<double, true, false>(mode, grid, stream, a);
    }
  } else {
    switch (dtype) {
      case MIFWT_F32: launch_mode<float, false, BWD>(mode, grid, stream, a); break;
      case MIFWT_F64: launch_mode<double, false, BWD>(mode, grid, stream, a); break;
      case MIFWT_F16: launch_mode<f16_t, false, BWD>(mode, grid, stream, a); break;
      default: launch_mode<bf16_t, false, BWD>(mode, grid, stream, a); break;
    }
  }
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  count_launch(BWD ? MIFWT_KID_THRESH_BWD : MIFWT_KID_THRESH_FWD);
  return MIFWT_OK;
}

}  // namespace
}  // namespace mifwt

using namespace mifwt;

extern "C" int mifwt_thresh_max_segments(void) { return kMaxSeg; }

extern "C" int64_t mifwt_thresh_plan(int dtype, int is_complex, const mifwt_thresh_seg* segs, int nseg, int64_t* unit_start) {
  const int rc = check_call(dtype, is_complex, MIFWT_THRESH_SOFT, nseg, segs);
  if (rc != MIFWT_OK) return rc;
  return build_args(dtype, is_complex, segs, nseg, false, nullptr, unit_start);
}

extern "C" int mifwt_thresh_fwd(int dtype, int is_complex, int mode, double substitute, const mifwt_thresh_seg* segs, int nseg, void* stream) {
  const int rc = check_call(dtype, is_complex, mode, nseg, segs);
  if (rc != MIFWT_OK) return rc;
  ThreshArgs a;
  const int64_t units = build_args(dtype, is_complex, segs, nseg, false, &a, nullptr);
  if (units <= 0) return (int)units;  // an error, or nothing to do
  a.sub = substitute;
  a.part = nullptr;
  return launch_type<false>(dtype, is_complex, mode, units, static_cast<hipStream_t>(stream), a);
}

extern "C" int mifwt_thresh_bwd(int dtype, int mode, const mifwt_thresh_seg* segs, int nseg, void* workspace, size_t workspace_bytes,
                                void* stream) {
  const int rc = check_call(dtype, 0, mode, nseg, segs);
  if (rc != MIFWT_OK) return rc;
  ThreshArgs a;
  const int64_t units = build_args(dtype, 0, segs, nseg, true, &a, nullptr);
  if (units < 0) return (int)units;
  // the threshold gradients wanted: entries (segment, threshold) with a destination, grouped by destination
  RedArgs r = {};
  const bool has_vgrad = mode == kSoft || mode == kGarrote || mode == kFirm;
  for (int i = 0; i < nseg && has_vgrad; ++i) {
    for (int k = 0; k < (mode == kFirm ? 2 : 1); ++k) {
      double* dst = segs[i].gvalue[k];
      if (dst == nullptr) continue;
      const uint32_t seg_units = a.ustart[i + 1] - a.ustart[i];
      const uint32_t groups = seg_units / a.seg[i].upg;
      const uint32_t ndest = a.seg[i].tdiv[k] ? groups / a.seg[i].tdiv[k] : 1;
      int d = 0;
      while (d < r.ndst && r.dst[d] != dst) ++d;
      if (d == r.ndst) {
        r.dst[d] = dst;
        r.dst_n[d] = ndest;
        ++r.ndst;
      } else if (r.dst_n[d] != ndest) {
        return MIFWT_ERR_BADARG;  // one destination, two shapes
      }
      const int e = r.nent++;
      r.dst_of[e] = (uint8_t)d;
      r.upd[e] = seg_units / ndest;  // (0 for an empty segment: it adds nothing)
      r.part[e] = static_cast<const double*>(workspace) + (size_t)k * (size_t)units + a.ustart[i];
    }
  }
  if (r.nent > 0 && (workspace == nullptr || workspace_bytes < 2 * sizeof(double) * (size_t)units)) return MIFWT_ERR_WORKSPACE;
  a.sub = 0.0;
  a.part = r.nent > 0 ? static_cast<double*>(workspace) : nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (units > 0) {
    const int rc2 = launch_type<true>(dtype, 0, mode, units, st, a);
    if (rc2 != MIFWT_OK) return rc2;
  }
  if (r.nent > 0) {
    uint32_t blocks = 0;
    for (int d = 0; d < r.ndst; ++d) {
      r.bstart[d] = blocks;
      blocks += r.dst_n[d];
    }
    r.bstart[r.ndst] = blocks;
    if (blocks > 0) {
      hipLaunchKernelGGL(thresh_reduce_kernel, dim3(blocks), dim3(kRedThreads), 0, st, r);
      if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
    }
  }
  return MIFWT_OK;
}
