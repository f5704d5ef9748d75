// mifwt_estim.hip — noise and threshold estimators over coefficient bands (C ABI mifwt_estim_*, include/mifwt.h; kernel ids 50 .. 53).
//
// Bands, slots and keys: mifwt_bands.h (shared with mifwt_select.hip).
//
// ORDER STATISTICS of |x| per image (ids 50 / 51).  A radix selection on the keys finds the exact order statistic, the bits a sort gives.
// A count c has the ranks (c - 1) / 2 and c / 2; both are tracked in the same passes as two STATES (resolved high bits, rank among the
// keys that share them).  While the two prefixes agree one histogram serves both.
//   50  LDS-resident: one workgroup per image stages the image's keys in LDS (kLdsKeyBytes) and selects with 8-bit digits.
//   51  streaming: digit passes of 11 / 10 bits from the top (stream_plan).  A pass reads the band once; every workgroup histograms
//       its part of an image in LDS and flushes the non-zero bins with integer atomics into the image's [2][2048] counters.  The next
//       pass — every workgroup for itself — resolves the previous pass's counters into the new states; the first workgroup of an
//       image stores them (two state buffers alternate, so no workgroup reads what another one writes in the same launch).  Counters
//       are zeroed on the stream before the pass that fills them.  Integer counters only: the same input gives the same bits.
// Both end in sigma = (lo + hi) / 2 / 0.6744897501960817 in float64, rounded once to the data's type.
//
// BAND MOMENTS AND THRESHOLDS (ids 52 / 53).  52: sum of d^2 per (segment, image) for up to kMaxSeg bands in one launch, the segment
// table in the kernel arguments; products and sums in float64, per thread, then across the wave (shuffles) and the workgroup (LDS) in
// a fixed order, one plain store per unit; a second small launch sums the units of an image in order and turns sigma and the moment
// into the BayesShrink threshold sigma^2 / sqrt(max(mean(d^2) - sigma^2, eps)).  53: that second launch alone for VisuShrink,
// sigma * factor.  No float atomics anywhere.
#include "mifwt_bands.h"

namespace mifwt {
namespace {

using namespace bands;

constexpr uint32_t kMomSlots = kThreads * 8;     // moments: slots per unit at least
constexpr uint32_t kMaxParts = 256;              // moments: units per image at most
constexpr int kMaxGrid = 8192;
constexpr double kMadScale = 0.6744897501960817;

template <typename K>
struct SelState {
  K pref[2];         // resolved high bits of the key of rank (c - 1) / 2 and of rank c / 2
  uint32_t rank[2];  // their ranks among the keys that share those bits
};

// Inclusive scan of two values per thread over the workgroup (kThreads threads); every thread calls it.
__device__ __forceinline__ void block_scan2(uint32_t& v0, uint32_t& v1, uint32_t (*wsum)[kThreads / 64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t0 = __shfl_up(v0, o, 64), t1 = __shfl_up(v1, o, 64);
    if (lane >= o) v0 += t0, v1 += t1;
  }
  __syncthreads();  // (the sums of an earlier scan have been read)
  if (lane == 63) wsum[0][wave] = v0, wsum[1][wave] = v1;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v0 += wsum[0][w], v1 += wsum[1][w];
}

// sigma from the two order statistics, float64, rounded once
template <typename C>
__device__ __forceinline__ void write_sigma(const typename KeyOf<C>::type* pref, uint32_t g, C* stats, C* sigma, double* sigma64) {
  const C lo = __builtin_bit_cast(C, pref[0]), hi = __builtin_bit_cast(C, pref[1]);
  if (stats) stats[2 * (size_t)g] = lo, stats[2 * (size_t)g + 1] = hi;
  const C s = (C)((((double)lo + (double)hi) * 0.5) / kMadScale);
  if (sigma) sigma[g] = s;
  if (sigma64) sigma64[g] = (double)s;
}

// ---- 50: the image's keys in LDS ---------------------------------------------------------------------------------------------------
template <typename C>
__global__ __launch_bounds__(kThreads) void select_lds_kernel(const Band b, const uint32_t cnt, C* stats, C* sigma, double* sigma64) {
  typedef typename KeyOf<C>::type K;
  constexpr int W = 8 * sizeof(K);
  __shared__ K keys[kLdsKeyBytes / sizeof(K)];
  __shared__ uint32_t hist[2][kLdsBins];
  __shared__ uint32_t wsum[2][kThreads / 64];
  __shared__ SelState<K> st;
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  const uint32_t slots = b.rp * b.vpr;
  for (uint32_t t = tid; t < slots; t += kThreads) {
    const uint32_t r = t / b.vpr, sl = t - r * b.vpr;
    visit_slot<C>(b, g * b.rp + r, sl, [&](uint32_t c, C v) { keys[r * b.n + c] = key_of(v); });
  }
  if (tid == 0) {
    st.pref[0] = st.pref[1] = 0;
    st.rank[0] = (cnt - 1) / 2;
    st.rank[1] = cnt / 2;
  }
  for (int shift = W - 8; shift >= 0; shift -= 8) {
    for (uint32_t i = tid; i < 2 * kLdsBins; i += kThreads) (&hist[0][0])[i] = 0;
    __syncthreads();  // (also: the keys and the state are written)
    const K p0 = st.pref[0], p1 = st.pref[1];
    const uint32_t r0 = st.rank[0], r1 = st.rank[1];
    const bool same = p0 == p1;
    const K himask = shift + 8 >= W ? K(0) : ~K(0) << (shift + 8);
    for (uint32_t i = tid; i < cnt; i += kThreads) {
      const K k = keys[i], h = k & himask;
      const uint32_t d = (uint32_t)(k >> shift) & (kLdsBins - 1);
      if (h == p0) atomicAdd(&hist[0][d], 1u);
      if (!same && h == p1) atomicAdd(&hist[1][d], 1u);
    }
    __syncthreads();
    const uint32_t c0 = hist[0][tid], c1 = same ? c0 : hist[1][tid];
    uint32_t i0 = c0, i1 = c1;
    block_scan2(i0, i1, wsum);
    if (i0 - c0 <= r0 && r0 < i0) st.pref[0] = p0 | ((K)tid << shift), st.rank[0] = r0 - (i0 - c0);
    if (i1 - c1 <= r1 && r1 < i1) st.pref[1] = p1 | ((K)tid << shift), st.rank[1] = r1 - (i1 - c1);
    __syncthreads();
  }
  if (tid == 0) write_sigma<C>(st.pref, g, stats, sigma, sigma64);
}

// ---- 51: streaming digit passes ----------------------------------------------------------------------------------------------------
// The states after the pass whose counters are `counts` ([2][kStreamBins] of this image), from the states `in` before it.  Every thread of
// the workgroup calls it; the result is in *out (LDS) after the final barrier.
template <typename K>
__device__ __forceinline__ void resolve(const SelState<K>& in, const uint32_t* counts, int shift, SelState<K>* out,
                                        uint32_t (*wsum)[kThreads / 64]) {
  constexpr int PER = kStreamBins / kThreads;
  const bool same = in.pref[0] == in.pref[1];
  const uint32_t* h0 = counts + threadIdx.x * PER;
  const uint32_t* h1 = same ? h0 : h0 + kStreamBins;
  uint32_t a0[PER], a1[PER], t0 = 0, t1 = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    a0[j] = h0[j], a1[j] = h1[j];
    t0 += a0[j], t1 += a1[j];
  }
  uint32_t i0 = t0, i1 = t1;
  block_scan2(i0, i1, wsum);
  uint32_t e0 = i0 - t0, e1 = i1 - t1;  // keys in the bins before this thread's
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (e0 <= in.rank[0] && in.rank[0] < e0 + a0[j]) {
      out->pref[0] = in.pref[0] | ((K)(threadIdx.x * PER + j) << shift);
      out->rank[0] = in.rank[0] - e0;
    }
    if (e1 <= in.rank[1] && in.rank[1] < e1 + a1[j]) {
      out->pref[1] = in.pref[1] | ((K)(threadIdx.x * PER + j) << shift);
      out->rank[1] = in.rank[1] - e1;
    }
    e0 += a0[j], e1 += a1[j];
  }
  __syncthreads();
}

template <typename K>
__device__ __forceinline__ SelState<K> first_state(uint32_t cnt) {
  SelState<K> s;
  s.pref[0] = s.pref[1] = 0;
  s.rank[0] = (cnt - 1) / 2;
  s.rank[1] = cnt / 2;
  return s;
}

// Pass `pass` of the selection: grid = images x wgs workgroups.  prev: the counters of pass - 1, counts: this pass's (zeroed), states:
// [2][images], buffer (q & 1) holding the states before pass q for q >= 1.
template <typename C>
__global__ __launch_bounds__(kThreads) void select_stream_kernel(const Band b, const uint32_t cnt, const int pass, const uint32_t wgs,
                                                                 const uint32_t spw, const uint32_t images, const uint32_t* prev,
                                                                 uint32_t* counts, SelState<typename KeyOf<C>::type>* states) {
  typedef typename KeyOf<C>::type K;
  constexpr int T = KeyOf<C>::bits;
  __shared__ uint32_t hist[2][kStreamBins];
  __shared__ uint32_t wsum[2][kThreads / 64];
  __shared__ SelState<K> st;
  const uint32_t g = blockIdx.x / wgs, w = blockIdx.x - g * wgs, tid = threadIdx.x;
  for (uint32_t i = tid; i < 2 * kStreamBins; i += kThreads) (&hist[0][0])[i] = 0;
  int shift, width;
  if (pass == 0) {
    if (tid == 0) st = first_state<K>(cnt);
    __syncthreads();
  } else {
    const SelState<K> in = pass == 1 ? first_state<K>(cnt) : states[(size_t)((pass - 1) & 1) * images + g];
    stream_plan(T, pass - 1, &shift, &width);
    resolve<K>(in, prev + (size_t)g * 2 * kStreamBins, shift, &st, wsum);
    if (w == 0 && tid == 0) states[(size_t)(pass & 1) * images + g] = st;
  }
  stream_plan(T, pass, &shift, &width);
  const K p0 = st.pref[0], p1 = st.pref[1];
  const bool same = p0 == p1;
  const K himask = shift + width >= 8 * (int)sizeof(K) ? K(0) : ~K(0) << (shift + width);
  const uint32_t dmask = (1u << width) - 1u;
  const uint32_t slots = b.rp * b.vpr;
  const uint32_t t0 = w * spw, t1 = min(slots, t0 + spw);
  for (uint32_t t = t0 + tid; t < t1; t += kThreads) {
    const uint32_t r = t / b.vpr, sl = t - r * b.vpr;
    visit_slot<C>(b, g * b.rp + r, sl, [&](uint32_t, C v) {
      const K k = key_of(v), h = k & himask;
      const uint32_t d = (uint32_t)(k >> shift) & dmask;
      if (h == p0) atomicAdd(&hist[0][d], 1u);
      if (!same && h == p1) atomicAdd(&hist[1][d], 1u);
    });
  }
  __syncthreads();
  uint32_t* dst = counts + (size_t)g * 2 * kStreamBins;
  for (uint32_t i = tid; i < (same ? 1u : 2u) * kStreamBins; i += kThreads) {
    const uint32_t c = (&hist[0][0])[i];
    if (c) atomicAdd(&dst[i], c);
  }
}

// after the last pass: resolve its counters, write sigma.  One workgroup per image.
template <typename C>
__global__ __launch_bounds__(kThreads) void select_stream_finish_kernel(const uint32_t cnt, const uint32_t images, const uint32_t* prev,
                                                                        const SelState<typename KeyOf<C>::type>* states, C* stats, C* sigma,
                                                                        double* sigma64) {
  typedef typename KeyOf<C>::type K;
  constexpr int T = KeyOf<C>::bits;
  __shared__ uint32_t wsum[2][kThreads / 64];
  __shared__ SelState<K> st;
  const uint32_t g = blockIdx.x;
  const int last = stream_passes(T) - 1;
  const SelState<K> in = last == 0 ? first_state<K>(cnt) : states[(size_t)(last & 1) * images + g];
  int shift, width;
  stream_plan(T, last, &shift, &width);
  resolve<K>(in, prev + (size_t)g * 2 * kStreamBins, shift, &st, wsum);
  if (threadIdx.x == 0) write_sigma<C>(st.pref, g, stats, sigma, sigma64);
}

// ---- 52 / 53: band moments and thresholds ---------------------------------------------------------------------------------------------
struct MSeg {
  Band b;
  uint32_t slots;  // slots per image
  uint32_t ppi;    // units (parts) per image
  uint32_t spp;    // slots per part
  uint32_t pad_;
  double count;    // elements per image
};

struct MomArgs {
  MSeg seg[kMaxSeg];
  uint32_t ustart[kMaxSeg + 1];
  int nseg;
  uint32_t images;
  double* part;  // [units]
};
static_assert(sizeof(MomArgs) <= 4096, "the segment table must fit the kernel-argument segment");

template <typename C>
__global__ __launch_bounds__(kThreads) void moments_kernel(const MomArgs a) {
  __shared__ double red[kThreads / 64];
  const uint32_t total = a.ustart[a.nseg];
  for (uint32_t u = blockIdx.x; u < total; u += gridDim.x) {
    int si = 0;
    while (si + 1 < a.nseg && u >= a.ustart[si + 1]) ++si;
    const MSeg& s = a.seg[si];
    const uint32_t lu = u - a.ustart[si];
    const uint32_t g = lu / s.ppi, part = lu - g * s.ppi;
    const uint32_t t0 = part * s.spp, t1 = min(s.slots, t0 + s.spp);
    double acc = 0.0;
    for (uint32_t t = t0 + threadIdx.x; t < t1; t += kThreads) {
      const uint32_t r = t / s.b.vpr, sl = t - r * s.b.vpr;
      visit_slot<C>(s.b, g * s.b.rp + r, sl, [&](uint32_t, C v) { acc += (double)v * (double)v; });
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int w = 0; w < kThreads / 64; ++w) t += red[w];
      a.part[u] = t;
    }
    __syncthreads();
  }
}

struct ThrArgs {
  uint32_t ustart[kMaxSeg];
  uint32_t ppi[kMaxSeg];
  double count[kMaxSeg];
  int nseg;
  uint32_t images;
  int method;
  double factor, eps;
  const double* part;
  const double* sigma64;
  void* thr;
  double* thr64;
  double* moments;
};

// one thread per (segment, image): the units of the image in order, then the threshold
template <typename C>
__global__ __launch_bounds__(kThreads) void thresholds_kernel(const ThrArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (uint64_t)a.nseg * a.images) return;
  const uint32_t si = (uint32_t)(i / a.images), g = (uint32_t)(i - (uint64_t)si * a.images);
  const double sg = a.sigma64[g];
  double t;
  if (a.method == MIFWT_ESTIM_VISU) {
    t = sg * a.factor;
  } else {
    const double* p = a.part + a.ustart[si] + (size_t)g * a.ppi[si];
    double sum = 0.0;
    for (uint32_t k = 0; k < a.ppi[si]; ++k) sum += p[k];
    if (a.moments) a.moments[i] = sum;
    const double s2 = sg * sg, excess = sum / a.count[si] - s2;
    t = s2 / __builtin_sqrt(excess > a.eps ? excess : a.eps);
  }
  const C tc = (C)t;
  if (a.thr) static_cast<C*>(a.thr)[i] = tc;
  if (a.thr64) a.thr64[i] = (double)tc;
}

// ---- host (band_geometry, lds_capacity: mifwt_bands.h) --------------------------------------------------------------------------------
struct StreamShape {
  uint32_t wgs, spw;
};
StreamShape stream_shape(const Geo& g) {
  const uint64_t slots = (uint64_t)g.b.rp * g.b.vpr;
  uint64_t per_image = kMaxWgs / g.images;
  if (per_image < 1) per_image = 1;
  uint64_t wgs = (slots + kSlotsPerWg - 1) / kSlotsPerWg;
  if (wgs > per_image) wgs = per_image;
  if (wgs < 1) wgs = 1;
  const uint64_t spw = (slots + wgs - 1) / wgs;
  wgs = (slots + spw - 1) / spw;
  return StreamShape{(uint32_t)wgs, (uint32_t)spw};
}

size_t stream_ws_bytes(int dtype, const Geo& g) {
  const size_t counters = 2 * (size_t)g.images * 2 * kStreamBins * sizeof(uint32_t);
  const size_t states = 2 * (size_t)g.images * (dtype == MIFWT_F64 ? sizeof(SelState<uint64_t>) : sizeof(SelState<uint32_t>));
  return counters + states;
}

template <typename C>
int run_select(const Geo& g, int route, void* stats, void* sigma, double* sigma64, void* ws, hipStream_t st) {
  typedef typename KeyOf<C>::type K;
  const uint32_t cnt = (uint32_t)g.count, images = (uint32_t)g.images;
  if (route == MIFWT_KID_ESTIM_SELECT_LDS) {
    hipLaunchKernelGGL(select_lds_kernel<C>, dim3(images), dim3(kThreads), 0, st, g.b, cnt, static_cast<C*>(stats), static_cast<C*>(sigma),
                       sigma64);
    if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
    return MIFWT_OK;
  }
  const StreamShape sh = stream_shape(g);
  if ((uint64_t)sh.wgs * images >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;
  const size_t one = (size_t)images * 2 * kStreamBins;  // counters of one pass
  uint32_t* counters = static_cast<uint32_t*>(ws);
  SelState<K>* states = reinterpret_cast<SelState<K>*>(counters + 2 * one);
  const int passes = stream_passes(KeyOf<C>::bits);
  for (int p = 0; p < passes; ++p) {
    uint32_t* cur = counters + (size_t)(p & 1) * one;
    const uint32_t* prev = counters + (size_t)((p + 1) & 1) * one;
    if (hipMemsetAsync(cur, 0, one * sizeof(uint32_t), st) != hipSuccess) return MIFWT_ERR_LAUNCH;
    hipLaunchKernelGGL(select_stream_kernel<C>, dim3(sh.wgs * images), dim3(kThreads), 0, st, g.b, cnt, p, sh.wgs, sh.spw, images, prev, cur,
                       states);
    if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(select_stream_finish_kernel<C>, dim3(images), dim3(kThreads), 0, st, cnt, images,
                     counters + (size_t)((passes - 1) & 1) * one, states, static_cast<C*>(stats), static_cast<C*>(sigma), sigma64);
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  return MIFWT_OK;
}

}  // namespace
}  // namespace mifwt

using namespace mifwt;

extern "C" int mifwt_estim_max_segments(void) { return kMaxSeg; }

extern "C" int mifwt_estim_lds_capacity(int dtype) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return MIFWT_ERR_BADARG;
  return lds_capacity(dtype);
}

extern "C" int mifwt_estim_stream_plan(int dtype, int pass, int* shift, int* width) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return MIFWT_ERR_BADARG;
  const int bits = dtype == MIFWT_F64 ? 63 : 31;
  if (pass >= 0 && pass < stream_passes(bits) && shift && width) stream_plan(bits, pass, shift, width);
  return stream_passes(bits);
}

extern "C" int mifwt_estim_select_route(int dtype, const mifwt_estim_band* band, int force_stream) {
  if (band == nullptr) return MIFWT_ERR_BADARG;
  Geo g;
  const int rc = band_geometry(dtype, *band, &g);
  if (rc != MIFWT_OK) return rc;
  if (g.count == 0) return 0;
  return !force_stream && g.count <= (uint64_t)lds_capacity(dtype) ? MIFWT_KID_ESTIM_SELECT_LDS : MIFWT_KID_ESTIM_SELECT_STREAM;
}

extern "C" size_t mifwt_estim_select_workspace(int dtype, const mifwt_estim_band* band, int route) {
  Geo g;
  if (band == nullptr || band_geometry(dtype, *band, &g) != MIFWT_OK || g.count == 0) return 0;
  return route == MIFWT_KID_ESTIM_SELECT_STREAM ? stream_ws_bytes(dtype, g) : 0;
}

extern "C" int mifwt_estim_sigma(int dtype, const mifwt_estim_band* band, int route, void* order_stats, void* sigma, double* sigma64,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (band == nullptr) return MIFWT_ERR_BADARG;
  if (route != MIFWT_KID_ESTIM_SELECT_LDS && route != MIFWT_KID_ESTIM_SELECT_STREAM) return MIFWT_ERR_BADARG;
  Geo g;
  const int rc = band_geometry(dtype, *band, &g);
  if (rc != MIFWT_OK) return rc;
  if (g.count == 0) return MIFWT_OK;  // nothing to select from
  if (band->x == nullptr) return MIFWT_ERR_BADARG;
  if (route == MIFWT_KID_ESTIM_SELECT_LDS && g.count > (uint64_t)lds_capacity(dtype)) return MIFWT_ERR_UNSUPPORTED;
  if (route == MIFWT_KID_ESTIM_SELECT_STREAM && (workspace == nullptr || workspace_bytes < stream_ws_bytes(dtype, g)))
    return MIFWT_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc2 = dtype == MIFWT_F64 ? run_select<double>(g, route, order_stats, sigma, sigma64, workspace, st)
                                     : run_select<float>(g, route, order_stats, sigma, sigma64, workspace, st);
  return rc2;
}

namespace {
// fills the table; returns the number of units or an error code
int64_t build_moments(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, MomArgs* a) {
  if (segs == nullptr || nseg < 1 || nseg > kMaxSeg || images < 0 || images >= 2147483648ll) return MIFWT_ERR_BADARG;
  uint64_t total = 0;
  for (int i = 0; i < nseg; ++i) {
    Geo g;
    const int rc = band_geometry(dtype, segs[i], &g);
    if (rc != MIFWT_OK) return rc;
    if (g.count == 0 || g.images != (uint64_t)images) return MIFWT_ERR_BADARG;  // (empty bands are the caller's)
    const uint64_t slots = (uint64_t)g.b.rp * g.b.vpr;
    uint64_t ppi = (slots + kMomSlots - 1) / kMomSlots;
    if (ppi > kMaxParts) ppi = kMaxParts;
    const uint64_t spp = (slots + ppi - 1) / ppi;
    ppi = (slots + spp - 1) / spp;
    if (a) {
      MSeg& m = a->seg[i];
      m.b = g.b;
      m.slots = (uint32_t)slots, m.ppi = (uint32_t)ppi, m.spp = (uint32_t)spp, m.pad_ = 0;
      m.count = (double)g.count;
      a->ustart[i] = (uint32_t)total;
    }
    total += ppi * g.images;
    if (total >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;
  }
  if (a) {
    a->ustart[nseg] = (uint32_t)total;
    a->nseg = nseg;
    a->images = (uint32_t)images;
  }
  return (int64_t)total;
}
}  // namespace

extern "C" int64_t mifwt_estim_moments_plan(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images) {
  return build_moments(dtype, segs, nseg, images, nullptr);
}

extern "C" int mifwt_estim_thresholds(int dtype, int method, const mifwt_estim_band* segs, int nseg, int64_t images, const double* sigma64,
                                      double factor, void* thr, double* thr64, double* moments, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return MIFWT_ERR_BADARG;
  if (method != MIFWT_ESTIM_VISU && method != MIFWT_ESTIM_BAYES) return MIFWT_ERR_BADARG;
  if (nseg < 1 || nseg > kMaxSeg || images < 0 || images >= 2147483648ll) return MIFWT_ERR_BADARG;
  if (images == 0) return MIFWT_OK;
  if (sigma64 == nullptr) return MIFWT_ERR_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ThrArgs t = {};
  t.nseg = nseg, t.images = (uint32_t)images, t.method = method, t.factor = factor;
  t.eps = dtype == MIFWT_F64 ? 2.220446049250313e-16 : 1.1920928955078125e-07;
  t.sigma64 = sigma64, t.thr = thr, t.thr64 = thr64, t.moments = moments;
  if (method == MIFWT_ESTIM_BAYES) {
    MomArgs a;
    const int64_t units = build_moments(dtype, segs, nseg, images, &a);
    if (units < 0) return (int)units;
    for (int i = 0; i < nseg; ++i)
      if (segs[i].x == nullptr) return MIFWT_ERR_BADARG;
    if (workspace == nullptr || workspace_bytes < sizeof(double) * (size_t)units) return MIFWT_ERR_WORKSPACE;
    a.part = static_cast<double*>(workspace);
    const dim3 grid((unsigned)(units < kMaxGrid ? units : kMaxGrid));
    if (dtype == MIFWT_F64)
      hipLaunchKernelGGL(moments_kernel<double>, grid, dim3(kThreads), 0, st, a);
    else
      hipLaunchKernelGGL(moments_kernel<float>, grid, dim3(kThreads), 0, st, a);
    if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
    for (int i = 0; i < nseg; ++i) t.ustart[i] = a.ustart[i], t.ppi[i] = a.seg[i].ppi, t.count[i] = a.seg[i].count;
    t.part = a.part;
  }
  const uint64_t n = (uint64_t)nseg * (uint64_t)images;
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
  if (dtype == MIFWT_F64)
    hipLaunchKernelGGL(thresholds_kernel<double>, grid, dim3(kThreads), 0, st, t);
  else
    hipLaunchKernelGGL(thresholds_kernel<float>, grid, dim3(kThreads), 0, st, t);
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  return MIFWT_OK;
}
