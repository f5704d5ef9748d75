// mifwt_select.hip — the k-th largest magnitude of a coefficient container, pooled per image (C ABI mifwt_select_*, include/mifwt.h;
// kernel ids 54 / 55).  Bands, slots and keys: mifwt_bands.h.
//
// All SEGMENTS (bands) of a container that share their images form, per image, ONE multiset of keys with n elements.  The k-th largest
// is the key of ascending rank n - k; it is found by a radix selection with ONE state per image: the resolved high bits `pref` and the
// rank among the keys that share them.  A digit pass counts, per value of the next digit, the keys whose resolved bits equal `pref`; the
// bin b with  below(b) <= rank < below(b) + count(b)  is the digit, and the rank drops by below(b), the keys in the bins under it.
// k is a number or comes from device memory (one per image, clipped to [0, n] where it is read); k = 0 selects nothing and gives +inf
// (the passes then run for k = 1 and the last kernel discards their result).
//   54  LDS-resident: one workgroup per image stages the keys of all segments in LDS (kLdsKeyBytes) and selects with 8-bit digits.
//   55  streaming: digit passes of 11 / 10 bits from the top (stream_plan).  The segment table travels in the kernel arguments; a unit
//       table maps a workgroup to (segment, image, chunk of slots).  Every workgroup histograms its chunk in LDS and flushes the non-zero
//       bins with integer atomics into the image's [2048] counters.  The next pass — every workgroup for itself — resolves the previous
//       pass's counters into the new state; the first workgroup of an image stores it (two state buffers alternate, so no workgroup
//       reads what another one writes in the same launch).  Counters are zeroed on the stream before the pass that fills them.  A
//       container of more than kMaxSeg segments runs several launches of the same pass into the same counters.  A finish launch, one
//       workgroup per image, resolves the last pass and writes the value.  Integer counters only: the same input gives the same bits.
#include <vector>

#include "mifwt_bands.h"

namespace mifwt {
namespace {

using namespace bands;

template <typename K>
struct KthState {
  K pref;         // resolved high bits of the key of ascending rank n - k
  uint32_t rank;  // its rank among the keys that share those bits
};

template <typename K>
__device__ __forceinline__ KthState<K> first_state(const KSource& s, uint32_t g, uint32_t n) {
  const uint32_t k = k_of(s, g, n);
  KthState<K> st;
  st.pref = 0;
  st.rank = n - (k ? k : 1u);
  return st;
}

// Inclusive scan of one value per thread over the workgroup (kThreads threads); every thread calls it.
__device__ __forceinline__ void block_scan(uint32_t& v, uint32_t* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  __syncthreads();  // (the sums of an earlier scan have been read)
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += wsum[w];
}

template <typename C>
__device__ __forceinline__ void write_value(typename KeyOf<C>::type key, bool none, uint32_t g, C* value, double* value64) {
  const C v = none ? (C)__builtin_huge_val() : __builtin_bit_cast(C, key);
  if (value) value[g] = v;
  if (value64) value64[g] = (double)v;
}

struct KSeg {
  Band b;
  uint32_t slots;  // slots per image
  uint32_t wpi;    // 55: units (chunks) per image
  uint32_t spw;    // 55: slots per unit
  uint32_t kbase;  // 54: where the segment's keys start in the image's LDS array
};

struct KthArgs {
  KSeg seg[kMaxSeg];
  uint32_t ustart[kMaxSeg + 1];  // 55: first unit of a segment
  int nseg;
  uint32_t images;
  uint32_t count;  // n: pooled elements per image, over every launch of the pass
  int pass;
  KSource src;
  const uint32_t* prev;  // 55: the counters of pass - 1, [images][kStreamBins]
  uint32_t* counts;      // 55: this pass's
  void* states;          // 55: [2][images], buffer (q & 1) holding the states before pass q for q >= 1
  void* value;           // 54
  double* value64;       // 54
};
static_assert(sizeof(KthArgs) <= 4096, "the segment table must fit the kernel-argument segment");

// ---- 54: the image's keys in LDS ---------------------------------------------------------------------------------------------------
template <typename C>
__global__ __launch_bounds__(kThreads) void kth_lds_kernel(const KthArgs a) {
  typedef typename KeyOf<C>::type K;
  constexpr int W = 8 * sizeof(K);
  static_assert(kLdsBins == kThreads, "one bin per thread");
  __shared__ K keys[kLdsKeyBytes / sizeof(K)];
  __shared__ uint32_t hist[kLdsBins];
  __shared__ uint32_t wsum[kThreads / 64];
  __shared__ KthState<K> st;
  const uint32_t g = blockIdx.x, tid = threadIdx.x, cnt = a.count;
  for (int si = 0; si < a.nseg; ++si) {
    const KSeg& s = a.seg[si];
    for (uint32_t t = tid; t < s.slots; t += kThreads) {
      const uint32_t r = t / s.b.vpr, sl = t - r * s.b.vpr;
      visit_slot<C>(s.b, g * s.b.rp + r, sl, [&](uint32_t c, C v) { keys[s.kbase + r * s.b.n + c] = key_of(v); });
    }
  }
  if (tid == 0) st = first_state<K>(a.src, g, cnt);
  for (int shift = W - 8; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();  // (also: the keys and the state are written)
    const K p = st.pref;
    const uint32_t r = st.rank;
    const K himask = shift + 8 >= W ? K(0) : ~K(0) << (shift + 8);
    for (uint32_t i = tid; i < cnt; i += kThreads) {
      const K k = keys[i];
      if ((k & himask) == p) atomicAdd(&hist[(uint32_t)(k >> shift) & (kLdsBins - 1)], 1u);
    }
    __syncthreads();
    const uint32_t c = hist[tid];
    uint32_t incl = c;
    block_scan(incl, wsum);
    if (incl - c <= r && r < incl) st.pref = p | ((K)tid << shift), st.rank = r - (incl - c);
    __syncthreads();
  }
  if (tid == 0) write_value<C>(st.pref, k_of(a.src, g, cnt) == 0, g, static_cast<C*>(a.value), a.value64);
}

// ---- 55: streaming digit passes ----------------------------------------------------------------------------------------------------
// The state after the pass whose counters are `counts` ([kStreamBins] of this image), from the state `in` before it.  Every thread of the
// workgroup calls it; the result is in *out (LDS) after the final barrier.
template <typename K>
__device__ __forceinline__ void resolve(const KthState<K>& in, const uint32_t* counts, int shift, KthState<K>* out, uint32_t* wsum) {
  constexpr int PER = kStreamBins / kThreads;
  const uint32_t* h = counts + threadIdx.x * PER;
  uint32_t a[PER], t = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    a[j] = h[j];
    t += a[j];
  }
  uint32_t incl = t;
  block_scan(incl, wsum);
  uint32_t below = incl - t;  // keys in the bins before this thread's
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (below <= in.rank && in.rank < below + a[j]) {
      out->pref = in.pref | ((K)(threadIdx.x * PER + j) << shift);
      out->rank = in.rank - below;
    }
    below += a[j];
  }
  __syncthreads();
}

// Pass a.pass of the selection over the segments of `a`: one workgroup per unit.
template <typename C>
__global__ __launch_bounds__(kThreads) void kth_stream_kernel(const KthArgs a) {
  typedef typename KeyOf<C>::type K;
  constexpr int T = KeyOf<C>::bits;
  __shared__ uint32_t hist[kStreamBins];
  __shared__ uint32_t wsum[kThreads / 64];
  __shared__ KthState<K> st;
  const uint32_t u = blockIdx.x, tid = threadIdx.x;
  int si = 0;
  while (si + 1 < a.nseg && u >= a.ustart[si + 1]) ++si;
  const KSeg& s = a.seg[si];
  const uint32_t lu = u - a.ustart[si];
  const uint32_t g = lu / s.wpi, w = lu - g * s.wpi;
  KthState<K>* states = static_cast<KthState<K>*>(a.states);
  for (uint32_t i = tid; i < (uint32_t)kStreamBins; i += kThreads) hist[i] = 0;
  int shift, width;
  if (a.pass == 0) {
    if (tid == 0) st = first_state<K>(a.src, g, a.count);
    __syncthreads();
  } else {
    const KthState<K> in = a.pass == 1 ? first_state<K>(a.src, g, a.count) : states[(size_t)((a.pass - 1) & 1) * a.images + g];
    stream_plan(T, a.pass - 1, &shift, &width);
    resolve<K>(in, a.prev + (size_t)g * kStreamBins, shift, &st, wsum);
    if (si == 0 && w == 0 && tid == 0) states[(size_t)(a.pass & 1) * a.images + g] = st;  // (every launch of the pass: the same value)
  }
  stream_plan(T, a.pass, &shift, &width);
  const K p = st.pref;
  const K himask = shift + width >= 8 * (int)sizeof(K) ? K(0) : ~K(0) << (shift + width);
  const uint32_t dmask = (1u << width) - 1u;
  const uint32_t t0 = w * s.spw, t1 = min(s.slots, t0 + s.spw);
  for (uint32_t t = t0 + tid; t < t1; t += kThreads) {
    const uint32_t r = t / s.b.vpr, sl = t - r * s.b.vpr;
    visit_slot<C>(s.b, g * s.b.rp + r, sl, [&](uint32_t, C v) {
      const K k = key_of(v);
      if ((k & himask) == p) atomicAdd(&hist[(uint32_t)(k >> shift) & dmask], 1u);
    });
  }
  __syncthreads();
  uint32_t* dst = a.counts + (size_t)g * kStreamBins;
  for (uint32_t i = tid; i < (uint32_t)kStreamBins; i += kThreads) {
    const uint32_t c = hist[i];
    if (c) atomicAdd(&dst[i], c);
  }
}

// the counters of a pass, zeroed on the stream before the launches that fill them
__global__ __launch_bounds__(kThreads) void zero_counters_kernel(uint32_t* counts, const size_t n) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) counts[i] = 0;
}

// after the last pass: resolve its counters, write the value.  One workgroup per image.
template <typename C>
__global__ __launch_bounds__(kThreads) void kth_stream_finish_kernel(const uint32_t cnt, const uint32_t images, const KSource src,
                                                                     const uint32_t* prev, const KthState<typename KeyOf<C>::type>* states,
                                                                     C* value, double* value64) {
  typedef typename KeyOf<C>::type K;
  constexpr int T = KeyOf<C>::bits;
  __shared__ uint32_t wsum[kThreads / 64];
  __shared__ KthState<K> st;
  const uint32_t g = blockIdx.x;
  const int last = stream_passes(T) - 1;
  const KthState<K> in = last == 0 ? first_state<K>(src, g, cnt) : states[(size_t)(last & 1) * images + g];
  int shift, width;
  stream_plan(T, last, &shift, &width);
  resolve<K>(in, prev + (size_t)g * kStreamBins, shift, &st, wsum);
  if (threadIdx.x == 0) write_value<C>(st.pref, k_of(src, g, cnt) == 0, g, value, value64);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
size_t state_bytes(int dtype) { return dtype == MIFWT_F64 ? sizeof(KthState<uint64_t>) : sizeof(KthState<uint32_t>); }

size_t stream_ws_bytes(int dtype, uint64_t images) {
  return 2 * (size_t)images * kStreamBins * sizeof(uint32_t) + 2 * (size_t)images * state_bytes(dtype);
}

// the unit table of the segments [c0, c0 + n) of the pool; the number of units
uint64_t fill_units(const Pool& p, size_t c0, int n, uint64_t images, KthArgs* a) {
  uint64_t total = 0;
  for (int i = 0; i < n; ++i) {
    uint64_t slots, wpi, spw;
    unit_plan(p.segs[c0 + i], images, &slots, &wpi, &spw);
    const Geo& g = p.segs[c0 + i];
    KSeg& s = a->seg[i];
    s.b = g.b;
    s.slots = (uint32_t)slots, s.wpi = (uint32_t)wpi, s.spw = (uint32_t)spw, s.kbase = 0;
    a->ustart[i] = (uint32_t)total;
    total += wpi * images;
    if (total >= 2147483648ull) return total;
  }
  a->ustart[n] = (uint32_t)total;
  a->nseg = n;
  return total;
}

template <typename C>
int run_kth(const Pool& p, uint64_t images, const KSource& src, int route, void* value, double* value64, void* ws, hipStream_t st) {
  typedef typename KeyOf<C>::type K;
  KthArgs a = {};
  a.images = (uint32_t)images, a.count = (uint32_t)p.count, a.src = src;
  if (route == MIFWT_KID_SELECT_KTH_LDS) {
    uint32_t base = 0;
    a.nseg = (int)p.segs.size();
    for (int i = 0; i < a.nseg; ++i) {
      const Geo& g = p.segs[i];
      a.seg[i].b = g.b;
      a.seg[i].slots = g.b.rp * g.b.vpr;
      a.seg[i].kbase = base;
      base += (uint32_t)g.count;
    }
    a.value = value, a.value64 = value64;
    hipLaunchKernelGGL(kth_lds_kernel<C>, dim3(a.images), dim3(kThreads), 0, st, a);
    return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
  }
  const size_t one = (size_t)images * kStreamBins;  // counters of one pass
  uint32_t* counters = static_cast<uint32_t*>(ws);
  a.states = counters + 2 * one;
  const int passes = stream_passes(KeyOf<C>::bits);
  for (size_t c0 = 0; c0 < p.segs.size(); c0 += kMaxSeg)  // (before anything is enqueued)
    if (fill_units(p, c0, (int)std::min<size_t>(kMaxSeg, p.segs.size() - c0), images, &a) >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;
  for (int pass = 0; pass < passes; ++pass) {
    a.pass = pass;
    a.counts = counters + (size_t)(pass & 1) * one;
    a.prev = counters + (size_t)((pass + 1) & 1) * one;
    // (a kernel, not a memset: in a replayed HIP graph the counters must be zeroed strictly between the launches that read and fill them,
    // and kernel launches of one stream keep that order among themselves)
    hipLaunchKernelGGL(zero_counters_kernel, dim3((unsigned)std::min<size_t>((one + kThreads - 1) / kThreads, kMaxWgs)), dim3(kThreads), 0, st, a.counts, one);
    if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
    for (size_t c0 = 0; c0 < p.segs.size(); c0 += kMaxSeg) {
      const uint64_t units = fill_units(p, c0, (int)std::min<size_t>(kMaxSeg, p.segs.size() - c0), images, &a);
      hipLaunchKernelGGL(kth_stream_kernel<C>, dim3((unsigned)units), dim3(kThreads), 0, st, a);
      if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(kth_stream_finish_kernel<C>, dim3(a.images), dim3(kThreads), 0, st, a.count, a.images, src,
                     counters + (size_t)((passes - 1) & 1) * one, static_cast<const KthState<K>*>(a.states), static_cast<C*>(value), value64);
  return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
}

}  // namespace
}  // namespace mifwt

using namespace mifwt;

extern "C" int mifwt_select_max_segments(void) { return kMaxSeg; }

extern "C" int mifwt_select_route(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int force_stream) {
  Pool p;
  const int rc = pool_of(dtype, segs, nseg, images, &p);
  if (rc != MIFWT_OK) return rc;
  if (p.count == 0 || images == 0) return 0;
  const bool lds = !force_stream && p.segs.size() <= (size_t)kMaxSeg && p.count <= (uint64_t)lds_capacity(dtype);
  return lds ? MIFWT_KID_SELECT_KTH_LDS : MIFWT_KID_SELECT_KTH_STREAM;
}

extern "C" size_t mifwt_select_workspace(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int route) {
  Pool p;
  if (pool_of(dtype, segs, nseg, images, &p) != MIFWT_OK || p.count == 0 || images == 0) return 0;
  return route == MIFWT_KID_SELECT_KTH_STREAM ? stream_ws_bytes(dtype, (uint64_t)images) : 0;
}

extern "C" int mifwt_select_kth(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int64_t k, const int64_t* dk,
                                int64_t dk_stride, int route, void* value, double* value64, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (route != MIFWT_KID_SELECT_KTH_LDS && route != MIFWT_KID_SELECT_KTH_STREAM) return MIFWT_ERR_BADARG;
  Pool p;
  const int rc = pool_of(dtype, segs, nseg, images, &p);
  if (rc != MIFWT_OK) return rc;
  if (dk == nullptr ? (k < 0 || (uint64_t)k > p.count) : (dk_stride != 0 && dk_stride != 1)) return MIFWT_ERR_BADARG;
  if (p.count == 0 || images == 0) return MIFWT_OK;  // nothing to select from
  for (const Geo& g : p.segs)
    if (g.b.x == nullptr) return MIFWT_ERR_BADARG;
  if (route == MIFWT_KID_SELECT_KTH_LDS && (p.segs.size() > (size_t)kMaxSeg || p.count > (uint64_t)lds_capacity(dtype)))
    return MIFWT_ERR_UNSUPPORTED;
  if (route == MIFWT_KID_SELECT_KTH_STREAM && (workspace == nullptr || workspace_bytes < stream_ws_bytes(dtype, (uint64_t)images)))
    return MIFWT_ERR_WORKSPACE;
  const KSource src = {k, dk, dk_stride};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == MIFWT_F64 ? run_kth<double>(p, (uint64_t)images, src, route, value, value64, workspace, st)
                            : run_kth<float>(p, (uint64_t)images, src, route, value, value64, workspace, st);
}
