// mifwt_compact.hip — the k kept coefficients of every image of a container, compacted: (values, ascending flat indices) and back (C ABI
// mifwt_compact_*, include/mifwt.h; kernel ids 56 .. 58).  Bands, slots, keys, pools and units: mifwt_bands.h.
//
// The FLAT INDEX of a pooled element is its position in the image's pool: the non-empty segments in order, segment s at [fbase_s,
// fbase_s + count_s), inside it the row-major index of the element within its image, row * n + column.  Ascending slots of a segment
// are ascending flat indices, and so are the elements of a slot.
//
// With v the k-th largest key of the image (mifwt_select_kth), G = #{key > v} and the tie quota E = k - G, the element of flat index i is
// KEPT iff  key > v  or  (key == v and #{j < i : key_j == v} < E):  every greater element and the first E ties, exactly k elements.  The
// output slot of a kept element is  #{j < i : key_j > v} + min(#{j < i : key_j == v}, E),  so two counters per element — the greater ones
// and the ties before it — decide both, and the same pair per UNIT (chunk of slots) carries the rule across workgroups.
//   56  LDS-resident: one workgroup per image stages the values of all segments in LDS in flat order; every thread counts a contiguous
//       range, one block scan of the pairs, every thread writes its range.
//   57  streaming, three steps on the unit table of kernel 55:  COUNT — one workgroup per unit stores its pair with a plain store into
//       table[image][unit];  SCAN — one workgroup per image sums the greater counts (E), replaces every pair by the exclusive prefix over
//       the image's units in flat order (segment, then chunk), writes counts[image] and fills the padding [k, K) with 0 / -1;  WRITE — the
//       grid of COUNT again: every workgroup re-reads its chunk and scans the pairs of its threads in slot order with a carry across its
//       iterations.  A container of more than kMaxSeg segments runs several COUNT / WRITE launches against the same table.
//   58  scatter / gather: one thread per (image, j < K) moves values[image][j] to / from the element its index names in dense per-tensor
//       storage ([images][count_s] each), the segment found from the offset table in the kernel arguments.
// No atomics: every output slot has one writer, the same input gives the same bits.  Every store is guarded by its slot being below
// counts[image] <= K (56 / 57) or by the index lying inside the launch's segments (58), whatever the data holds.
#include "mifwt_bands.h"

namespace mifwt {
namespace {

using namespace bands;

// Inclusive scan of one pair per thread over the workgroup (kThreads threads); every thread calls it.  Afterwards wsum holds the
// per-wave sums, so pair_total() is the workgroup's total until the next scan.
__device__ __forceinline__ void block_scan2(uint32_t& g, uint32_t& e, uint32_t* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t tg = __shfl_up(g, o, 64), te = __shfl_up(e, o, 64);
    if (lane >= o) g += tg, e += te;
  }
  __syncthreads();  // (the sums of an earlier scan have been read)
  if (lane == 63) wsum[2 * wave] = g, wsum[2 * wave + 1] = e;
  __syncthreads();
  for (int w = 0; w < wave; ++w) g += wsum[2 * w], e += wsum[2 * w + 1];
}

__device__ __forceinline__ void pair_total(const uint32_t* wsum, uint32_t* g, uint32_t* e) {
  *g = 0, *e = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) *g += wsum[2 * w], *e += wsum[2 * w + 1];
}

struct CSeg {
  Band b;
  uint32_t slots;  // slots per image
  uint32_t wpi;    // 57: units (chunks) per image
  uint32_t spw;    // 57: slots per unit
  uint32_t fbase;  // flat index of the segment's first element
  uint32_t ubase;  // 57: the segment's first unit among the image's units
};

struct CompactArgs {
  CSeg seg[kMaxSeg];
  uint32_t ustart[kMaxSeg + 1];  // 57: first unit of a segment in this launch
  int nseg;
  uint32_t images;
  uint32_t count;  // n: pooled elements per image
  uint32_t cap;    // K: output slots per image
  uint32_t upi;    // 57: units per image, over every launch
  KSource src;
  const void* value;  // [images] the k-th largest magnitude, the data's type
  uint32_t* table;    // 57: [images][upi][2]
  uint32_t* quota;    // 57: [images] E
  void* values;       // [images][K]
  int32_t* indices;   // [images][K]
  int32_t* counts;    // [images]
};
static_assert(sizeof(CompactArgs) <= 4096, "the segment table must fit the kernel-argument segment");

// slots [k, K) of image g: value 0, index -1
template <typename C>
__device__ __forceinline__ void fill_padding(uint32_t g, uint32_t k, uint32_t cap, C* values, int32_t* indices) {
  C* vo = values + (size_t)g * cap;
  int32_t* io = indices + (size_t)g * cap;
  for (uint32_t j = k + threadIdx.x; j < cap; j += kThreads) vo[j] = C(0), io[j] = -1;
}

// ---- 56: the image's values in LDS -----------------------------------------------------------------------------------------------------
template <typename C>
__global__ __launch_bounds__(kThreads) void compact_lds_kernel(const CompactArgs a) {
  typedef typename KeyOf<C>::type K;
  __shared__ C vals[kLdsKeyBytes / sizeof(C)];
  __shared__ uint32_t wsum[2 * kThreads / 64];
  const uint32_t g = blockIdx.x, tid = threadIdx.x, cnt = a.count;
  for (int si = 0; si < a.nseg; ++si) {
    const CSeg& s = a.seg[si];
    for (uint32_t t = tid; t < s.slots; t += kThreads) {
      const uint32_t r = t / s.b.vpr, sl = t - r * s.b.vpr;
      visit_slot<C>(s.b, g * s.b.rp + r, sl, [&](uint32_t c, C x) { vals[s.fbase + r * s.b.n + c] = x; });
    }
  }
  __syncthreads();
  const K v = key_of(static_cast<const C*>(a.value)[g]);
  const uint32_t k = k_of(a.src, g, min(cnt, a.cap));
  const uint32_t per = (cnt + kThreads - 1) / kThreads;
  const uint32_t i0 = min(cnt, tid * per), i1 = min(cnt, i0 + per);
  uint32_t lg = 0, le = 0;
  for (uint32_t i = i0; i < i1; ++i) {
    const K key = key_of(vals[i]);
    lg += key > v, le += key == v;
  }
  uint32_t pg = lg, pe = le;
  block_scan2(pg, pe, wsum);
  pg -= lg, pe -= le;  // greater elements / ties before this thread's range
  uint32_t big, ties;
  pair_total(wsum, &big, &ties);
  const uint32_t quota = k > big ? k - big : 0;
  C* vo = static_cast<C*>(a.values) + (size_t)g * a.cap;
  int32_t* io = a.indices + (size_t)g * a.cap;
  for (uint32_t i = i0; i < i1; ++i) {
    const C x = vals[i];
    const K key = key_of(x);
    const bool isg = key > v, ise = key == v;
    if (isg || (ise && pe < quota)) {
      const uint32_t pos = pg + min(pe, quota);
      if (pos < k) vo[pos] = x, io[pos] = (int32_t)i;
    }
    pg += isg, pe += ise;
  }
  if (tid == 0) a.counts[g] = (int32_t)k;
  fill_padding<C>(g, k, a.cap, static_cast<C*>(a.values), a.indices);
}

// ---- 57: streaming ------------------------------------------------------------------------------------------------------------------------
// (segment, image, chunk) of workgroup u of a launch
__device__ __forceinline__ int locate(const CompactArgs& a, uint32_t u, uint32_t* g, uint32_t* w) {
  int si = 0;
  while (si + 1 < a.nseg && u >= a.ustart[si + 1]) ++si;
  const uint32_t lu = u - a.ustart[si];
  *g = lu / a.seg[si].wpi;
  *w = lu - *g * a.seg[si].wpi;
  return si;
}

template <typename C>
__global__ __launch_bounds__(kThreads) void compact_count_kernel(const CompactArgs a) {
  typedef typename KeyOf<C>::type K;
  __shared__ uint32_t wsum[2 * kThreads / 64];
  uint32_t g, w;
  const CSeg& s = a.seg[locate(a, blockIdx.x, &g, &w)];
  const K v = key_of(static_cast<const C*>(a.value)[g]);
  const uint32_t t0 = w * s.spw, t1 = min(s.slots, t0 + s.spw);
  uint32_t lg = 0, le = 0;
  for (uint32_t t = t0 + threadIdx.x; t < t1; t += kThreads) {
    const uint32_t r = t / s.b.vpr, sl = t - r * s.b.vpr;
    visit_slot<C>(s.b, g * s.b.rp + r, sl, [&](uint32_t, C x) {
      const K key = key_of(x);
      lg += key > v, le += key == v;
    });
  }
  block_scan2(lg, le, wsum);
  if (threadIdx.x == kThreads - 1) {
    uint32_t* e = a.table + 2 * ((size_t)g * a.upi + s.ubase + w);
    e[0] = lg, e[1] = le;
  }
}

// one workgroup per image: pairs -> exclusive prefixes in unit order, the quota, the count, the padding
template <typename C>
__global__ __launch_bounds__(kThreads) void compact_scan_kernel(const uint32_t cnt, const uint32_t cap, const uint32_t upi, const KSource src,
                                                                uint32_t* table, uint32_t* quota, C* values, int32_t* indices, int32_t* counts) {
  __shared__ uint32_t wsum[2 * kThreads / 64];
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  uint32_t* t = table + 2 * (size_t)g * upi;
  uint32_t cg = 0, ce = 0;  // carries: the pairs of the units before this round
  for (uint32_t base = 0; base < upi; base += kThreads) {
    const uint32_t u = base + tid;
    uint32_t lg = 0, le = 0;
    if (u < upi) lg = t[2 * u], le = t[2 * u + 1];
    uint32_t pg = lg, pe = le;
    block_scan2(pg, pe, wsum);
    if (u < upi) t[2 * u] = cg + pg - lg, t[2 * u + 1] = ce + pe - le;
    uint32_t tg, te;
    pair_total(wsum, &tg, &te);
    cg += tg, ce += te;
  }
  const uint32_t k = k_of(src, g, min(cnt, cap));
  if (tid == 0) {
    quota[g] = k > cg ? k - cg : 0;
    counts[g] = (int32_t)k;
  }
  fill_padding<C>(g, k, cap, values, indices);
}

template <typename C>
__global__ __launch_bounds__(kThreads) void compact_write_kernel(const CompactArgs a) {
  typedef typename KeyOf<C>::type K;
  __shared__ uint32_t wsum[2 * kThreads / 64];
  uint32_t g, w;
  const CSeg& s = a.seg[locate(a, blockIdx.x, &g, &w)];
  const K v = key_of(static_cast<const C*>(a.value)[g]);
  const uint32_t* e = a.table + 2 * ((size_t)g * a.upi + s.ubase + w);
  uint32_t cg = e[0], ce = e[1];  // greater elements / ties of the image before this round
  const uint32_t quota = a.quota[g], kept = (uint32_t)a.counts[g];
  C* vo = static_cast<C*>(a.values) + (size_t)g * a.cap;
  int32_t* io = a.indices + (size_t)g * a.cap;
  const uint32_t t0 = w * s.spw, t1 = min(s.slots, t0 + s.spw);
  for (uint32_t tb = t0; tb < t1; tb += kThreads) {  // (every thread takes every round: the scan has barriers)
    const uint32_t t = tb + threadIdx.x;
    const uint32_t r = t / s.b.vpr, sl = t - r * s.b.vpr;
    uint32_t lg = 0, le = 0;
    if (t < t1)
      visit_slot<C>(s.b, g * s.b.rp + r, sl, [&](uint32_t, C x) {
        const K key = key_of(x);
        lg += key > v, le += key == v;
      });
    uint32_t pg = lg, pe = le;
    block_scan2(pg, pe, wsum);
    pg += cg - lg, pe += ce - le;
    if (t < t1 && (lg != 0 || (le != 0 && pe < quota)))
      visit_slot<C>(s.b, g * s.b.rp + r, sl, [&](uint32_t c, C x) {
        const K key = key_of(x);
        const bool isg = key > v, ise = key == v;
        if (isg || (ise && pe < quota)) {
          const uint32_t pos = pg + min(pe, quota);
          if (pos < kept) vo[pos] = x, io[pos] = (int32_t)(s.fbase + r * s.b.n + c);
        }
        pg += isg, pe += ise;
      });
    uint32_t tg, te;
    pair_total(wsum, &tg, &te);
    cg += tg, ce += te;
  }
}

// ---- 58: scatter / gather -----------------------------------------------------------------------------------------------------------------
struct MoveArgs {
  char* x[kMaxSeg];             // dense storage of a segment: [images][start[s + 1] - start[s]]
  uint32_t start[kMaxSeg + 1];  // flat index of a segment's first element
  int nseg;
  uint32_t cap;
  uint64_t total;  // images * K
  void* values;
  const int32_t* indices;
  const int32_t* counts;
};

template <typename C, bool GATHER>
__global__ __launch_bounds__(kThreads) void compact_move_kernel(const MoveArgs a) {
  const uint64_t id = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (id >= a.total) return;
  const uint64_t g = id / a.cap;
  const uint32_t j = (uint32_t)(id - g * a.cap);
  const int32_t kept = a.counts[g];
  if (kept < 0 || j >= (uint32_t)kept) return;
  const int32_t idx = a.indices[id];
  if (idx < 0) return;
  const uint32_t i = (uint32_t)idx;
  if (i < a.start[0] || i >= a.start[a.nseg]) return;  // another launch's segments, or no element of the pool
  int si = 0;
  while (i >= a.start[si + 1]) ++si;
  C* p = reinterpret_cast<C*>(a.x[si]) + (g * (uint64_t)(a.start[si + 1] - a.start[si]) + (i - a.start[si]));
  C* val = static_cast<C*>(a.values) + id;
  if (GATHER)
    *val = *p;
  else
    *p = *val;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// units per image over all segments of the pool; 0 where one launch would exceed the grid
uint64_t units_per_image(const Pool& p, uint64_t images) {
  uint64_t upi = 0;
  for (size_t c0 = 0; c0 < p.segs.size(); c0 += kMaxSeg) {
    uint64_t launch = 0;
    for (size_t i = c0; i < std::min(p.segs.size(), c0 + kMaxSeg); ++i) {
      uint64_t slots, wpi, spw;
      unit_plan(p.segs[i], images, &slots, &wpi, &spw);
      launch += wpi;
    }
    if (launch * images >= 2147483648ull) return 0;
    upi += launch;
  }
  return upi;
}

size_t stream_ws_bytes(uint64_t upi, uint64_t images) { return (2 * upi + 1) * images * sizeof(uint32_t); }

// the segment table of segments [c0, c0 + n) of the pool, whose first element / unit in the image are fbase / ubase; the launch's units
uint32_t fill_segments(const Pool& p, size_t c0, int n, uint64_t images, uint32_t fbase, uint32_t ubase, CompactArgs* a) {
  uint64_t total = 0;
  for (int i = 0; i < n; ++i) {
    const Geo& g = p.segs[c0 + i];
    uint64_t slots, wpi, spw;
    unit_plan(g, images, &slots, &wpi, &spw);
    CSeg& s = a->seg[i];
    s.b = g.b;
    s.slots = (uint32_t)slots, s.wpi = (uint32_t)wpi, s.spw = (uint32_t)spw, s.fbase = fbase, s.ubase = ubase;
    a->ustart[i] = (uint32_t)total;
    total += wpi * images;
    fbase += (uint32_t)g.count, ubase += (uint32_t)wpi;
  }
  a->ustart[n] = (uint32_t)total;
  a->nseg = n;
  return (uint32_t)total;
}

template <typename C>
int run_encode(const Pool& p, uint64_t images, const KSource& src, uint32_t cap, int route, const void* value, void* values, int32_t* indices,
               int32_t* counts, void* ws, hipStream_t st) {
  CompactArgs a = {};
  a.images = (uint32_t)images, a.count = (uint32_t)p.count, a.cap = cap, a.src = src;
  a.value = value, a.values = values, a.indices = indices, a.counts = counts;
  if (route == MIFWT_KID_COMPACT_LDS) {
    fill_segments(p, 0, (int)p.segs.size(), images, 0, 0, &a);
    hipLaunchKernelGGL(compact_lds_kernel<C>, dim3(a.images), dim3(kThreads), 0, st, a);
    return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
  }
  const uint64_t upi = units_per_image(p, images);
  if (upi == 0 || upi >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;
  a.upi = (uint32_t)upi;
  a.table = static_cast<uint32_t*>(ws);
  a.quota = a.table + 2 * (size_t)upi * images;
  for (int step = 0; step < 2; ++step) {  // COUNT over every launch's segments, SCAN, WRITE over the same launches
    uint32_t fbase = 0, ubase = 0;
    for (size_t c0 = 0; c0 < p.segs.size(); c0 += kMaxSeg) {
      const int n = (int)std::min<size_t>(kMaxSeg, p.segs.size() - c0);
      const uint32_t units = fill_segments(p, c0, n, images, fbase, ubase, &a);
      if (step == 0)
        hipLaunchKernelGGL(compact_count_kernel<C>, dim3(units), dim3(kThreads), 0, st, a);
      else
        hipLaunchKernelGGL(compact_write_kernel<C>, dim3(units), dim3(kThreads), 0, st, a);
      if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
      for (int i = 0; i < n; ++i) fbase += (uint32_t)p.segs[c0 + i].count, ubase += a.seg[i].wpi;
    }
    if (step == 0) {
      hipLaunchKernelGGL(compact_scan_kernel<C>, dim3(a.images), dim3(kThreads), 0, st, a.count, a.cap, a.upi, src, a.table, a.quota,
                         static_cast<C*>(values), indices, counts);
      if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
    }
  }
  return MIFWT_OK;
}

template <typename C>
int run_move(bool gather, void* const* tensors, const int64_t* sizes, int nseg, uint64_t images, uint32_t cap, void* values,
             const int32_t* indices, const int32_t* counts, hipStream_t st) {
  MoveArgs a = {};
  a.cap = cap, a.total = images * cap, a.values = values, a.indices = indices, a.counts = counts;
  const unsigned grid = (unsigned)((a.total + kThreads - 1) / kThreads);
  uint32_t start = 0;
  for (int c0 = 0; c0 < nseg; c0 += kMaxSeg) {
    a.nseg = std::min(kMaxSeg, nseg - c0);
    for (int i = 0; i < a.nseg; ++i) {
      a.x[i] = static_cast<char*>(tensors[c0 + i]);
      a.start[i] = start;
      start += (uint32_t)sizes[c0 + i];
    }
    a.start[a.nseg] = start;
    if (gather)
      hipLaunchKernelGGL((compact_move_kernel<C, true>), dim3(grid), dim3(kThreads), 0, st, a);
    else
      hipLaunchKernelGGL((compact_move_kernel<C, false>), dim3(grid), dim3(kThreads), 0, st, a);
    if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  }
  return MIFWT_OK;
}

}  // namespace
}  // namespace mifwt

using namespace mifwt;

extern "C" int mifwt_compact_max_segments(void) { return kMaxSeg; }

extern "C" int mifwt_compact_route(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int force_stream) {
  Pool p;
  const int rc = pool_of(dtype, segs, nseg, images, &p);
  if (rc != MIFWT_OK) return rc;
  if (p.count == 0 || images == 0) return 0;
  const bool lds = !force_stream && p.segs.size() <= (size_t)kMaxSeg && p.count <= (uint64_t)lds_capacity(dtype);
  return lds ? MIFWT_KID_COMPACT_LDS : MIFWT_KID_COMPACT_STREAM;
}

extern "C" size_t mifwt_compact_workspace(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int route) {
  Pool p;
  if (pool_of(dtype, segs, nseg, images, &p) != MIFWT_OK || p.count == 0 || images == 0) return 0;
  return route == MIFWT_KID_COMPACT_STREAM ? stream_ws_bytes(units_per_image(p, (uint64_t)images), (uint64_t)images) : 0;
}

extern "C" int mifwt_compact_encode(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int64_t k, const int64_t* dk,
                                    int64_t dk_stride, int64_t capacity, int route, const void* value, void* values, int32_t* indices,
                                    int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  if (route != MIFWT_KID_COMPACT_LDS && route != MIFWT_KID_COMPACT_STREAM) return MIFWT_ERR_BADARG;
  Pool p;
  const int rc = pool_of(dtype, segs, nseg, images, &p);
  if (rc != MIFWT_OK) return rc;
  if (capacity < 0 || (uint64_t)capacity > p.count) return MIFWT_ERR_BADARG;
  if (dk == nullptr ? (k < 0 || k > capacity) : (dk_stride != 0 && dk_stride != 1)) return MIFWT_ERR_BADARG;
  if (p.count == 0 || images == 0 || capacity == 0) return MIFWT_OK;  // nothing to write
  for (const Geo& g : p.segs)
    if (g.b.x == nullptr) return MIFWT_ERR_BADARG;
  if (value == nullptr || values == nullptr || indices == nullptr || counts == nullptr) return MIFWT_ERR_BADARG;
  if (route == MIFWT_KID_COMPACT_LDS && (p.segs.size() > (size_t)kMaxSeg || p.count > (uint64_t)lds_capacity(dtype)))
    return MIFWT_ERR_UNSUPPORTED;
  if (route == MIFWT_KID_COMPACT_STREAM) {
    const uint64_t upi = units_per_image(p, (uint64_t)images);
    if (upi == 0) return MIFWT_ERR_UNSUPPORTED;
    if (workspace == nullptr || workspace_bytes < stream_ws_bytes(upi, (uint64_t)images)) return MIFWT_ERR_WORKSPACE;
  }
  const KSource src = {k, dk, dk_stride};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == MIFWT_F64
             ? run_encode<double>(p, (uint64_t)images, src, (uint32_t)capacity, route, value, values, indices, counts, workspace, st)
             : run_encode<float>(p, (uint64_t)images, src, (uint32_t)capacity, route, value, values, indices, counts, workspace, st);
}

extern "C" int mifwt_compact_move(int dtype, int gather, void* const* tensors, const int64_t* sizes, int nseg, int64_t images,
                                  int64_t capacity, void* values, const int32_t* indices, const int32_t* counts, void* stream) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return MIFWT_ERR_BADARG;
  if (nseg < 0 || (nseg > 0 && (tensors == nullptr || sizes == nullptr)) || images < 0 || images >= 2147483648ll || capacity < 0)
    return MIFWT_ERR_BADARG;
  uint64_t n = 0;
  for (int i = 0; i < nseg; ++i) {
    if (sizes[i] < 0) return MIFWT_ERR_BADARG;
    n += (uint64_t)sizes[i];
    if (n >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;  // int32 indices
  }
  for (int i = 0; i < nseg; ++i)
    if (sizes[i] > 0 && tensors[i] == nullptr) return MIFWT_ERR_BADARG;
  if ((uint64_t)capacity > n) return MIFWT_ERR_BADARG;
  if (n == 0 || images == 0 || capacity == 0) return MIFWT_OK;  // nothing to move
  if (values == nullptr || indices == nullptr || counts == nullptr) return MIFWT_ERR_BADARG;
  if (((uint64_t)images * (uint64_t)capacity + kThreads - 1) / kThreads >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == MIFWT_F64
             ? run_move<double>(gather != 0, tensors, sizes, nseg, (uint64_t)images, (uint32_t)capacity, values, indices, counts, st)
             : run_move<float>(gather != 0, tensors, sizes, nseg, (uint64_t)images, (uint32_t)capacity, values, indices, counts, st);
}
