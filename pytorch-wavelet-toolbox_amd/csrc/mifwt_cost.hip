// mifwt_cost.hip — additive costs of the nodes of a wavelet packet tree (C ABI mifwt_cost_*, include/mifwt.h; kernel ids 61 / 62): what the
// Coifman-Wickerhauser best-basis search reads.
//
// Bands and slots: mifwt_bands.h.  A SEGMENT is a band whose `rows_per_index` consecutive rows form one NODE; every segment has its own
// node count and its own output (one float64 per node).  A packet level buffer [B, nb^s, extents..] is one segment, a tree one table.
//
// The term of an element t, evaluated in float64 for both data types (param: p of the norm, the value of threshold / sure):
//   SHANNON   -t^2 ln t^2 (0 where t^2 == 0)     LOGENERGY  ln t^2 (0 where t^2 == 0)     NORM  |t|^p (no pow for p == 1, p == 2)
//   THRESHOLD [|t| > param]                      SURE       [|t| > param] + min(t^2, param^2)  (= n - #{|t| <= param} + sum min(..))
// The indicator parts are counted in integers and added to the float64 sum once per unit, so THRESHOLD is exact.
//
// 61: the regime of a segment follows from the node length and the dtype alone.
//   LONG nodes (more than kShortSlots * VEC elements): units are (node, chunk of at most kChunkSlots slots); a workgroup sums a chunk
//   per thread, across the wave (shuffles) and the workgroup (LDS) in a fixed order and writes ONE plain store to the workspace.
//   SHORT nodes: a workgroup takes a run of consecutive nodes; a node is summed by a group of 4 / 16 / 64 lanes (short_width) — a deep
//   level spends 4 lanes, not a wave, on a 25-element node — and lane 0 of the group stores the node's cost.  No workspace slot.
// 62: one thread per long node adds the node's chunks in index order and stores the cost.
// No atomics; the unit plan depends on dtype and shapes only: the same input gives the same bits.
#include <cmath>

#include "mifwt_bands.h"

namespace mifwt {
namespace {

using namespace bands;

constexpr uint32_t kShortSlots = 512;         // a node of at most kShortSlots * VEC elements is short
constexpr uint32_t kChunkSlots = kThreads * 8;  // long nodes: slots per unit at most
constexpr uint32_t kMaxChunks = 1024;         // long nodes: units per node at most (longer chunks beyond)
constexpr uint32_t kShortUnitSlots = 1024;    // short nodes: slots a unit takes, about
constexpr uint32_t kShortReps = 8;            // short nodes: passes of a workgroup per unit at most
constexpr int kMaxGrid = 8192;

struct CSeg {
  Band b;
  double* out;     // [nodes]
  uint32_t nodes;
  uint32_t slots;  // slots per node
  uint32_t ppi;    // long: units (chunks) per node; short: 0
  uint32_t spp;    // long: slots per chunk; short: nodes per unit (a multiple of kThreads / width)
  uint32_t width;  // short: lanes per node
  uint32_t lstart; // long: nodes of the long segments before this one
};

struct CostArgs {
  CSeg seg[kMaxSeg];
  uint32_t ustart[kMaxSeg + 1];
  int nseg;
  double param, param2;  // param2: param^2
  double* part;          // [units]; long units only
};
static_assert(sizeof(CostArgs) <= 4096, "the segment table must fit the kernel-argument segment");

struct FinArgs {
  double* out[kMaxSeg];
  uint32_t ustart[kMaxSeg];
  uint32_t ppi[kMaxSeg];
  uint32_t lstart[kMaxSeg + 1];  // long nodes before segment i (a short segment has none)
  int nseg;
  const double* part;
};
static_assert(sizeof(FinArgs) <= 4096, "the segment table must fit the kernel-argument segment");

struct Acc {
  double sum;
  uint32_t cnt;
};

template <int F>
__device__ __forceinline__ void add_term(Acc& a, double t, double param, double param2) {
  if (F == MIFWT_COST_SHANNON) {
    const double t2 = t * t;
    if (t2 > 0.0) a.sum -= t2 * log(t2);
  } else if (F == MIFWT_COST_LOGENERGY) {
    const double t2 = t * t;
    if (t2 > 0.0) a.sum += log(t2);
  } else if (F == MIFWT_COST_NORM) {
    const double m = fabs(t);
    a.sum += param == 1.0 ? m : param == 2.0 ? m * m : pow(m, param);
  } else if (F == MIFWT_COST_THRESHOLD) {
    a.cnt += fabs(t) > param ? 1u : 0u;
  } else {
    const double t2 = t * t;
    a.cnt += fabs(t) > param ? 1u : 0u;
    a.sum += t2 < param2 ? t2 : param2;
  }
}

// the slots [t0, t1) of node g, every `step`-th from `first` on
template <typename C, int F>
__device__ __forceinline__ void add_slots(Acc& a, const Band& b, uint32_t g, uint32_t first, uint32_t t1, uint32_t step, double param,
                                          double param2) {
  if (b.rp == 1) {  // (a node of one row: no division per slot)
    for (uint32_t t = first; t < t1; t += step) visit_slot<C>(b, g, t, [&](uint32_t, C v) { add_term<F>(a, (double)v, param, param2); });
    return;
  }
  for (uint32_t t = first; t < t1; t += step) {
    const uint32_t r = t / b.vpr, sl = t - r * b.vpr;
    visit_slot<C>(b, g * b.rp + r, sl, [&](uint32_t, C v) { add_term<F>(a, (double)v, param, param2); });
  }
}

template <int F>
__device__ __forceinline__ double total_of(const Acc& a) {
  return F == MIFWT_COST_THRESHOLD ? (double)a.cnt : F == MIFWT_COST_SURE ? (double)a.cnt + a.sum : a.sum;
}

// a run of short nodes, W lanes per node.  Every thread of the workgroup makes the same number of passes.
template <typename C, int F, int W>
__device__ __forceinline__ void short_nodes(const CSeg& s, uint32_t lu, double param, double param2) {
  constexpr uint32_t PER = kThreads / W;
  const uint32_t sub = threadIdx.x / W, l = threadIdx.x & (W - 1);
  const uint32_t first = lu * s.spp;
  for (uint32_t k = 0; k < s.spp; k += PER) {
    const uint32_t g = first + k + sub;
    Acc a = {0.0, 0u};
    if (g < s.nodes) add_slots<C, F>(a, s.b, g, l, s.slots, W, param, param2);
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
      a.sum += __shfl_xor(a.sum, o, 64);
      a.cnt += __shfl_xor(a.cnt, o, 64);
    }
    if (l == 0 && g < s.nodes) s.out[g] = total_of<F>(a);
  }
}

// ---- 61 ----------------------------------------------------------------------------------------------------------------------------------
template <typename C, int F>
__global__ __launch_bounds__(kThreads) void cost_kernel(const CostArgs a) {
  __shared__ double red[kThreads / 64];
  __shared__ uint32_t redc[kThreads / 64];
  const uint32_t total = a.ustart[a.nseg];
  for (uint32_t u = blockIdx.x; u < total; u += gridDim.x) {
    int si = 0;
    while (si + 1 < a.nseg && u >= a.ustart[si + 1]) ++si;
    const CSeg& s = a.seg[si];
    const uint32_t lu = u - a.ustart[si];
    if (s.ppi == 0) {
      if (s.width == 4)
        short_nodes<C, F, 4>(s, lu, a.param, a.param2);
      else if (s.width == 16)
        short_nodes<C, F, 16>(s, lu, a.param, a.param2);
      else
        short_nodes<C, F, 64>(s, lu, a.param, a.param2);
      continue;
    }
    const uint32_t g = lu / s.ppi, part = lu - g * s.ppi;
    const uint32_t t0 = part * s.spp, t1 = min(s.slots, t0 + s.spp);
    Acc acc = {0.0, 0u};
    add_slots<C, F>(acc, s.b, g, t0 + threadIdx.x, t1, kThreads, a.param, a.param2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      acc.sum += __shfl_xor(acc.sum, o, 64);
      acc.cnt += __shfl_xor(acc.cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc.sum, redc[threadIdx.x >> 6] = acc.cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      Acc t = {0.0, 0u};
      for (int w = 0; w < kThreads / 64; ++w) t.sum += red[w], t.cnt += redc[w];
      a.part[u] = total_of<F>(t);
    }
    __syncthreads();
  }
}

// ---- 62: one thread per long node, its chunks in index order --------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cost_finish_kernel(const FinArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.lstart[a.nseg]) return;
  int si = 0;
  while (i >= a.lstart[si + 1]) ++si;
  const uint32_t g = (uint32_t)i - a.lstart[si];
  const double* p = a.part + a.ustart[si] + (size_t)g * a.ppi[si];
  double sum = 0.0;
  for (uint32_t k = 0; k < a.ppi[si]; ++k) sum += p[k];
  a.out[si][g] = sum;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
inline int vec_of(int dtype) { return dtype == MIFWT_F64 ? 2 : 4; }

// lanes per short node: from the node length and the dtype alone
inline uint32_t short_width(int dtype, uint64_t count) {
  const uint64_t nominal = (count + vec_of(dtype) - 1) / vec_of(dtype);  // 16-byte slots of an aligned node
  return nominal <= 8 ? 4 : nominal <= 64 ? 16 : 64;
}

// fills the table (a may be NULL); returns the number of units or an error code.  *long_nodes: nodes of the long segments.
int64_t build_cost(int dtype, const mifwt_estim_band* segs, int nseg, CostArgs* a, int64_t* unit_start, uint64_t* long_nodes) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return MIFWT_ERR_BADARG;
  if (segs == nullptr || nseg < 1 || nseg > kMaxSeg) return MIFWT_ERR_BADARG;
  uint64_t total = 0, lnodes = 0;
  for (int i = 0; i < nseg; ++i) {
    Geo g;
    const int rc = band_geometry(dtype, segs[i], &g);
    if (rc != MIFWT_OK) return rc;
    if (g.count == 0) return MIFWT_ERR_BADARG;  // (empty nodes cost nothing and are the caller's)
    const uint64_t slots = (uint64_t)g.b.rp * g.b.vpr;
    uint64_t ppi = 0, spp, units;
    uint32_t width = 0;
    if (g.count > (uint64_t)kShortSlots * vec_of(dtype)) {
      ppi = (slots + kChunkSlots - 1) / kChunkSlots;
      if (ppi > kMaxChunks) ppi = kMaxChunks;
      spp = (slots + ppi - 1) / ppi;
      ppi = (slots + spp - 1) / spp;
      units = ppi * g.images;
    } else {
      width = short_width(dtype, g.count);
      const uint64_t per = kThreads / width;
      uint64_t reps = (kShortUnitSlots + per * slots - 1) / (per * slots);
      if (reps > kShortReps) reps = kShortReps;
      spp = per * reps;
      units = (g.images + spp - 1) / spp;
    }
    if (a) {
      CSeg& c = a->seg[i];
      c.b = g.b;
      if (segs[i].extent[0] == 1) c.b.s0 = c.b.s1, c.b.e1 = 1;  // (one outer extent: the row index is the inner one, no division per slot)
      c.out = nullptr;
      c.nodes = (uint32_t)g.images, c.slots = (uint32_t)slots, c.ppi = (uint32_t)ppi, c.spp = (uint32_t)spp, c.width = width;
      c.lstart = (uint32_t)lnodes;
      a->ustart[i] = (uint32_t)total;
    }
    if (unit_start) unit_start[i] = (int64_t)total;
    total += units;
    if (ppi) lnodes += g.images;
    if (total >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;
  }
  if (a) a->ustart[nseg] = (uint32_t)total, a->nseg = nseg;
  if (unit_start) unit_start[nseg] = (int64_t)total;
  if (long_nodes) *long_nodes = lnodes;
  return (int64_t)total;
}

template <typename C>
void launch_cost(int functional, dim3 grid, hipStream_t st, const CostArgs& a) {
  switch (functional) {
    case MIFWT_COST_SHANNON: hipLaunchKernelGGL((cost_kernel<C, MIFWT_COST_SHANNON>), grid, dim3(kThreads), 0, st, a); break;
    case MIFWT_COST_LOGENERGY: hipLaunchKernelGGL((cost_kernel<C, MIFWT_COST_LOGENERGY>), grid, dim3(kThreads), 0, st, a); break;
    case MIFWT_COST_NORM: hipLaunchKernelGGL((cost_kernel<C, MIFWT_COST_NORM>), grid, dim3(kThreads), 0, st, a); break;
    case MIFWT_COST_THRESHOLD: hipLaunchKernelGGL((cost_kernel<C, MIFWT_COST_THRESHOLD>), grid, dim3(kThreads), 0, st, a); break;
    default: hipLaunchKernelGGL((cost_kernel<C, MIFWT_COST_SURE>), grid, dim3(kThreads), 0, st, a); break;
  }
}

}  // namespace
}  // namespace mifwt

using namespace mifwt;

extern "C" int mifwt_cost_max_segments(void) { return kMaxSeg; }

extern "C" int64_t mifwt_cost_short_limit(int dtype) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return MIFWT_ERR_BADARG;
  return (int64_t)kShortSlots * vec_of(dtype);
}

extern "C" int64_t mifwt_cost_chunk(int dtype) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return MIFWT_ERR_BADARG;
  return (int64_t)kChunkSlots * vec_of(dtype);
}

extern "C" int64_t mifwt_cost_plan(int dtype, const mifwt_estim_band* segs, int nseg, int64_t* unit_start) {
  return build_cost(dtype, segs, nseg, nullptr, unit_start, nullptr);
}

extern "C" int mifwt_cost_nodes(int dtype, int functional, double param, const mifwt_estim_band* segs, int nseg, double* const* out,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (functional < MIFWT_COST_SHANNON || functional > MIFWT_COST_SURE) return MIFWT_ERR_BADARG;
  CostArgs a;
  uint64_t long_nodes = 0;
  const int64_t units = build_cost(dtype, segs, nseg, &a, nullptr, &long_nodes);
  if (units < 0) return (int)units;
  if (out == nullptr) return MIFWT_ERR_BADARG;
  for (int i = 0; i < nseg; ++i) {
    if (segs[i].x == nullptr || out[i] == nullptr) return MIFWT_ERR_BADARG;
    a.seg[i].out = out[i];
  }
  if (long_nodes && (workspace == nullptr || workspace_bytes < sizeof(double) * (size_t)units)) return MIFWT_ERR_WORKSPACE;
  a.param = param, a.param2 = param * param;
  a.part = static_cast<double*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(units < kMaxGrid ? units : kMaxGrid));
  if (dtype == MIFWT_F64)
    launch_cost<double>(functional, grid, st, a);
  else
    launch_cost<float>(functional, grid, st, a);
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  if (long_nodes) {
    FinArgs f = {};
    for (int i = 0; i < nseg; ++i) {
      f.out[i] = a.seg[i].out, f.ustart[i] = a.ustart[i], f.ppi[i] = a.seg[i].ppi, f.lstart[i] = a.seg[i].lstart;
    }
    f.lstart[nseg] = (uint32_t)long_nodes;
    f.nseg = nseg, f.part = a.part;
    hipLaunchKernelGGL(cost_finish_kernel, dim3((unsigned)((long_nodes + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, f);
    if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  }
  return MIFWT_OK;
}
