// mifwt_pack.hip — a coefficient container as ONE tensor and back (C ABI mifwt_pack_*, include/mifwt.h; kernel ids 59 / 60): the copies
// behind coeffs_to_array / ravel_coeffs (59, padding included) and the copy=True forms of array_to_coeffs / unravel_coeffs (60).
//
// A launch takes up to kMaxBox BOXES.  A box is a block of at most four extents — three outer ones and a row — that lies somewhere in the
// destination: the rows of the destination are dense, everything else (the outer extents of both sides, the source's row) is addressed
// through 64-bit element strides, so a band is read as the strided view it is and no copy is staged.  A box without a source is FILLED
// with the call's padding element.  The host (coeff_array.py) cuts the destination into boxes that tile it: every destination element
// has one writer, every source element one reader.  The box table travels in the kernel arguments (no device-side table: capturable).
//
// THE MAP is kernel 48's with the slots anchored on the DESTINATION.  A row is cut into slots of 16 bytes (VEC elements); slot s covers
// columns [s VEC - h, s VEC - h + VEC) clipped to [0, n), h the misalignment (in elements) of the destination row's first element, so a
// whole slot is one aligned 16-byte store.  Its source is one 16-byte load where the source row is dense and the slot's first source
// element is 16-byte aligned (rows that share their alignment), VEC element loads elsewhere.  The head and the tail of a row are peeled
// element by element; nothing is rounded down to an aligned address.  A row has vpr = (n + 2 VEC - 2) / VEC slots whatever h is.  A UNIT,
// the work of one block iteration, is part of one row (vpr >= kUnitSlots: upr units of su slots) or kUnitSlots / vpr whole rows.  Blocks
// walk the units of all boxes in a grid-stride loop and find a unit's box in the prefix table `ustart`.  The element type is a size (2,
// 4, 8 or 16 bytes): nothing is computed, the bits move.
#include "mifwt_common.h"

namespace mifwt {
namespace {

constexpr int kMaxBox = 40;
constexpr int kMaxTensors = 24;
constexpr int kThreads = 256;
constexpr uint32_t kUnitSlots = kThreads * 4;  // slots of a full unit
constexpr int kMaxGrid = 4096;                 // memory-bound: cap the grid and stride over the rest

struct alignas(16) Slot16 {
  uint32_t w[4];
};
struct alignas(16) e16_t {
  uint32_t w[4];
};

struct KBox {
  const char* src;  // null: fill
  char* dst;
  int64_t ss[4];  // source element strides: three outer extents, the row
  int64_t ds[3];  // destination element strides of the outer extents
  uint32_t e1, e2;  // row = (i0 * e1 + i1) * e2 + i2
  uint32_t n;       // elements per row
  uint32_t rows;
};

struct PackArgs {
  KBox box[kMaxBox];
  uint32_t ustart[kMaxBox + 1];
  int nbox;
  Slot16 pad;  // the padding element, repeated over 16 bytes
};
static_assert(sizeof(PackArgs) <= 4096, "the box table must fit the kernel-argument segment");

template <typename C>
__device__ __forceinline__ void slot(const KBox& s, const C* px, C* py, const Slot16& pad, uint32_t sl) {
  constexpr int VEC = 16 / sizeof(C);
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const int64_t head = (int64_t)(((uintptr_t)py & 15) / sizeof(C));
  const int64_t c0 = (int64_t)sl * VEC - head;  // (column c0 of the destination row is 16-byte aligned)
  const int64_t n = (int64_t)s.n, st = s.ss[3];
  if (c0 >= 0 && c0 + VEC <= n) {
    Slot16 v;
    if (px == nullptr) {
      v = pad;
    } else if (st == 1 && ((uintptr_t)(px + c0) & 15) == 0) {
      v = __builtin_bit_cast(Slot16, *reinterpret_cast<const u4*>(px + c0));
    } else {
      C e[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) e[j] = px[(c0 + j) * st];
      __builtin_memcpy(&v, e, 16);
    }
    *reinterpret_cast<u4*>(py + c0) = __builtin_bit_cast(u4, v);
  } else {
    C fill;
    __builtin_memcpy(&fill, &pad, sizeof(C));
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int64_t c = c0 + j;
      if (c >= 0 && c < n) py[c] = px == nullptr ? fill : px[c * st];
    }
  }
}

template <typename C>
__global__ __launch_bounds__(kThreads) void pack_kernel(const PackArgs a) {
  constexpr uint32_t VEC = 16 / sizeof(C);
  const uint32_t total = a.ustart[a.nbox];
  for (uint32_t u = blockIdx.x; u < total; u += gridDim.x) {
    int bi = 0;
    while (bi + 1 < a.nbox && u >= a.ustart[bi + 1]) ++bi;
    const KBox& s = a.box[bi];
    const uint32_t lu = u - a.ustart[bi];
    const uint32_t vpr = (s.n + 2 * VEC - 2) / VEC;
    const C* src = reinterpret_cast<const C*>(s.src);
    C* dst = reinterpret_cast<C*>(s.dst);
    if (vpr >= kUnitSlots) {  // part of one row
      uint32_t upr = (vpr + kUnitSlots - 1) / kUnitSlots;
      const uint32_t su = (vpr + upr - 1) / upr;
      upr = (vpr + su - 1) / su;  // (no empty unit at the end of a row)
      const uint32_t row = lu / upr, s0 = (lu - row * upr) * su;
      const uint32_t cnt = min(su, vpr - s0);
      const uint32_t i2 = row % s.e2, t = row / s.e2;
      const int64_t i1 = t % s.e1, i0 = t / s.e1;
      const C* px = src ? src + (i0 * s.ss[0] + i1 * s.ss[1] + (int64_t)i2 * s.ss[2]) : nullptr;
      C* py = dst + (i0 * s.ds[0] + i1 * s.ds[1] + (int64_t)i2 * s.ds[2]);
      for (uint32_t l = threadIdx.x; l < cnt; l += kThreads) slot<C>(s, px, py, a.pad, s0 + l);
    } else {  // whole short rows
      const uint32_t rb = kUnitSlots / vpr;
      const uint32_t r0 = lu * rb;
      const uint32_t cnt = min(rb, s.rows - r0) * vpr;
      for (uint32_t l = threadIdx.x; l < cnt; l += kThreads) {
        const uint32_t rr = l / vpr, sl = l - rr * vpr;
        const uint32_t row = r0 + rr;
        const uint32_t i2 = row % s.e2, t = row / s.e2;
        const int64_t i1 = t % s.e1, i0 = t / s.e1;
        const C* px = src ? src + (i0 * s.ss[0] + i1 * s.ss[1] + (int64_t)i2 * s.ss[2]) : nullptr;
        C* py = dst + (i0 * s.ds[0] + i1 * s.ds[1] + (int64_t)i2 * s.ds[2]);
        slot<C>(s, px, py, a.pad, sl);
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
constexpr int64_t kLimit = (int64_t)1 << 31;

// units of a box, or an error code
int64_t box_units(int elem_bytes, const mifwt_pack_box& b, uint32_t* rows_out) {
  for (int k = 0; k < 4; ++k)
    if (b.extent[k] < 0) return MIFWT_ERR_BADARG;
  const int64_t n = b.extent[3];
  *rows_out = 0;
  if (b.extent[0] == 0 || b.extent[1] == 0 || b.extent[2] == 0 || n == 0) return 0;
  if (n >= kLimit || b.extent[1] >= kLimit || b.extent[2] >= kLimit) return MIFWT_ERR_UNSUPPORTED;
  const double rows_d = (double)b.extent[0] * (double)b.extent[1] * (double)b.extent[2];
  if (rows_d >= 2147483648.0) return MIFWT_ERR_UNSUPPORTED;
  const uint64_t rows = (uint64_t)b.extent[0] * (uint64_t)b.extent[1] * (uint64_t)b.extent[2];
  *rows_out = (uint32_t)rows;
  const uint64_t vec = 16 / (uint64_t)elem_bytes;
  const uint64_t vpr = ((uint64_t)n + 2 * vec - 2) / vec;
  if (vpr >= kUnitSlots) {
    uint64_t upr = (vpr + kUnitSlots - 1) / kUnitSlots;
    const uint64_t su = (vpr + upr - 1) / upr;
    upr = (vpr + su - 1) / su;
    return (int64_t)(rows * upr);
  }
  const uint64_t rb = kUnitSlots / vpr;
  return (int64_t)((rows + rb - 1) / rb);
}

int check_call(int elem_bytes, const mifwt_pack_box* boxes, int nbox) {
  if (elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16) return MIFWT_ERR_BADARG;
  if (boxes == nullptr || nbox < 1 || nbox > kMaxBox) return MIFWT_ERR_BADARG;
  return MIFWT_OK;
}

// fills the table (a != nullptr); returns the number of units or an error code
int64_t build_args(int elem_bytes, const mifwt_pack_box* boxes, int nbox, bool may_fill, PackArgs* a) {
  uint64_t total = 0;
  for (int i = 0; i < nbox; ++i) {
    const mifwt_pack_box& b = boxes[i];
    uint32_t rows = 0;
    const int64_t units = box_units(elem_bytes, b, &rows);
    if (units < 0) return units;
    if (a) {
      if (units > 0 && (b.dst == nullptr || (b.src == nullptr && !may_fill))) return MIFWT_ERR_BADARG;
      if (units > 0 && (((uintptr_t)b.dst | (uintptr_t)b.src) & (uintptr_t)(elem_bytes - 1))) return MIFWT_ERR_BADARG;
      KBox& k = a->box[i];
      k.src = static_cast<const char*>(b.src);
      k.dst = static_cast<char*>(b.dst);
      for (int j = 0; j < 4; ++j) k.ss[j] = b.src_stride[j];
      for (int j = 0; j < 3; ++j) k.ds[j] = b.dst_stride[j];
      k.e1 = units ? (uint32_t)b.extent[1] : 1, k.e2 = units ? (uint32_t)b.extent[2] : 1;
      k.n = units ? (uint32_t)b.extent[3] : 0, k.rows = rows;
      a->ustart[i] = (uint32_t)total;
    }
    total += (uint64_t)units;
    if (total >= 2147483648ull) return MIFWT_ERR_UNSUPPORTED;
  }
  if (a) {
    a->ustart[nbox] = (uint32_t)total;
    a->nbox = nbox;
  }
  return (int64_t)total;
}

int launch(int elem_bytes, int64_t units, int kid, hipStream_t stream, const PackArgs& a) {
  const dim3 grid((unsigned)(units < kMaxGrid ? units : kMaxGrid)), blk(kThreads);
  switch (elem_bytes) {
    case 2: hipLaunchKernelGGL(pack_kernel<uint16_t>, grid, blk, 0, stream, a); break;
    case 4: hipLaunchKernelGGL(pack_kernel<uint32_t>, grid, blk, 0, stream, a); break;
    case 8: hipLaunchKernelGGL(pack_kernel<uint64_t>, grid, blk, 0, stream, a); break;
    default: hipLaunchKernelGGL(pack_kernel<e16_t>, grid, blk, 0, stream, a); break;
  }
  if (hipGetLastError() != hipSuccess) return MIFWT_ERR_LAUNCH;
  count_launch(kid);
  return MIFWT_OK;
}

int run(int elem_bytes, const mifwt_pack_box* boxes, int nbox, const void* padding, int kid, void* stream) {
  const int rc = check_call(elem_bytes, boxes, nbox);
  if (rc != MIFWT_OK) return rc;
  PackArgs a;
  const int64_t units = build_args(elem_bytes, boxes, nbox, padding != nullptr, &a);
  if (units <= 0) return (int)units;  // an error, or nothing to do
  Slot16 pad = {};
  if (padding != nullptr)
    for (int o = 0; o < 16; o += elem_bytes) __builtin_memcpy(reinterpret_cast<char*>(&pad) + o, padding, (size_t)elem_bytes);
  a.pad = pad;
  return launch(elem_bytes, units, kid, static_cast<hipStream_t>(stream), a);
}

}  // namespace
}  // namespace mifwt

using namespace mifwt;

extern "C" int mifwt_pack_max_boxes(void) { return kMaxBox; }

extern "C" int mifwt_pack_max_tensors(void) { return kMaxTensors; }

extern "C" int64_t mifwt_pack_plan(int elem_bytes, const mifwt_pack_box* boxes, int nbox) {
  const int rc = check_call(elem_bytes, boxes, nbox);
  if (rc != MIFWT_OK) return rc;
  return build_args(elem_bytes, boxes, nbox, true, nullptr);
}

extern "C" int mifwt_pack_to_array(int elem_bytes, const mifwt_pack_box* boxes, int nbox, const void* padding, void* stream) {
  if (padding == nullptr) return MIFWT_ERR_BADARG;
  return run(elem_bytes, boxes, nbox, padding, MIFWT_KID_PACK_TO_ARRAY, stream);
}

extern "C" int mifwt_pack_to_bands(int elem_bytes, const mifwt_pack_box* boxes, int nbox, void* stream) {
  return run(elem_bytes, boxes, nbox, nullptr, MIFWT_KID_PACK_TO_BANDS, stream);
}
