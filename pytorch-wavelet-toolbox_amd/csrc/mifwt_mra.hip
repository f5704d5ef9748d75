// mifwt_mra.hip — multiresolution analysis: every component of a decomposition projected back into the signal domain in ONE launch
// (C ABI mifwt_mra_*, include/mifwt.h; kernel ids 63 / 64).
//
// A COMPONENT is the reconstruction from one band alone: a cascade of `depth` one-input synthesis stages, the first with rec_hi (a
// detail band) or rec_lo (the approximation), the others with rec_lo.  A workgroup takes one (tile of outputs, component, row): it
// stages the window of the band that the tile depends on into LDS through the index map of the boundary, runs the stages between two
// LDS buffers and writes its tile once, the last stage straight to global memory.  Every band is read once (plus the halo of its
// tiles), every component written once; nothing else touches memory.
//
// 63, stationary (mifwt_swt_inv with one band absent), stage at dilation D = 2^(l-1), l = depth .. 1:
//     y[n] = 0.5 sum_i r[i] c[(n + D (L/2 - 1 - i)) mod N]
//   the window shrinks by D (L - 1) per stage, D L/2 of it on the left: a tile needs (2^depth - 1)(L - 1) extra samples of the band.
//   The window is periodic in N as a whole, so only the staging wraps (as often as needed).
// 64, decimated, stage from level l to l - 1 with S = L - 2 (padded) or L/2 - 1 (circular):
//     y[n] = sum_{t == n + S mod 2} r[t] c[(n + S - t) / 2]
//   even / odd outputs take the even / odd taps.  Padded: c outside [0, len_l) and y outside [0, len_{l-1}) are absent (zero).
//   Circular: c is read mod len_l; a level cropped by one sample (len_{l-1} = 2 len_l - 1) has that period itself, so the position
//   p = q + w len_{l-1} of a window reads c at (q + S - t) / 2 + w len_l = (p + w crop + S - t) / 2 in unwrapped coordinates.
//   The windows per level are worked backwards from the tile by the same formulas on the device.
// float32 data: float32 FMAs; float64: float64.  Taps arrive as host doubles.  64-bit offsets, no atomics, no host read.
#include "mifwt_common.h"

namespace mifwt {
namespace {

constexpr int kMraThreads = 256;
constexpr int kMraTile = 2048;     // outputs per workgroup
constexpr int kMraBuf = 4096;      // 63: elements per LDS buffer: two of them, 64 KiB in float64
constexpr int kMraDwtBuf = 3072;   // 64: likewise (the window of level 1 is half a tile and L/2 + 1 samples)
constexpr int kMraMaxBands = 33;   // components per launch
constexpr int kMraMaxLevels = 32;  // deepest component
constexpr int kMraMaxFilt = 20;
constexpr int64_t kMraMaxN = (int64_t)1 << 30;

struct MraBand {
  const void* x;
  int64_t rs;  // row stride, elements
  int32_t index, depth, detail, pad;
};

template <typename T>
struct MraArgs {
  MraBand band[kMraMaxBands];
  T lo[kMraMaxFilt], hi[kMraMaxFilt];
  int32_t len[kMraMaxLevels + 1];  // 64: samples per row at level l (0: the signal)
  T* out;
  int64_t out_cs, out_rs;  // component / row stride of the output, elements
  int64_t units;
  int32_t nbands, ntiles, n, flen, circular;
};
static_assert(sizeof(MraArgs<double>) <= 4096, "the band table must fit the kernel-argument segment");

__device__ __forceinline__ int floordiv(int a, int b) {  // b > 0
  int q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// ---- 63 ------------------------------------------------------------------------------------------------------------------------------
template <typename T, int L>
__global__ __launch_bounds__(kMraThreads) void mra_swt_kernel(const MraArgs<T> a) {
  __shared__ T buf[2][kMraBuf];
  const int N = a.n;
  for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int tile = (int)(u % a.ntiles);
    const int64_t r = u / a.ntiles;
    const int c = (int)(r % a.nbands);
    const int64_t row = r / a.nbands;
    const MraBand& b = a.band[c];
    const int depth = b.depth;
    const int o0 = tile * kMraTile;
    const int tlen = min(kMraTile, N - o0);
    const int span = (1 << depth) - 1;
    const int left = span * (L / 2);
    int w = tlen + span * (L - 1);
    if (w > kMraBuf) w = kMraBuf;  // (never: the host refuses such a depth; a guard against a write past the buffer)
    const T* __restrict__ src = static_cast<const T*>(b.x) + row * b.rs;
    int start = (o0 - left) % N;
    if (start < 0) start += N;
    if (start + w <= N) {
      for (int k = threadIdx.x; k < w; k += kMraThreads) buf[0][k] = src[start + k];
    } else {
      for (int k = threadIdx.x; k < w; k += kMraThreads) buf[0][k] = src[(start + k) % N];
    }
    __syncthreads();
    T* __restrict__ dst = a.out + b.index * a.out_cs + row * a.out_rs + o0;
    int cur = 0;
    for (int s = 0; s < depth; ++s) {
      const int D = 1 << (depth - 1 - s);
      const T* __restrict__ taps = (s == 0 && b.detail) ? a.hi : a.lo;
      const T* __restrict__ in = buf[cur];
      T* __restrict__ out = buf[cur ^ 1];
      const bool last = s == depth - 1;
      w -= D * (L - 1);
      for (int m = threadIdx.x; m < w; m += kMraThreads) {
        T acc = T(0);
#pragma unroll
        for (int i = 0; i < L; ++i) acc = fma(taps[i], in[m + D * (L - 1 - i)], acc);
        acc *= T(0.5);
        if (last) {
          if (m < tlen) dst[m] = acc;
        } else {
          out[m] = acc;
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }
}

// ---- 64 ------------------------------------------------------------------------------------------------------------------------------
// the window [wa, wb) of level l that the window [a, b) of level l - 1 reads
__device__ __forceinline__ void window_below(int a, int b, int len_out, int crop, int L, int S, int& wa, int& wb) {
  const int ca = crop ? floordiv(a, len_out) : 0, cb = crop ? floordiv(b - 1, len_out) : 0;
  wa = floordiv(a + ca - (L - 1) + S, 2);
  wb = floordiv(b - 1 + cb + S, 2) + 1;
}

template <typename T, int L>
__global__ __launch_bounds__(kMraThreads) void mra_dwt_kernel(const MraArgs<T> a) {
  __shared__ T buf[2][kMraDwtBuf];
  __shared__ int win[2][kMraMaxLevels + 1];
  const int N = a.n;
  const int S = a.circular ? L / 2 - 1 : L - 2;
  for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int tile = (int)(u % a.ntiles);
    const int64_t r = u / a.ntiles;
    const int c = (int)(r % a.nbands);
    const int64_t row = r / a.nbands;
    const MraBand& b = a.band[c];
    const int depth = b.depth;
    const int o0 = tile * kMraTile;
    const int tlen = min(kMraTile, N - o0);
    if (threadIdx.x == 0) {
      int wa = o0, wb = o0 + tlen;
      win[0][0] = wa, win[1][0] = wb;
      for (int l = 1; l <= depth; ++l) {
        const int crop = a.circular ? 2 * a.len[l] - a.len[l - 1] : 0;
        window_below(wa, wb, a.len[l - 1], crop, L, S, wa, wb);
        if (wb - wa > kMraDwtBuf) wb = wa + kMraDwtBuf;  // (never: the host refuses such a table; a guard against a write past the buffer)
        win[0][l] = wa, win[1][l] = wb;
      }
    }
    __syncthreads();
    {
      const int wa = win[0][depth], w = win[1][depth] - wa, len = a.len[depth];
      const T* __restrict__ src = static_cast<const T*>(b.x) + row * b.rs;
      if (wa >= 0 && wa + w <= len) {
        for (int k = threadIdx.x; k < w; k += kMraThreads) buf[0][k] = src[wa + k];
      } else if (a.circular) {
        int start = wa % len;
        if (start < 0) start += len;
        for (int k = threadIdx.x; k < w; k += kMraThreads) buf[0][k] = src[(start + k) % len];
      } else {
        for (int k = threadIdx.x; k < w; k += kMraThreads) {
          const int p = wa + k;
          buf[0][k] = (p >= 0 && p < len) ? src[p] : T(0);
        }
      }
    }
    __syncthreads();
    T* __restrict__ dst = a.out + b.index * a.out_cs + row * a.out_rs;
    int cur = 0;
    for (int l = depth; l >= 1; --l) {
      const T* __restrict__ taps = (l == depth && b.detail) ? a.hi : a.lo;
      T even[L / 2], odd[L / 2];  // the stage's taps, in registers for its whole loop
#pragma unroll
      for (int i = 0; i < L / 2; ++i) even[i] = taps[2 * i], odd[i] = taps[2 * i + 1];
      const T* __restrict__ in = buf[cur];
      T* __restrict__ out = buf[cur ^ 1];
      const int ia = win[0][l];  // where the input window starts
      const int oa = win[0][l - 1], ow = win[1][l - 1] - oa;
      const int len_out = a.len[l - 1];
      const int crop = a.circular ? 2 * a.len[l] - len_out : 0;
      const bool inside = oa >= 0 && oa + ow <= len_out;
      for (int m = threadIdx.x; m < ow; m += kMraThreads) {
        const int p = oa + m;
        T acc = T(0);
        bool present = true;
        int base = p + S;
        if (!inside) {
          if (a.circular)
            base += crop ? floordiv(p, len_out) : 0;
          else
            present = p >= 0 && p < len_out;
        }
        if (present) {
          const int t0 = base & 1;
          const int k0 = ((base - t0) >> 1) - ia;  // the input of tap t0; tap t0 + 2 i reads k0 - i, inside the window by its formulas
#pragma unroll
          for (int i = 0; i < L / 2; ++i) acc = fma(t0 ? odd[i] : even[i], in[k0 - i], acc);
        }
        if (l == 1)
          dst[p] = acc;
        else
          out[m] = acc;
      }
      __syncthreads();
      cur ^= 1;
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
int swt_max_depth(int flen) {
  int d = 0;
  while (d < kMraMaxLevels && (((int64_t)1 << (d + 1)) - 1) * (flen - 1) <= kMraBuf - kMraTile) ++d;
  return d;
}

template <typename T>
int fill_args(MraArgs<T>& a, int flen, int64_t rows, int64_t n, const mifwt_mra_band* bands, int nbands, void* out, int64_t out_cs,
              int64_t out_rs, const double* lo, const double* hi, int max_depth) {
  for (int i = 0; i < nbands; ++i) {
    const mifwt_mra_band& s = bands[i];
    if (s.x == nullptr || s.index < 0 || s.depth < 1) return MIFWT_ERR_BADARG;
    if (s.depth > max_depth) return MIFWT_ERR_UNSUPPORTED;
    a.band[i] = {s.x, s.row_stride, s.index, s.depth, s.detail ? 1 : 0, 0};
  }
  for (int t = 0; t < flen; ++t) a.lo[t] = (T)lo[t], a.hi[t] = (T)hi[t];
  a.out = static_cast<T*>(out), a.out_cs = out_cs, a.out_rs = out_rs;
  a.nbands = nbands, a.n = (int32_t)n, a.flen = flen;
  a.ntiles = (int32_t)((n + kMraTile - 1) / kMraTile);
  a.units = (int64_t)a.ntiles * nbands * rows;
  return MIFWT_OK;
}

int check_common(int dtype, int flen, int64_t rows, int64_t n, const mifwt_mra_band* bands, int nbands, const void* out, const double* lo,
                 const double* hi) {
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return dtype == MIFWT_F16 || dtype == MIFWT_BF16 ? MIFWT_ERR_UNSUPPORTED : MIFWT_ERR_BADARG;
  if (flen < 2 || (flen & 1) || bands == nullptr || out == nullptr || lo == nullptr || hi == nullptr) return MIFWT_ERR_BADARG;
  if (nbands < 1 || rows < 0 || n < 1) return MIFWT_ERR_BADARG;
  if (flen > kMraMaxFilt || nbands > kMraMaxBands || n > kMraMaxN || rows > kMraMaxN) return MIFWT_ERR_UNSUPPORTED;
  return MIFWT_OK;
}

inline unsigned grid_of(int64_t units) { return (unsigned)(units < 0x7fffffffll ? units : 0x7fffffffll); }

template <typename T, int L>
void launch_swt(const MraArgs<T>& a, hipStream_t st) {
  hipLaunchKernelGGL((mra_swt_kernel<T, L>), dim3(grid_of(a.units)), dim3(kMraThreads), 0, st, a);
}

template <typename T>
int run_swt(int flen, int64_t rows, int64_t n, const mifwt_mra_band* bands, int nbands, void* out, int64_t out_cs, int64_t out_rs,
            const double* lo, const double* hi, hipStream_t st) {
  MraArgs<T> a = {};
  const int rc = fill_args(a, flen, rows, n, bands, nbands, out, out_cs, out_rs, lo, hi, swt_max_depth(flen));
  if (rc != MIFWT_OK) return rc;
  if (a.units == 0) return MIFWT_OK;
  switch (flen) {
    case 2: launch_swt<T, 2>(a, st); break;
    case 4: launch_swt<T, 4>(a, st); break;
    case 6: launch_swt<T, 6>(a, st); break;
    case 8: launch_swt<T, 8>(a, st); break;
    case 10: launch_swt<T, 10>(a, st); break;
    case 12: launch_swt<T, 12>(a, st); break;
    case 14: launch_swt<T, 14>(a, st); break;
    case 16: launch_swt<T, 16>(a, st); break;
    case 18: launch_swt<T, 18>(a, st); break;
    default: launch_swt<T, 20>(a, st); break;
  }
  return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
}

// an upper bound of the window of level l (the device's formulas, for a tile anywhere): MIFWT_OK if every level fits the buffer
int dwt_windows_fit(int flen, int circular, const int64_t* len, int depth) {
  int64_t w = len[0] < kMraTile ? len[0] : kMraTile;
  for (int l = 1; l <= depth; ++l) {
    const int64_t crop = circular ? 2 * len[l] - len[l - 1] : 0;
    w = ((w * (len[l - 1] + crop) + len[l - 1] - 1) / len[l - 1] + 1) / 2 + flen / 2 + 2;
    if (w > kMraDwtBuf) return MIFWT_ERR_UNSUPPORTED;
  }
  return MIFWT_OK;
}

template <typename T, int L>
void launch_dwt(const MraArgs<T>& a, hipStream_t st) {
  hipLaunchKernelGGL((mra_dwt_kernel<T, L>), dim3(grid_of(a.units)), dim3(kMraThreads), 0, st, a);
}

template <typename T>
int run_dwt(int flen, int circular, int64_t rows, const int64_t* len, int nlevels, const mifwt_mra_band* bands, int nbands, void* out,
            int64_t out_cs, int64_t out_rs, const double* lo, const double* hi, hipStream_t st) {
  MraArgs<T> a = {};
  const int rc = fill_args(a, flen, rows, len[0], bands, nbands, out, out_cs, out_rs, lo, hi, nlevels);
  if (rc != MIFWT_OK) return rc;
  for (int l = 0; l <= nlevels; ++l) a.len[l] = (int32_t)len[l];
  a.circular = circular ? 1 : 0;
  if (a.units == 0) return MIFWT_OK;
  switch (flen) {
    case 2: launch_dwt<T, 2>(a, st); break;
    case 4: launch_dwt<T, 4>(a, st); break;
    case 6: launch_dwt<T, 6>(a, st); break;
    case 8: launch_dwt<T, 8>(a, st); break;
    case 10: launch_dwt<T, 10>(a, st); break;
    case 12: launch_dwt<T, 12>(a, st); break;
    case 14: launch_dwt<T, 14>(a, st); break;
    case 16: launch_dwt<T, 16>(a, st); break;
    case 18: launch_dwt<T, 18>(a, st); break;
    default: launch_dwt<T, 20>(a, st); break;
  }
  return hipGetLastError() == hipSuccess ? MIFWT_OK : MIFWT_ERR_LAUNCH;
}

}  // namespace
}  // namespace mifwt

using namespace mifwt;

extern "C" int64_t mifwt_mra_tile(void) { return kMraTile; }

extern "C" int mifwt_mra_max_bands(void) { return kMraMaxBands; }

extern "C" int mifwt_mra_max_depth(int dtype, int filt_len, int transform) {
  if (transform != MIFWT_MRA_SWT && transform != MIFWT_MRA_DWT) return MIFWT_ERR_BADARG;
  if (filt_len < 2 || (filt_len & 1)) return MIFWT_ERR_BADARG;
  if (dtype != MIFWT_F32 && dtype != MIFWT_F64) return dtype == MIFWT_F16 || dtype == MIFWT_BF16 ? 0 : MIFWT_ERR_BADARG;
  if (filt_len > kMraMaxFilt) return 0;
  return transform == MIFWT_MRA_SWT ? swt_max_depth(filt_len) : kMraMaxLevels;
}

extern "C" int mifwt_mra_swt(int dtype, int filt_len, int64_t rows, int64_t n, const mifwt_mra_band* bands, int nbands, void* out,
                             int64_t out_comp_stride, int64_t out_row_stride, const double* rec_lo, const double* rec_hi, void* stream) {
  const int rc = check_common(dtype, filt_len, rows, n, bands, nbands, out, rec_lo, rec_hi);
  if (rc != MIFWT_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MIFWT_F64) return run_swt<double>(filt_len, rows, n, bands, nbands, out, out_comp_stride, out_row_stride, rec_lo, rec_hi, st);
  return run_swt<float>(filt_len, rows, n, bands, nbands, out, out_comp_stride, out_row_stride, rec_lo, rec_hi, st);
}

extern "C" int mifwt_mra_dwt(int dtype, int filt_len, int circular, int64_t rows, const int64_t* level_len, int nlevels,
                             const mifwt_mra_band* bands, int nbands, void* out, int64_t out_comp_stride, int64_t out_row_stride,
                             const double* rec_lo, const double* rec_hi, void* stream) {
  if (level_len == nullptr || nlevels < 1) return MIFWT_ERR_BADARG;
  if (nlevels > kMraMaxLevels) return MIFWT_ERR_UNSUPPORTED;
  int rc = check_common(dtype, filt_len, rows, level_len[0], bands, nbands, out, rec_lo, rec_hi);
  if (rc != MIFWT_OK) return rc;
  for (int l = 1; l <= nlevels; ++l) {  // the lengths of one decomposition: a level is the full synthesis of the one below or one sample less
    if (level_len[l] < 1 || level_len[l] > kMraMaxN) return MIFWT_ERR_BADARG;
    const int64_t full = circular ? 2 * level_len[l] : 2 * level_len[l] - filt_len + 2;
    if (level_len[l - 1] != full && level_len[l - 1] != full - 1) return MIFWT_ERR_BADARG;
  }
  int deepest = 0;
  for (int i = 0; i < nbands; ++i) deepest = bands[i].depth > deepest ? bands[i].depth : deepest;
  if (deepest > nlevels) return MIFWT_ERR_BADARG;
  rc = dwt_windows_fit(filt_len, circular, level_len, deepest);
  if (rc != MIFWT_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MIFWT_F64)
    return run_dwt<double>(filt_len, circular, rows, level_len, nlevels, bands, nbands, out, out_comp_stride, out_row_stride, rec_lo, rec_hi, st);
  return run_dwt<float>(filt_len, circular, rows, level_len, nlevels, bands, nbands, out, out_comp_stride, out_row_stride, rec_lo, rec_hi, st);
}
