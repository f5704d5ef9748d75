// mifwt_dwt2_inv_mfma.hip — matrix-core 2-D synthesis level (mifwt_dwt2_inv_mfma.h), id 23: the envelope, the _Float16 instantiation and
// the dispatch on the 16-bit storage type.
#include "mifwt_dwt2_inv_mfma.h"

namespace mifwt {

int dwt2_inv_mfma_bf16(const mifwt_level_desc*, const void*, const void* const*, void*, const double*, const double*, hipStream_t);  // (mifwt_dwt2_inv_mfma_bf16.hip)

bool dwt2_inv_mfma_supported(const mifwt_level_desc* d) {
  if (d->ndim != 2 || !is_storage16(d->dtype) || g_options[MIFWT_OPT_MFMA_MODE] == 2) return false;
  const int L = d->filt_len;
  if (L < 18 || L > 32 || (L & 1)) return false;
  if (d->sig_stride[2] != 1 || d->approx_stride[2] != 1 || d->detail_stride[2] != 1) return false;
  for (int i = 0; i < 2; ++i)
    if (d->approx_stride[i] < 0 || d->detail_stride[i] < 0 || d->sig_stride[i] < 0) return false;
  const int64_t lim = int64_t(1) << 29;  // 32-bit byte offsets inside a plane
  if ((d->coef_extent[0] - 1) * d->approx_stride[1] + d->coef_extent[1] >= lim) return false;
  if ((d->coef_extent[0] - 1) * d->detail_stride[1] + d->coef_extent[1] >= lim) return false;
  for (int ax = 0; ax < 2; ++ax)
    if (d->sig_extent[ax] < 1 || d->sig_extent[ax] > 2 * d->coef_extent[ax] - L + 2) return false;
  // where it pays: wherever there is a tile per workgroup or so (32 x 542^2 sym16: 0.026 against 0.205 ms for the vector tile kernel,
  // 32 x 1052^2: 0.049 against 0.172, tools/c5_rec_time.py; MIFWT_OPT_MFMA_MODE 4: always)
  // The threshold looks at ONE image's tiles, never at the batch: this kernel rounds the intermediate image to f16, the vector tile
  // kernel keeps it in f32 — a batch and its images one by one must take the same path to agree to the bit.
  const int64_t tiles_per_image = ((d->sig_extent[0] + kSOR - 1) / kSOR) * ((d->sig_extent[1] + kSOC - 1) / kSOC);
  return g_options[MIFWT_OPT_MFMA_MODE] == 4 || tiles_per_image >= 4;
}

int dwt2_inv_mfma(const mifwt_level_desc* d, const void* approx, const void* const* details, void* y, const double* lo,
                  const double* hi, hipStream_t stream) {
  if (d->dtype == MIFWT_BF16) return dwt2_inv_mfma_bf16(d, approx, details, y, lo, hi, stream);
  return dwt2_inv_mfma_launch<_Float16>(d, approx, details, y, lo, hi, stream);
}

}  // namespace mifwt
