// mifwt_dwt2_fwd_mfma.hip — matrix-core 2-D analysis level (mifwt_dwt2_fwd_mfma.h), id 11: the envelope, the _Float16 instantiation and
// the dispatch on the 16-bit storage type.
#include "mifwt_dwt2_fwd_mfma.h"

namespace mifwt {

int dwt2_fwd_mfma_bf16(const mifwt_level_desc*, const void*, void*, void* const*, const double*, const double*, hipStream_t);  // (mifwt_dwt2_fwd_mfma_bf16.hip)

bool dwt2_fwd_mfma_supported(const mifwt_level_desc* d) {
  if (d->ndim != 2 || !is_storage16(d->dtype)) return false;
  const int L = d->filt_len;
  if (L < 18 || L > 32 || (L & 1)) return false;
  if (d->sig_stride[2] != 1 || d->approx_stride[2] != 1 || d->detail_stride[2] != 1) return false;
  const int64_t span = (d->sig_extent[0] - 1) * d->sig_stride[1] + d->sig_extent[1];
  if (d->sig_stride[1] < 0 || span >= (int64_t(1) << 29)) return false;
  for (int i = 0; i < 2; ++i)
    if (d->approx_stride[i] < 0 || d->detail_stride[i] < 0) return false;
  if (d->sig_extent[0] < L || d->sig_extent[1] < L) return false;  // single-fold boundary map
  return true;
}

int dwt2_fwd_mfma(const mifwt_level_desc* d, const void* x, void* approx, void* const* details, const double* lo,
                  const double* hi, hipStream_t stream) {
  if (d->dtype == MIFWT_BF16) return dwt2_fwd_mfma_bf16(d, x, approx, details, lo, hi, stream);
  return dwt2_fwd_mfma_launch<_Float16>(d, x, approx, details, lo, hi, stream);
}

}  // namespace mifwt
