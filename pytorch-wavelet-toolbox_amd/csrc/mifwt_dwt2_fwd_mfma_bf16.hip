// mifwt_dwt2_fwd_mfma_bf16.hip — matrix-core 2-D analysis level (mifwt_dwt2_fwd_mfma.h), id 11: the __bf16 instantiation.
#include "mifwt_dwt2_fwd_mfma.h"

namespace mifwt {

int dwt2_fwd_mfma_bf16(const mifwt_level_desc* d, const void* x, void* approx, void* const* details, const double* lo,
                       const double* hi, hipStream_t stream) {
  return dwt2_fwd_mfma_launch<__bf16>(d, x, approx, details, lo, hi, stream);
}

}  // namespace mifwt
