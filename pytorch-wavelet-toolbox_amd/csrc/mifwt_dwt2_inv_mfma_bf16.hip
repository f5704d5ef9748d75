// mifwt_dwt2_inv_mfma_bf16.hip — matrix-core 2-D synthesis level (mifwt_dwt2_inv_mfma.h), id 23: the __bf16 instantiation.
#include "mifwt_dwt2_inv_mfma.h"

namespace mifwt {

int dwt2_inv_mfma_bf16(const mifwt_level_desc* d, const void* approx, const void* const* details, void* y, const double* lo,
                       const double* hi, hipStream_t stream) {
  return dwt2_inv_mfma_launch<__bf16>(d, approx, details, y, lo, hi, stream);
}

}  // namespace mifwt
