// mifwt_dwt2_fwd_tile_long24.hip — LDS-tile 2-D analysis kernel (mifwt_dwt2_tile.h): 24-tap filters, f32, f16 and bf16 storage.
#include "mifwt_dwt2_tile.h"

namespace mifwt {

int dwt2_fwd_tile_long24(const mifwt_level_desc* d, const void* x, void* approx, void* const* details, LevelTaps t,
                         BatchSplit split, hipStream_t stream) {
  if (d->dtype == MIFWT_F16) return launch_tr<_Float16, 24>(d, x, approx, details, t, split, stream);
  if (d->dtype == MIFWT_BF16) return launch_tr<__bf16, 24>(d, x, approx, details, t, split, stream);
  return launch_tr<float, 24>(d, x, approx, details, t, split, stream);
}

}  // namespace mifwt
