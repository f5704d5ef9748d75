// mifwt_idwt2_tile_long_b.hip — LDS-tile 2-D synthesis kernel (mifwt_idwt2_tile.h): 24- and 32-tap filters, f32 / f16 / bf16.
#include "mifwt_idwt2_tile.h"

namespace mifwt {

int idwt2_tile_long_b(const mifwt_level_desc* d, const void* approx, const void* const* details, void* y,
                          LevelTaps t, hipStream_t stream) {
  switch (d->filt_len) {
    case 24:
      if (d->dtype == MIFWT_BF16) return launch_idwt_tr<__bf16, 24>(d, approx, details, y, t, stream);
      return d->dtype == MIFWT_F16 ? launch_idwt_tr<_Float16, 24>(d, approx, details, y, t, stream)
                                   : launch_idwt_tr<float, 24>(d, approx, details, y, t, stream);
    case 32:
      if (d->dtype == MIFWT_BF16) return launch_idwt_tr<__bf16, 32>(d, approx, details, y, t, stream);
      return d->dtype == MIFWT_F16 ? launch_idwt_tr<_Float16, 32>(d, approx, details, y, t, stream)
                                   : launch_idwt_tr<float, 32>(d, approx, details, y, t, stream);
    default: return MIFWT_ERR_UNSUPPORTED;
  }
}

}  // namespace mifwt
