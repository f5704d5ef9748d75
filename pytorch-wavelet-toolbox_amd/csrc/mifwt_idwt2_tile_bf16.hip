// mifwt_idwt2_tile_bf16.hip — LDS-tile 2-D synthesis kernel (mifwt_idwt2_tile.h): __bf16 storage, L <= 16.
#include "mifwt_idwt2_tile.h"

namespace mifwt {

int idwt2_tile_bf16_short(const mifwt_level_desc* d, const void* approx, const void* const* details, void* y,
                         LevelTaps t, hipStream_t stream) {
  switch (d->filt_len) {
    case 2: return launch_idwt_tr<__bf16, 2>(d, approx, details, y, t, stream);
    case 4: return launch_idwt_tr<__bf16, 4>(d, approx, details, y, t, stream);
    case 6: return launch_idwt_tr<__bf16, 6>(d, approx, details, y, t, stream);
    case 8: return launch_idwt_tr<__bf16, 8>(d, approx, details, y, t, stream);
    case 10: return launch_idwt_tr<__bf16, 10>(d, approx, details, y, t, stream);
    case 12: return launch_idwt_tr<__bf16, 12>(d, approx, details, y, t, stream);
    case 14: return launch_idwt_tr<__bf16, 14>(d, approx, details, y, t, stream);
    case 16: return launch_idwt_tr<__bf16, 16>(d, approx, details, y, t, stream);
    default: return MIFWT_ERR_UNSUPPORTED;
  }
}

}  // namespace mifwt
