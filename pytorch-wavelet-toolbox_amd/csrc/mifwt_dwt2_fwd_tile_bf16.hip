// mifwt_dwt2_fwd_tile_bf16.hip — LDS-tile 2-D analysis kernel (mifwt_dwt2_tile.h): bf16 storage / f32 arithmetic, L <= 16.
#include "mifwt_dwt2_tile.h"

namespace mifwt {

int dwt2_fwd_tile_bf16_short(const mifwt_level_desc* d, const void* x, void* approx, void* const* details,
                            LevelTaps t, BatchSplit split, hipStream_t stream) {
  switch (d->filt_len) {
    case 2: return launch_tr<__bf16, 2>(d, x, approx, details, t, split, stream);
    case 4: return launch_tr<__bf16, 4>(d, x, approx, details, t, split, stream);
    case 6: return launch_tr<__bf16, 6>(d, x, approx, details, t, split, stream);
    case 8: return launch_tr<__bf16, 8>(d, x, approx, details, t, split, stream);
    case 10: return launch_tr<__bf16, 10>(d, x, approx, details, t, split, stream);
    case 12: return launch_tr<__bf16, 12>(d, x, approx, details, t, split, stream);
    case 14: return launch_tr<__bf16, 14>(d, x, approx, details, t, split, stream);
    case 16: return launch_tr<__bf16, 16>(d, x, approx, details, t, split, stream);
    default: return MIFWT_ERR_UNSUPPORTED;
  }
}

}  // namespace mifwt
