// mifwt_axis_stream_bf16_b.hip — streaming single-axis kernels (mifwt_axis_stream.h): __bf16 storage, L = 10, 12.
#include "mifwt_axis_stream.h"

MIFWT_STREAM_DEFINE(bf16, __bf16, 10)
MIFWT_STREAM_DEFINE(bf16, __bf16, 12)
