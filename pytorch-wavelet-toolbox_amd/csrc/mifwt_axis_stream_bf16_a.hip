// mifwt_axis_stream_bf16_a.hip — streaming single-axis kernels (mifwt_axis_stream.h): __bf16 storage, L = 2, 4, 6, 8.
#include "mifwt_axis_stream.h"

MIFWT_STREAM_DEFINE(bf16, __bf16, 2)
MIFWT_STREAM_DEFINE(bf16, __bf16, 4)
MIFWT_STREAM_DEFINE(bf16, __bf16, 6)
MIFWT_STREAM_DEFINE(bf16, __bf16, 8)
