// mifwt_axis_stream_bf16_c.hip — streaming single-axis kernels (mifwt_axis_stream.h): __bf16 storage, L = 14, 16.
#include "mifwt_axis_stream.h"

MIFWT_STREAM_DEFINE(bf16, __bf16, 14)
MIFWT_STREAM_DEFINE(bf16, __bf16, 16)
