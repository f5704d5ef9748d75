// mifwt_axis_stream_bf16_f.hip — streaming single-axis kernels (mifwt_axis_stream.h): __bf16 storage, L = 24.
#include "mifwt_axis_stream.h"

MIFWT_STREAM_DEFINE(bf16, __bf16, 24)
