// The 8-bit scalar quantiser's decode, shared by the flat search over codes (dense_search_sq8.hip) and the IVF scan over codes
// (ivf_flat.hip): a stored byte is c' = c - 128 for the code c in 0 .. 255, and a value decodes with ONE rounding.
#pragma once
#include "rc_common.h"

__device__ __forceinline__ float dense_sq8_decode(signed char c, float step, float mid) {
    return __builtin_fmaf((float)c, step, mid);
}
