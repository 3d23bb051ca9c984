// exact_margin.h -- the bf16 rounding and the proven margin factor that the exact scan (kernels_exact.h) and multi-vector search
// (kernels_maxsim.h) share: ONE copy, because the proofs of both rest on the same numbers.
#pragma once
#include "common.h"

// two f32 -> packed bf16, round to nearest even (the rounding of asg_bf16_pair, kernels_coarse.h)
__device__ __forceinline__ uint32_t ex_bf16_pair(float lo, float hi) {
    uint32_t a = __builtin_bit_cast(uint32_t, lo), b = __builtin_bit_cast(uint32_t, hi);
    a += 0x7FFFu + ((a >> 16) & 1u);
    b += 0x7FFFu + ((b >> 16) & 1u);
    return (a >> 16) | (b & 0xFFFF0000u);
}
// c of the margin m = c (|x| + |q'|)^2 (kernels_exact.h, "Approximation"); the factor 1.05 is LOAD-BEARING: do not tighten it
__device__ __forceinline__ float ex_margin_factor(uint32_t dim) { return (0.00390625f + (float)(2 * dim + 64) * 5.9604645e-8f) * 1.05f; }
