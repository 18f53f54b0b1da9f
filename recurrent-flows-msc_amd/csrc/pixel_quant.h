// The byte of a model-space fp32 value, shared by the picture kernels (sheet.hip, clip_compose.hip):
// Solver.preprocess(x, reverse=True) (RFN/trainer.py:165-188 of the reference):
//   v = x + 0.5 (range_half) or x;  v = v * n_bins;  q = floor(v) * scale;  byte = clamp(q, 0, 255), NaN -> 0,
// with n_bins = 2^n_bits and scale = 256 / 2^n_bits, every operation rounded to fp32 on its own.  All factors are
// powers of two, so the products are exact and the result equals torch's on any device bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t rfn_quantise_u8(float x, int range_half, float n_bins, float scale) {
    float v = range_half ? __fadd_rn(x, 0.5f) : x;
    v = __fmul_rn(v, n_bins);
    const float q = __fmul_rn(floorf(v), scale);
    return (uint32_t)fminf(fmaxf(q, 0.f), 255.f);   // fmaxf(NaN, 0) = 0
}
