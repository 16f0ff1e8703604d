// Element conversions of the input packers (pack.hip, nesr12.hip): f32 -> the stored element of each activation layout
// (PackArgs::bf16) and back.  Not part of the public ABI.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nesr {

__device__ inline uint16_t f2bf(float f) {
    __hip_bfloat16 b = __float2bfloat16(f);
    return *reinterpret_cast<uint16_t*>(&b);
}
__device__ inline float bf2f(uint16_t u) { return __uint_as_float(((unsigned)u) << 16); }
// f32 -> (hi, lo) half pair of the f16x2 path, x = hi + lo * 2^-11 (conv3x3_f16x2.hip); returns false if x
// does not fit (|x| > 65504, NaN, Inf: clamped, and the caller raises the context's sticky range flag)
__device__ inline bool f2hl(float f, uint16_t& hi, uint16_t& lo) {
    const float x = fminf(fmaxf(f, -65504.f), 65504.f);
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)((x - (float)h) * 2048.f);
    hi = __builtin_bit_cast(uint16_t, h);
    lo = __builtin_bit_cast(uint16_t, l);
    return __builtin_fabsf(f) <= 65504.f;
}
__device__ inline float hl2f(uint16_t hi, uint16_t lo) {
    return fmaf((float)__builtin_bit_cast(_Float16, lo), 1.f / 2048.f, (float)__builtin_bit_cast(_Float16, hi));
}

}  // namespace nesr
