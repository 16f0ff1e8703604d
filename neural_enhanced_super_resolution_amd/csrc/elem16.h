// The 16-bit element of the MFMA kernels (conv3x3_mfma.hip, conv3x3_bf16.hip, rdb_bf16_strip.hip), by activation layout
// code K (PackArgs::bf16): 1 = bf16, 3 = f16.  Both store 16 channels per 32-byte K-chunk and have MFMAs of the same
// shapes, operand layouts and rate (v_mfma_f32_{32x32x16,16x16x32}_{bf16,f16}), so a kernel differs only in the builtin,
// the f32 <-> 16-bit conversions and, for f16, the range check: f16 tops out at 65504, so a kernel that stores an f16
// activation raises the context's range word (ConvArgs::status) for a value that is non-finite or beyond +-65504.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nesr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int K>
struct E16;

template <>
struct E16<1> {
    typedef __bf16 x8 __attribute__((ext_vector_type(8)));
    typedef __bf16 x4 __attribute__((ext_vector_type(4)));
    static constexpr bool RANGE = false;
    __device__ static __forceinline__ uint2 pack4(f32x4 v) {   // plain casts -> v_cvt_pk_bf16_f32 (RNE, NaN preserving)
        const x4 b = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        return __builtin_bit_cast(uint2, b);
    }
    __device__ static __forceinline__ f32x4 unpack4(uint2 u) {
        return f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
    }
    __device__ static __forceinline__ f32x16 mfma32(f32x4 a, f32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x8, a), __builtin_bit_cast(x8, b), c, 0, 0, 0);
    }
    __device__ static __forceinline__ f32x4 mfma16(f32x4 a, f32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(x8, a), __builtin_bit_cast(x8, b), c, 0, 0, 0);
    }
    __device__ static __forceinline__ unsigned amax(unsigned m, float) { return m; }
};

template <>
struct E16<3> {
    typedef _Float16 x8 __attribute__((ext_vector_type(8)));
    typedef _Float16 x4 __attribute__((ext_vector_type(4)));
    static constexpr bool RANGE = true;
    __device__ static __forceinline__ uint2 pack4(f32x4 v) {   // plain casts -> v_cvt_pk_f16_f32 (RNE, as torch's .half())
        const x4 h = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        return __builtin_bit_cast(uint2, h);
    }
    __device__ static __forceinline__ f32x4 unpack4(uint2 u) {
        const x4 h = __builtin_bit_cast(x4, u);
        return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    }
    __device__ static __forceinline__ f32x16 mfma32(f32x4 a, f32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(x8, a), __builtin_bit_cast(x8, b), c, 0, 0, 0);
    }
    __device__ static __forceinline__ f32x4 mfma16(f32x4 a, f32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(x8, a), __builtin_bit_cast(x8, b), c, 0, 0, 0);
    }
    // The range check in integer form: a lane keeps the largest |x| bit pattern of the values it stores (one VGPR, v_and +
    // v_max_u32 per value; a lane mask kept live across a kernel's main loop costs SGPRs the strip kernel does not have) and
    // compares it once with 65504's -- Inf and every NaN have larger patterns than any finite value
    __device__ static __forceinline__ unsigned amax(unsigned m, float x) { return max(m, __float_as_uint(x) & 0x7fffffffu); }
};

constexpr unsigned F16_MAX_BITS = 0x477fe000u;   // 65504.0f

// the range word: a lane-divergent vector store by every lane that stored a value f16 cannot carry (never a scalar store)
__device__ __forceinline__ void raise_range(unsigned* status, unsigned amax_bits) {
    if (amax_bits > F16_MAX_BITS && status) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace nesr
