// Shared pieces of the f16-pair kernels (conv3x3_f16x2.hip, rdb_f16x2.hip, upconv2x2_f16x2.hip): vector types, the
// LDS-DMA issue, the (hi, scaled lo) split of an f32 value, the whole-line regrouping of the 16x16x32 epilogue and, for
// the two 3x3 kernels, the tile geometry, the tap address plan and a tap-step's MFMAs.
#pragma once
#include "nesr_kernels.h"

namespace nesr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char lds_char;

namespace {

// LDS-DMA from inline asm (see conv3x3_bf16.hip): not counted by hipcc, waited for by hand; scalar 64-bit base and an
// unsigned 32-bit per-lane byte offset
__device__ __forceinline__ void glds16_s(const char* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}
// Plain (write-back) stores: every workgroup of a layer reaches its epilogue at about the same time, and
// the write-through form (sc1) that helps the Winograd kernel made this burst 3x longer here
// (in-kernel stamps: 12.4k -> 3.7k cycles per epilogue; -4 % / -6 % forward time on 1 / 6 tiles).
__device__ __forceinline__ void store16(uint16_t* p, uint4 v) {
#ifdef NESR_SC1_STORES
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(__builtin_bit_cast(f32x4, v)) : "memory");
#else
    *reinterpret_cast<uint4*>(p) = v;
#endif
}

constexpr float LO_SCALE = 2048.f, LO_INV = 1.f / 2048.f;   // lo is stored as f16((x - hi) * 2^11)

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// two values -> packed (hi, hi), (lo, lo) halves.  hi = f16(x) (round to nearest even), lo = f16((x - hi) * 2^11):
// x - hi is exact in f32 and so is the scaling, hence fma(hi, -2^11, x * 2^11) is that value bit for bit.  A value that
// does not fit (|x| >= 65520, Inf, NaN) makes hi Inf / NaN: `badbits` collects the all-ones exponent fields (bit 15 of a
// half after adding 0x0400 to its masked exponent), so nothing is clamped -- a non-finite half poisons the sums it enters,
// the sticky flag is raised and conv_last writes NaN.
__device__ __forceinline__ void split2(float x0, float x1, unsigned& hi, unsigned& lo, unsigned& badbits) {
    const f32x2 x = {x0, x1};
    const f16x2 h = __builtin_convertvector(x, f16x2);                        // v_cvt_pk_f16_f32
    const f32x2 hf = __builtin_convertvector(h, f32x2);
    const f32x2 d = __builtin_elementwise_fma(hf, f32x2{-LO_SCALE, -LO_SCALE}, x * LO_SCALE);   // packed f32 mul / fma
    const f16x2 l = __builtin_convertvector(d, f16x2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
    badbits |= (hi & 0x7C007C00u) + 0x04000400u;
}
// x -> (hi, scaled lo) halves of 4 values; `bad` collects "does not fit the pair" (|x| >= 65520, NaN, Inf)
__device__ __forceinline__ void split4(f32x4 v, uint2& hi, uint2& lo, bool& bad) {
    unsigned bits = 0;
    split2(v[0], v[1], hi.x, lo.x, bits);
    split2(v[2], v[3], hi.y, lo.y, bits);
    bad |= (bits & 0x80008000u) != 0u;
}


// ---- whole-line feature-map access for the 16x16x32 epilogue.  After the cout exchange lane (pixel j16, k-group g4)
// holds 8 consecutive couts of ONE pixel: base 0 / 16 / 8 / 24 for g4 = 0 / 1 / 2 / 3, i.e. piece g4>>1 (8 channels)
// of chunk X (g4 even) or X + 1 (g4 odd), as a hi and a lo 16-byte piece.  Stored like that, a wave instruction
// would write 16-byte fragments of 64 different 64-byte slots (measured: ~4.6 us per epilogue, the stores crawl
// through the address coalescer).  One v_permlane16_swap per register (odd rows of `hi` <-> even rows of `lo`)
// regroups the pieces by CHUNK: afterwards `hi` holds, for every lane, a piece of chunk X -- piece index
// 2 (g4 & 1) + (g4 >> 1) of the pixel's 64-byte slot [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15] -- and `lo` the same piece
// of chunk X + 1: two store instructions of 16 pixels x 64 bytes = 1 KiB of whole lines each.  The swap is its own
// inverse, so residuals are loaded the same way.  All 64 lanes must execute these (no divergence around them).
__device__ __forceinline__ void regroup_pairs(uint4& hi, uint4& lo) {
    auto s0 = __builtin_amdgcn_permlane16_swap(hi.x, lo.x, false, false);
    auto s1 = __builtin_amdgcn_permlane16_swap(hi.y, lo.y, false, false);
    auto s2 = __builtin_amdgcn_permlane16_swap(hi.z, lo.z, false, false);
    auto s3 = __builtin_amdgcn_permlane16_swap(hi.w, lo.w, false, false);
    hi = uint4{s0[0], s1[0], s2[0], s3[0]};
    lo = uint4{s0[1], s1[1], s2[1], s3[1]};
}
// v0, v1 = this lane's 8 couts -> split, regrouped: `cx` goes to chunk X, `cx1` to chunk X + 1 (at piece offset)
__device__ __forceinline__ void split_regroup(f32x4 v0, f32x4 v1, uint4& cx, uint4& cx1, bool& bad) {
    uint2 h0, l0, h1, l1;
    split4(v0, h0, l0, bad);
    split4(v1, h1, l1, bad);
    cx = uint4{h0.x, h0.y, h1.x, h1.y};
    cx1 = uint4{l0.x, l0.y, l1.x, l1.y};
    regroup_pairs(cx, cx1);
}
// the inverse for residuals: p = the pixel's slot in chunk X (2-byte units), piece8 = this lane's piece offset
__device__ __forceinline__ void load_regrouped(const uint16_t* p, long long chunk_el, f32x4& q0, f32x4& q1) {
    uint4 cx = *reinterpret_cast<const uint4*>(p);
    uint4 cx1 = *reinterpret_cast<const uint4*>(p + chunk_el);
    regroup_pairs(cx, cx1);      // -> own hi, own lo
    const f16x8 h = __builtin_bit_cast(f16x8, cx), l = __builtin_bit_cast(f16x8, cx1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        q0[i] = fmaf((float)l[i], LO_INV, (float)h[i]);
        q1[i] = fmaf((float)l[4 + i], LO_INV, (float)h[4 + i]);
    }
}

// ---- the 3x3 kernels.  Per-layer (conv3x3_f16x2_kernel): 4 MFMA waves x 2 rows; fused (rdb_f16x2_kernel): Geo<4>'s
// input tile and DMA rounds, 8 MFMA waves x 1 row.  Both: output tile 8 rows x 32 cols, 32-cout weight slabs.
constexpr int TW = 32, PW = TW + 2;
constexpr int WAVES = 4;   // MFMA waves per workgroup of the per-layer kernel
constexpr int RW = 2;      // rows per MFMA wave of the per-layer kernel
// DMAW = extra waves that only issue the LDS-DMAs (0: the MFMA waves issue them themselves)
template <int DMAW>
struct Geo {
    static constexpr int LAUNCH_THREADS = 64 * (WAVES + DMAW);
    static constexpr int THREADS = 64 * (DMAW ? DMAW : WAVES);   // lanes that share one DMA round
    static constexpr int TH = WAVES * RW;
    static constexpr int PH = TH + 2;
    static constexpr int NPIX = PH * PW;
    static constexpr int IN_ITEMS = 4 * NPIX;   // 16-byte items per input slot
    static constexpr int IN_ROUNDS = (IN_ITEMS + THREADS - 1) / THREADS;
    static constexpr int IN_BYTES = IN_ITEMS * 16;
};
constexpr int W_ITEMS = 9 * 2 * 2 * 32;   // 16-byte items of one 32-cout weight slab (per K-chunk)
constexpr int W_BYTES = W_ITEMS * 16;

// The tap address plan (the five tap-steps: conv3x3_f16x2_kernel, "operands") for lane (j16, un, kh) of a wave whose first
// tile row is `row`: byte offset of its XH fragment of tap-step st_, pixel half nh, in an input slot / of its WH fragment
// in a weight slab.  (The st_ / nh loops stay in the kernels: moved in here, the per-layer kernel's instructions change.)
__device__ __forceinline__ int tap_pixel_offset(int st_, int row, int nh, int j16, int un, int kh) {
    const int dy = st_ < 3 ? un : 2;
    const int dx = st_ < 3 ? st_ : (st_ == 3 ? un : 2);
    const int col = 16 * nh + j16 + dx;
    return ((row + dy) * PW + col) * 64 + ((kh ^ (((col >> 2) & 1) << 1)) << 4);
}
__device__ __forceinline__ int tap_weight_offset(int st_, int j16, int un, int kh) {
    const int dy = st_ < 3 ? un : 2;
    const int dx = st_ < 3 ? st_ : (st_ == 3 ? un : 2);
    return ((((dy * 3 + dx) * 2) * 2 + kh) * 32 + j16) * 16;
}
// One tap-step's MFMAs for one (cout half, pixel half), a0 | a1 = WH | WL, x0 | x1 = XH | XL: tap-steps 0..3
__device__ __forceinline__ void mfma_tap3(f16x8 a0, f16x8 a1, f16x8 x0, f16x8 x1, f32x4& mn, f32x4& cr) {
    cr = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, x1, cr, 0, 0, 0);
    mn = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, x0, mn, 0, 0, 0);
    cr = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, x0, cr, 0, 0, 0);
}
// the last tap alone (a0 = [w_hi | 0], a1 = [w_hi | w_lo], x0 = [x_hi | x_hi], x1 = [x_lo | x_hi])
__device__ __forceinline__ void mfma_tap2(f16x8 a0, f16x8 a1, f16x8 x0, f16x8 x1, f32x4& mn, f32x4& cr) {
    mn = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, x0, mn, 0, 0, 0);
    cr = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, x1, cr, 0, 0, 0);
}
// The cout exchange.  C/D layout: lane (pixel j16, k-group g4) holds couts 16 mt + 4 g4 + i; v_permlane16_swap of the
// mt = 0 (e) / mt = 1 (o) values leaves every lane with 8 consecutive couts of its pixel, v0 | v1 = base .. +3 | +4 .. +7,
// base 0 / 16 / 8 / 24 for g4 = 0 / 1 / 2 / 3 (tools/probes/mfma16_layout.hip).  All 64 lanes.
__device__ __forceinline__ void cout_exchange(f32x4 e, f32x4 o, f32x4& v0, f32x4& v1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const auto sw_ = __builtin_amdgcn_permlane16_swap(__float_as_uint(e[i]), __float_as_uint(o[i]), false, false);
        v0[i] = __uint_as_float(sw_[0]);
        v1[i] = __uint_as_float(sw_[1]);
    }
}
// the same from the [main | cross] accumulators of the two cout halves: value = main + cross / 2^11
__device__ __forceinline__ void cout_exchange_acc(const f32x4 (&ae)[2], const f32x4 (&ao)[2], f32x4& v0, f32x4& v1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float e = fmaf(ae[1][i], LO_INV, ae[0][i]);
        const float o = fmaf(ao[1][i], LO_INV, ao[0][i]);
        const auto sw_ = __builtin_amdgcn_permlane16_swap(__float_as_uint(e), __float_as_uint(o), false, false);
        v0[i] = __uint_as_float(sw_[0]);
        v1[i] = __uint_as_float(sw_[1]);
    }
}

inline uint16_t f2h(float f) {
    const _Float16 h = (_Float16)f;
    return __builtin_bit_cast(uint16_t, h);
}
inline float h2f(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }

}  // namespace
}  // namespace nesr
