// SRVGGNetCompact (Real-ESRGAN's compact network, upstream realesrgan/archs/srvgg_arch.py) as HIP kernels for gfx950:
//
//   body = conv3x3(in, 64), act, (conv3x3(64, 64), act) x num_conv, conv3x3(64, out * s * s)
//   out  = pixel_shuffle(body(x), s) + nearest_upsample(x, s)
//
// Three kernels, one launch per layer (no inter-workgroup waits):
//   compact_pack_kernel  : NCHW f32 or u8 HWC (/255, optional BGR<->RGB) -> the first conv's input (NHWC, 32 channels, zero
//                          padded) and an f32 NHWC copy of the image for the tail's residual
//   compact_conv_kernel  : one 3x3 / stride 1 / zero-pad 1 conv, Cin 32 | 64 -> 64, bias, and the activation as a per-channel
//                          slope (PReLU: the checkpoint's slopes, ReLU 0, LeakyReLU 0.1).  With TAIL the last conv instead:
//                          64 -> out * s^2, pixel shuffle and the nearest-upsampled input added in the epilogue, every LR pixel
//                          writing its s x s block of the NCHW f32 result or of the u8 HWC image (clamp, x255, round | trunc)
//
// Operand forms (FORM template parameter, the activation layout codes of elem16.h plus the pair form):
//   bf16  : activations NHWC bf16, v_mfma_f32_16x16x32_bf16, f32 accumulation
//   f16   : bf16's kernel on f16 elements (E16<3>: v_mfma_f32_16x16x32_f16, round to nearest even as torch's .half()).  f16 tops
//           out at 65504, so the split form's range contract holds: the pack kernel checks the image it stages, every layer that
//           stores an f16 activation keeps the largest |x| bit pattern it stored in one VGPR and raises the range word once, and
//           the tail, which reads the word as it does for the split form, then writes NaN everywhere
//   split : the project's f32 form: activations NHWC f32; on the way into LDS every value becomes a pair of halves
//           x = hi + lo 2^-11 and each product is three v_mfma_f32_16x16x32_f16 (hi*hi into one accumulator, hi*lo + lo*hi into a
//           second one scaled by 2^-11 at the end).  A value beyond +-65504 or non-finite sets the sticky range word instead
//           of saturating: the first conv checks the image as it stages it, every feature layer checks the activations it
//           writes, so when the tail starts the word covers every value it or an earlier layer read; the tail then writes
//           NaN everywhere (nesr_check_range reports NESR_ERR_RANGE).
//
// Tiling: 4 waves, a wave owns WR output rows x 32 columns (two 16-pixel MFMA blocks) x all output channels; the MFMA A operand
// is the weights (16 output channels), B the pixels, so a lane's accumulator holds 4 consecutive channels of one pixel.  For
// one horizontal tap dx a wave reads the WR + 2 input rows it needs once and uses each fragment for up to three vertical taps.
// The (4 WR + 2) x 34 input tile sits in LDS with its 16-byte chunks XOR-swizzled by pixel (conflict-free ds_read_b128).
//   bf16, f16 : WR = 4 (16 x 32 tiles); the layer's weights (73.7 KB) stay resident in LDS and a grid of one workgroup per CU walks
//           the tiles, so weights are read once per CU and layer
//   split : WR = 2 (8 x 32 tiles); the f16-pair weights (147 KB) do not fit beside a tile, so the three taps of one column dx
//           (49 KB) are streamed into LDS per dx
#include <hip/hip_bf16.h>

#include "compact_api.h"
#include "elem16.h"

namespace nesr {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int TW = 32, PW = TW + 2, NWAVES = 4, THREADS = 64 * NWAVES;
constexpr int NF = 64;   // feature channels (num_feat)

template <bool SPLIT>
struct Form {
    static constexpr int WR = SPLIT ? 2 : 4;          // output rows per wave
    static constexpr int TH = NWAVES * WR;
    static constexpr int PH = TH + 2;
    static constexpr int NPIX = PH * PW;
    static constexpr int FRAG = SPLIT ? 2048 : 1024;  // bytes of one weight fragment (16 couts x 32 cin x 64 lanes' layout; hi|lo)
};

// LDS bytes of one padded pixel: Cin values as bf16, or Cin hi halves then Cin lo halves
template <bool SPLIT, int CIN>
constexpr int pix_bytes() { return SPLIT ? CIN * 4 : CIN * 2; }

// 16-byte chunk c of padded pixel p -> LDS byte offset (chunk index XOR-swizzled with the pixel's low bits)
template <bool SPLIT, int CIN>
__device__ __forceinline__ int lds_off(int p, int c) {
    constexpr int NCH = pix_bytes<SPLIT, CIN>() / 16;
    constexpr int SW = (NCH < 8 ? NCH : 8) - 1;
    return p * pix_bytes<SPLIT, CIN>() + ((c ^ (p & SW)) << 4);
}

__device__ __forceinline__ uint4 split_hi_lo(const float* v, uint4& lo_out, unsigned& bad) {
    _Float16 hi[8], lo[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = v[i];
        bad |= !(fabsf(x) <= 65504.f);
        const _Float16 h = (_Float16)x;
        hi[i] = h;
        lo[i] = (_Float16)((x - (float)h) * 2048.f);
    }
    lo_out = __builtin_bit_cast(uint4, lo);
    return __builtin_bit_cast(uint4, hi);
}

struct TailOut {
    const float* res;    // f32 NHWC [n][h][w][4] (channels 0..2: the network input)
    float* y;            // NCHW f32 [n][3][h s][w s] or null
    uint8_t* y8;         // u8 HWC [h s][w s][3] (n == 1) or null
    int flip, round;
};

// CIN: 32 (first layer, 3 channels zero padded) or 64.  NCB: output 16-channel blocks (4 for a feature layer; tail: 3 for
// s = 4 (48 channels), 1 for s = 2 (12 of 16)).  TAIL: the epilogue of the last conv.
template <int FORM, int CIN, int NCB, bool TAIL>
__global__ __launch_bounds__(THREADS, 1) void compact_conv_kernel(CompactConv a, TailOut t) {
    constexpr bool SPLIT = FORM == COMPACT_SPLIT, F16 = FORM == COMPACT_F16;
    typedef Form<SPLIT> G;
    constexpr int WR = G::WR, TH = G::TH, NPIX = G::NPIX;
    constexpr int PB = pix_bytes<SPLIT, CIN>();
    constexpr int KC = CIN / 32;                        // 32-channel K chunks
    constexpr int IN_BYTES = NPIX * PB;
    constexpr int SLAB = 3 * KC * NCB;                  // fragments of one tap column dx
    constexpr int W_BYTES = (SPLIT ? 1 : 3) * SLAB * G::FRAG;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* s_in = smem;
    char* s_w = smem + IN_BYTES;
    static_assert(IN_BYTES % 16 == 0 && IN_BYTES + W_BYTES <= 160 * 1024, "LDS budget");

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, col = lane & 15;
    const int H = a.h, W = a.w;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int ntiles = tiles_x * tiles_y * a.n;
    unsigned bad = 0;                                   // split: a value did not fit; f16: the largest |x| bit pattern stored

    auto stage_w = [&](int first, int count) {          // fragments [first, first + count) -> s_w
        const uint4* src = reinterpret_cast<const uint4*>(static_cast<const char*>(a.wt) + (size_t)first * G::FRAG);
        uint4* dst = reinterpret_cast<uint4*>(s_w);
        const int items = count * (G::FRAG / 16);
        for (int i = tid; i < items; i += THREADS) dst[i] = src[i];
    };
    if (!SPLIT) {
        stage_w(0, 3 * SLAB);                           // bf16: the whole layer, resident for every tile of this workgroup
    }

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int n = tile / (tiles_x * tiles_y);
        const int rem = tile - n * tiles_x * tiles_y;
        const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
        const int y0 = ty * TH, x0 = tx * TW;

        f32x4 acc[WR][2][NCB];
        f32x4 acx[SPLIT ? WR : 1][2][NCB];              // split: the hi*lo + lo*hi sums
#pragma unroll
        for (int o = 0; o < WR; ++o)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    acc[o][b][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (SPLIT) acx[SPLIT ? o : 0][b][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
                }

        __syncthreads();                                // the previous tile's reads of s_in (and s_w) are done
        // ---- input tile -> LDS (zero outside the image)
        if (!SPLIT) {
            constexpr int NCH = CIN / 8;
            const uint16_t* in = static_cast<const uint16_t*>(a.in);
            for (int i = tid; i < NPIX * NCH; i += THREADS) {
                const int p = i / NCH, c = i - p * NCH;
                const int pr = p / PW, pc = p - pr * PW;
                const int gy = y0 - 1 + pr, gx = x0 - 1 + pc;
                uint4 v = {0u, 0u, 0u, 0u};
                if (gy >= 0 && gy < H && gx >= 0 && gx < W)
                    v = *reinterpret_cast<const uint4*>(in + (((size_t)n * H + gy) * W + gx) * CIN + c * 8);
                *reinterpret_cast<uint4*>(s_in + lds_off<SPLIT, CIN>(p, c)) = v;
            }
        } else {
            constexpr int NG = CIN / 8;                 // 8-channel groups: one hi chunk and one lo chunk each
            const float* in = static_cast<const float*>(a.in);
            for (int i = tid; i < NPIX * NG; i += THREADS) {
                const int p = i / NG, c = i - p * NG;
                const int pr = p / PW, pc = p - pr * PW;
                const int gy = y0 - 1 + pr, gx = x0 - 1 + pc;
                float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    const f32x4* src = reinterpret_cast<const f32x4*>(in + (((size_t)n * H + gy) * W + gx) * CIN + c * 8);
                    const f32x4 u0 = src[0], u1 = src[1];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[j] = u0[j]; v[4 + j] = u1[j]; }
                }
                uint4 lo;
                const uint4 hi = split_hi_lo(v, lo, bad);
                *reinterpret_cast<uint4*>(s_in + lds_off<SPLIT, CIN>(p, c)) = hi;
                *reinterpret_cast<uint4*>(s_in + lds_off<SPLIT, CIN>(p, NG + c)) = lo;
            }
        }

        for (int dx = 0; dx < 3; ++dx) {
            if (SPLIT) {
                if (dx) __syncthreads();                // everyone is done with the previous column's weights
                stage_w(dx * SLAB, SLAB);
            }
            __syncthreads();
            const char* wbase = s_w + (SPLIT ? 0 : dx * SLAB * G::FRAG);
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                // pixel fragments of the WR + 2 input rows this wave needs: pixel (row, b*16 + col + dx), channels kc*32 + 8g ..
                uint4 bh[WR + 2][2], bl[SPLIT ? WR + 2 : 1][2];
#pragma unroll
                for (int r = 0; r < WR + 2; ++r)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int p = (wave * WR + r) * PW + b * 16 + col + dx;
                        bh[r][b] = *reinterpret_cast<const uint4*>(s_in + lds_off<SPLIT, CIN>(p, kc * 4 + g));
                        if (SPLIT) bl[SPLIT ? r : 0][b] = *reinterpret_cast<const uint4*>(s_in + lds_off<SPLIT, CIN>(p, CIN / 8 + kc * 4 + g));
                    }
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) {
                        const char* f = wbase + (size_t)((dy * KC + kc) * NCB + cb) * G::FRAG + lane * 16;
                        const uint4 wh = *reinterpret_cast<const uint4*>(f);
                        if (F16) {
                            const f32x4 A = __builtin_bit_cast(f32x4, wh);
#pragma unroll
                            for (int o = 0; o < WR; ++o)
#pragma unroll
                                for (int b = 0; b < 2; ++b)
                                    acc[o][b][cb] = E16<3>::mfma16(A, __builtin_bit_cast(f32x4, bh[o + dy][b]), acc[o][b][cb]);
                        } else if (!SPLIT) {
                            const bf16x8 A = __builtin_bit_cast(bf16x8, wh);
#pragma unroll
                            for (int o = 0; o < WR; ++o)
#pragma unroll
                                for (int b = 0; b < 2; ++b)
                                    acc[o][b][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, __builtin_bit_cast(bf16x8, bh[o + dy][b]),
                                                                                             acc[o][b][cb], 0, 0, 0);
                        } else {
                            const f16x8 Ah = __builtin_bit_cast(f16x8, wh);
                            const f16x8 Al = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(f + 1024));
#pragma unroll
                            for (int o = 0; o < WR; ++o)
#pragma unroll
                                for (int b = 0; b < 2; ++b) {
                                    const f16x8 Bh = __builtin_bit_cast(f16x8, bh[o + dy][b]);
                                    const f16x8 Bl = __builtin_bit_cast(f16x8, bl[SPLIT ? o + dy : 0][b]);
                                    acc[o][b][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bh, acc[o][b][cb], 0, 0, 0);
                                    f32x4& x = acx[SPLIT ? o : 0][b][cb];
                                    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bl, x, 0, 0, 0);
                                    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al, Bh, x, 0, 0, 0);
                                }
                        }
                    }
            }
        }

        // ---- epilogue: lane holds channels cb*16 + 4g .. +3 of pixel (y0 + wave*WR + o, x0 + b*16 + col)
        const bool poisoned = TAIL && (SPLIT || F16) && a.status && *reinterpret_cast<volatile const unsigned*>(a.status);
#pragma unroll
        for (int o = 0; o < WR; ++o) {
            const int y = y0 + wave * WR + o;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int x = x0 + b * 16 + col;
                if (y >= H || x >= W) continue;
                const size_t pix = ((size_t)n * H + y) * W + x;
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const int c0 = cb * 16 + 4 * g;
                    f32x4 v = acc[o][b][cb];
                    if (SPLIT) v += acx[SPLIT ? o : 0][b][cb] * (1.f / 2048.f);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] += a.bias[c0 + i];
                    if (!TAIL) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = v[i] < 0.f ? v[i] * a.slope[c0 + i] : v[i];
                        if (F16) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) bad = E16<3>::amax(bad, v[i]);
                            *reinterpret_cast<uint2*>(static_cast<uint16_t*>(a.out) + pix * NF + c0) = E16<3>::pack4(v);
                        } else if (!SPLIT) {
                            const __bf16 q[4] = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
                            *reinterpret_cast<uint2*>(static_cast<uint16_t*>(a.out) + pix * NF + c0) = __builtin_bit_cast(uint2, q);
                        } else {
                            // the range check of what the next layer reads is published by THIS launch, so the tail (a later
                            // launch) sees every out-of-range activation of the forward, its own input included
#pragma unroll
                            for (int i = 0; i < 4; ++i) bad |= !(fabsf(v[i]) <= 65504.f);
                            *reinterpret_cast<f32x4*>(static_cast<float*>(a.out) + pix * NF + c0) = v;
                        }
                    } else {
                        // output channel co = c s^2 + i s + j -> pixel (y s + i, x s + j) of image channel c
                        constexpr int S = NCB == 3 ? 4 : 2;
                        const int Hs = H * S, Ws = W * S;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int co = c0 + i;
                            const int c = co / (S * S), sub = co - c * S * S;
                            if (c >= 3) continue;
                            const int yy = y * S + sub / S, xx = x * S + sub % S;
                            float r = v[i] + t.res[pix * 4 + c];
                            if (poisoned) r = __builtin_nanf("");
                            if (t.y) t.y[(((size_t)n * 3 + c) * Hs + yy) * Ws + xx] = r;
                            if (t.y8) {
                                float q = fminf(fmaxf(r, 0.f), 1.f) * 255.0f;
                                q = t.round ? rintf(q) : truncf(q);
                                t.y8[((size_t)yy * Ws + xx) * 3 + (t.flip ? 2 - c : c)] = (uint8_t)q;
                            }
                        }
                    }
                }
            }
        }
    }
    if (SPLIT && a.status && bad) atomicOr(a.status, 1u);
    if (F16 && !TAIL) raise_range(a.status, bad);
}

template <int FORM>
__global__ void compact_pack_kernel(CompactPack p) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t npix = (size_t)p.n * p.h * p.w;
    if (i >= npix) return;
    const size_t n = i / ((size_t)p.h * p.w), yx = i - n * p.h * p.w;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (p.u8) v[c] = (float)p.u8[yx * 3 + (p.flip ? 2 - c : c)] / 255.0f;
        else v[c] = p.x[(n * 3 + c) * p.h * p.w + yx];
    }
    *reinterpret_cast<f32x4*>(p.res + i * 4) = f32x4{v[0], v[1], v[2], 0.f};
    if (FORM == COMPACT_SPLIT) {
        f32x4* d = reinterpret_cast<f32x4*>(static_cast<float*>(p.out) + i * 32);
        d[0] = f32x4{v[0], v[1], v[2], 0.f};
#pragma unroll
        for (int k = 1; k < 8; ++k) d[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else if (FORM == COMPACT_F16) {
        // the first conv reads f16: what the split form checks as it stages the image is checked here
        unsigned m = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) m = E16<3>::amax(m, v[c]);
        raise_range(p.status, m);
        uint4* d = reinterpret_cast<uint4*>(static_cast<uint16_t*>(p.out) + i * 32);
        const uint2 lo = E16<3>::pack4(f32x4{v[0], v[1], v[2], 0.f});
        d[0] = uint4{lo.x, lo.y, 0u, 0u};
#pragma unroll
        for (int k = 1; k < 4; ++k) d[k] = uint4{0u, 0u, 0u, 0u};
    } else {
        uint4* d = reinterpret_cast<uint4*>(static_cast<uint16_t*>(p.out) + i * 32);
        const __bf16 q[8] = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
        d[0] = __builtin_bit_cast(uint4, q);
#pragma unroll
        for (int k = 1; k < 4; ++k) d[k] = uint4{0u, 0u, 0u, 0u};
    }
}

template <int FORM, int CIN, int NCB, bool TAIL>
hipError_t launch_one(const CompactConv& a, const TailOut& t, int cus, hipStream_t s) {
    constexpr bool SPLIT = FORM == COMPACT_SPLIT;
    typedef Form<SPLIT> G;
    constexpr int KC = CIN / 32;
    const size_t lds = (size_t)G::NPIX * pix_bytes<SPLIT, CIN>() + (size_t)(SPLIT ? 1 : 3) * 3 * KC * NCB * G::FRAG;
    static unsigned long long done = 0;
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&compact_conv_kernel<FORM, CIN, NCB, TAIL>), lds, done);
    if (e != hipSuccess) return e;
    const long tiles = (long)a.n * ((a.h + G::TH - 1) / G::TH) * ((a.w + TW - 1) / TW);
    // one resident workgroup per CU walks the tiles (bf16, f16: the layer's weights are loaded once per CU)
    const int grid = (int)(tiles < cus ? tiles : cus);
    hipLaunchKernelGGL((compact_conv_kernel<FORM, CIN, NCB, TAIL>), dim3(grid), dim3(THREADS), lds, s, a, t);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_compact_pack(const CompactPack& p, hipStream_t s) {
    const size_t npix = (size_t)p.n * p.h * p.w;
    const dim3 grid((unsigned)((npix + 255) / 256));
    if (p.form == COMPACT_SPLIT) hipLaunchKernelGGL(compact_pack_kernel<COMPACT_SPLIT>, grid, dim3(256), 0, s, p);
    else if (p.form == COMPACT_F16) hipLaunchKernelGGL(compact_pack_kernel<COMPACT_F16>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(compact_pack_kernel<COMPACT_BF16>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_compact_conv(const CompactConv& a, int form, int cin, int cus, hipStream_t s) {
    const TailOut t{nullptr, nullptr, nullptr, 0, 0};
    if (form == COMPACT_SPLIT)
        return cin == 32 ? launch_one<COMPACT_SPLIT, 32, 4, false>(a, t, cus, s) : launch_one<COMPACT_SPLIT, 64, 4, false>(a, t, cus, s);
    if (form == COMPACT_F16)
        return cin == 32 ? launch_one<COMPACT_F16, 32, 4, false>(a, t, cus, s) : launch_one<COMPACT_F16, 64, 4, false>(a, t, cus, s);
    return cin == 32 ? launch_one<COMPACT_BF16, 32, 4, false>(a, t, cus, s) : launch_one<COMPACT_BF16, 64, 4, false>(a, t, cus, s);
}

hipError_t launch_compact_tail(const CompactConv& a, int form, int scale, const float* res, float* y, uint8_t* y8, int flip, int round,
                               int cus, hipStream_t s) {
    const TailOut t{res, y, y8, flip, round};
    if (form == COMPACT_SPLIT)
        return scale == 4 ? launch_one<COMPACT_SPLIT, 64, 3, true>(a, t, cus, s) : launch_one<COMPACT_SPLIT, 64, 1, true>(a, t, cus, s);
    if (form == COMPACT_F16)
        return scale == 4 ? launch_one<COMPACT_F16, 64, 3, true>(a, t, cus, s) : launch_one<COMPACT_F16, 64, 1, true>(a, t, cus, s);
    return scale == 4 ? launch_one<COMPACT_BF16, 64, 3, true>(a, t, cus, s) : launch_one<COMPACT_BF16, 64, 1, true>(a, t, cus, s);
}

// OIHW f32 [cout][cin][3][3] -> fragments f = ((dx * 3 + dy) * KC + kc) * ncb + cb, each the MFMA A operand of 16 output
// channels x 32 input channels: lane l holds W[cb*16 + (l & 15)][kc*32 + 8 (l >> 4) + i], i = 0..7 (bf16, f16: 16 B per lane;
// split: the hi fragment, then the lo fragment, 1 KiB each).  Padded channels are zero.
size_t compact_weight_bytes(int cin_p, int ncb, int form) { return (size_t)9 * (cin_p / 32) * ncb * (form == COMPACT_SPLIT ? 2048 : 1024); }

void pack_compact_weights(const float* oihw, int cout, int cin, int cin_p, int ncb, int form, uint16_t* dst) {
    const int KC = cin_p / 32;
    const bool split = form == COMPACT_SPLIT;
    for (int dx = 0; dx < 3; ++dx)
        for (int dy = 0; dy < 3; ++dy)
            for (int kc = 0; kc < KC; ++kc)
                for (int cb = 0; cb < ncb; ++cb) {
                    const size_t f = ((size_t)(dx * 3 + dy) * KC + kc) * ncb + cb;
                    uint16_t* d = dst + f * (split ? 1024 : 512);
                    for (int l = 0; l < 64; ++l)
                        for (int i = 0; i < 8; ++i) {
                            const int co = cb * 16 + (l & 15), ci = kc * 32 + 8 * (l >> 4) + i;
                            const float w = (co < cout && ci < cin) ? oihw[((size_t)co * cin + ci) * 9 + dy * 3 + dx] : 0.f;
                            if (form == COMPACT_F16) {
                                d[l * 8 + i] = __builtin_bit_cast(uint16_t, (_Float16)w);   // nearest even, as torch's .half()
                            } else if (!split) {
                                d[l * 8 + i] = __builtin_bit_cast(uint16_t, (__bf16)w);
                            } else {
                                const _Float16 h = (_Float16)w;
                                d[l * 8 + i] = __builtin_bit_cast(uint16_t, h);
                                d[512 + l * 8 + i] = __builtin_bit_cast(uint16_t, (_Float16)((w - (float)h) * 2048.f));
                            }
                        }
                }
}

}  // namespace nesr
