// conv3x3(nearest_x2(x)) as four 2x2-tap convolutions on the LOW-resolution input, f16-pair form (conv3x3_f16x2.hip has
// the arithmetic: x = hi + lo 2^-11, three v_mfma_f32_16x16x32_f16 per product, main + cross accumulators in f32;
// f16x2_common.h has the pieces the f16-pair kernels share).
//
// Output pixel (2y + py, 2x + px) of a 3x3 conv over the nearest-x2 upsample reads only the low-res pixels
// (y + py - 1 + a, x + px - 1 + b), a, b in {0, 1}: the three kernel rows fall onto two input rows ({0 | 1,2} for py = 0,
// {0,1 | 2} for py = 1), the same for the columns.  The taps that share an input pixel are summed once on the host
// (fold_upconv_weights, f32, ky then kx ascending), so a low-res pixel costs 16 taps instead of 36: 2.25x fewer MACs.
// The zero padding carries over exactly: a high-res tap outside the image is a low-res tap outside the image.
//
//   workgroup : 4 waves, low-res tile 4 rows x 32 cols (= 8 x 64 output pixels) x 32 output channels; wave w owns low-res
//               row w and all four parities of it.  64-channel layers run two workgroups per tile.
//   K loop    : steps (16-channel chunk c, row parity py).  The input halo tile [6 x 34 pixels][64 B] of chunk c serves
//               both of its steps; the weight slab of a step is [px][b][a][hi|lo][k half][32 couts][16 B] = 16 KiB.  Both by
//               LDS-DMA into two-slot rings, one vmcnt(0) + one barrier per step (as conv3x3_f16x2_kernel).
//   MFMA      : K = 32 = 16 channels x the two tap ROWS a = 0 | 1 (lanes 0-31 | 32-63), one MFMA triple per (px, b).
//               The input fragments of a step depend on px + b only: 3 column offsets x 2 pixel halves x 2 planes = 12 reads
//               feed 48 MFMAs (with 16 weight reads).
//   epilogue  : as conv3x3_f16x2_kernel (bias, LeakyReLU, split, regroup, 16-byte stores); the two column parities are
//               interleaved across lanes first, so a store instruction writes 16 consecutive output pixels x 64 B.
#include <cstdlib>

#include "f16x2_common.h"
#include "nesr_kernels.h"

namespace nesr {

namespace {

constexpr int UTW = 32, UPW = UTW + 2;    // low-res tile width, with halo
constexpr int UWAVES = 4;
constexpr int ULH = UWAVES;               // low-res rows per tile: one per wave
constexpr int UPH = ULH + 2;
constexpr int UTHREADS = 64 * UWAVES;
constexpr int UIN_ITEMS = 4 * UPH * UPW;  // 16-byte items of one input slot
constexpr int UIN_ROUNDS = (UIN_ITEMS + UTHREADS - 1) / UTHREADS;
constexpr int UIN_BYTES = UIN_ITEMS * 16;
constexpr int UW_ITEMS = 8 * 2 * 2 * 32;  // one step's weight slab: 8 (px, b, a) taps x plane x k half x 32 couts
constexpr int UW_ROUNDS = UW_ITEMS / UTHREADS;
constexpr int UW_BYTES = UW_ITEMS * 16;
constexpr int UWRING = 2 * UIN_BYTES;     // LDS: [input ring: 2 slots][weight ring: 2 slots]
constexpr size_t USHM = (size_t)UWRING + 2 * UW_BYTES;
static_assert(UW_ITEMS % UTHREADS == 0, "whole DMA rounds");
static_assert(UIN_ROUNDS <= 32, "okmask");

#ifndef NESR_UABL
#define NESR_UABL 0   // timing ablations (wrong results): 4 no epilogue, 8 no MFMA, 16 no K-loop DMA
#endif
#ifndef NESR_UP_HALF_LINES
#define NESR_UP_HALF_LINES 0   // 1: the epilogue without the parity exchange (a store instruction writes 64-byte half lines)
#endif

__global__ __launch_bounds__(UTHREADS, 2) void upconv2x2_f16x2_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = wave * 64 + lane;

    // ---- XCD-aware work index (bijective for any count); the cout groups of one tile are neighbours.  Geometry in
    // low-res pixels: a.in_h x a.in_w (a.h = 2 in_h, a.w_ = 2 in_w)
    const int CG = a.coutp / 32;
    const int lh = a.in_h, lw = a.in_w;
    const int tiles_x = (lw + UTW - 1) / UTW;
    const int tiles_y = (lh + ULH - 1) / ULH;
    const int total = tiles_x * tiles_y * a.n * CG;
    const int idx = xcd_work_index(total);
    const int cg = idx % CG;
    int tile = idx / CG;
    const int n = tile / (tiles_x * tiles_y);
    tile -= n * tiles_x * tiles_y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * ULH, x0 = tx * UTW;

    // ---- LDS-DMA plan (conv3x3_f16x2_kernel's, on the stored image): item k of an input slot = padded pixel k>>2,
    // physical slot k&3 holding logical slot (k&3) ^ (bit 2 of the padded column << 1).  Out-of-image items are the zero
    // padding: zeroed once in both ring slots and left out of the DMAs.
    const unsigned lds_base = (unsigned)(size_t)(lds_char*)(smem);
    unsigned voff[UIN_ROUNDS];
    unsigned okmask = 0;
    const int row0 = y0 > 0 ? y0 - 1 : 0;
    const char* in_img = static_cast<const char*>(a.in) + ((size_t)n * lh + row0) * lw * 64;
    const long long in_cstride = a.in_map.chunk * 2;   // bytes between K-chunks
    const char* wbase = static_cast<const char*>(a.w) + (size_t)cg * (2 * UW_BYTES);
    const long long w_cstride = (long long)CG * (2 * UW_BYTES);
    auto dma_weights = [&](int st, int slot) {   // step st = 2 c + py
#pragma unroll
        for (int j = 0; j < UW_ROUNDS; ++j) {
            const unsigned dst = lds_base + UWRING + slot * UW_BYTES + j * (UTHREADS * 16) + wave * 1024;
            glds16_s(wbase + (long long)(st >> 1) * w_cstride + (st & 1) * UW_BYTES, (unsigned)(tid + UTHREADS * j) * 16u,
                     __builtin_amdgcn_readfirstlane(dst));
        }
    };
    auto dma_input_round = [&](int c, int slot, int i) {
        const unsigned dst = lds_base + slot * UIN_BYTES + i * (UTHREADS * 16) + wave * 1024;
        if ((okmask >> i) & 1u) glds16_s(in_img + (long long)c * in_cstride, voff[i], __builtin_amdgcn_readfirstlane(dst));
    };
    dma_weights(0, 0);
    {
        int p = tid >> 2;
        int py_ = p / UPW, px_ = p - py_ * UPW;
        const int sl = tid & 3;
#pragma unroll
        for (int i = 0; i < UIN_ROUNDS; ++i) {
            const int k = tid + UTHREADS * i;
            const int sg = sl ^ (((px_ >> 2) & 1) << 1);
            const int Y = y0 - 1 + py_, X = x0 - 1 + px_;
            const bool has = k < UIN_ITEMS;
            const bool ok = has && Y >= 0 && Y < lh && X >= 0 && X < lw;
            voff[i] = ((unsigned)(Y - row0) * (unsigned)lw + (unsigned)X) * 64u + sg * 16;
            okmask |= ok ? (1u << i) : 0u;
            dma_input_round(0, 0, i);
            if (has && !ok) {
#pragma unroll
                for (int sl2 = 0; sl2 < 2; ++sl2) *reinterpret_cast<f32x4*>(smem + sl2 * UIN_BYTES + k * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            px_ += (UTHREADS / 4) % UPW;
            py_ += (UTHREADS / 4) / UPW;
            if (px_ >= UPW) { px_ -= UPW; py_ += 1; }
        }
    }

    const bool active = (y0 + wave) < lh;

    // ---- operands.  Lane (j16, g4): unit un = g4 >> 1 is tap row a, kh = g4 & 1 the channel half.  Step (c, py), column
    // offset d = px + b: the input fragment is padded pixel (wave + py + un, 16 nh + j16 + d); the weight fragment of
    // (px, b) is tap t = (2 px + b) 2 + un of the step's slab.
    const int j16 = lane & 15, g4 = lane >> 4, un = g4 >> 1, kh = g4 & 1;
    int boff[3][2], aoff[2][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int nh = 0; nh < 2; ++nh) {
            const int col = 16 * nh + j16 + d;
            boff[d][nh] = ((wave + un) * UPW + col) * 64 + ((kh ^ (((col >> 2) & 1) << 1)) << 4);
        }
#pragma unroll
    for (int px = 0; px < 2; ++px)
#pragma unroll
        for (int b = 0; b < 2; ++b) aoff[px][b] = (((((px * 2 + b) * 2 + un) * 2) * 2 + kh) * 32 + j16) * 16;

    f32x4 acc[2][2][2][2][2];       // [py][px][pixel half][cout half][main | cross]
#pragma unroll
    for (int i = 0; i < 32; ++i) (&acc[0][0][0][0][0])[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int cb16 = 32 * cg + (g4 & 1) * 16 + (g4 >> 1) * 8;   // this lane's 8 output channels after the epilogue's exchange
    const int piece8 = ((g4 & 1) * 2 + (g4 >> 1)) * 8;          // its 16-byte piece of a 64-byte slot after regroup_pairs
    const f32x4 bz0 = *reinterpret_cast<const f32x4*>(a.bias + cb16), bz1 = *reinterpret_cast<const f32x4*>(a.bias + cb16 + 4);

    const int nsteps = 2 * (a.cin / 16);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the zero padding is in LDS before the first barrier
    for (int c = 0; 2 * c < nsteps; ++c)
#pragma unroll
    for (int py = 0; py < 2; ++py) {   // unrolled: the accumulators are indexed by constants
        const int st = 2 * c + py;
        // this wave's DMAs of step st (issued during step st - 1) have landed; after the barrier, everybody's
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (st + 1 < nsteps && !(NESR_UABL & 16)) {
            dma_weights(st + 1, (st + 1) & 1);
            if (py) {   // the next step opens chunk c + 1; its input slot was last read in chunk c - 1
#pragma unroll
                for (int i = 0; i < UIN_ROUNDS; ++i) dma_input_round(c + 1, (c + 1) & 1, i);
            }
        }
        if (active) {
            const char* sin = smem + (c & 1) * UIN_BYTES + py * (UPW * 64);   // row parity py shifts the tap rows down by one
            const char* swb = smem + UWRING + py * UW_BYTES;
            f16x8 XH[3][2], XL[3][2];
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int nh = 0; nh < 2; ++nh) {
                    XH[d][nh] = __builtin_bit_cast(f16x8, *reinterpret_cast<const f32x4*>(sin + boff[d][nh]));
                    XL[d][nh] = __builtin_bit_cast(f16x8, *reinterpret_cast<const f32x4*>(sin + (boff[d][nh] ^ 32)));
                }
#pragma unroll
            for (int px = 0; px < 2; ++px)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int d = px + b;
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const f16x8 wh = __builtin_bit_cast(f16x8, *reinterpret_cast<const f32x4*>(swb + aoff[px][b] + mt * 256));
                        const f16x8 wl = __builtin_bit_cast(f16x8, *reinterpret_cast<const f32x4*>(swb + aoff[px][b] + mt * 256 + 1024));
#pragma unroll
                        for (int nh = 0; nh < 2; ++nh) {
                            f32x4* ac = acc[py][px][nh][mt];
                            if (NESR_UABL & 8) {
                                ac[0][0] += (float)wh[0] + (float)wl[0] + (float)XH[d][nh][0] + (float)XL[d][nh][0];
                                continue;
                            }
                            ac[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, XL[d][nh], ac[1], 0, 0, 0);
                            ac[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, XH[d][nh], ac[0], 0, 0, 0);
                            ac[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, XH[d][nh], ac[1], 0, 0, 0);
                        }
                    }
                }
        }
    }
    if (!active) return;

    // ---- epilogue (conv3x3_f16x2_kernel's): lane (pixel j16, k-group g4) holds couts 16 mt + 4 g4 + i; after the cout
    // exchange (f16x2_common.h) 8 consecutive couts of its pixel.  The two column parities of a low-res pixel are neighbours in the output
    // row: lanes exchange pieces (ds_bpermute inside their 16-lane row) so that store instruction h writes output pixels
    // 16 h .. 16 h + 15 of the 32 this (row, pixel half) produces -- 16 x 64 B = whole 128-byte lines per instruction.
    if (NESR_UABL & 4) {
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) sum += (&acc[0][0][0][0][0])[i][i & 3];
        if (sum == 12345.678f) static_cast<float*>(a.out)[0] = sum;
        return;
    }
    uint16_t* out = static_cast<uint16_t*>(a.out);
    bool bad = false;
    const int yl = y0 + wave;
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int nh = 0; nh < 2; ++nh) {
            const bool lvalid = x0 + 16 * nh + j16 < lw;
            uint4 c[2], c1[2];
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                f32x4 v0, v1;
                cout_exchange_acc(acc[py][px][nh][0], acc[py][px][nh][1], v0, v1);
                v0 += bz0;
                v1 += bz1;
                if (a.lrelu) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) { v0[i] = fmaxf(v0[i], v0[i] * 0.2f); v1[i] = fmaxf(v1[i], v1[i] * 0.2f); }
                }
                bool bad_here = false;
                split_regroup(v0, v1, c[px], c1[px], bad_here);
                bad |= bad_here && lvalid;
            }
            const int Y = 2 * yl + py;
            uint16_t* row = out + (size_t)((a.out_coff + 32 * cg) >> 4) * a.out_map.chunk + piece8;
#if NESR_UP_HALF_LINES
#pragma unroll
            for (int px = 0; px < 2; ++px) {   // a store instruction = the 64-byte slots of 16 pixels of ONE column parity
                const size_t pix = ((size_t)n * a.h + Y) * a.w_ + 2 * (lvalid ? x0 + 16 * nh + j16 : 0) + px;
                if (lvalid) {
                    store16(row + pix * a.out_map.pix, c[px]);
                    store16(row + pix * a.out_map.pix + a.out_map.chunk, c1[px]);
                }
            }
#else
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // output pixel 16 h + j16 = low-res pixel 8 h + (j16 >> 1), column parity j16 & 1, same k-group
                const int src = ((lane & 48) | (8 * h + (j16 >> 1))) << 2;
                const bool odd = j16 & 1;
                auto pull1 = [&](unsigned q0, unsigned q1) {
                    const unsigned e0 = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)q0);
                    const unsigned e1 = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)q1);
                    return odd ? e1 : e0;
                };
                auto pull = [&](const uint4 (&q)[2]) {
                    return uint4{pull1(q[0].x, q[1].x), pull1(q[0].y, q[1].y), pull1(q[0].z, q[1].z), pull1(q[0].w, q[1].w)};
                };
                const uint4 w0 = pull(c), w1 = pull(c1);
                const int X = 2 * (x0 + 16 * nh) + 16 * h + j16;
                const bool valid = X < a.w_;
                const size_t pix = ((size_t)n * a.h + Y) * a.w_ + (valid ? X : 0);
                if (valid) {
                    store16(row + pix * a.out_map.pix, w0);
                    store16(row + pix * a.out_map.pix + a.out_map.chunk, w1);
                }
            }
#endif
        }
    if (bad && a.status) __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// W[py][px][a][b][o][ci] = sum of the 3x3 taps (ky, kx) that read low-res pixel (y + py - 1 + a, x + px - 1 + b) at output
// parity (py, px): kernel row ky lands on a = (py + ky + 1) / 2 - py, the same for the columns.  f32 sums, ky ascending, then kx.
void fold_upconv_weights(const float* oihw, int cout, int cin, float* dst) {
    const size_t plane = (size_t)cout * cin;
    for (size_t i = 0; i < 16 * plane; ++i) dst[i] = 0.f;
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    const int ta = (py + ky + 1) / 2 - py, tb = (px + kx + 1) / 2 - px;
                    float* d = dst + ((((size_t)py * 2 + px) * 2 + ta) * 2 + tb) * plane;
                    for (size_t i = 0; i < plane; ++i) d[i] += oihw[i * 9 + ky * 3 + kx];
                }
}

size_t packed_upconv_elems_f16x2(int cin_p, int coutp) { return (size_t)cin_p * 16 * coutp * 2; }

// folded f32 -> [chunk = ci/16][cout group = o/32][py][tap = (2 px + b) 2 + a][plane hi|lo][k half][o%32][ci%8] halves
void pack_upconv_weights_f16x2(const float* folded, int cout, int cin, int cin_p, int coutp, uint16_t* dst) {
    const size_t total = packed_upconv_elems_f16x2(cin_p, coutp);
    for (size_t i = 0; i < total; ++i) dst[i] = 0;
    const int groups = coutp / 32;
    const size_t plane = (size_t)cout * cin;
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
            for (int ta = 0; ta < 2; ++ta)
                for (int tb = 0; tb < 2; ++tb)
                    for (int o = 0; o < cout; ++o)
                        for (int ci = 0; ci < cin; ++ci) {
                            const float wv = folded[((((size_t)py * 2 + px) * 2 + ta) * 2 + tb) * plane + (size_t)o * cin + ci];
                            const uint16_t hi = f2h(wv);
                            const uint16_t lo = f2h((wv - h2f(hi)) * LO_SCALE);
                            const int c = ci / 16, kh = (ci % 16) / 8, kk = ci % 8;
                            const int tap = (px * 2 + tb) * 2 + ta;
                            const size_t slab = (((size_t)c * groups + o / 32) * 2 + py) * (size_t)(UW_ITEMS * 8);
                            dst[slab + ((((size_t)tap * 2 + 0) * 2 + kh) * 32 + o % 32) * 8 + kk] = hi;
                            dst[slab + ((((size_t)tap * 2 + 1) * 2 + kh) * 32 + o % 32) * 8 + kk] = lo;
                        }
}

hipError_t launch_upconv2x2_f16x2(const ConvArgs& a, hipStream_t s) {
    if (a.up != 1 || a.h != 2 * a.in_h || a.w_ != 2 * a.in_w) return hipErrorInvalidValue;
    if (a.cin % 16 || (a.coutp != 32 && a.coutp != 64)) return hipErrorInvalidValue;
    // feature-map layers, whole dense images (no row range, no ragged batch: the kernel would not see the sizes)
    if (a.y_lo || a.y_hi || a.rag_n || a.res1 || a.res2 || a.out2 || a.out_nchw || a.out_u8 || !a.out) return hipErrorInvalidValue;
    if ((long long)a.in_w * 64 * 8 >= (1ll << 32)) return hipErrorInvalidValue;   // 32-bit byte offsets inside one tile's rows
    if (a.in_map.pix != 32 || a.out_map.pix % 32 || a.out_coff % 16) return hipErrorInvalidValue;
    const long total = (long)((a.in_w + UTW - 1) / UTW) * ((a.in_h + ULH - 1) / ULH) * a.n * (a.coutp / 32);
    if (total <= 0) return hipSuccess;
    if (total > 0x7fffffffL) return hipErrorInvalidValue;
    note_conv_kernel(CONV_KERNEL_UPCONV2X2);
    hipLaunchKernelGGL(upconv2x2_f16x2_kernel, dim3((unsigned)total), dim3(UTHREADS), USHM, s, a);
    return hipGetLastError();
}

}  // namespace nesr
