// f32 3x3 convolution on the f16 matrix cores: every f32 operand travels as an exact-sum pair of
// halves, x = hi + lo * 2^-11 with hi = f16(x), lo = f16((x - hi) * 2^11), and the product is
// accumulated in f32 from three MFMAs
//
//     w*x  ~=  w_hi*x_hi + 2^-11 (w_hi*x_lo + w_lo*x_hi)        (dropped: w_lo*x_lo ~ 2^-22 |w x|)
//
// The two cross terms have their own f32 accumulator and are scaled once in the epilogue.  Precision of
// the pair: hi carries 11 significant bits and lo (kept normal by the 2^11 scale) the next 11, so
// |x - (hi + lo 2^-11)| <= 2^-22 |x| for 6.1e-5 <= |x| <= 65504; below 6.1e-5 hi is an f16 subnormal
// (absolute step 2^-24) and the scaled lo resolves the rest to an absolute 2^-35.  Range: |x| >= 65520
// or a non-finite x does not fit; nothing is clamped (f16x2_common.h, split2): its hi half is Inf / NaN
// and poisons the sums it enters, and it is reported -- a sticky device flag (ConvArgs::status) that
// nesr_check_status / nesr_check_range turn into NESR_ERR_RANGE and that makes conv_last write NaN
// instead of a saturated image (a diverged network gives NaN in the reference too).
//
// v_mfma_f32_32x32x16_f16 runs at 16x the rate of the f32 MFMA, so three of them cost 3/16 of the
// direct f32 kernel's matrix time and 27/64 of the Winograd kernel's.  Measured on the 23-block
// network against an f64 evaluation of the same weights (tools/probes/split_accuracy.py): max abs
// error 3.1e-6 for this scheme, 1.2e-6 for plain f32 (torch CPU), i.e. the same class of error
// as the Winograd kernel -- 300x inside the 1e-3 tolerance.  (The MFMA honours f16 subnormal inputs on
// gfx950, tools/probes/mfma_f16_denorm.hip: hi needs no special case.)
//
// Activations live pre-split in HBM, channel-blocked like the bf16 path: per 16-channel K-chunk a
// pixel owns 64 bytes = [16 hi halves | 16 scaled-lo halves] (Map: pix = 32, chunk = pixels * 32, in
// 2-byte units); the producing kernel's epilogue splits once, the consumers feed LDS by LDS-DMA
// without touching a VGPR.  Same 4 bytes per value as f32 storage.
//
//   workgroup : 4 MFMA waves (+ 4 DMA-only waves when a CU gets one workgroup), output tile 8 rows x 32 cols
//               x 32 output channels; wave w owns rows 2w, 2w+1.  Layers with 64 output channels run two
//               workgroups per tile (adjacent in the launch order).
//   K loop    : 16-channel chunks; input halo tile [(rows+2) x 34 pixels][64 B] and weight slab
//               [9 taps][hi|lo][k half][32 couts][16 B] by LDS-DMA into 2-slot rings, counted
//               vmcnt waits + one barrier per chunk (as conv3x3_bf16.hip).
//   LDS image : pixel p's 16-byte slot s = 2*plane + k-half sits at p*64 + (s ^ ((col>>2)&3))*16:
//               the 16-lane groups of ds_read_b128 (MI355X_MICROARCH.md, LDS) then cover all 16
//               slots of a 256-byte bank row for every horizontal tap.
//   epilogue  : bias / LeakyReLU / residuals in f32 (residuals re-joined hi + lo; v * s + res in two
//               roundings, scale_add_2r), split, 16-byte
//               write-through stores of 8 channels per plane; conv_last writes planar f32 / u8.
//
// The fused dense block (conv1..conv5 of an RDB in one launch, the same arithmetic) is rdb_f16x2.hip; what the two share
// (tile geometry, tap address plan, a tap-step's MFMAs, the cout exchange) is f16x2_common.h.
#include <cstdlib>

#include "f16x2_common.h"
#include "nesr_kernels.h"

namespace nesr {

namespace {

constexpr int ISLOTS = 2;   // two-slot rings: every wait is vmcnt(0)

#ifndef NESR_ABL
#define NESR_ABL 0   // timing ablations: 1 empty kernel, 2 stop after the prologue, 4 no epilogue, 8 no MFMA, 16 no K-loop DMA, 64 cycle stamps, 512 no per-chunk barrier
#endif
#if NESR_ABL & 64
__device__ unsigned long long g_stamps[256];
#define STAMP(i) do { if (stamping) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); if (lane == 0 && (i) < 200) g_stamps[(i)] = t_; \
    if ((i) == 0 || (i) == 4) { unsigned long long r_ = __builtin_amdgcn_s_memrealtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); if (lane == 0) g_stamps[200 + (i)] = r_; } } } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

// NMT = 16-cout MFMA column blocks a workgroup computes: 2 = all 32 channels of its cout group; 1 = channels 0..15 only, for
// conv_last (cout_real <= 4, image outputs only): the same products in the same order for the channels that are written,
// half the MFMAs and weight reads of the layer -- bit-identical output
template <int DMAW, int NMT = 2>
__global__ __launch_bounds__(64 * (WAVES + DMAW), DMAW ? (WAVES + DMAW) / 4 : 2) void conv3x3_f16x2_kernel(ConvArgs a) {
    if (NESR_ABL & 1) return;
    typedef Geo<DMAW> G;
    constexpr int THREADS = G::THREADS, TH = G::TH;
    constexpr int IN_ITEMS = G::IN_ITEMS, IN_ROUNDS = G::IN_ROUNDS, IN_BYTES = G::IN_BYTES;
    constexpr int W_ROUNDS = (W_ITEMS + THREADS - 1) / THREADS;
    constexpr int WRING = ISLOTS * IN_BYTES;   // LDS: [input ring][weight ring: 2 x W_BYTES]
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool is_dma = DMAW ? wave_all >= WAVES : true;     // issues the LDS-DMAs
    const bool is_cmp = wave_all < WAVES;                    // runs the MFMAs and the epilogue
    const int wave = is_cmp ? wave_all : wave_all - WAVES;   // index inside its role
    const int tid = wave * 64 + lane;
#if NESR_ABL & 64
    const bool stamping = blockIdx.x == 77 && wave_all == 1;
#endif
    STAMP(0);

    // ---- XCD-aware work index (bijective for any count); the cout groups of one tile are neighbours
    const int CG = a.coutp / 32;
    const int y_lo = a.y_lo, y_hi = a.y_hi > 0 ? a.y_hi : a.h;      // output rows of this launch
    const int tiles_x = (a.w_ + TW - 1) / TW;
    const int tiles_y = (y_hi - y_lo + TH - 1) / TH;
    const int total = tiles_x * tiles_y * a.n * CG;
    const int idx = xcd_work_index(total);
    STAMP(5);
    const int cg = idx % CG;
    int tile = idx / CG;
    const int n = tile / (tiles_x * tiles_y);
    tile -= n * tiles_x * tiles_y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = y_lo + ty * TH, x0 = tx * TW;

    // ---- LDS-DMA plan.  LDS item k of an input slot = padded pixel k>>2, physical slot k&3; it holds
    // logical slot (k&3) ^ (bit 2 of the padded column << 1) of that pixel's 64 bytes.  Item k = tid + THREADS*i
    // belongs to this lane in round i; its source is (scalar base of image n and chunk c) + voff[i].
    // Out-of-image items (the conv's zero padding) are the same for every chunk: they are zeroed once in
    // every ring slot and left out of the DMAs (EXEC-masked lanes do not write).
    const unsigned lds_base = (unsigned)(size_t)(lds_char*)(smem);
    unsigned voff[IN_ROUNDS];
    unsigned okmask = 0;
    // scalar base = image n, first stored row this tile reads; the per-lane offsets below are relative to it and stay
    // below (tile rows + 2) * in_w * 64 bytes, so frames of any size address correctly (64-bit base, 32-bit offsets)
    const int row0 = (y0 > 0 ? y0 - 1 : 0) >> a.up;
    const char* in_img = static_cast<const char*>(a.in) + ((size_t)n * a.in_h + row0) * a.in_w * 64;
    const long long in_cstride = a.in_map.chunk * 2;   // bytes between K-chunks
    const char* wbase = static_cast<const char*>(a.w) + (size_t)cg * W_BYTES;
    const long long w_cstride = (long long)CG * W_BYTES;
    // DMA round j of chunk c: rounds [0, W_ROUNDS) move the weight slab, the rest the input tile
    constexpr int NDMA = W_ROUNDS + IN_ROUNDS;
    auto dma_round = [&](int c, int slot, int j) {   // j is a compile-time constant at every call site
        if (j < W_ROUNDS) {
            const int k = tid + THREADS * j;
            const unsigned dst = lds_base + WRING + slot * W_BYTES + j * (THREADS * 16) + wave * 1024;
            if (k < W_ITEMS) glds16_s(wbase + (long long)c * w_cstride, (unsigned)k * 16u, __builtin_amdgcn_readfirstlane(dst));
        } else if (j < NDMA) {
            const int i = j - W_ROUNDS;
            const unsigned dst = lds_base + slot * IN_BYTES + i * (THREADS * 16) + wave * 1024;
            if ((okmask >> i) & 1u) glds16_s(in_img + (long long)c * in_cstride, voff[i], __builtin_amdgcn_readfirstlane(dst));
        }
    };
    // the plan and chunk 0's DMAs together: the weight slab first (needs no plan), then every input round as
    // soon as its offsets exist, so the first bytes are under way while the rest is still being computed
    if (is_dma) {
#pragma unroll
        for (int j = 0; j < W_ROUNDS; ++j) dma_round(0, 0, j);
        int p = tid >> 2;
        int py = p / PW, px = p - py * PW;
        const int sl = tid & 3;
#pragma unroll
        for (int i = 0; i < IN_ROUNDS; ++i) {
            const int k = tid + THREADS * i;
            const int sg = sl ^ (((px >> 2) & 1) << 1);
            const int Y = y0 - 1 + py, X = x0 - 1 + px;
            const bool has = k < IN_ITEMS;
            const bool ok = has && Y >= 0 && Y < a.h && X >= 0 && X < a.w_;
            voff[i] = ((unsigned)((Y >> a.up) - row0) * (unsigned)a.in_w + (unsigned)(X >> a.up)) * 64u + sg * 16;
            okmask |= ok ? (1u << i) : 0u;
            dma_round(0, 0, W_ROUNDS + i);
            if (has && !ok) {
#pragma unroll
                for (int sl2 = 0; sl2 < ISLOTS; ++sl2) *reinterpret_cast<f32x4*>(smem + sl2 * IN_BYTES + k * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            px += (THREADS / 4) % PW;
            py += (THREADS / 4) / PW;
            if (px >= PW) { px -= PW; py += 1; }
        }
    }
    STAMP(6);

    const bool active = is_cmp && (y0 + RW * wave) < y_hi;

    // ---- operands.  The MFMA (v_mfma_f32_16x16x32_f16) has K = 32 = two units of 16 channels: lanes 0-31
    // (k-groups g = 0,1 = channel halves) feed unit 0, lanes 32-63 unit 1, and a unit is one (tap, plane)
    // choice -- just another per-lane LDS address.  Steps 0-2 pair the taps (dy 0 | dy 1) of column dx = step,
    // step 3 pairs (2,0) | (2,1); with WH/WL = [w(tap a) | w(tap b)] and XH/XL = [x(tap a) | x(tap b)] a step is
    // main += WH*XH, cross += WH*XL + WL*XH.  Step 4 is tap (2,2) alone: main += [w_hi | 0] * [x_hi | .] and
    // cross += [w_hi | w_lo] * [x_lo | x_hi], i.e. both cross terms in one MFMA.  14 MFMAs per 16x16 tile and
    // chunk instead of 13.5; the chip holds a ~20 % higher clock on this shape than on 32x32x16
    // (tools/probes/mfma_shape.hip).  Tiles of a wave: rows r, pixel halves nh (16 px), cout halves mt
    // (16 couts).  LDS slot swizzle for this lane order: physical slot = slot ^ (bit 2 of the padded column << 1)
    // (conflict-free for the ds_read_b128 lane groups).
    const int j16 = lane & 15, g4 = lane >> 4, un = g4 >> 1, kh = g4 & 1;
    int b16[5][2], a16[5];
#pragma unroll
    for (int st_ = 0; st_ < 5; ++st_) {
#pragma unroll
        for (int nh = 0; nh < 2; ++nh) b16[st_][nh] = tap_pixel_offset(st_, RW * wave, nh, j16, un, kh);
        a16[st_] = tap_weight_offset(st_, j16, un, kh);
    }
    f32x4 acc16[RW][2][2][2];       // [row][pixel half][cout half][main | cross]
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc16[r][nh][mt][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // this lane's 8 output channels after the epilogue's permlane16 exchange, and their bias (fetched now: the
    // latency hides under the K loop)
    const int cb16 = 32 * cg + (g4 & 1) * 16 + (g4 >> 1) * 8;
    const int piece8 = ((g4 & 1) * 2 + (g4 >> 1)) * 8;    // this lane's 16-byte piece of a 64-byte slot after regroup_pairs (2-byte units)
    const f32x4 bz0 = *reinterpret_cast<const f32x4*>(a.bias + cb16), bz1 = *reinterpret_cast<const f32x4*>(a.bias + cb16 + 4);

    const int nchunks = a.cin / 16;
    STAMP(7);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the zero padding is in LDS before the first barrier
    STAMP(1);
    if (NESR_ABL & 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        return;
    }
    for (int c = 0; c < nchunks; ++c) {
        // this wave's DMAs of chunk c (issued during chunk c-1) have landed; after the barrier, everybody's
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        STAMP(8 + 4 * c);
        if (!(NESR_ABL & 512)) __builtin_amdgcn_s_barrier();   // 512: timing only (races)
        asm volatile("" ::: "memory");
        STAMP(9 + 4 * c);
        // the next chunk's DMAs go out first (beside the MFMAs each costs 150+ cycles of issue instead of ~85:
        // measured, in-kernel stamps)
        if (is_dma && c + 1 < nchunks && !(NESR_ABL & 16)) {
#pragma unroll
            for (int j = 0; j < NDMA; ++j) dma_round(c + 1, (c + 1) & 1, j);
        }
        STAMP(10 + 4 * c);
        if (active) {
            const char* st = smem + (c & 1) * IN_BYTES;
            const char* swb = smem + WRING + (c & 1) * W_BYTES;
            f32x4 Af[2][2][2];        // [buffer][cout half][variant]
            f32x4 Bf[2][RW][2][2];    // [buffer][row][pixel half][variant]
            auto load_step = [&](int s_, int buf) {   // s_ is a compile-time constant at every call site
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt) {
                    if (s_ < 4) {
                        Af[buf][mt][0] = *reinterpret_cast<const f32x4*>(swb + a16[s_] + mt * 256);          // WH
                        Af[buf][mt][1] = *reinterpret_cast<const f32x4*>(swb + a16[s_] + mt * 256 + 1024);   // WL
                    } else {
                        f32x4 hi = *reinterpret_cast<const f32x4*>(swb + a16[4] + mt * 256);
                        Af[buf][mt][1] = *reinterpret_cast<const f32x4*>(swb + a16[4] + mt * 256 + un * 1024);   // [w_hi | w_lo]
                        if (un) hi = f32x4{0.f, 0.f, 0.f, 0.f};
                        Af[buf][mt][0] = hi;                                                                      // [w_hi | 0]
                    }
                }
#pragma unroll
                for (int r = 0; r < RW; ++r)
#pragma unroll
                    for (int nh = 0; nh < 2; ++nh) {
                        const int o0 = b16[s_][nh];                                             // XH; last tap: [x_hi | x_hi]
                        const int o1 = s_ == 4 ? (b16[4][nh] ^ ((un ^ 1) << 5)) : (b16[s_][nh] ^ 32);   // XL; last tap: [x_lo | x_hi]
                        Bf[buf][r][nh][0] = *reinterpret_cast<const f32x4*>(st + o0 + r * (PW * 64));
                        Bf[buf][r][nh][1] = *reinterpret_cast<const f32x4*>(st + o1 + r * (PW * 64));
                    }
            };
            load_step(0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s_ = 0; s_ < 5; ++s_) {
                const int buf = s_ & 1;
                if (s_ + 1 < 5) load_step(s_ + 1, buf ^ 1);
                if (NESR_ABL & 8) {
                    acc16[0][0][0][0][0] += Af[buf][0][0][0] + Af[buf][NMT - 1][1][0] + Bf[buf][0][0][0][0] + Bf[buf][RW - 1][1][1][0];
                    continue;
                }
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt) {
                    const f16x8 a0 = __builtin_bit_cast(f16x8, Af[buf][mt][0]), a1 = __builtin_bit_cast(f16x8, Af[buf][mt][1]);
#pragma unroll
                    for (int r = 0; r < RW; ++r)
#pragma unroll
                        for (int nh = 0; nh < 2; ++nh) {
                            const f16x8 x0_ = __builtin_bit_cast(f16x8, Bf[buf][r][nh][0]), x1_ = __builtin_bit_cast(f16x8, Bf[buf][r][nh][1]);
                            if (s_ < 4) mfma_tap3(a0, a1, x0_, x1_, acc16[r][nh][mt][0], acc16[r][nh][mt][1]);
                            else mfma_tap2(a0, a1, x0_, x1_, acc16[r][nh][mt][0], acc16[r][nh][mt][1]);
                        }
                }
                // the next step's 2 NMT + 4 RW fragment reads ride between this step's MFMAs (two MFMAs, one read)
                // instead of in front of them
                if (s_ + 1 < 5) {
#pragma unroll
                    for (int i = 0; i < 2 * NMT + 4 * RW; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        STAMP(11 + 4 * c);
    }
    STAMP(2);
    if (!active) return;
    if (NESR_ABL & 4) {
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int e = 0; e < 16; ++e) sum += acc16[r][e & 1][(e >> 1) & 1][(e >> 2) & 1][e & 3];
        if (sum == 12345.678f) static_cast<float*>(a.out)[0] = sum;
        return;
    }

    // ---- epilogue: after the cout exchange a lane holds 8 consecutive couts of its pixel, from cb16 on
    const int cb = cb16;
    const uint16_t* res1 = static_cast<const uint16_t*>(a.res1);
    const uint16_t* res2 = static_cast<const uint16_t*>(a.res2);
    uint16_t* out = static_cast<uint16_t*>(a.out);
    uint16_t* out2 = static_cast<uint16_t*>(a.out2);
    bool bad = false;
    // conv_last: a range failure anywhere upstream in this forward (sticky word, set by earlier launches on this
    // stream) turns the image into NaN instead of a saturated picture
    const bool poison = a.cout_real > 0 && a.status && __builtin_nontemporal_load(a.status) != 0u;
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int nh = 0; nh < 2; ++nh) {
            const int Y = y0 + RW * wave + r, X = x0 + 16 * nh + j16;
            const bool valid = X < a.w_ && Y < y_hi;
            const size_t pix = ((size_t)n * a.h + (Y < a.h ? Y : 0)) * a.w_ + (X < a.w_ ? X : 0);
            f32x4 v0, v1;   // couts cb .. cb+3, cb+4 .. cb+7
            cout_exchange_acc(acc16[r][nh][0], acc16[r][nh][1], v0, v1);
            v0 += bz0;
            v1 += bz1;
            if (a.lrelu) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { v0[i] = fmaxf(v0[i], v0[i] * 0.2f); v1[i] = fmaxf(v1[i], v1[i] * 0.2f); }   // LeakyReLU(0.2), same values as the select form
            }
            // slot of this pixel in chunk X = (coff + 32 cg) / 16 of a map, at this lane's piece
            auto slot = [&](const Map& mp, int coff) -> size_t { return (size_t)((coff + 32 * cg) >> 4) * mp.chunk + pix * mp.pix + piece8; };
            if (res1) {
                f32x4 q0, q1;
                load_regrouped(res1 + slot(a.res1_map, 0), a.res1_map.chunk, q0, q1);
#pragma unroll
                for (int i = 0; i < 4; ++i) { v0[i] = scale_add_2r(v0[i], a.s1, q0[i]); v1[i] = scale_add_2r(v1[i], a.s1, q1[i]); }
            }
            if (res2) {
                f32x4 q0, q1;
                load_regrouped(res2 + slot(a.res2_map, 0), a.res2_map.chunk, q0, q1);
#pragma unroll
                for (int i = 0; i < 4; ++i) { v0[i] = scale_add_2r(v0[i], a.s2, q0[i]); v1[i] = scale_add_2r(v1[i], a.s2, q1[i]); }
            }
            if (out || out2) {
                uint4 cx, cx1;
                bool bad_here = false;
                split_regroup(v0, v1, cx, cx1, bad_here);
                bad |= bad_here && valid;
                if (valid && out) {
                    uint16_t* p = out + slot(a.out_map, a.out_coff);
                    store16(p, cx);
                    store16(p + a.out_map.chunk, cx1);
                }
                if (valid && out2) {
                    uint16_t* p = out2 + slot(a.out2_map, 0);
                    store16(p, cx);
                    store16(p + a.out2_map.chunk, cx1);
                }
            }
            if (!valid) continue;
            if (a.cout_real > 0 && cb == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q >= a.cout_real) break;
                    const float x = poison ? __builtin_nanf("") : v0[q];
                    if (a.out_nchw) a.out_nchw[(((size_t)n * a.cout_real + q) * a.h + Y) * a.w_ + X] = x;
                    if (a.out_u8) {
                        float qv = fminf(fmaxf(x, 0.f), 1.f) * 255.0f;
                        qv = a.u8_round ? rintf(qv) : truncf(qv);
                        const int ch = a.u8_flip ? (a.cout_real - 1 - q) : q;
                        a.out_u8[pix * a.cout_real + ch] = (uint8_t)qv;
                    }
                }
            }
        }
    if (bad && a.status) __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    STAMP(3);
#if NESR_ABL & 64
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(4);
#endif
}

template <int DMAW, int NMT = 2>
hipError_t launch_split(const ConvArgs& a, hipStream_t s) {
    typedef Geo<DMAW> G;
    constexpr size_t shm = (size_t)ISLOTS * G::IN_BYTES + 2 * (size_t)W_BYTES;
    static unsigned long long attr_done = 0;
    {
        const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&conv3x3_f16x2_kernel<DMAW, NMT>), shm, attr_done);
        if (e != hipSuccess) return e;
    }
    const int rows = (a.y_hi > 0 ? a.y_hi : a.h) - a.y_lo;
    const long total = (long)((a.w_ + TW - 1) / TW) * ((rows + G::TH - 1) / G::TH) * a.n * (a.coutp / 32);
    if (total <= 0) return hipSuccess;
    if (total > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((conv3x3_f16x2_kernel<DMAW, NMT>), dim3((unsigned)total), dim3(G::LAUNCH_THREADS), shm, s, a);
    return hipGetLastError();
}

}  // namespace

#if NESR_ABL & 64
extern "C" int nesr_debug_stamps(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * (n < 256 ? n : 256));
}
#endif

size_t packed_weight_elems_f16x2(int cin_p, int coutp) { return (size_t)cin_p * 9 * coutp * 2; }

// OIHW f32 -> [chunk = ci/16][cout group = o/32][tap][plane hi|lo][k half = (ci%16)/8][o%32][ci%8] halves
void pack_weights_f16x2(const float* oihw, int cout, int cin, int cin_p, int coutp, uint16_t* dst) {
    const size_t total = packed_weight_elems_f16x2(cin_p, coutp);
    for (size_t i = 0; i < total; ++i) dst[i] = 0;
    const int groups = coutp / 32;
    for (int o = 0; o < cout; ++o)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < 9; ++tap) {
                // |w| <= 65504 and finite: nesr_finalize_weights rejects anything else (NESR_ERR_RANGE)
                const float wv = oihw[((size_t)o * cin + ci) * 9 + tap];
                const uint16_t hi = f2h(wv);
                const uint16_t lo = f2h((wv - h2f(hi)) * LO_SCALE);
                const int c = ci / 16, kh = (ci % 16) / 8, kk = ci % 8;
                const size_t slab = ((size_t)c * groups + o / 32) * (size_t)(W_ITEMS * 8);
                const size_t ihi = slab + ((((size_t)tap * 2 + 0) * 2 + kh) * 32 + o % 32) * 8 + kk;
                const size_t ilo = slab + ((((size_t)tap * 2 + 1) * 2 + kh) * 32 + o % 32) * 8 + kk;
                dst[ihi] = hi;
                dst[ilo] = lo;
            }
}

hipError_t launch_conv3x3_f16x2(const ConvArgs& a, hipStream_t s) {
    if (a.cin % 16 || (a.coutp != 32 && a.coutp != 64)) return hipErrorInvalidValue;
    if (a.y_lo < 0 || (a.y_hi > 0 && (a.y_hi > a.h || a.y_hi <= a.y_lo)) || (a.y_hi == 0 && a.y_lo != 0)) return hipErrorInvalidValue;
    if ((long long)a.in_w * 64 * 12 >= (1ll << 32)) return hipErrorInvalidValue;   // 32-bit byte offsets inside one tile's rows
    if (a.in_map.pix != 32 || (a.out && (a.out_map.pix % 32 || a.out_coff % 16))) return hipErrorInvalidValue;
    if ((a.out_nchw || a.out_u8) && (a.coutp != 32 || a.cout_real < 1 || a.cout_real > 4)) return hipErrorInvalidValue;
    // 8x32-px tiles.  Launches that give a CU at most one workgroup (a 512x512 frame's 32-channel layers): four
    // extra waves issue the DMAs, so the MFMA waves never stall on LDS-DMA issue (~85 cycles each, 10 per chunk
    // and wave; in-kernel stamps: -15 % per K-chunk).  With two workgroups per CU the other workgroup already
    // fills those gaps and the extra waves only cost occupancy (measured +21 % on 6 tiles of 532x532).
    static const int cus = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
        return n;
    }();
    static const int dmaw = [] { const char* e = getenv("NESR_SPLIT_DMAW"); return e ? atoi(e) : -1; }();
    const long t1 = (long)((a.w_ + TW - 1) / TW) * (((a.y_hi > 0 ? a.y_hi : a.h) - a.y_lo + 7) / 8) * a.n * (a.coutp >> 5);
    // ... and only when this context has the device to itself: with frames in flight on other streams the 8-wave
    // workgroups (166 registers) keep a second kernel's workgroups off the CU (2 frames in flight: 158 -> 166 MP/s
    // without them; one frame alone: 134 -> 138 MP/s with them)
    const bool producer = dmaw >= 0 ? dmaw > 0 : (t1 <= cus && !a.shared_device);
    note_conv_kernel(CONV_KERNEL_F16_PAIR);
    // conv_last (image outputs of <= 4 channels, no feature map): one 16-cout column block instead of two, by the caller's
    // setting alone (ConvArgs::narrow_last), never by the shape
    if (a.narrow_last && (a.out_nchw || a.out_u8) && !a.out && !a.out2 && !a.res1 && !a.res2)
        return producer ? launch_split<4, 1>(a, s) : launch_split<0, 1>(a, s);
    return producer ? launch_split<4>(a, s) : launch_split<0>(a, s);
}

}  // namespace nesr