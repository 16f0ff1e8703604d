// The fused f32 dense block: one residual dense block per launch, in the f16-pair arithmetic of conv3x3_f16x2.hip (frames whose 8x32-pixel tiles fit the CUs, e.g. 512x512 x2plus: 256 tiles).
//
// A per-layer launch of such a frame is one round of 256-512 workgroups that all wait for their first bytes at the
// same time, all compute, all store: ~6.6 us of every ~20 us launch is not matrix work.  Here
// a workgroup keeps its tile through conv1..conv5 of the block: 40 K-chunk steps (4 + 6 + 8 + 10 + 12) in ONE
// software pipeline -- the DMA waves run ahead straight across the layer boundaries, the LDS-DMA plan is
// computed once, and a layer's stores drain while the next layer's first chunks are already being multiplied.
// conv1..conv4 have 32 output channels: a step is one input chunk and one weight slab.  conv5 has 64: a step is one
// input chunk and the chunk's TWO weight slabs, and every MFMA wave carries both cout groups' accumulators (64
// registers), so the input tile is fetched and its pixel fragments are read once for all 64 channels, and conv5 has no
// layer boundary in its middle.  The input ring has 4 slots (fetched three steps ahead); the weight ring has 4 slabs,
// addressed in slab units: one per step in conv1..conv4 (three steps ahead), two per step in conv5 (this step's and the
// next one's: one step ahead, each step being twice as long).
//
// The only thing a layer needs from other workgroups is the 1-pixel halo of the 32 channels the previous layer has
// just produced -- and in a dense block those are the LAST two of its 6..12 input chunks.  So the wait is placed there:
// the DMA waves poll the neighbours' progress words (one per tile: x1..x4 published) just before they fetch those two
// chunks, several microseconds after the neighbours stored them.  Protocol (MI355X_MICROARCH.md, inter-workgroup
// visibility): producer = write-through (sc1) 16-byte stores, every storing wave's s_waitcnt vmcnt(0), the
// workgroup barrier, one lane's relaxed agent-scope store of the progress word; consumer = relaxed agent-scope
// (sc1) polls by the wave that then issues the loads, loads that bypass L1 (sc1).  Nothing is read before it has
// been written inside one launch and a kernel boundary invalidates L1/L2, so no line can be stale.  Every tile has its
// own resident workgroup (grid <= CUs, one workgroup per CU): waits are bounded and set an abort word instead of hanging.
//
// The step schedule and its proof are rdb_f16x2_schedule.h; geometry and MFMA helpers shared with the per-layer kernel
// are f16x2_common.h.
#include <type_traits>

#include "f16x2_common.h"
#include "nesr_kernels.h"
#include "rdb_f16x2_schedule.h"

namespace nesr {

namespace {

// Switches whose question is answered are gone; a build that sets one must not silently be the default.
#if defined(NESR_RDB_PAR) || defined(NESR_RDB_EPI_STEPS) || defined(NESR_RDB_DMAPRIO) || defined(NESR_RDB_YPRIO) || NESR_RDB_LAG == 0
#error "NESR_RDB_PAR, NESR_RDB_EPI_STEPS, NESR_RDB_DMAPRIO, NESR_RDB_YPRIO and NESR_RDB_LAG=0 were removed; the last commit that had them is 19ed2fc (tools/build_variant.sh 19ed2fc out.so -D... still builds it)"
#endif

#ifndef NESR_RDB_ABL
#define NESR_RDB_ABL 0   // timing ablations, a sum of the bits below (WRONG results, except stamps)
#endif
namespace abl {
constexpr bool no_poll = NESR_RDB_ABL & 1;         // no neighbour polling
constexpr bool plain_loads = NESR_RDB_ABL & 2;     // activation LDS-DMAs without sc1
constexpr bool plain_stores = NESR_RDB_ABL & 4;    // x1..x4 by write-back stores
constexpr bool no_mfma = NESR_RDB_ABL & 8;
constexpr bool no_epilogue = NESR_RDB_ABL & 16;
constexpr bool no_in_dma = NESR_RDB_ABL & 32;
constexpr bool no_w_dma = NESR_RDB_ABL & 64;
// 256 (stamps): the in-kernel timeline below (tools/probes/rdb_stamps.py); right results
constexpr bool no_barrier = NESR_RDB_ABL & 512;    // races
constexpr bool no_dma = no_in_dma || no_w_dma;     // the counted waits would wait for instructions that were not issued
}  // namespace abl

// The timeline of workgroup 77 (bit 256); every macro expands to nothing without it.  `mstep` = the MFMA role's step counter.
// RSTAMP_M keeps its wave test inside: an `if` around an empty statement is enough to change the default build's registers.
#if NESR_RDB_ABL & 256
__device__ unsigned long long g_rdb_stamps[2][64][8];     // [role: MFMA wave 1 | DMA wave 0][step][event]
__device__ unsigned long long g_rdb_taps[2][8][8];         // [MFMA wave 1 | 5 (one SIMD)][step - 20][start of tap-step 0..4, end]
__device__ unsigned long long g_rdb_arrive[12][8][2];      // [wave][step - 20][arrival at | release from the step's barrier]
#define RARRIVE(w, step, ev) do { if (blockIdx.x == 77 && lane == 0 && (step) >= 20 && (step) < 28) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); g_rdb_arrive[w][(step) - 20][ev] = t_; } } while (0)
#define RSTAMP(role, step, ev) do { if (blockIdx.x == 77 && lane == 0) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); g_rdb_stamps[role][step][ev] = t_; } } while (0)
#define RMSTEP_INIT() int mstep = 0
#define RSTAMP_M(ev) do { if (wave == 1) RSTAMP(0, mstep, ev); } while (0)      // MFMA wave 1, event ev of its current step
#define RARRIVE_M(d, ev) RARRIVE(wave, mstep + (d), ev)      // an MFMA wave at the barrier of its step mstep + d
#define RMSTEP_NEXT() ++mstep
#define RKEEP(x, y) asm volatile("" :: "v"(x), "v"(y))      // the values exist before the stamp that follows
#define RTAPS_INIT() unsigned long long tt_[6]
#define RTAP(i, fence) do { tt_[i] = __builtin_amdgcn_s_memtime(); if (fence) __builtin_amdgcn_sched_barrier(0); } while (0)      // no wait here: read at the end of the step
#define RTAPS_WRITE() do { if (blockIdx.x == 77 && (wave == 1 || wave == 5) && lane == 0 && mstep >= 20 && mstep < 28) { \
    _Pragma("unroll") for (int i_ = 0; i_ < 6; ++i_) g_rdb_taps[wave == 5][mstep - 20][i_] = tt_[i_]; } } while (0)
// shader clock = d memtime / d memrealtime x 100 MHz, between the first and the last step (DMA wave 0)
#define RCLOCKS(step) do { if (((step) == 0 || (step) == RDB_STEPS - 1) && wave == 0 && blockIdx.x == 77 && lane == 0) { \
    const unsigned long long r_ = __builtin_amdgcn_s_memrealtime(), t_ = __builtin_amdgcn_s_memtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    g_rdb_stamps[1][(step) == 0 ? 62 : 63][0] = r_; g_rdb_stamps[1][(step) == 0 ? 62 : 63][1] = t_; } } while (0)
#define RSTAMP_RETIRED() do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (wave == 1) RSTAMP(0, 61, 1); } while (0)      // the final epilogue's last store has retired
#else
#define RSTAMP(role, step, ev) do { } while (0)
#define RARRIVE(w, step, ev) do { } while (0)
#define RMSTEP_INIT() do { } while (0)
#define RSTAMP_M(ev) do { } while (0)
#define RARRIVE_M(d, ev) do { } while (0)
#define RMSTEP_NEXT() do { } while (0)
#define RKEEP(x, y) do { } while (0)
#define RTAPS_INIT() do { } while (0)
#define RTAP(i, fence) do { } while (0)
#define RTAPS_WRITE() do { } while (0)
#define RCLOCKS(step) do { } while (0)
#define RSTAMP_RETIRED() do { } while (0)
#endif

struct RdbArgs {
    const void* cur;         // the block's 192-channel buffer: x0 read, x1..x4 written then read
    long long chunk_bytes;   // bytes between its 16-channel chunks (pixels * 64)
    void* out;               // conv5's destination: the x0 slice of the next block's buffer (same geometry)
    const void* res2;        // second residual (the RRDB's input, x0 slice of its first buffer) or null
    float s1, s2;
    const void* w[5];        // packed weights of conv1..conv5 (pack_weights_f16x2)
    const float* bias[5];
    int n, h, w_;
    unsigned* progress;      // [tiles] epoch + layers published
    unsigned epoch;          // progress == epoch + j  <=>  x_j of this launch is visible
    unsigned* abort_flag;
    unsigned* status;        // sticky range word (ConvArgs::status)
    unsigned long long timeout_ticks;   // s_memrealtime ticks (100 MHz) a neighbour wait may take
};

__device__ __forceinline__ void glds16_s_sc1(const char* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2 sc1\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}
__device__ __forceinline__ void store16_wt_s(const char* sbase, unsigned voff, uint4 v) {   // write-through (visible device-wide once vmcnt retires it): wave-uniform base + 32-bit lane offset
    asm volatile("global_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" ::"v"(voff), "v"(__builtin_bit_cast(f32x4, v)), "s"(sbase) : "memory");
}
// Plain 16-byte load through a global (not flat) pointer, known to the compiler: it places the waits itself, counted
// (vmcnt(N)) where younger loads may stay in flight -- a flat access also counts in lgkmcnt and makes every wait vmcnt(0).
// (Not inline asm: a register that an uncounted load is still writing may be copied by the register allocator.)
__device__ __forceinline__ f32x4 load16_s(const char* sbase, unsigned voff) {
    return *(const __attribute__((address_space(1))) f32x4*)(sbase + voff);
}

// s_waitcnt vmcnt(k) for a wave-uniform run-time k (the count is an immediate)
__device__ __forceinline__ void wait_vmcnt_le(int k) {
    switch (k) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    }
}

constexpr int RSLOTS = 4;   // ring slots of the fused kernel: the DMA waves run two steps ahead in conv1..conv4 (step s has landed at barrier s), three in conv5 (rdb_f16x2_schedule.h)
constexpr int W5_ROUNDS = 2 * W_ITEMS / (64 * 4);
static_assert(RSLOTS == 4 && RDB_STEP5 % RSLOTS == 0 && W5_ROUNDS * 64 * 4 == 2 * W_ITEMS, "conv5's slab pairs sit at ring positions 0,1 / 2,3 and fill whole DMA rounds");
constexpr int MW = 8;       // MFMA waves of the fused kernel: one tile row each, two per SIMD
constexpr int DW = 4;       // DMA waves: LDS-DMA, neighbour polling, progress words
// A finished layer's epilogue rides in the first step of the next one, and no later: the DMA waves fetch at most RSLOTS - 1
// steps ahead, so the first x1 chunk of conv2 (its step 4) is requested in conv2's step 1 at the earliest, and that request
// polls this tile's own progress word among the nine -- which goes out EPI_STEPS steps into the layer.
constexpr int EPI_STEPS = 1;

// Roles.  MFMA waves (0..7): row w of the 8x32-pixel tile, 32 couts (conv5: 64): LDS fragment reads, MFMAs, and the epilogue of
// the PREVIOUS layer (conv5's own follows its last step) -- its sums wait in 16 registers (main + cross / 2^11) and are finished (bias,
// LeakyReLU / residuals, split, whole-line stores) at the start of the next layer's first step, by both waves of a SIMD
// at the same point.  Waves 4..7 run part of a step behind waves 0..3 inside conv1..conv4 (NESR_RDB_LAG).  Measured alternatives: the epilogue in the DMA waves, or in
// four waves of its own -- a VALU instruction of a wave that shares its SIMD with two MFMA waves gets one issue slot
// per MFMA, ~16 cycles each: layer boundaries cost 23 % of the kernel; staggered between the two MFMA waves of a SIMD
// (one before, one after its MFMAs) -- a VALU block beside the partner's MFMA stream crawls just the same.
// DMA waves (8..11): one step's LDS-DMAs two steps ahead in conv1..conv4, three in conv5 (4-slot ring; conv5's weight slabs one step ahead), polling of the neighbours' progress words
// before the first chunk of each x_l, and this tile's own progress word EPI_STEPS steps into the next layer.
//
// CHAIN (rdb_f16x2_chain_kernel): the same body for a run of `nblocks` consecutive dense blocks of one forward.  Block k of
// the launch takes cur / out / res2 and its weight and bias pointers from table[k] (a.cur .. a.bias are not used) and
// publishes epoch + 8 k + 1 .. + 5; a new level 5 means "`out` visible", published like x1..x4: write-through stores,
// every storing wave's vmcnt(0), a workgroup barrier (the block's last, behind the final epilogue: no wave reads the
// rings or the bias table past it), one lane's relaxed agent-scope store.  Behind that barrier the DMA waves issue the
// next block's first IN_LEAD weight slabs, wait for level 5 of block k - 1 from all nine tiles, and issue its first
// input chunks (conv1 reads the neighbours' `out` in its very first chunk); the MFMA waves refill the bias table.  The
// plan, the zero padding and the geometry are per launch; the 40-step walk is per block (rdb_f16x2_schedule.h,
// chain_reentry_ok).
// Buffer reuse: three buffers rotate, so what block k + 1 writes (x1..x4 into its own buffer, `out` into the next one's
// x0 slice) was last read by block k - 2, or by block k - 1 where `out` lands in the buffer block k - 1 ran in -- reads
// of the nine tiles only.  A tile starts block k + 1 behind level 5 of block k of all nine, and a tile that has
// published level 5 of block k has finished every read of blocks <= k (its last barrier stands behind them): no write
// of block k + 1 can meet a read of an earlier block (rdb_f16x2_schedule.h, chain_war_ok).  Every load of bytes that
// another workgroup wrote is an sc1 LDS-DMA and every such byte an sc1 store, in a chain as in a single block -- but a
// chained launch does re-read lines that another workgroup has rewritten since (a rotated buffer, three blocks on): that
// no stale copy is served there is measured ("Across blocks"), not guaranteed by the architecture.
template <bool CHAIN>
__device__ __forceinline__ void rdb_blocks(RdbArgs a, const RdbChainBlock* table, int nblocks) {
    typedef Geo<4> G;
    constexpr int THREADS = G::THREADS, TH = G::TH;      // THREADS = DMA lanes (256), TH = 8 rows
    constexpr int IN_ITEMS = G::IN_ITEMS, IN_ROUNDS = G::IN_ROUNDS, IN_BYTES = G::IN_BYTES;
    constexpr int W_ROUNDS = (W_ITEMS + THREADS - 1) / THREADS;
    constexpr int WRING = RSLOTS * IN_BYTES;             // LDS: [input ring][weight ring][bias table]
    constexpr int BIAS = RSLOTS * (IN_BYTES + W_BYTES);  // 6 x 32 f32: conv1..conv4, conv5 couts 0-31, conv5 couts 32-63
    static_assert(TH == MW, "one tile row per MFMA wave");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool is_dma = wave_all >= MW;
    const bool is_cmp = !is_dma;
    const int wave = is_cmp ? wave_all : wave_all - MW;
    const int tid = wave * 64 + lane;

    const int tiles_x = (a.w_ + TW - 1) / TW;
    const int tiles_y = (a.h + TH - 1) / TH;
    const int total = tiles_x * tiles_y * a.n;
    const int tile = xcd_work_index(total);
    const int n = tile / (tiles_x * tiles_y);
    const int t2 = tile - n * tiles_x * tiles_y;
    const int ty = t2 / tiles_x, tx = t2 - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;

    // CHAIN: the pointers of the block in hand are read from its table entry where they are used, through the scalar cache
    // (the host writes the table before the launch).  The entry pointer is all a block keeps in registers: the scalar
    // file is full too, and a changed copy of `a` indexed by a run-time layer would live in scratch.
    typedef const __attribute__((address_space(4))) RdbChainBlock* entry_ptr;
    entry_ptr ent = (entry_ptr)table;
    auto cur_of = [&]() -> const void* { if constexpr (CHAIN) return ent->cur; else return a.cur; };
    auto out_of = [&]() -> const void* { if constexpr (CHAIN) return ent->out; else return a.out; };
    auto res2_of = [&]() -> const void* { if constexpr (CHAIN) return ent->res2; else return a.res2; };
    auto w_of = [&](int l) -> const void* { if constexpr (CHAIN) return ent->w[l]; else return a.w[l]; };
    auto bias_of = [&](int l) -> const float* { if constexpr (CHAIN) return ent->bias[l]; else return a.bias[l]; };
    unsigned epoch = a.epoch;      // of the block in hand

    // (layer, chunk) of the step after (l, c); l == 5: past the end.  A conv5 step is one chunk of all 64 output channels.
    auto advance = [](int& l, int& c) {
        const int nc = l == 4 ? 12 : 4 + 2 * l;
        if (++c == nc) { c = 0; ++l; }
    };

    // The two roles run separate loops over the same RDB_STEPS steps (one s_barrier per step, one more before the first):
    // their register sets never coexist.
    if (is_dma) {
        if (wave == 0) RSTAMP(1, 61, 0);      // kernel entry
        // ---- the plan (once per block) and the neighbours' progress words
        const unsigned lds_base = (unsigned)(size_t)(lds_char*)(smem);
        unsigned voff[IN_ROUNDS];
        unsigned okmask = 0;       // per lane: rounds in which this lane has an in-image item
        unsigned wavemask = 0;     // wave-uniform: rounds in which any lane of the wave has one (= instructions issued)
        const int row0 = y0 > 0 ? y0 - 1 : 0;
        const char* in_img = static_cast<const char*>(cur_of()) + ((size_t)n * a.h + row0) * a.w_ * 64;
        const unsigned* watch = nullptr;    // lanes 0..8: progress word of tile (ty + i/3 - 1, tx + i%3 - 1), if it exists
        int kin = 0, kw = 0;                // LDS-DMA instructions this wave issues per input chunk / per 32-cout weight slab (vmcnt counts wave instructions)
        if (lane < 9) {
            const int ny = ty + lane / 3 - 1, nx = tx + lane % 3 - 1;
            if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x) watch = a.progress + (n * tiles_y + ny) * tiles_x + nx;
        }
        {
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
                voff[i] = ((unsigned)(Y - row0) * (unsigned)a.w_ + (unsigned)X) * 64u + sg * 16;
                okmask |= ok ? (1u << i) : 0u;
                if (__builtin_amdgcn_ballot_w64(ok) != 0ull) { wavemask |= 1u << i; ++kin; }
                if (has && !ok) {
#pragma unroll
                    for (int sl2 = 0; sl2 < RSLOTS; ++sl2) *reinterpret_cast<f32x4*>(smem + sl2 * IN_BYTES + k * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                px += (THREADS / 4) % PW;
                py += (THREADS / 4) / PW;
                if (px >= PW) { px -= PW; py += 1; }
            }
#pragma unroll
            for (int j = 0; j < W_ROUNDS; ++j) kw += (wave * 64 + THREADS * j) < W_ITEMS ? 1 : 0;
        }
        unsigned seen = 0;     // layers of this launch known to be published by all nine tiles
        // an abort word raised earlier in this forward (or by another workgroup): nothing is waited for any more -- the forward's
        // output is invalid either way and the host turns the word into NESR_ERR_HIP (nesr_check_range)
        // (read below, behind the first issues: dma_in looks at it from step 1 on)
        bool gave_up = false;
        // The weight ring is addressed in 32-cout slabs (RSLOTS of them).  conv1..conv4: one slab per step, slab position =
        // step & 3, fetched three steps ahead like the input.  conv5: the chunk's two slabs ([chunk][cout group], contiguous in
        // the packed weights and in the ring: 2 x W_ITEMS = 9 full rounds) at positions 0,1 / 2,3 -- the ring holds the
        // current and the next step, so they are fetched one step ahead (conv5 starts at a multiple of RSLOTS steps).
        auto dma_w = [&](int l, int c, int wpos) {
            const char* wsrc = static_cast<const char*>(w_of(l)) + (size_t)c * W_BYTES;
#pragma unroll
            for (int j = 0; j < W_ROUNDS; ++j) {
                const int k = tid + THREADS * j;
                const unsigned dst = lds_base + WRING + wpos * W_BYTES + j * (THREADS * 16) + wave * 1024;
                if (k < W_ITEMS && !abl::no_w_dma) glds16_s(wsrc, (unsigned)k * 16u, __builtin_amdgcn_readfirstlane(dst));
            }
        };
        auto dma_w5 = [&](int c, int wpos) {
            const char* wsrc = static_cast<const char*>(w_of(4)) + (size_t)c * (2 * W_BYTES);
#pragma unroll
            for (int j = 0; j < W5_ROUNDS; ++j) {
                const unsigned dst = lds_base + WRING + wpos * W_BYTES + j * (THREADS * 16) + wave * 1024;
                if (!abl::no_w_dma) glds16_s(wsrc, (unsigned)(tid + THREADS * j) * 16u, __builtin_amdgcn_readfirstlane(dst));
            }
        };
        // all nine tiles have published `target`; c = the chunk that waits (goes into the abort word)
        auto wait_nine = [&](unsigned target, int c) {
            {
                unsigned long long t0 = 0;
                for (unsigned it = 0;; ++it) {
                    const unsigned v = watch ? __hip_atomic_load(watch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : target;
                    if (__builtin_amdgcn_ballot_w64((int)(v - target) < 0) == 0ull) break;
                    if ((it & 63u) == 0u) {
                        // bounded by wall clock: a neighbour that never arrives (workgroups not co-resident: another process's
                        // persistent kernel on the device) ends in an abort word within timeout_ticks, and once the word is up --
                        // here or in any other workgroup -- every later wait of the launch and of the forward is skipped
                        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                        if (it == 0) t0 = now;
                        const unsigned ab = __hip_atomic_load(a.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (ab != 0u || now - t0 > a.timeout_ticks) {
                            if (ab == 0u && lane == 0) __hip_atomic_store(a.abort_flag, 1u | ((unsigned)c << 8) | ((unsigned)tile << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            gave_up = true;
                            break;
                        }
                    }
                    __builtin_amdgcn_s_sleep(4);
                }
            }
        };
        // input chunk c -- after the nine tiles have published the layer that produced it (chunks 4.. hold x1..: chunk c
        // belongs to x_((c-4)/2+1)).  Exactly kin wave instructions.
        auto dma_in = [&](int c, int slot) {
            const unsigned need = c < 4 ? 0u : (unsigned)((c - 4) >> 1) + 1u;
            if (need > seen && !gave_up && !abl::no_poll) {
                wait_nine(epoch + need, c);
                seen = need;
            }
            const char* isrc = in_img + (long long)c * a.chunk_bytes;
#pragma unroll
            for (int i = 0; i < IN_ROUNDS; ++i) {
                const unsigned dst = lds_base + slot * IN_BYTES + i * (THREADS * 16) + wave * 1024;
                if (((wavemask >> i) & 1u) && !abl::no_in_dma) {          // wave-uniform: the instruction count is the same every step
                    if ((okmask >> i) & 1u) {
                        if (abl::plain_loads) glds16_s(isrc, voff[i], __builtin_amdgcn_readfirstlane(dst));
                        else glds16_s_sc1(isrc, voff[i], __builtin_amdgcn_readfirstlane(dst));
                    }
                }
            }
        };
        // Nothing in front of the first LDS-DMAs waits for memory, and no full vmcnt wait stands between them: the bias
        // table is filled by the MFMA waves, and the abort word is a scalar load (lgkmcnt) issued behind them.
      for (int blk = 0;; ++blk) {      // CHAIN: the blocks of the launch; otherwise one pass
        int fl = 0, fc = 0;      // the next step to fetch
        int inflight;            // instructions of the latest issue that the next barrier does not need
        if (!CHAIN || blk == 0) {
#pragma unroll
            for (int i = 0; i < rdbs::IN_LEAD; ++i) {
                dma_w(0, i, i);
                dma_in(i, i);
                advance(fl, fc);
            }
            // The word can only have been raised by an earlier launch of this forward at this point (a kernel boundary away:
            // the scalar cache cannot hold a stale copy); what other workgroups raise during the launch is seen by the polls.
            gave_up = *(const __attribute__((address_space(4))) unsigned*)a.abort_flag != 0u;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the zero padding is in LDS before the first barrier
            // chunk 0 has landed: the MFMA waves request the launch's first fragments behind the next barrier
            wait_vmcnt_le(abl::no_dma ? 0 : (rdbs::IN_LEAD - 1) * (kw + kin));
            inflight = kw + kin;
        } else {
            // Re-entry (behind the previous block's last barrier: no wave reads a ring position any more).  The weights do
            // not depend on any other workgroup: all IN_LEAD slabs go out before the poll.  The input chunks are the
            // nine tiles' `out` of the previous block: behind its level 5.  Issue order w0 w1 w2 in0 in1 in2, so the
            // counted waits leave in1 and in2 in flight at the block's first barrier and in2 at barrier 0.
#pragma unroll
            for (int i = 0; i < rdbs::IN_LEAD; ++i) dma_w(0, i, i);
            if (!gave_up && !abl::no_poll) wait_nine(epoch - 8u + 5u, 0);
#if NESR_RDB_ABL & 256
            if (blk + 1 == nblocks && wave == 0) RSTAMP(1, 59, 2);      // the last block: the nine tiles' level 5 seen
#endif
#pragma unroll
            for (int i = 0; i < rdbs::IN_LEAD; ++i) {
                dma_in(i, i);
                advance(fl, fc);
            }
            wait_vmcnt_le(abl::no_dma ? 0 : rdbs::REENTRY_TAIL_FIRST * kin);
            inflight = rdbs::REENTRY_TAIL_0 * kin;
        }
        int fill = rdbs::IN_LEAD;      // ring position of the next step to fetch (= that step & 3)
        int cl = 0, cc = 0;      // the current step
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        for (int step = 0; step < RDB_STEPS; ++step) {
            // everything the MFMA waves read before the next barrier has landed: this step and the first fragments of the next
            // (conv5: the next step's pixels only); what was issued one step ago for later may stay in flight
            if (wave == 0) RSTAMP(1, step, 0);
            RCLOCKS(step);
            wait_vmcnt_le(abl::no_dma ? 0 : inflight);
            if (wave == 0) RSTAMP(1, step, 1);
            RARRIVE(MW + wave, step, 0);
            if (!abl::no_barrier) __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            RARRIVE(MW + wave, step, 1);
            if (wave == 0) RSTAMP(1, step, 2);
            // layer cl - 1 of this tile is in memory: its MFMA waves stored it during steps 0 .. EPI_STEPS - 1 of layer cl
            // and waited for those stores (vmcnt(0)) before this barrier
            if (cc == EPI_STEPS && cl >= 1 && wave == 0 && lane == 0)
                __hip_atomic_store(a.progress + tile, epoch + (unsigned)cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // Issue order = the order the waits count in: what the next barrier needs first.
            // (the schedule and its proof: rdb_f16x2_schedule.h)
            if (rdbs::w_pair(step)) {
                // conv5's next step: both slabs into the half of the ring that step - 1 has just left; needed at the next barrier
                dma_w5(step + 1 - RDB_STEP5, ((step + 1) & 1) * 2);
            } else if (rdbs::w_slab(step)) {
                dma_w(fl, fc, fill);      // conv1..conv4: with the step's input chunk, into the same ring position
            }
            // two steps ahead in conv1..conv4, three in conv5 (two chunks in conv5's first interval), into slots no wave reads any more
            for (int k = rdbs::in_end(step) - rdbs::in_end(step - 1); k > 0; --k) {
                dma_in(fc, fill);
                advance(fl, fc);
                fill = fill == RSLOTS - 1 ? 0 : fill + 1;
            }
            inflight = rdbs::tail_w(step) * kw + rdbs::tail_in(step) * kin;
            if (wave == 0) RSTAMP(1, step, 3);
            advance(cl, cc);
        }
        if (!CHAIN) break;
        // Every LDS-DMA of the block has landed (barrier 39's wait is vmcnt(0)).  The next block's pointers arrive while the
        // MFMA waves run the final epilogue; behind the block's last barrier their `out` stores have retired: level 5.
        const bool more = blk + 1 < nblocks;
        if (more) {
            in_img += static_cast<const char*>(ent[1].cur) - static_cast<const char*>(ent[0].cur);
            ent += 1;
        }
#if NESR_RDB_ABL & 256
        if (blk + 2 == nblocks && wave == 0) RSTAMP(1, 59, 0);      // DMA wave 0 at the last barrier of the last block but one ...
#endif
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#if NESR_RDB_ABL & 256
        if (blk + 2 == nblocks && wave == 0) RSTAMP(1, 59, 1);      // ... and released from it
#endif
        if (wave == 0 && lane == 0) __hip_atomic_store(a.progress + tile, epoch + 5u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!more) break;
        epoch += 8u;
        seen = 0;
      }
        return;
    }

    // ---- MFMA role: operand addresses as in conv3x3_f16x2_kernel, one row per wave
    const bool active = (y0 + wave) < a.h;
    if (wave == 1) RSTAMP(0, 61, 0);
    bool bad = false;
    // a stored value beyond the pair format's range.  CHAIN: reported where it is found -- collected for the end of the
    // launch, the test would be put off to there too, its operands (the split values of every epilogue) waiting in registers.
    auto note_bad = [&](bool b) {
        if constexpr (CHAIN) {
            if (b && a.status) __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            bad |= b;
        }
    };
  for (int blk = 0;; ++blk) {      // CHAIN: the blocks of the launch; otherwise one pass
    // CHAIN: every block derives its lane's addresses and constants anew, from a lane id the compiler cannot see through.
    // Hoisted out of the block loop they would all stay live through the 40 steps, and the body has two registers to spare.
    // (the lane id itself from the execution mask -- every lane of a wave is here -- so that no register carries it either)
    int lane_blk = threadIdx.x & 63;
    if (CHAIN) {
        int zero = 0;
        asm volatile("" : "+v"(zero));
        lane_blk = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)zero)) & 63;
    }
    const int lane = lane_blk;
    const int j16 = lane & 15, g4 = lane >> 4;
    // The six bias vectors of the block sit in LDS (768 B: conv1..conv4, conv5's couts 0-31 and 32-63), first read at
    // step 4: a global load inside the step loop would cost a vmcnt wait per use.  Waves 0..5 (active or not) fetch one
    // vector each through a wave-uniform pointer while the DMA waves issue the first chunks; the first barrier publishes it.
    const bool fills_bias = wave < 6 && lane < 8;
    f32x4 bias_v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (fills_bias) bias_v = *(const __attribute__((address_space(1))) f32x4*)(bias_of(wave < 4 ? wave : 4) + (wave == 5 ? 32 : 0) + 4 * lane);
    if (CHAIN && !active) {
        // A wave without a row: its bias vector and the block's barriers (one in front of step 0's, one per step, one behind
        // the final epilogue).  On its own path, so that below `active` is known: registers that are written and read under
        // `active` only would otherwise count as live around the block loop, the previous block's contents in them.
        if (fills_bias) *reinterpret_cast<f32x4*>(smem + BIAS + wave * 128 + lane * 16) = bias_v;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int i = 0; i < rdbs::CHAIN_BARS; ++i) {
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        if (blk + 1 == nblocks) break;
        ent += 1;
        continue;
    }
    const int un = g4 >> 1, kh = g4 & 1;
    int b16[5][2], a16[5];
#pragma unroll
    for (int st_ = 0; st_ < 5; ++st_) {
#pragma unroll
        for (int nh = 0; nh < 2; ++nh) b16[st_][nh] = tap_pixel_offset(st_, wave, nh, j16, un, kh);
        a16[st_] = tap_weight_offset(st_, j16, un, kh);
    }
    int slot = 0;       // input ring slot of the current step
    int wpos = 0;       // weight ring slab of the current step (conv5: the first of its two)
    RMSTEP_INIT();
    // Fragment addresses live in registers as absolute LDS addresses of the slot they are read from next; each is used
    // once per step and moved on to the next slot right away (one v_add per register and step; the pixel half and the
    // weight variants are immediate offsets) instead of slot base + offset per read (one v_add per ds_read).
    typedef const __attribute__((address_space(3))) f32x4* lds_f32x4;
    const unsigned lds0 = (unsigned)(size_t)(lds_char*)(smem);
    // Pixels: one register per tap-step (XH; XL is the other plane: address ^ 32, for the last tap ^ xl4).  Weights: the
    // tap is an immediate offset from one of four registers -- tap-steps 0..2 (taps (un, dx)) from aw012, tap-step 3
    // (tap (2, un)) from aw3, tap-step 4 (tap (2, 2): [w_hi | 0] and [w_hi | w_lo]) from aw4 / aw4b -- which all move on
    // by one slab (conv5: two) at the end of a step.
    unsigned bcur[5], aw012, aw3, aw4, aw4b;
#pragma unroll
    for (int t = 0; t < 5; ++t) bcur[t] = lds0 + (unsigned)b16[t][0];
    const unsigned xl4 = (unsigned)((un ^ 1) << 5);
    aw012 = lds0 + (unsigned)(WRING + a16[0]);
    aw3 = lds0 + (unsigned)(WRING + a16[3]);
    aw4 = lds0 + (unsigned)(WRING + a16[4]);
    aw4b = aw4 + (unsigned)un * 1024u;
    // ---- the deferred epilogue
    const int cbl = (g4 & 1) * 16 + (g4 >> 1) * 8;      // a lane's 8 output channels inside a 32-cout group after the permlane16 exchange
    const int piece8 = ((g4 & 1) * 2 + (g4 >> 1)) * 8;  // its 16-byte piece of a 64-byte slot after regroup_pairs (2-byte units)
    f32x4 ep[2][2];                                     // [pixel half][cout half]: sums of the finished (layer, cout group)
#pragma unroll
    for (int nh = 0; nh < 2; ++nh)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) ep[nh][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int ep_l = -1;
    auto unpack_res = [&](f32x4 rx, f32x4 rx1, f32x4& q0, f32x4& q1) {
        uint4 cx = __builtin_bit_cast(uint4, rx), cx1 = __builtin_bit_cast(uint4, rx1);
        regroup_pairs(cx, cx1);      // -> own hi, own lo
        const f16x8 h = __builtin_bit_cast(f16x8, cx), lo = __builtin_bit_cast(f16x8, cx1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            q0[i] = fmaf((float)lo[i], LO_INV, (float)h[i]);
            q1[i] = fmaf((float)lo[4 + i], LO_INV, (float)h[4 + i]);
        }
    };
    // pixel half nh of (layer l, cout group cg): conv1..4 -> LeakyReLU into cur's channels 64 + 32 l; conv5 ->
    // x5 * s1 + x0 (and * s2 + RRDB input) into `out`'s channels 32 cg.  All 64 lanes (v_permlane16_swap).
    // Addresses: a wave-uniform row base (SGPRs) plus a 32-bit lane offset -- pixel slot and 16-byte piece -- so that
    // the epilogue carries two VGPRs of addressing instead of 64-bit pointers.
    const long long row_bytes = (((long long)n * a.h + (y0 + wave)) * a.w_) * 64;
    unsigned lane_off[2];
    bool lane_ok[2];
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
        const int X = x0 + 16 * nh + j16;
        lane_ok[nh] = X < a.w_;
        lane_off[nh] = (unsigned)(lane_ok[nh] ? X : 0) * 64u + (unsigned)piece8 * 2u;
    }
    auto uni = [](const char* p) -> const char* {      // tell the compiler the pointer is wave-uniform
        const unsigned long long v = (unsigned long long)p;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return (const char*)(((unsigned long long)hi << 32) | lo);
    };
    // pixel half nh of conv1..4 (layer l): LeakyReLU into cur's channels 64 + 32 l.  All 64 lanes (v_permlane16_swap).
    auto epi_half = [&](int l, const f32x4& e0, const f32x4& e1, int nh) {
        RSTAMP_M(3);
        const bool valid = lane_ok[nh];
        const unsigned voff = lane_off[nh];
        const char* bsrc = smem + BIAS + (l * 32 + cbl) * 4;
        f32x4 v0, v1;   // couts cbl .. cbl+3, cbl+4 .. cbl+7
        cout_exchange(e0, e1, v0, v1);
        v0 += *reinterpret_cast<const f32x4*>(bsrc);
        v1 += *reinterpret_cast<const f32x4*>(bsrc + 16);
        const int dchunk = 4 + 2 * l;
#pragma unroll
        for (int i = 0; i < 4; ++i) { v0[i] = fmaxf(v0[i], v0[i] * 0.2f); v1[i] = fmaxf(v1[i], v1[i] * 0.2f); }   // LeakyReLU(0.2), same values as the select form
        RKEEP(v0, v1);
        RSTAMP_M(4);
        uint4 cx, cx1;
        bool bad_here = false;
        split_regroup(v0, v1, cx, cx1, bad_here);
        note_bad(bad_here && valid);
        RKEEP(__builtin_bit_cast(f32x4, cx), __builtin_bit_cast(f32x4, cx1));
        RSTAMP_M(5);
        if (valid) {
            const char* d0 = uni(static_cast<const char*>(cur_of()) + (long long)dchunk * a.chunk_bytes + row_bytes);
            if (!abl::plain_stores) {
                store16_wt_s(d0, voff, cx);
                store16_wt_s(d0 + a.chunk_bytes, voff, cx1);
            } else {
                *reinterpret_cast<uint4*>(const_cast<char*>(d0) + voff) = cx;
                *reinterpret_cast<uint4*>(const_cast<char*>(d0) + a.chunk_bytes + voff) = cx1;
            }
        }
        RSTAMP_M(6);
    };
    // the pending epilogue: both pixel halves in the running layer's first step
    auto epi_pending = [&]() {
        if (abl::no_epilogue) return;
        epi_half(ep_l, ep[0][0], ep[0][1], 0);
        epi_half(ep_l, ep[1][0], ep[1][1], 1);
    };
    // conv5's residuals, piece p = 2 * (cout group) + (pixel half), as the two 16-byte lines (chunks 2g, 2g + 1) a lane
    // later writes: x0 of this block (R1) and, in the third block of an RRDB, the RRDB's input (R2).  In that block `out`
    // IS res2's buffer: a lane reads exactly the pieces it writes and no other workgroup touches them, so the one ordering
    // that matters is load before own store -- every load below is issued before the first store of the wave.  Lanes
    // past the image width load the row's first pixel (lane_off) and store nothing.
    f32x4 R1[4][2], R2[4][2];
    auto issue_res = [&](const void* base, int g, f32x4 (&R)[4][2]) {
        const char* r = uni(static_cast<const char*>(base) + (long long)(2 * g) * a.chunk_bytes + row_bytes);
#pragma unroll
        for (int nh = 0; nh < 2; ++nh) {
            R[2 * g + nh][0] = load16_s(r, lane_off[nh]);
            R[2 * g + nh][1] = load16_s(r + a.chunk_bytes, lane_off[nh]);
        }
    };
    f32x4 acc16[2][2][2][2];    // [cout group (conv5 only: 1)][pixel half][cout half][main | cross]
    f32x4 Af[2][2][2];          // [buffer][cout half][variant]; in a conv5 step the buffer is the cout group
    f32x4 Bf[2][2][2];          // [buffer][pixel half][variant]
    // Weight fragments of tap-step s_ -> buffer `buf`, from the slab `off` bytes behind the address registers (conv5's second
    // cout group: the next slab, an immediate offset).  Pixel fragments of tap-step s_ -> buffer `buf` (the second pixel
    // half is 16 pixels = 1024 bytes on: the slot swizzle looks at bit 2 of the column only).  Each address register is
    // moved on to where it is read next (`d` bytes) by its last read of a step.
    auto load_a = [&](int s_, int buf, unsigned off) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            if (s_ < 4) {
                const unsigned ad = s_ < 3 ? aw012 + s_ * 2048 : aw3;
                Af[buf][mt][0] = *((lds_f32x4)(size_t)(ad + off + mt * 256));
                Af[buf][mt][1] = *((lds_f32x4)(size_t)(ad + off + mt * 256 + 1024));
            } else {
                f32x4 hi = *((lds_f32x4)(size_t)(aw4 + off + mt * 256));
                Af[buf][mt][1] = *((lds_f32x4)(size_t)(aw4b + off + mt * 256));
                if (un) hi = f32x4{0.f, 0.f, 0.f, 0.f};
                Af[buf][mt][0] = hi;
            }
        }
    };
    auto move_a = [&](unsigned d) {
        aw012 += d;
        aw3 += d;
        aw4 += d;
        aw4b += d;
    };
    auto load_b = [&](int sl, int s_, int buf) {
        const unsigned dB = sl == RSLOTS - 1 ? (unsigned)(-(RSLOTS - 1) * IN_BYTES) : (unsigned)IN_BYTES;
        const unsigned xl = bcur[s_] ^ (s_ == 4 ? xl4 : 32u);
#pragma unroll
        for (int nh = 0; nh < 2; ++nh) {
            Bf[buf][nh][0] = *((lds_f32x4)(size_t)(bcur[s_] + nh * 1024));
            Bf[buf][nh][1] = *((lds_f32x4)(size_t)(xl + nh * 1024));
        }
        bcur[s_] += dB;
    };
    // the products of one tap-step for one cout group, in the per-layer kernel's order
    auto mfma_tap = [&](int s_, int g, int abuf, int bbuf) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const f16x8 a0 = __builtin_bit_cast(f16x8, Af[abuf][mt][0]), a1 = __builtin_bit_cast(f16x8, Af[abuf][mt][1]);
#pragma unroll
            for (int nh = 0; nh < 2; ++nh) {
                const f16x8 x0_ = __builtin_bit_cast(f16x8, Bf[bbuf][nh][0]), x1_ = __builtin_bit_cast(f16x8, Bf[bbuf][nh][1]);
                if (s_ < 4) mfma_tap3(a0, a1, x0_, x1_, acc16[g][nh][mt][0], acc16[g][nh][mt][1]);
                else mfma_tap2(a0, a1, x0_, x1_, acc16[g][nh][mt][0], acc16[g][nh][mt][1]);
            }
        }
    };
    auto zero_acc = [&](int g) {
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc16[g][nh][mt][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // One step of conv1..conv4 = 5 tap-steps of the chunk in input slot `slot` and weight slab `wpos`; P = buffer parity of
    // its first tap-step (5 is odd: it flips every step, and every layer has an even number of steps).
    // The mode M (NESR_RDB_LAG, namespace rdbs) says where the step's barriers sit -- on top, in front of a
    // tap-step (waves 4..7: that one opens the NEXT step's interval; the fragments of the tap-step behind it are in
    // registers or on their way across it), or nowhere -- and whether tap-step 0's fragments are requested behind the top
    // barrier (the chunk has landed at that barrier, not earlier: the DMA waves run two steps ahead) or were requested
    // beside the previous step's last MFMAs (waves 4..7 inside a layer: those MFMAs run behind the barrier).
    auto step_body = [&](auto Pc, auto Mc, int c) {
        constexpr int P = decltype(Pc)::value, M = decltype(Mc)::value;
        constexpr int BT = rdbs::bar_tap(M);
        // the barrier that opens the interval of the layer's step cb
        auto bar = [&](int cb) {
            // the x_l stores of this wave have retired before the barrier after which the progress word goes out
            if (cb == EPI_STEPS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            RSTAMP_M(0);
            RARRIVE_M(cb - c, 0);
            if (!abl::no_barrier) __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            RARRIVE_M(cb - c, 1);
            RSTAMP_M(1);
        };
        if (rdbs::bar_top(M)) bar(c);
        const bool epi_now = active && ep_l >= 0 && c < EPI_STEPS;
        const int nslot = slot == RSLOTS - 1 ? 0 : slot + 1;
        const unsigned dA = wpos == RSLOTS - 1 ? (unsigned)(-(RSLOTS - 1) * W_BYTES) : (unsigned)W_BYTES;
        if (!active || abl::no_mfma) {
            if (BT >= 0) bar(c + 1);      // a wave without a row takes the same barriers
        } else {
            if (rdbs::req_behind(M)) {
                load_a(0, P, 0);
                load_b(slot, 0, P);
            }
            if (epi_now) {
                epi_pending();
                __builtin_amdgcn_sched_barrier(0);
            }
            RTAPS_INIT();
#pragma unroll
            for (int s_ = 0; s_ < 5; ++s_) {
                const int buf = (s_ + P) & 1;
                RTAP(s_, true);
                if (s_ == BT) {
                    bar(c + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (s_ + 1 < 5) {
                    load_a(s_ + 1, buf ^ 1, 0);
                    load_b(slot, s_ + 1, buf ^ 1);
                } else if (rdbs::req_early(M)) {
                    load_a(0, buf ^ 1, dA);      // the next step's slab
                    load_b(nslot, 0, buf ^ 1);
                }
                mfma_tap(s_, 0, buf, buf);
                // the next tap-step's 8 fragment reads ride between this one's MFMAs
                if (s_ + 1 < 5 || rdbs::req_early(M)) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            RTAP(5, false);
            RTAPS_WRITE();
        }
        move_a(dA);
        slot = nslot;
        wpos = wpos == RSLOTS - 1 ? 0 : wpos + 1;
        RSTAMP_M(2);
        RMSTEP_NEXT();
    };
    // One step of conv5 = 5 tap-steps of the chunk in input slot `slot` for BOTH cout groups: weight slabs wpos (group 0) and
    // wpos + 1 (group 1).  Per tap-step the pixel fragments are read once; group 0's products run while group 1's weight
    // fragments and the next tap-step's pixel fragments arrive, group 1's while the next tap-step's group 0 weights do --
    // one weight fragment buffer per group, so the fragment registers are those of a 32-cout step.  Every accumulator gets
    // the per-layer kernel's sequence of products.  The step's slabs were fetched one step ahead (4 slabs = this step and
    // the next) and land before this step's barrier, so tap-step 0's group 0 weights are read behind the barrier; the
    // pixel fragments of the next step's tap-step 0 are requested beside the last MFMAs as in the other layers.
    // FIRST: conv4's deferred epilogue, then the accumulators start at zero.
    // LAST (the launch's last step): no next step's fragments; in their place, beside tap-step 4, the x0 residual loads of
    // the final epilogue -- group 0's into the registers of the pixel fragments that are not fetched, group 1's into
    // group 0's weight fragments once its last products are issued.
    auto step_body5 = [&](auto Pc, auto Fc, auto Lc, int c) {
        constexpr int P = decltype(Pc)::value;
        constexpr bool FIRST = decltype(Fc)::value == 1;
        constexpr bool last_of_all = decltype(Lc)::value != 0;
        if (c == EPI_STEPS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        RSTAMP_M(0);
        RARRIVE_M(0, 0);
        if (!abl::no_barrier) __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        RARRIVE_M(0, 1);
        RSTAMP_M(1);
        const bool epi_now = active && ep_l >= 0 && c < EPI_STEPS;
        const int nslot = slot == RSLOTS - 1 ? 0 : slot + 1;
        const unsigned dA = wpos == 0 ? (unsigned)(2 * W_BYTES) : (unsigned)(-2 * W_BYTES);
        if (active && !abl::no_mfma) {
            load_a(0, 0, 0);
            // conv4's last step could not ask for this step's first pixel fragments (step 28 lands at this barrier)
            if (FIRST) load_b(slot, 0, P);
            if (epi_now) {
                epi_pending();
                __builtin_amdgcn_sched_barrier(0);
            }
            if (FIRST) { zero_acc(0); zero_acc(1); }
#pragma unroll
            for (int s_ = 0; s_ < 5; ++s_) {
                const int buf = (s_ + P) & 1;
                if (last_of_all && s_ == 4 && !abl::no_epilogue) {
                    issue_res(cur_of(), 0, R1);
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
                load_a(s_, 1, W_BYTES);
                if (s_ + 1 < 5) load_b(slot, s_ + 1, buf ^ 1);
                else if (!last_of_all) load_b(nslot, 0, buf ^ 1);
                mfma_tap(s_, 0, 0, buf);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
                }
                __builtin_amdgcn_sched_barrier(0);
                if (s_ + 1 < 5) load_a(s_ + 1, 0, 0);
                else if (last_of_all && !abl::no_epilogue) {
                    issue_res(cur_of(), 1, R1);
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
                mfma_tap(s_, 1, 1, buf);
                if (s_ + 1 < 5) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        move_a(dA);
        slot = nslot;
        wpos = wpos == 0 ? 2 : 0;
        RSTAMP_M(2);
        RMSTEP_NEXT();
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, rdbs::M_LEAD> MLead;      // waves 0..3, any step of conv1..conv4
    typedef std::integral_constant<int, rdbs::M_LAG_FIRST> MFirst;
    typedef std::integral_constant<int, rdbs::M_LAG_MID> MMid;
    typedef std::integral_constant<int, rdbs::M_LAG_LAST> MLast;
    // waves 4..7: first step, pairs of middle steps, last step (every layer has an even number of steps >= 4)
    static_assert(rdbs::mode_of(true, 4) == rdbs::M_LAG_FIRST && rdbs::mode_of(true, 5) == rdbs::M_LAG_MID &&
                  rdbs::mode_of(true, 8) == rdbs::M_LAG_MID && rdbs::mode_of(true, 9) == rdbs::M_LAG_LAST &&
                  rdbs::mode_of(false, 0) == rdbs::M_LEAD && rdbs::mode_of(false, RDB_STEP5 - 1) == rdbs::M_LEAD, "the loops below are the walk's sequence");
    // the layer's sums (main + cross / 2^11) wait for the next layer's first steps
    auto layer_done = [&](int l) {
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) ep[nh][mt][i] = fmaf(acc16[0][nh][mt][1][i], LO_INV, acc16[0][nh][mt][0][i]);
        ep_l = l;
    };
    if (fills_bias) *reinterpret_cast<f32x4*>(smem + BIAS + wave * 128 + lane * 16) = bias_v;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the bias table is in LDS before the first barrier
    // the block's first fragments: chunk 0 is in LDS once every DMA wave has passed its first wait -- one extra barrier
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (wave < 4) {
        for (int l = 0; l < 4; ++l) {
            const int nc = 4 + 2 * l;
            zero_acc(0);
            for (int c = 0; c < nc; c += 2) {
                step_body(I0{}, MLead{}, c);
                step_body(I1{}, MLead{}, c + 1);
            }
            layer_done(l);
        }
    } else {
        for (int l = 0; l < 4; ++l) {
            const int nc = 4 + 2 * l;
            zero_acc(0);
            step_body(I0{}, MFirst{}, 0);
            for (int c = 1; c < nc - 1; c += 2) {
                step_body(I1{}, MMid{}, c);
                step_body(I0{}, MMid{}, c + 1);
            }
            step_body(I1{}, MLast{}, nc - 1);
            layer_done(l);
        }
    }
    // conv5: 12 steps of 64 output channels
    step_body5(I0{}, I1{}, I0{}, 0);
    step_body5(I1{}, I0{}, I0{}, 1);
    for (int c = 2; c < 10; c += 2) {
        step_body5(I0{}, I0{}, I0{}, c);
        step_body5(I1{}, I0{}, I0{}, c + 1);
    }
    step_body5(I0{}, I0{}, I0{}, 10);
    step_body5(I1{}, I0{}, I1{}, 11);
#if NESR_RDB_ABL & 256
    // a block boundary of a chained launch: the end of the last MFMA step of the launch's last block but one (slot 59);
    // the last block's step 0 then holds the other side
    if (CHAIN && blk + 2 == nblocks && wave == 1) RSTAMP(0, 59, 0);
#endif
    // Both cout groups of conv5: x5 * s1 + x0 (and * s2 + RRDB input) into `out`'s channels 32 g.  Nothing is left to
    // overlap them with, so the memory round trips are taken once for all four pieces: x0's loads are in flight since
    // tap-step 4, the RRDB input's go out here, straight behind the last MFMA; each piece waits for its own lines only
    // (loads return in issue order: vmcnt(N) leaves the N issued after them in flight), and the eight stores follow the
    // last piece, so no wait ever covers a store.
    auto final_epilogue = [&](auto Rc) {
        constexpr bool RES2 = decltype(Rc)::value != 0;
        if (RES2) {
            issue_res(res2_of(), 0, R2);
            issue_res(res2_of(), 1, R2);
        }
        asm volatile("" ::: "memory");      // the loads stay here: none is moved down towards its use
        __builtin_amdgcn_sched_barrier(0);
        RSTAMP_M(3);
        uint4 cx[4], cx1[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int g = p >> 1, nh = p & 1;
            f32x4 e0, e1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                e0[i] = fmaf(acc16[g][nh][0][1][i], LO_INV, acc16[g][nh][0][0][i]);
                e1[i] = fmaf(acc16[g][nh][1][1][i], LO_INV, acc16[g][nh][1][0][i]);
            }
            const char* bsrc = smem + BIAS + (4 * 32 + 32 * g + cbl) * 4;      // conv5's second group follows its first
            f32x4 v0, v1;   // couts cbl .. cbl+3, cbl+4 .. cbl+7
            cout_exchange(e0, e1, v0, v1);
            v0 += *reinterpret_cast<const f32x4*>(bsrc);
            v1 += *reinterpret_cast<const f32x4*>(bsrc + 16);
            f32x4 q0, q1;
            unpack_res(R1[p][0], R1[p][1], q0, q1);
#pragma unroll
            for (int i = 0; i < 4; ++i) { v0[i] = scale_add_2r(v0[i], a.s1, q0[i]); v1[i] = scale_add_2r(v1[i], a.s1, q1[i]); }
            if (RES2) {
                unpack_res(R2[p][0], R2[p][1], q0, q1);
#pragma unroll
                for (int i = 0; i < 4; ++i) { v0[i] = scale_add_2r(v0[i], a.s2, q0[i]); v1[i] = scale_add_2r(v1[i], a.s2, q1[i]); }
            }
            bool bad_here = false;
            split_regroup(v0, v1, cx[p], cx1[p], bad_here);
            note_bad(bad_here && lane_ok[nh]);
            __builtin_amdgcn_sched_barrier(0);      // piece by piece, in the order the lines were asked for: counted waits
        }
        RSTAMP_M(5);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (lane_ok[p & 1]) {
                const char* d0 = uni(static_cast<const char*>(out_of()) + (long long)(2 * (p >> 1)) * a.chunk_bytes + row_bytes);
                // write-through like x1..x4: 16.8 MB of dirty lines less for the kernel boundary to write back (measured
                // against plain stores: 6.185 -> 6.130 ms per frame, profiles/rdb_edges/)
                store16_wt_s(d0, lane_off[p & 1], cx[p]);
                store16_wt_s(d0 + a.chunk_bytes, lane_off[p & 1], cx1[p]);
            }
        }
        RSTAMP_M(6);
        RSTAMP_RETIRED();
    };
    if (active && !abl::no_epilogue) {
        if (res2_of() != nullptr) final_epilogue(I1{});
        else final_epilogue(I0{});
    }
    if (!CHAIN) break;
    // The block's last barrier: this wave's `out` stores have retired in front of it (level 5 goes out behind it), and no
    // wave reads the rings or the bias table past it.  Then the next block's pointers and its bias table; the ring
    // positions are back at 0 (RDB_STEPS is a multiple of RSLOTS).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#if NESR_RDB_ABL & 256
    if (blk + 2 == nblocks && wave == 1) RSTAMP(0, 59, 1);      // ... and its last store retired
#endif
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (blk + 1 == nblocks) break;
    ent += 1;
  }
    if (bad && a.status) __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one dense block per launch
__global__ __launch_bounds__(64 * (MW + DW), 3) void rdb_f16x2_kernel(RdbArgs a) { rdb_blocks<false>(a, nullptr, 1); }
// a run of consecutive dense blocks of one forward per launch
__global__ __launch_bounds__(64 * (MW + DW), 3) void rdb_f16x2_chain_kernel(RdbArgs a, const RdbChainBlock* table, int nblocks) { rdb_blocks<true>(a, table, nblocks); }

}  // namespace

#if NESR_RDB_ABL & 256
extern "C" int nesr_debug_rdb_steps() { return RDB_STEPS; }
extern "C" int nesr_debug_rdb_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rdb_stamps), sizeof(unsigned long long) * 2 * 64 * 8);
}
extern "C" int nesr_debug_rdb_taps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rdb_taps), sizeof(unsigned long long) * 2 * 8 * 8);
}
extern "C" int nesr_debug_rdb_arrive(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rdb_arrive), sizeof(unsigned long long) * 12 * 8 * 2);
}
#endif

int rdb_f16x2_tiles(int n, int h, int w) { return ((w + TW - 1) / TW) * ((h + 7) / 8) * n; }

namespace {

// One dense block (table == null) or the `nblocks` blocks of `table` (device memory; r.cur .. r.bias are not used) in one launch
template <typename Kernel>
hipError_t launch_rdb(Kernel kernel, unsigned long long& attr_done, int& resident, const RdbLaunch& r, const RdbChainBlock* table, int nblocks, hipStream_t s) {
    typedef Geo<4> G;
    constexpr size_t shm = (size_t)RSLOTS * (G::IN_BYTES + (size_t)W_BYTES) + 768;
    {
        const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), shm, attr_done);
        if (e != hipSuccess) return e;
    }
    if ((long long)r.w_ * 64 * 12 >= (1ll << 32)) return hipErrorInvalidValue;
    RdbArgs a;
    a.cur = r.cur; a.chunk_bytes = r.chunk_bytes; a.out = r.out; a.res2 = r.res2; a.s1 = r.s1; a.s2 = r.s2;
    for (int i = 0; i < 5; ++i) { a.w[i] = r.w[i]; a.bias[i] = r.bias[i]; }
    a.n = r.n; a.h = r.h; a.w_ = r.w_;
    a.progress = r.progress; a.epoch = r.epoch; a.abort_flag = r.abort_flag; a.status = r.status;
    a.timeout_ticks = r.timeout_ticks ? r.timeout_ticks : 20000000ull;
    int total = rdb_f16x2_tiles(r.n, r.h, r.w_);
    if (total <= 0) return hipSuccess;
    // every tile needs its own RESIDENT workgroup: what the device admits of this kernel (registers, LDS) times its compute units
    if (resident < 0) {
        int per_cu = 0, dev = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64 * (MW + DW), shm) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return hipErrorUnknown;
        resident = per_cu * cus;
    }
    if (total > resident) return hipErrorLaunchOutOfResources;
    total -= r.debug_drop;       // test hook (nesr_debug_fault): the last workgroups never start, their neighbours' waits must end in the abort word
    if (total <= 0) return hipSuccess;
    if constexpr (std::is_same<Kernel, void (*)(RdbArgs)>::value) hipLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(64 * (MW + DW)), shm, s, a);
    else hipLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(64 * (MW + DW)), shm, s, a, table, nblocks);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rdb_f16x2(const RdbLaunch& r, hipStream_t s) {
    static unsigned long long attr_done = 0;
    static int resident = -1;
    return launch_rdb(&rdb_f16x2_kernel, attr_done, resident, r, nullptr, 1, s);
}

hipError_t launch_rdb_f16x2_chain(const RdbLaunch& r, const RdbChainBlock* table, int nblocks, hipStream_t s) {
    static unsigned long long attr_done = 0;
    static int resident = -1;
    if (!table || nblocks <= 0) return hipErrorInvalidValue;
    return launch_rdb(&rdb_f16x2_chain_kernel, attr_done, resident, r, table, nblocks, s);
}

}  // namespace nesr
