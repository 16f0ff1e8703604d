// The RRDBNet forward graph as a sequence of fused conv launches: the table of compute forms, workspace layout, the choice of
// kernel per conv and per dense block (per-layer, fused f16-pair block, LDS-resident 16-bit strip, opt-in persistent trunk),
// the per-device lease of the persistent kernels and the strip-plan cache.
//
// What it stands behind in the reference: basicsr RRDBNet.forward, as called from nesr/nesr.py:216-229,887-891 and
// standalone/direct_esrgan.py:104-148.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "rdb_f16x2_schedule.h"
#include "rrdb_ctx.h"

namespace nesr {

namespace {

// the pack functions differ in destination type only
template <class T, void (*F)(const float*, int, int, int, int, T*)>
void pack_to(const float* oihw, int cout, int cin, int cin_p, int coutp, void* dst) { F(oihw, cout, cin, cin_p, coutp, static_cast<T*>(dst)); }

// indexed by NESR_DTYPE_*.  The f16-pair slab is counted in 2-byte units; f16 uses bf16's slab size.
const Form FORMS[] = {
    /* F32          */ {0, 4, 8, packed_weight_elems_f32, 4, pack_to<float, pack_weights_f32>, launch_conv3x3_f32, false},
    /* BF16         */ {1, 2, 16, packed_weight_elems_bf16, 2, pack_to<uint16_t, pack_weights_bf16>, launch_conv3x3_bf16, false},
    /* F32_WINOGRAD */ {0, 4, 8, packed_weight_elems_wino_f32, 4, pack_to<float, pack_weights_wino_f32>, launch_conv3x3_wino_f32, false},
    /* F32_SPLIT    */ {2, 4, 16, packed_weight_elems_f16x2, 2, pack_to<uint16_t, pack_weights_f16x2>, launch_conv3x3_f16x2, true},
    /* F16          */ {3, 2, 16, packed_weight_elems_bf16, 2, pack_to<uint16_t, pack_weights_f16>, launch_conv3x3_f16, true},
};
static_assert(NESR_DTYPE_F32 == 0 && NESR_DTYPE_BF16 == 1 && NESR_DTYPE_F32_WINOGRAD == 2 && NESR_DTYPE_F32_SPLIT == 3 && NESR_DTYPE_F16 == 4,
              "FORMS is indexed by NESR_DTYPE_*");

}  // namespace

const Form* form_of(int dtype) { return dtype >= 0 && dtype < (int)(sizeof(FORMS) / sizeof(FORMS[0])) ? &FORMS[dtype] : nullptr; }

Map make_map(int kind, int channels, size_t pixels) {
    Map m;
    if (kind == 2) { m.pix = 32; m.chunk = (long long)pixels * 32; }
    else if (kind == 1 || kind == 3) { m.pix = 16; m.chunk = (long long)pixels * 16; }
    else { m.pix = channels; m.chunk = 8; }
    return m;
}

WsLayout ws_layout(const nesr_ctx* c, int N, int h, int w) {
    const size_t es = c->esize();
    const size_t px = (size_t)N * h * w;
    WsLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    L.in = take(px * c->layers[0].cin_p * es);
    L.f = take(px * c->nf * es);
    L.a = take(px * c->ct() * es);
    L.b = take(px * c->ct() * es);
    L.c = take(px * c->ct() * es);
    L.u1 = take(px * 4 * c->nf * es);
    L.u2 = take(px * 16 * c->nf * es);
    L.u3 = take(px * 16 * c->nf * es);
    // per-tile progress counters of the persistent trunk kernel (8x16-pixel tiles) + abort word
    L.sync_words = N * ((h + 7) / 8) * ((w + 15) / 16) + 64;
    L.sync = take((size_t)L.sync_words * 4);
    L.total = off;
    return L;
}

int ensure_ws(nesr_ctx* c, size_t bytes) {
    if (bytes <= c->ws_bytes) return NESR_OK;
    if (c->ws) {
        NESR_TRY(hipDeviceSynchronize());
        NESR_TRY(hipFree(c->ws));
        c->ws = nullptr;
        c->ws_bytes = 0;
        c->last_sync = nullptr;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return set_error(NESR_ERR_NOMEM, "hipMalloc(workspace " + std::to_string(bytes) + " B): " + hipGetErrorString(e));
    c->ws = static_cast<char*>(p);
    c->ws_bytes = bytes;
    return NESR_OK;
}

namespace {

// One conv of the context's form.  What is not a property of a single form is spelled out here: the folded up-convs of the
// f16-pair form and the Winograd slab of an f32 context.
hipError_t launch_conv(const nesr_ctx* c, const ConvArgs& a, hipStream_t s, const Layer& L) {
    // by the context's setting alone, never by the shape: one arithmetic for a tile however it is batched
    if (c->dtype == NESR_DTYPE_F32_SPLIT && a.up && c->upconv_2x2) {
        if (!L.d_w2) return hipErrorInvalidValue;   // never a silent 3x3: the folded slabs are built at finalisation
        ConvArgs u = a;
        u.w = L.d_w2;
        return launch_upconv2x2_f16x2(u, s);
    }
    if (c->winograd && L.d_ww && (!(a.out_nchw || a.out_u8) || (a.cout_real >= 1 && a.cout_real <= 4 && a.coutp == 32))) {
        ConvArgs w = a;
        w.w = L.d_ww;
        return launch_conv3x3_wino_f32(w, s);
    }
    return c->form->launch(a, s);
}

ConvArgs base_args(const nesr_ctx* c, const Layer& L, int N, int h, int w) {
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.zeros = c->d_weights;
    a.cin = L.cin_p;
    a.w = L.d_w;
    a.bias = L.d_b;
    a.coutp = L.cout_p;
    a.n = N;
    a.h = h;
    a.w_ = w;
    a.in_h = h;
    a.in_w = w;
    a.s1 = a.s2 = 1.f;
    a.cout_real = 0;
    a.shared_device = c->shared_device;
    a.size_independent = c->size_independent;
    if (c->rag_n) {
        a.rag_n = c->rag_n;
        a.rag_shift = h == c->rag_base_h ? 0 : (h == 2 * c->rag_base_h ? 1 : 2);
        std::memcpy(a.rag_h, c->rag_h, sizeof(a.rag_h));
        std::memcpy(a.rag_w, c->rag_w, sizeof(a.rag_w));
    }
    a.status = c->ranged() ? c->d_status : nullptr;
    return a;
}

// ---- persistent kernels need the device to themselves: every workgroup of rdb_f16x2_kernel / rdb_bf16_strip_kernel waits for
// other workgroups of the same launch, so two such launches that share the compute units (two contexts on two streams) can
// each hold CUs the other one's missing workgroups need.  Within a process they are therefore serialised per device:
// a stream that is about to launch one first waits for the event recorded behind the previous holder's last launch.
// (Across processes nothing can order them: the kernels bound their waits and raise an abort word, nesr_check_range.)
struct DeviceLease {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t owner = nullptr;
    const nesr_ctx* owner_ctx = nullptr;
    bool pending = false;
};
DeviceLease g_lease[64];

int lease_acquire(const nesr_ctx* c, hipStream_t s) {
    if (c->device < 0 || c->device >= 64) return NESR_OK;
    DeviceLease& L = g_lease[c->device];
    std::lock_guard<std::mutex> lock(L.mu);
    if (L.pending && (L.owner_ctx != c || L.owner != s)) NESR_TRY(hipStreamWaitEvent(s, L.ev, 0));
    return NESR_OK;
}
int lease_release(const nesr_ctx* c, hipStream_t s) {
    if (c->device < 0 || c->device >= 64) return NESR_OK;
    DeviceLease& L = g_lease[c->device];
    std::lock_guard<std::mutex> lock(L.mu);
    if (!L.ev) NESR_TRY(hipEventCreateWithFlags(&L.ev, hipEventDisableTiming));
    NESR_TRY(hipEventRecord(L.ev, s));
    L.owner = s;
    L.owner_ctx = c;
    L.pending = true;
    return NESR_OK;
}

}  // namespace

void lease_forget(const nesr_ctx* c) {
    if (c->device < 0 || c->device >= 64) return;
    DeviceLease& L = g_lease[c->device];
    std::lock_guard<std::mutex> lock(L.mu);
    if (L.owner_ctx == c) { L.owner_ctx = nullptr; L.owner = nullptr; }   // the event stays valid: later holders still wait for it
}

void free_strip_plans(nesr_ctx* c) {
    for (auto& P : c->strip_plans) {
        if (P.d_items) (void)hipFree(P.d_items);
        if (P.d_first) (void)hipFree(P.d_first);
        if (P.d_xch) (void)hipFree(P.d_xch);
    }
    c->strip_plans.clear();
}

namespace {

// the strip schedule + mailboxes of one batch geometry (cached: a video stream asks for the same one every frame)
int strip_plan_for(nesr_ctx* c, int N, int h, int w, const nesr_ctx::StripPlan** out) {
    std::vector<int> key{N, h, w};
    std::vector<int> hw(2 * (size_t)N);
    for (int i = 0; i < N; ++i) {
        hw[2 * i] = c->rag_n ? c->rag_h[i] : h;
        hw[2 * i + 1] = c->rag_n ? c->rag_w[i] : w;
    }
    key.insert(key.end(), hw.begin(), hw.end());
    for (const auto& P : c->strip_plans)
        if (P.key == key) { *out = &P; return NESR_OK; }
    if (c->strip_plans.size() >= 32) {
        NESR_TRY(hipDeviceSynchronize());
        free_strip_plans(c);
    }
    nesr_ctx::StripPlan P;
    P.key = key;
    const StripSchedule S = strip_schedule(N, hw.data(), c->strip_cus > 0 ? c->strip_cus : c->cus, c->strip_seg);
    P.makespan = S.makespan;
    if (strip_plan_applies(S)) {       // by the images' own positions (the tag space), not by the length of the schedule
        P.grid = S.grid; P.smax = S.smax; P.efficiency = S.efficiency;
        const size_t xb = (size_t)S.nvimg * S.smax * STRIP_XCH_BYTES;
        NESR_TRY(hipMalloc(&P.d_items, S.items.size() * 4));
        NESR_TRY(hipMalloc((void**)&P.d_first, S.wg_first.size() * 4));
        NESR_TRY(hipMalloc((void**)&P.d_xch, xb));
        NESR_TRY(hipMemcpy(P.d_items, S.items.data(), S.items.size() * 4, hipMemcpyHostToDevice));
        NESR_TRY(hipMemcpy(P.d_first, S.wg_first.data(), S.wg_first.size() * 4, hipMemcpyHostToDevice));
        NESR_TRY(hipMemset(P.d_xch, 0, xb));
    } else {
        P.makespan = -1;
    }
    if (getenv("NESR_STRIP_DEBUG"))
        fprintf(stderr, "[nesr] strip plan: %d images (slot %dx%d) as %d row segments: grid %d workgroups, makespan %d positions, efficiency %.3f\n", N, h, w,
                S.nvimg, P.grid, P.makespan, P.efficiency);
    c->strip_plans.push_back(std::move(P));
    *out = &c->strip_plans.back();
    return NESR_OK;
}

// does this evaluation's trunk run as persistent (lease-holding) launches?
bool strip_wanted(const nesr_ctx* c) {
    return c->half16() && c->d_strip && c->strip_mode != 0 && c->nf == 64 && c->gc == 32;
}

// What a fused dense-block form answers: it went out (NESR_OK), it does not apply to this block (the next form is tried),
// or an error code (those are negative)
constexpr int FUSED_LAUNCHED = NESR_OK, FUSED_NA = 1;

// bf16 / f16: the dense block with its working set resident in LDS (rdb_bf16_strip_kernel), whenever the context is
// size-independent (a tiling wrapper: one arithmetic for every tile, however it is batched) or the batch fills the device
int try_strip(nesr_ctx* c, const FwState& F, int b, int r, hipStream_t s) {
    if (!strip_wanted(c)) return FUSED_NA;
    const nesr_ctx::StripPlan* P = nullptr;
    int rc = strip_plan_for(c, F.N, F.h, F.w, &P);
    if (rc) return rc;
    if (!(P->makespan > 0 && (c->strip_mode == 1 || c->size_independent || P->efficiency >= 0.55))) return FUSED_NA;
    StripLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.cur = F.buf[r];
    L.chunk_bytes = F.m_t.chunk * 2;
    L.out = r < 2 ? F.buf[r + 1] : F.buf[0];
    L.res2 = r < 2 ? nullptr : F.buf[0];
    L.s1 = 0.2f; L.s2 = 0.2f;
    const char* blk = c->d_strip + (size_t)(b * 3 + r) * c->strip_stride;
    L.wstream = blk;
    L.bias = reinterpret_cast<const float*>(blk + strip_weight_bytes());
    L.H = F.h; L.W = F.w;
    L.items = P->d_items; L.wg_first = P->d_first; L.grid = P->grid; L.smax = P->smax; L.xch = P->d_xch;
    c->strip_epoch += STRIP_EPOCH_STEP;
    L.epoch = c->strip_epoch;
    L.abort_flag = c->d_status + 2;
    L.timeout_ticks = c->strip_timeout_ticks;
    L.debug_drop = c->debug_drop;
    c->debug_drop = 0;
    L.f16 = c->dtype == NESR_DTYPE_F16 ? 1 : 0;
    L.status = L.f16 ? c->d_status : nullptr;
    const hipError_t le = launch_rdb_bf16_strip(L, s);
    if (le == hipErrorLaunchOutOfResources) {
        c->strip_mode = 0;      // the device does not admit the kernel's workgroups (LDS / registers): per-layer launches
        return FUSED_NA;
    }
    NESR_TRY(le);
    c->strip_used = true;
    if (c->timer.on) {
        double px_real = 0.0;      // ragged batches: the images' own pixels
        for (int i = 0; i < F.N; ++i) px_real += c->rag_n ? (double)c->rag_h[i] * c->rag_w[i] : (double)F.h * F.w;
        for (int k = 0; k < 5; ++k) c->timer.flops += conv_flops(c->layers[layer_id(b, r, k)], px_real);
        c->timer.launches += 1;
    }
    return FUSED_LAUNCHED;
}

// small frames, f16-pair form: the whole dense block in one launch (rdb_f16x2_kernel).  Every tile needs its own
// resident workgroup, so the frame's tiles must fit the compute units and the device must be this context's
// (frames in flight on other streams would compete for the one workgroup slot per CU).
bool fused_rdb_applies(const nesr_ctx* c, const FwState& F) {
    if (c->dtype != NESR_DTYPE_F32_SPLIT || c->rdb_mode == 0 || c->nf != 64 || c->gc != 32 || c->shared_device) return false;
    const int tiles = rdb_f16x2_tiles(F.N, F.h, F.w);
    return tiles <= c->cus && tiles <= 4096;
}

// everything of a fused launch that does not depend on the block (the epoch is the caller's)
RdbLaunch fused_rdb_launch(nesr_ctx* c, const FwState& F) {
    RdbLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.chunk_bytes = F.m_t.chunk * 2;
    L.s1 = 0.2f; L.s2 = 0.2f;
    L.n = F.N; L.h = F.h; L.w_ = F.w;
    L.progress = c->d_status + 64;
    L.abort_flag = c->d_status + 1;
    L.status = c->d_status;
    L.timeout_ticks = c->strip_timeout_ticks;
    L.debug_drop = c->debug_drop;
    c->debug_drop = 0;
    return L;
}

int try_fused_rdb(nesr_ctx* c, const FwState& F, int b, int r, hipStream_t s) {
    if (!fused_rdb_applies(c, F)) return FUSED_NA;
    const double px = (double)F.N * F.h * F.w;
    RdbLaunch L = fused_rdb_launch(c, F);
    RdbChainBlock e;
    rdb_block_entry(F.buf, c->layers.data(), b, r, e);
    L.cur = e.cur; L.out = e.out; L.res2 = e.res2;
    for (int k = 0; k < 5; ++k) {
        L.w[k] = e.w[k];
        L.bias[k] = e.bias[k];
        if (c->timer.on) c->timer.flops += conv_flops(c->layers[layer_id(b, r, k)], px);
    }
    c->rdb_epoch += 8;
    L.epoch = c->rdb_epoch;
    const hipError_t le = launch_rdb_f16x2(L, s);
    if (le == hipErrorLaunchOutOfResources) {
        c->rdb_mode = 0;        // fewer resident workgroups than tiles: per-layer launches (the same bits)
        return FUSED_NA;
    }
    NESR_TRY(le);
    c->strip_used = true;       // (the abort word of either persistent kernel is looked at by nesr_check_range)
    c->chain_launches += 1;
    c->chain_blocks += 1;
    if (c->timer.on) c->timer.launches += 1;
    return FUSED_LAUNCHED;
}

// The whole trunk of a forward as ONE launch of the chained kernel, where try_fused_rdb would take every block and nothing
// sits between the blocks (run_forward's loop: no row-band phase, no single-block entry).  The device table of per-block
// pointers is kept with the context and rewritten when the workspace or the weights have moved.
int try_chained_rdb(nesr_ctx* c, const FwState& F, hipStream_t s) {
    const int nblocks = 3 * c->nb;
    if (!c->rdb_chain || nblocks <= 0 || !fused_rdb_applies(c, F)) return FUSED_NA;
    std::vector<RdbChainBlock> table((size_t)nblocks);
    for (int i = 0; i < nblocks; ++i) rdb_block_entry(F.buf, c->layers.data(), i / 3, i % 3, table[(size_t)i]);
    const size_t bytes = table.size() * sizeof(RdbChainBlock);
    if (!c->d_chain || c->h_chain.size() != table.size() || std::memcmp(c->h_chain.data(), table.data(), bytes) != 0) {
        if (c->d_chain && c->h_chain.size() != table.size()) {
            NESR_TRY(hipStreamSynchronize(s));
            NESR_TRY(hipFree(c->d_chain));
            c->d_chain = nullptr;
        }
        if (!c->d_chain) NESR_TRY(hipMalloc((void**)&c->d_chain, bytes));
        c->h_chain.swap(table);       // the copy's source stays as it is until the next rebuild
        NESR_TRY(hipMemcpyAsync(c->d_chain, c->h_chain.data(), bytes, hipMemcpyHostToDevice, s));
    }
    RdbLaunch L = fused_rdb_launch(c, F);
    L.epoch = c->rdb_epoch + 8;       // block k publishes epoch + 8 k + 1 .. + 5
    const hipError_t le = launch_rdb_f16x2_chain(L, c->d_chain, nblocks, s);
    if (le == hipErrorLaunchOutOfResources) {
        c->rdb_chain = 0;             // the chained kernel does not fit: one block per launch, if that kernel does
        return FUSED_NA;
    }
    NESR_TRY(le);
    c->rdb_epoch += 8u * (unsigned)nblocks;
    c->strip_used = true;
    c->chain_launches += 1;
    c->chain_blocks += nblocks;
    if (c->timer.on) {
        const double px = (double)F.N * F.h * F.w;
        for (int i = 0; i < nblocks * 5; ++i) c->timer.flops += conv_flops(c->layers[1 + i], px);
        c->timer.launches += nblocks;      // dense blocks dispatched through a fused route, not kernel launches
    }
    return FUSED_LAUNCHED;
}

}  // namespace

void rdb_block_entry(char* const buf[3], const Layer* layers, int b, int r, RdbChainBlock& e) {
    e.cur = buf[rdbs::rdb_cur_buf(r)];
    e.out = buf[rdbs::rdb_out_buf(r)];
    e.res2 = rdbs::rdb_res2_buf(r) >= 0 ? buf[rdbs::rdb_res2_buf(r)] : nullptr;
    for (int k = 0; k < 5; ++k) {
        const Layer& Ly = layers[layer_id(b, r, k)];
        e.w[k] = Ly.d_w;
        e.bias[k] = Ly.d_b;
    }
}

int fw_setup(nesr_ctx* c, int N, int C, int H, int W, FwState& F) {
    if (!c->finalized) return set_error(NESR_ERR_STATE, "weights not finalized (call nesr_finalize_weights)");
    const int u = c->ufac();
    if (N <= 0 || H <= 0 || W <= 0) return set_error(NESR_ERR_ARG, "empty input");
    if (C * u * u != c->cin0)
        return set_error(NESR_ERR_ARG, "input has " + std::to_string(C) + " channels; conv_first expects " +
                                           std::to_string(c->cin0) + " after unshuffle " + std::to_string(u));
    if (H % u || W % u) return set_error(NESR_ERR_ARG, "H and W must be multiples of the unshuffle factor");
    NESR_TRY(hipSetDevice(c->device));
    F.N = N; F.h = H / u; F.w = W / u;
    F.L = ws_layout(c, N, F.h, F.w);
    int rc = ensure_ws(c, F.L.total);
    if (rc) return rc;
    const int kind = c->kind();
    const size_t P1 = (size_t)N * F.h * F.w;
    F.m_in = make_map(kind, c->layers[0].cin_p, P1);
    F.m_f = make_map(kind, c->nf, P1);
    F.m_t = make_map(kind, c->ct(), P1);
    F.m_u1 = make_map(kind, c->nf, P1 * 4);
    F.m_u2 = make_map(kind, c->nf, P1 * 16);
    F.buf[0] = c->ws + F.L.a; F.buf[1] = c->ws + F.L.b; F.buf[2] = c->ws + F.L.c;
    return NESR_OK;
}

// pack (pixel_unshuffle, layout, u8 normalisation; or the NESR pipeline's 12-channel synthesis from `nesr12`'s window) + conv_first:
// IN -> P.x0 and F (feat is needed again after the trunk)
int fw_first(nesr_ctx* c, const FwState& F, const float* x_f32, const uint8_t* x_u8, int flip, int C, int H, int W, hipStream_t s, const Pack12Args* nesr12) {
    char* ws = c->ws;
    PackArgs p;
    std::memset(&p, 0, sizeof(p));
    p.src = x_u8 ? static_cast<const void*>(x_u8) : static_cast<const void*>(x_f32);
    p.src_u8 = x_u8 ? 1 : 0;
    p.flip = flip;
    p.n = F.N; p.c = C; p.hin = H; p.win = W;
    p.unshuffle = c->ufac();
    p.dst = ws + F.L.in;
    p.dst_map = F.m_in;
    p.cp = c->layers[0].cin_p;
    p.bf16 = c->kind();
    p.status = c->ranged() ? c->d_status : nullptr;
    if (p.status) NESR_TRY(launch_status_latch(c->d_status, s));      // the range word is per forward (nesr_check_range reports a latched one once)
    if (nesr12) {
        Pack12Args q = *nesr12;
        q.dst = p.dst; q.dst_map = p.dst_map; q.cp = p.cp; q.bf16 = p.bf16; q.status = p.status;
        NESR_TRY(launch_pack_nesr12(q, s));
    } else {
        NESR_TRY(launch_pack_input(p, s));
    }
    ConvArgs a = base_args(c, c->layers[0], F.N, F.h, F.w);
    a.in = ws + F.L.in; a.in_map = F.m_in;
    a.out = ws + F.L.a; a.out_map = F.m_t; a.out_coff = 0;
    a.out2 = ws + F.L.f; a.out2_map = F.m_f;
    NESR_TRY(launch_conv(c, a, s, c->layers[0]));
    return NESR_OK;
}

// RDB r (0..2) of RRDB b.  Buffers P,Q,R hold x0|x1|x2|x3|x4 of RDB1,2,3; RDB3's conv5 applies both residuals
// (x5*0.2+x0 then *0.2 + RRDB input) and lands in P.x0 in place, so every RRDB starts and ends in P.
// phase: -1 the whole block; 0 conv1..conv4 and conv5 on the `edge` band rows next to each apron (what the neighbours
// wait for); 1 conv5 on the band rows in between.  Phases need the f16-pair kernel's row ranges: for the other dtypes
// phase 0 is the whole block and phase 1 nothing.  `top` / `bottom` = apron rows of the band image (conv5 skips them in
// the phased form: they are overwritten by the neighbours' rows before anything reads them).
int fw_rdb(nesr_ctx* c, const FwState& F, int b, int r, hipStream_t s, int phase, int top, int bottom, int edge) {
    const int nf = c->nf, gc = c->gc;
    const double px = (double)F.N * F.h * F.w;
    char* cur = F.buf[r];
    const bool ranged = phase >= 0 && c->dtype == NESR_DTYPE_F32_SPLIT && F.N == 1 && F.h >= top + bottom + 2 * edge;
    if (phase == 1 && !ranged) return NESR_OK;
    if (phase >= 0 && !ranged) phase = -1;
    if (phase < 0) {   // one launch for the block: the strip kernel if it applies, else the fused f16-pair kernel if it applies
        int rc = try_strip(c, F, b, r, s);
        if (rc == FUSED_NA) rc = try_fused_rdb(c, F, b, r, s);
        if (rc != FUSED_NA) return rc;
    }
    for (int k = 0; k < 4 && phase != 1; ++k) {
        const Layer& Ly = c->layers[layer_id(b, r, k)];
        ConvArgs a = base_args(c, Ly, F.N, F.h, F.w);
        a.in = cur; a.in_map = F.m_t;
        a.out = cur; a.out_map = F.m_t; a.out_coff = nf + k * gc;
        a.lrelu = 1;
        NESR_TRY(launch_conv(c, a, s, Ly));
        if (c->timer.on) c->timer.flops += conv_flops(Ly, px);
    }
    const Layer& L5 = c->layers[layer_id(b, r, 4)];
    ConvArgs a = base_args(c, L5, F.N, F.h, F.w);
    a.in = cur; a.in_map = F.m_t;
    a.res1 = cur; a.res1_map = F.m_t; a.s1 = 0.2f;
    if (r < 2) {
        a.out = F.buf[r + 1];
    } else {
        a.out = F.buf[0];
        a.res2 = F.buf[0]; a.res2_map = F.m_t; a.s2 = 0.2f;
    }
    a.out_map = F.m_t; a.out_coff = 0;
    if (phase < 0) {
        NESR_TRY(launch_conv(c, a, s, L5));
    } else {
        // band rows [top, h - bottom); a side without an apron (a frame edge) has no neighbour waiting: its rows belong
        // to the interior launch
        const int lo = top, hi = F.h - bottom;
        const int e0 = top ? lo + edge : lo, e1 = bottom ? hi - edge : hi;      // interior = [e0, e1)
        auto rows = [&](int y0, int y1) -> int {
            if (y1 <= y0) return NESR_OK;
            ConvArgs q = a;
            q.y_lo = y0; q.y_hi = y1;
            NESR_TRY(launch_conv(c, q, s, L5));
            return NESR_OK;
        };
        int rc;
        if (phase == 0) {
            if (top && (rc = rows(lo, e0 < e1 ? e0 : e1))) return rc;
            if (bottom && (rc = rows(e1 > e0 ? e1 : e0, hi))) return rc;
        } else if ((rc = rows(e0, e1))) {
            return rc;
        }
    }
    if (c->timer.on && phase != 0) { c->timer.flops += conv_flops(L5, px); c->timer.launches += 5; }
    return NESR_OK;
}

// conv_body + trunk skip, the two nearest-x2 + conv stages, conv_hr, conv_last
int fw_tail(nesr_ctx* c, const FwState& F, float* y_f32, uint8_t* y_u8, int flip, int round_mode, hipStream_t s) {
    char* ws = c->ws;
    const int N = F.N, h = F.h, w = F.w;
    const Layer* tail = &c->layers[1 + c->nb * 15];
    {   // feat = feat + conv_body(trunk)   (in place on F)
        ConvArgs a = base_args(c, tail[0], N, h, w);
        a.in = F.buf[0]; a.in_map = F.m_t;
        a.out = ws + F.L.f; a.out_map = F.m_f;
        a.res1 = ws + F.L.f; a.res1_map = F.m_f; a.s1 = 1.0f;
        NESR_TRY(launch_conv(c, a, s, tail[0]));
    }
    {   // lrelu(conv_up1(nearest2x(feat)))
        ConvArgs a = base_args(c, tail[1], N, 2 * h, 2 * w);
        a.in = ws + F.L.f; a.in_map = F.m_f; a.in_h = h; a.in_w = w; a.up = 1;
        a.out = ws + F.L.u1; a.out_map = F.m_u1; a.lrelu = 1;
        NESR_TRY(launch_conv(c, a, s, tail[1]));
    }
    {   // lrelu(conv_up2(nearest2x(feat)))
        ConvArgs a = base_args(c, tail[2], N, 4 * h, 4 * w);
        a.in = ws + F.L.u1; a.in_map = F.m_u1; a.in_h = 2 * h; a.in_w = 2 * w; a.up = 1;
        a.out = ws + F.L.u2; a.out_map = F.m_u2; a.lrelu = 1;
        NESR_TRY(launch_conv(c, a, s, tail[2]));
    }
    {   // lrelu(conv_hr(feat))
        ConvArgs a = base_args(c, tail[3], N, 4 * h, 4 * w);
        a.in = ws + F.L.u2; a.in_map = F.m_u2;
        a.out = ws + F.L.u3; a.out_map = F.m_u2; a.lrelu = 1;
        NESR_TRY(launch_conv(c, a, s, tail[3]));
    }
    {   // conv_last -> planar f32 NCHW, or clamped + quantised u8 HWC
        ConvArgs a = base_args(c, tail[4], N, 4 * h, 4 * w);
        a.in = ws + F.L.u3; a.in_map = F.m_u2;
        a.cout_real = c->nout;
        a.out_nchw = y_f32;
        a.out_u8 = y_u8;
        a.u8_flip = flip;
        a.u8_round = round_mode;
        a.narrow_last = c->last_narrow;
        NESR_TRY(launch_conv(c, a, s, tail[4]));
    }
    return NESR_OK;
}

int run_forward(nesr_ctx* c, const float* x_f32, const uint8_t* x_u8, int flip, int N, int C, int H, int W,
                float* y_f32, uint8_t* y_u8, int round_mode, hipStream_t s, const Pack12Args* nesr12, long long y_u8_row_bytes) {
    FwState F;
    int rc = fw_setup(c, N, C, H, W, F);
    if (rc) return rc;
    c->band_valid = false;   // the workspace no longer holds a banded evaluation
    if ((rc = fw_first(c, F, x_f32, x_u8, flip, C, H, W, s, nesr12))) return rc;

    NESR_TRY(c->timer.begin(s));
    // opt-in (NESR_TRUNK=persist): measured slower at 2 tiles/CU, see DESIGN.md.  f32 and bf16 only: f16 runs per-layer launches
    const bool persist = c->trunk_mode == 2 && c->dtype != NESR_DTYPE_F16;
    if (persist && c->nb > 0) {
        // one cooperative launch for all 15*nb dense-block convs (tile-level dataflow sync)
        unsigned* sync = reinterpret_cast<unsigned*>(c->ws + F.L.sync);
        NESR_TRY(hipMemsetAsync(sync, 0, (size_t)F.L.sync_words * 4, s));
        TrunkArgs t;
        std::memset(&t, 0, sizeof(t));
        t.layers = c->d_trunk;
        t.nlayers = c->nb * 15;
        t.buf[0] = F.buf[0]; t.buf[1] = F.buf[1]; t.buf[2] = F.buf[2];
        t.map = F.m_t;
        t.n = N; t.h = F.h; t.w = F.w;
        t.progress = sync + 64;
        t.abort_flag = sync;
        t.zeros = c->d_weights;
        NESR_TRY(launch_trunk_persist(t, c->kind() == 1, s));
        c->last_sync = sync;
        if (c->timer.on) {
            for (int i = 0; i < c->nb * 15; ++i) c->timer.flops += conv_flops(c->layers[1 + i], (double)N * F.h * F.w);
            c->timer.launches += 1;
        }
    } else {
        // the fused dense-block kernels hold the device: serialised per device against other streams' (see DeviceLease)
        const bool lease = (strip_wanted(c) || (c->dtype == NESR_DTYPE_F32_SPLIT && c->rdb_mode != 0 && !c->shared_device)) && c->nb > 0;
        if (lease && (rc = lease_acquire(c, s))) return rc;
        c->chain_launches = c->chain_blocks = 0;
        rc = try_chained_rdb(c, F, s);
        if (rc < 0) return rc;
        if (rc == FUSED_NA)
            for (int b = 0; b < c->nb; ++b)
                for (int r = 0; r < 3; ++r)
                    if ((rc = fw_rdb(c, F, b, r, s))) return rc;
        if (lease && (rc = lease_release(c, s))) return rc;
    }
    NESR_TRY(c->timer.end(s));
    // conv_last's u8 epilogue writes whole rows.  Rows further apart than that: the image lands in the workspace's conv_up2 map
    // (48 of its >= 2048 bytes per input pixel; nothing reads that map once conv_hr has run) and is copied out row by row
    const long long dense = (long long)4 * F.w * c->nout;
    if (y_u8 && y_u8_row_bytes && y_u8_row_bytes != dense) {
        uint8_t* stage = reinterpret_cast<uint8_t*>(c->ws + F.L.u2);
        if ((rc = fw_tail(c, F, nullptr, stage, flip, round_mode, s))) return rc;
        NESR_TRY(hipMemcpy2DAsync(y_u8, (size_t)y_u8_row_bytes, stage, (size_t)dense, (size_t)dense, (size_t)4 * F.h, hipMemcpyDeviceToDevice, s));
        return NESR_OK;
    }
    return fw_tail(c, F, y_f32, y_u8, flip, round_mode, s);
}

}  // namespace nesr
