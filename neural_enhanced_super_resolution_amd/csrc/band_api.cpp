// C ABI of the banded evaluation (exact multi-GPU mode: one row band of the frame per rank, SURVEY.md section 8(e) mode 2).
// The caller runs the stages of the forward graph (rrdb_forward.cpp) in order and refreshes the apron rows of the feature map each
// stage reads (nesr_band_rows) with its neighbours' band rows in between; banded.py holds that protocol.
//
// Inside ONE process the bands are contexts that know each other (nesr_band_link): a band's edge rows are written straight into its
// neighbours' landing buffers (band_exchange.hip), ordered by HIP events, and nesr_forward_banded / nesr_forward_banded_u8 run a
// whole untiled frame that way below Python.
#include <vector>

#include "rrdb_ctx.h"

using namespace nesr;

namespace {

int band_ready(const nesr_ctx* c) {
    if (!c->band_valid) return set_error(NESR_ERR_STATE, "nesr_band_begin has not run (or a whole-frame forward reused the workspace)");
    return NESR_OK;
}

// ---- row bands inside one process: links, landing buffers, the push and the frame driver

const char* SIDE_NAME[2] = {"upper", "lower"};

bool same_network(const nesr_ctx* a, const nesr_ctx* b) {
    return a->cin0 == b->cin0 && a->unshuffle == b->unshuffle && a->nf == b->nf && a->nb == b->nb && a->gc == b->gc && a->nout == b->nout &&
           a->dtype == b->dtype && a->winograd == b->winograd;
}

// the band forms: the f32 ones, whose per-pixel arithmetic does not depend on where a row lies (bit for bit the whole frame)
bool exact_form(const nesr_ctx* c) { return c->kind() == 0 || c->kind() == 2; }

// grows `*p` (on c's device) to `bytes`; a buffer that is replaced may still be in use, on this device or by a neighbour's push
int grow(nesr_ctx* c, char** p, size_t* have, size_t bytes) {
    if (bytes <= *have) return NESR_OK;
    NESR_TRY(hipSetDevice(c->device));
    if (*p) {
        for (nesr_ctx* nb : c->link.nb)
            if (nb && nb->device != c->device) {
                NESR_TRY(hipSetDevice(nb->device));
                NESR_TRY(hipDeviceSynchronize());
                NESR_TRY(hipSetDevice(c->device));
            }
        NESR_TRY(hipDeviceSynchronize());
        NESR_TRY(hipFree(*p));
        *p = nullptr;
        *have = 0;
    }
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return set_error(NESR_ERR_NOMEM, "hipMalloc(band buffer " + std::to_string(bytes) + " B): " + hipGetErrorString(e));
    *p = static_cast<char*>(q);
    *have = bytes;
    return NESR_OK;
}

// the four landing buffers of a receiver (two sides x two step parities), BAND_APRON rows of `row_bytes` each
int ensure_landing(nesr_ctx* c, size_t row_bytes) {
    const size_t bytes = align_up((size_t)BAND_APRON * row_bytes, 256);
    if (bytes <= c->link.land_bytes) return NESR_OK;
    size_t have = 0;
    for (int side = 0; side < 2; ++side)
        for (int par = 0; par < 2; ++par) {
            have = c->link.land_bytes;
            if (int rc = grow(c, &c->link.land[side][par], &have, bytes)) return rc;
        }
    c->link.land_bytes = have;
    return NESR_OK;
}

int ensure_events(nesr_ctx* c, bool own_stream) {
    BandLink& K = c->link;
    NESR_TRY(hipSetDevice(c->device));
    for (hipEvent_t* e : {&K.pushed[0], &K.pushed[1], &K.start, &K.done})
        if (!*e) NESR_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    if (own_stream && !K.stream) NESR_TRY(hipStreamCreateWithFlags(&K.stream, hipStreamNonBlocking));
    return NESR_OK;
}

// is the link c -> nb written by the push kernel?  Same device: the plain pointer.  Another device: peer access, enabled once here.
int decide_direct(nesr_ctx* c, nesr_ctx* nb, bool* direct) {
    *direct = false;
    if (c->link.force_staged || (c->nf * c->esize()) % 16 || (c->kind() == 0 && (c->ct() * c->esize()) % 16)) return NESR_OK;
    if (nb->device == c->device) { *direct = true; return NESR_OK; }
    int can = 0;
    NESR_TRY(hipDeviceCanAccessPeer(&can, c->device, nb->device));
    if (!can) return NESR_OK;
    NESR_TRY(hipSetDevice(c->device));
    const hipError_t e = hipDeviceEnablePeerAccess(nb->device, 0);
    if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
    else if (e != hipSuccess) { (void)hipGetLastError(); return NESR_OK; }     // refused by the runtime: the staged copy carries the rows
    *direct = true;
    return NESR_OK;
}

void unlink_side(nesr_ctx* c, int side) {
    nesr_ctx* nb = c->link.nb[side];
    if (nb && nb->link.nb[1 - side] == c) { nb->link.nb[1 - side] = nullptr; nb->link.direct[1 - side] = false; }
    c->link.nb[side] = nullptr;
    c->link.direct[side] = false;
}

int link_check(const nesr_ctx* c, const nesr_ctx* nb, const char* which) {
    if (!nb) return NESR_OK;
    if (nb == c) return set_error(NESR_ERR_ARG, "nesr_band_link: a context cannot be its own neighbour");
    if (nb->compact) return set_error(NESR_ERR_ARG, std::string("nesr_band_link: the ") + which + " neighbour is an SRVGGNetCompact context");
    if (!same_network(c, nb)) return set_error(NESR_ERR_ARG, std::string("nesr_band_link: the ") + which + " neighbour is a network of another geometry or dtype");
    return NESR_OK;
}

int link_one(nesr_ctx* c, int side, nesr_ctx* nb) {
    if (c->link.nb[side] == nb && (!nb || nb->link.nb[1 - side] == c)) return NESR_OK;      // as it is
    unlink_side(c, side);
    if (!nb) return NESR_OK;
    unlink_side(nb, 1 - side);
    c->link.nb[side] = nb;
    nb->link.nb[1 - side] = c;
    if (int rc = decide_direct(c, nb, &c->link.direct[side])) return rc;
    return decide_direct(nb, c, &nb->link.direct[1 - side]);
}

// source description of rows [row0, row0 + nrows) of the num_feat-channel slice of `buffer`, for the push kernel
void edge_source(const nesr_ctx* c, int buffer, int row0, int nrows, EdgePush& a, const char** src) {
    const FwState& F = c->band;
    const char* base = buffer < 3 ? F.buf[buffer] : c->ws + F.L.f;
    const Map& m = buffer < 3 ? F.m_t : F.m_f;
    a.npieces = nrows * F.w;
    if (c->kind() == 0) {
        a.nseg = 1; a.seg_stride = 0;
        a.piece_stride = (long long)m.pix * 4; a.piece_vecs = c->nf * 4 / 16;
        *src = base + (size_t)row0 * F.w * m.pix * 4;
    } else {
        const long long pixbytes = (long long)m.pix * 2;
        a.nseg = c->nf / 16; a.seg_stride = m.chunk * 2;
        a.piece_stride = pixbytes; a.piece_vecs = (int)(pixbytes / 16);
        *src = base + (size_t)row0 * F.w * pixbytes;
    }
}

int copy_rows(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t s) {
    if (dst_dev == src_dev) NESR_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    else NESR_TRY(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, s));
    return NESR_OK;
}

int push_edges(nesr_ctx* c, int buffer, int top, int bottom, int edge, int parity, hipStream_t s) {
    const FwState& F = c->band;
    const size_t row_bytes = (size_t)F.w * c->nf * c->esize(), bytes = (size_t)edge * row_bytes;
    const int row0[2] = {top, F.h - bottom - edge};
    for (int side = 0; side < 2; ++side)
        if (nesr_ctx* nb = c->link.nb[side])
            if (int rc = ensure_landing(nb, row_bytes)) return rc;
    EdgePush a{};
    bool any = false;
    for (int side = 0; side < 2; ++side) {
        nesr_ctx* nb = c->link.nb[side];
        if (!nb || !c->link.direct[side]) continue;
        edge_source(c, buffer, row0[side], edge, a, &a.src[side]);
        a.dst[side] = nb->link.land[1 - side][parity];     // my upper neighbour receives from below, and the other way round
        any = true;
    }
    NESR_TRY(hipSetDevice(c->device));
    if (any) NESR_TRY(launch_band_push_edges(a, s));
    for (int side = 0; side < 2; ++side) {
        nesr_ctx* nb = c->link.nb[side];
        if (!nb || c->link.direct[side]) continue;
        // staged link: the existing pack, then one copy into the neighbour's landing buffer (the same bytes)
        size_t have = c->link.send_bytes;
        for (int k = 0; k < 2; ++k) {
            have = c->link.send_bytes;
            if (int rc = grow(c, &c->link.send[k], &have, align_up((size_t)BAND_APRON * row_bytes, 256))) return rc;
        }
        c->link.send_bytes = have;
        if (int rc = nesr_band_rows(c, buffer, row0[side], edge, c->link.send[side], 0, s)) return rc;
        if (int rc = copy_rows(nb->link.land[1 - side][parity], nb->device, c->link.send[side], c->device, bytes, s)) return rc;
    }
    return NESR_OK;
}

int land_aprons(nesr_ctx* c, int buffer, int also_mask, int top, int bottom, int edge, int parity, hipStream_t s) {
    const int h = c->band.h;
    for (int b = 0; b < 4; ++b) {
        if (b != buffer && !((also_mask >> b) & 1)) continue;
        if (c->link.nb[0] && top)
            if (int rc = nesr_band_rows(c, b, top - edge, edge, c->link.land[0][parity], 1, s)) return rc;
        if (c->link.nb[1] && bottom)
            if (int rc = nesr_band_rows(c, b, h - bottom, edge, c->link.land[1][parity], 1, s)) return rc;
    }
    return NESR_OK;
}

int edge_args(const nesr_ctx* c, int buffer, int top, int bottom, int edge, int parity) {
    if (int rc = band_ready(c)) return rc;
    if (buffer < 0 || buffer > 3 || (parity != 0 && parity != 1)) return set_error(NESR_ERR_ARG, "bad buffer / parity");
    if (top < 0 || bottom < 0 || edge < 1 || edge > BAND_APRON || top + bottom + edge > c->band.h)
        return set_error(NESR_ERR_ARG, "bad apron / edge rows (1.." + std::to_string(BAND_APRON) + " edge rows inside the band)");
    return NESR_OK;
}

int plan_bands(int rows, int n, int* lo_hi) {
    if (rows < 1 || n < 1) return set_error(NESR_ERR_ARG, "nesr_band_plan: rows and bands from 1");
    for (int r = 0; r < n; ++r) {
        lo_hi[2 * r] = 2 * (int)(((long long)r * rows / n) / 2);
        if (r) lo_hi[2 * r - 1] = lo_hi[2 * r];
    }
    lo_hi[2 * n - 1] = rows;
    for (int r = 0; r < n; ++r)
        if (lo_hi[2 * r + 1] - lo_hi[2 * r] < BAND_APRON)
            return set_error(NESR_ERR_ARG, std::to_string(rows) + " internal rows over " + std::to_string(n) + " bands: bands shorter than the apron (" +
                                               std::to_string(BAND_APRON) + " rows)");
    return NESR_OK;
}

// One untiled frame as n row bands, one per context: exactly one of (x_f32, x_u8) and of (y_f32, y_u8), both on ctxs[0]'s device.
int forward_banded(nesr_ctx** ctxs, int n, const float* x_f32, const uint8_t* x_u8, int C, int H, int W, int flip, int round_mode, float* y_f32,
                   uint8_t* y_u8, void** streams, const char* entry) {
    const std::string w = entry;
    if (!ctxs || n < 1 || n > 64) return set_error(NESR_ERR_ARG, w + ": 1..64 contexts");
    for (int r = 0; r < n; ++r) {
        if (!ctxs[r]) return set_error(NESR_ERR_ARG, w + ": null context");
        if (int rc = rrdb_only(ctxs[r], entry)) return rc;
        for (int q = 0; q < r; ++q)
            if (ctxs[q] == ctxs[r]) return set_error(NESR_ERR_ARG, w + ": a context appears twice");
        if (!same_network(ctxs[0], ctxs[r])) return set_error(NESR_ERR_ARG, w + ": the contexts are networks of different geometry or dtype");
    }
    nesr_ctx* c0 = ctxs[0];
    if (!exact_form(c0)) return set_error(NESR_ERR_ARG, w + ": the f32 forms only (f32, f32-winograd, f32-direct: their bands are bit for bit the whole frame)");
    const int u = c0->ufac(), A = BAND_APRON;
    if (H < 1 || W < 1 || H % u || W % u) return set_error(NESR_ERR_ARG, w + ": H and W must be multiples of the unshuffle factor");
    if (C * u * u != c0->cin0) return set_error(NESR_ERR_ARG, w + ": input channels do not match conv_first");
    if (x_u8 && (C != 3 || c0->nout != 3)) return set_error(NESR_ERR_ARG, w + " needs a 3-channel-in / 3-channel-out network");
    const int h = H / u, wi = W / u, nout = c0->nout;
    std::vector<int> lo_hi(2 * (size_t)n);
    if (int rc = plan_bands(h, n, lo_hi.data())) return rc;

    // everything that may allocate or synchronise, before the first launch of the frame
    struct Band { int lo, hi, top, bottom, rows, Hin; hipStream_t s; const void* x; };
    std::vector<Band> B((size_t)n);
    const size_t out_px = y_u8 ? 1 : 4;     // bytes per output sample
    for (int r = 0; r < n; ++r) {
        nesr_ctx* c = ctxs[r];
        Band& b = B[r];
        b.lo = lo_hi[2 * r]; b.hi = lo_hi[2 * r + 1];
        b.top = r > 0 ? A : 0; b.bottom = r < n - 1 ? A : 0;
        b.rows = b.hi - b.lo + b.top + b.bottom; b.Hin = b.rows * u;
        if (int rc = ensure_events(c, !streams)) return rc;
        b.s = streams ? static_cast<hipStream_t>(streams[r]) : c->link.stream;
        if (int rc = link_one(c, 0, r > 0 ? ctxs[r - 1] : nullptr)) return rc;
        if (int rc = link_one(c, 1, r < n - 1 ? ctxs[r + 1] : nullptr)) return rc;
        c->band_valid = false;
        if (int rc = fw_setup(c, 1, C, b.Hin, W, c->band)) return rc;
        if (int rc = ensure_landing(c, (size_t)wi * c->nf * c->esize())) return rc;
        const bool stage_in = x_f32 || c->device != c0->device;
        if (stage_in)
            if (int rc = grow(c, &c->link.io[0], &c->link.io_bytes[0], (size_t)b.Hin * W * (x_u8 ? 3 : (size_t)C * 4))) return rc;
        if (int rc = grow(c, &c->link.io[1], &c->link.io_bytes[1], (size_t)4 * b.rows * 4 * wi * nout * out_px)) return rc;
    }

    NESR_TRY(hipSetDevice(c0->device));
    NESR_TRY(hipEventRecord(c0->link.start, B[0].s));
    std::vector<int> shared((size_t)n);
    int rc = NESR_OK;
    auto body = [&]() -> int {
        for (int r = 0; r < n; ++r) {      // the band's input rows, pixel_unshuffle + conv_first
            nesr_ctx* c = ctxs[r];
            Band& b = B[r];
            NESR_TRY(hipSetDevice(c->device));
            if (r) NESR_TRY(hipStreamWaitEvent(b.s, c0->link.start, 0));
            const size_t row0 = (size_t)(b.lo - b.top) * u;
            if (x_u8) {
                const uint8_t* src = x_u8 + row0 * W * 3;
                if (c->device != c0->device) {
                    if (int e = copy_rows(c->link.io[0], c->device, src, c0->device, (size_t)b.Hin * W * 3, b.s)) return e;
                    src = reinterpret_cast<const uint8_t*>(c->link.io[0]);
                }
                if (int e = fw_first(c, c->band, nullptr, src, flip, C, b.Hin, W, b.s)) return e;
            } else {
                float* xin = reinterpret_cast<float*>(c->link.io[0]);
                for (int ch = 0; ch < C; ++ch)
                    if (int e = copy_rows(xin + (size_t)ch * b.Hin * W, c->device, x_f32 + ((size_t)ch * H + row0) * W, c0->device, (size_t)b.Hin * W * 4, b.s))
                        return e;
                if (int e = fw_first(c, c->band, xin, nullptr, 0, C, b.Hin, W, b.s)) return e;
            }
            c->band_valid = true;
        }
        // 1 + 3 num_block exchange steps: step 0 carries conv_first's rows (they also refresh the trunk-skip copy, buffer 3), step i + 1 RDB i's
        for (int step = 0; step <= 3 * c0->nb; ++step) {
            const int i = step - 1, par = step & 1, buffer = step ? (i % 3 + 1) % 3 : 0;
            for (int r = 0; r < n; ++r) {
                nesr_ctx* c = ctxs[r];
                NESR_TRY(hipSetDevice(c->device));
                if (step)
                    if (int e = fw_rdb(c, c->band, i / 3, i % 3, B[r].s, 0, B[r].top, B[r].bottom, A)) return e;
                if (n > 1) {
                    if (int e = push_edges(c, buffer, B[r].top, B[r].bottom, A, par, B[r].s)) return e;
                    NESR_TRY(hipSetDevice(c->device));
                    NESR_TRY(hipEventRecord(c->link.pushed[par], B[r].s));
                }
            }
            for (int r = 0; r < n; ++r) {
                nesr_ctx* c = ctxs[r];
                NESR_TRY(hipSetDevice(c->device));
                if (step)
                    if (int e = fw_rdb(c, c->band, i / 3, i % 3, B[r].s, 1, B[r].top, B[r].bottom, A)) return e;
                for (int side = 0; side < 2; ++side)
                    if (nesr_ctx* nb = c->link.nb[side]) NESR_TRY(hipStreamWaitEvent(B[r].s, nb->link.pushed[par], 0));
                if (int e = land_aprons(c, buffer, step ? 0 : 8, B[r].top, B[r].bottom, A, par, B[r].s)) return e;
            }
        }
        for (int r = 0; r < n; ++r) {      // conv_body .. conv_last on the band image, its own rows to the frame's output
            nesr_ctx* c = ctxs[r];
            Band& b = B[r];
            NESR_TRY(hipSetDevice(c->device));
            const size_t Wo = (size_t)4 * wi, Ho = (size_t)4 * h, rows_o = (size_t)4 * (b.hi - b.lo), ext_o = (size_t)4 * b.rows;
            if (y_u8) {
                uint8_t* q = reinterpret_cast<uint8_t*>(c->link.io[1]);
                if (int e = fw_tail(c, c->band, nullptr, q, flip, round_mode, b.s)) return e;
                if (int e = copy_rows(y_u8 + (size_t)4 * b.lo * Wo * 3, c0->device, q + (size_t)4 * b.top * Wo * 3, c->device, rows_o * Wo * 3, b.s)) return e;
            } else {
                float* q = reinterpret_cast<float*>(c->link.io[1]);
                if (int e = fw_tail(c, c->band, q, nullptr, 0, 0, b.s)) return e;
                for (int ch = 0; ch < nout; ++ch)
                    if (int e = copy_rows(y_f32 + ((size_t)ch * Ho + (size_t)4 * b.lo) * Wo, c0->device, q + ((size_t)ch * ext_o + (size_t)4 * b.top) * Wo, c->device,
                                          rows_o * Wo * 4, b.s))
                        return e;
            }
            if (r) {
                NESR_TRY(hipEventRecord(c->link.done, b.s));
                NESR_TRY(hipSetDevice(c0->device));
                NESR_TRY(hipStreamWaitEvent(B[0].s, c->link.done, 0));     // the frame is complete behind the first band's stream
            }
        }
        return NESR_OK;
    };
    // bands share devices with each other and with whatever else the process runs: no persistent dense-block launch inside a band
    // (kernel selection only, never a value)
    for (int r = 0; r < n; ++r) { shared[r] = ctxs[r]->shared_device; ctxs[r]->shared_device = 1; }
    rc = body();
    for (int r = 0; r < n; ++r) ctxs[r]->shared_device = shared[r];
    return rc;
}

}  // namespace

void nesr::band_release(nesr_ctx* c) {
    BandLink& K = c->link;
    unlink_side(c, 0);
    unlink_side(c, 1);
    for (auto& side : K.land)
        for (char*& p : side) { if (p) (void)hipFree(p); p = nullptr; }
    for (char*& p : K.send) { if (p) (void)hipFree(p); p = nullptr; }
    for (char*& p : K.io) { if (p) (void)hipFree(p); p = nullptr; }
    for (hipEvent_t* e : {&K.pushed[0], &K.pushed[1], &K.start, &K.done}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
    if (K.stream) (void)hipStreamDestroy(K.stream);
    K = BandLink{};
}

extern "C" {

int nesr_band_begin(nesr_ctx* c, const void* x_dev, int C, int H, int W, void* stream) {
    RRDB_ONLY(c);
    if (!c || !x_dev) return set_error(NESR_ERR_ARG, "null argument");
    c->band_valid = false;
    int rc = fw_setup(c, 1, C, H, W, c->band);
    if (rc) return rc;
    if ((rc = fw_first(c, c->band, static_cast<const float*>(x_dev), nullptr, 0, C, H, W, static_cast<hipStream_t>(stream)))) return rc;
    c->band_valid = true;
    return NESR_OK;
}

int nesr_band_rdb(nesr_ctx* c, int index, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = band_ready(c)) return rc;
    if (index < 0 || index >= 3 * c->nb) return set_error(NESR_ERR_ARG, "RDB index out of range");
    NESR_TRY(hipSetDevice(c->device));
    return fw_rdb(c, c->band, index / 3, index % 3, static_cast<hipStream_t>(stream));
}

int nesr_band_rdb_phase(nesr_ctx* c, int index, int phase, int top, int bottom, int edge_rows, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = band_ready(c)) return rc;
    if (index < 0 || index >= 3 * c->nb) return set_error(NESR_ERR_ARG, "RDB index out of range");
    if ((phase != 0 && phase != 1) || top < 0 || bottom < 0 || edge_rows < 0 || top + bottom > c->band.h)
        return set_error(NESR_ERR_ARG, "bad phase / apron / edge rows");
    NESR_TRY(hipSetDevice(c->device));
    return fw_rdb(c, c->band, index / 3, index % 3, static_cast<hipStream_t>(stream), phase, top, bottom, edge_rows);
}

int nesr_band_pack_edges(nesr_ctx* c, int buffer, int top, int bottom, int nrows, void* top_dst, void* bottom_dst, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = band_ready(c)) return rc;
    const int h = c->band.h;
    if (top < 0 || bottom < 0 || nrows < 0 || top + bottom + nrows > h) return set_error(NESR_ERR_ARG, "bad apron / row count");
    int rc = NESR_OK;
    if (top_dst && (rc = nesr_band_rows(c, buffer, top, nrows, top_dst, 0, stream))) return rc;
    if (bottom_dst && (rc = nesr_band_rows(c, buffer, h - bottom - nrows, nrows, bottom_dst, 0, stream))) return rc;
    return NESR_OK;
}

int nesr_band_unpack_aprons(nesr_ctx* c, int buffer, int top, int bottom, int nrows, const void* top_src, const void* bottom_src, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = band_ready(c)) return rc;
    const int h = c->band.h;
    if ((top_src && nrows > top) || (bottom_src && nrows > bottom) || nrows < 0) return set_error(NESR_ERR_ARG, "more rows than the apron holds");
    int rc = NESR_OK;
    if (top_src && (rc = nesr_band_rows(c, buffer, top - nrows, nrows, const_cast<void*>(top_src), 1, stream))) return rc;
    if (bottom_src && (rc = nesr_band_rows(c, buffer, h - bottom, nrows, const_cast<void*>(bottom_src), 1, stream))) return rc;
    return NESR_OK;
}

int nesr_band_tail(nesr_ctx* c, void* y_dev, void* stream) {
    RRDB_ONLY(c);
    if (!c || !y_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (int rc = band_ready(c)) return rc;
    NESR_TRY(hipSetDevice(c->device));
    return fw_tail(c, c->band, static_cast<float*>(y_dev), nullptr, 0, 0, static_cast<hipStream_t>(stream));
}

size_t nesr_band_row_bytes(const nesr_ctx* c) {
    if (rrdb_only(c, __func__)) return 0;   // the error is set; a size cannot carry the code
    if (!c || !c->band_valid) return 0;
    return (size_t)c->band.w * c->nf * c->esize();
}

int nesr_band_rows(nesr_ctx* c, int buffer, int row0, int nrows, void* staging_dev, int write, void* stream) {
    RRDB_ONLY(c);
    if (!c || !staging_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (int rc = band_ready(c)) return rc;
    const FwState& F = c->band;
    if (buffer < 0 || buffer > 3 || row0 < 0 || nrows < 0 || row0 + nrows > F.h) return set_error(NESR_ERR_ARG, "bad buffer / row range");
    if (nrows == 0) return NESR_OK;
    NESR_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = buffer < 3 ? F.buf[buffer] : c->ws + F.L.f;
    const Map& m = buffer < 3 ? F.m_t : F.m_f;
    char* stg = static_cast<char*>(staging_dev);
    const int kind = c->kind();
    if (kind == 0) {
        // NHWC f32: channels [0, nf) of every pixel of the rows; the dense-block buffers have ct channels per pixel
        const size_t spitch = (size_t)m.pix * 4, width = (size_t)c->nf * 4, rows = (size_t)nrows * F.w;
        char* src = base + (size_t)row0 * F.w * spitch;
        if (write) NESR_TRY(hipMemcpy2DAsync(src, spitch, stg, width, width, rows, hipMemcpyDeviceToDevice, s));
        else NESR_TRY(hipMemcpy2DAsync(stg, width, src, spitch, width, rows, hipMemcpyDeviceToDevice, s));
        return NESR_OK;
    }
    // channel-blocked: the rows of one 16-channel chunk are one contiguous span; staging = [chunk][rows][w][pixel bytes]
    const size_t pixbytes = (size_t)m.pix * 2, span = (size_t)nrows * F.w * pixbytes;
    for (int ch = 0; ch < c->nf / 16; ++ch) {
        char* src = base + (size_t)ch * (size_t)m.chunk * 2 + (size_t)row0 * F.w * pixbytes;
        char* dst = stg + (size_t)ch * span;
        if (write) NESR_TRY(hipMemcpyAsync(src, dst, span, hipMemcpyDeviceToDevice, s));
        else NESR_TRY(hipMemcpyAsync(dst, src, span, hipMemcpyDeviceToDevice, s));
    }
    return NESR_OK;
}

int nesr_band_link(nesr_ctx* c, nesr_ctx* up, nesr_ctx* down) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = link_check(c, up, SIDE_NAME[0])) return rc;
    if (int rc = link_check(c, down, SIDE_NAME[1])) return rc;
    if (up && up == down) return set_error(NESR_ERR_ARG, "nesr_band_link: one context as both neighbours");
    if (int rc = ensure_events(c, false)) return rc;
    if (int rc = link_one(c, 0, up)) return rc;
    return link_one(c, 1, down);
}

int nesr_band_unlink(nesr_ctx* c) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    unlink_side(c, 0);
    unlink_side(c, 1);
    return NESR_OK;
}

int nesr_band_set_staged(nesr_ctx* c, int on) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    c->link.force_staged = on != 0;
    for (int side = 0; side < 2; ++side)
        if (nesr_ctx* nb = c->link.nb[side])
            if (int rc = decide_direct(c, nb, &c->link.direct[side])) return rc;
    return NESR_OK;
}

int nesr_band_link_state(const nesr_ctx* c) {
    if (int rc = rrdb_only(c, __func__)) return rc;
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    int v = 0;
    for (int side = 0; side < 2; ++side)
        if (const nesr_ctx* nb = c->link.nb[side])
            v |= (1 << side) | (c->link.direct[side] ? 4 << side : 0) | (nb->device != c->device ? 16 << side : 0);
    return v;
}

int nesr_band_push_edges(nesr_ctx* c, int buffer, int top, int bottom, int edge_rows, int parity, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = edge_args(c, buffer, top, bottom, edge_rows, parity)) return rc;
    for (const nesr_ctx* nb : c->link.nb)
        if (nb && (!nb->band_valid || nb->band.w != c->band.w))
            return set_error(NESR_ERR_STATE, "nesr_band_push_edges: a neighbour has no band image of this width (nesr_band_begin first)");
    return push_edges(c, buffer, top, bottom, edge_rows, parity, static_cast<hipStream_t>(stream));
}

int nesr_band_land_aprons(nesr_ctx* c, int buffer, int also_mask, int top, int bottom, int edge_rows, int parity, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = edge_args(c, buffer, top, bottom, edge_rows, parity)) return rc;
    if (also_mask & ~15) return set_error(NESR_ERR_ARG, "nesr_band_land_aprons: also_mask has bits 0..3");
    if ((c->link.nb[0] && top && edge_rows > top) || (c->link.nb[1] && bottom && edge_rows > bottom)) return set_error(NESR_ERR_ARG, "more rows than the apron holds");
    if ((c->link.nb[0] || c->link.nb[1]) && c->link.land_bytes < (size_t)edge_rows * c->band.w * c->nf * c->esize())
        return set_error(NESR_ERR_STATE, "nesr_band_land_aprons: nothing has been pushed to this context");
    NESR_TRY(hipSetDevice(c->device));
    return land_aprons(c, buffer, also_mask, top, bottom, edge_rows, parity, static_cast<hipStream_t>(stream));
}

int nesr_band_plan(int internal_rows, int n, int* lo_hi, int cap) {
    if (!lo_hi || n < 1 || cap < n) return set_error(NESR_ERR_ARG, "nesr_band_plan: lo_hi must hold n (lo, hi) pairs");
    return plan_bands(internal_rows, n, lo_hi);
}

int nesr_forward_banded_u8(nesr_ctx** ctxs, int n, const uint8_t* frame_u8, int H, int W, int flip_rgb, int round_mode, uint8_t* out_u8, void** streams) {
    if (!frame_u8 || !out_u8) return set_error(NESR_ERR_ARG, "null argument");
    return forward_banded(ctxs, n, nullptr, frame_u8, 3, H, W, flip_rgb ? 1 : 0, round_mode == NESR_ROUND_NEAREST ? 1 : 0, nullptr, out_u8, streams, __func__);
}

int nesr_forward_banded(nesr_ctx** ctxs, int n, const void* x_dev, int C, int H, int W, void* y_dev, void** streams) {
    if (!x_dev || !y_dev) return set_error(NESR_ERR_ARG, "null argument");
    return forward_banded(ctxs, n, static_cast<const float*>(x_dev), nullptr, C, H, W, 0, 0, static_cast<float*>(y_dev), nullptr, streams, __func__);
}

}  // extern "C"
