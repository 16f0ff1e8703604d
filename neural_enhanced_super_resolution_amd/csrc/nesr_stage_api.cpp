// C-ABI entries of the NESR pipeline's ESRGAN stage (include/nesr_hip.h): SuperResolutionPipeline._apply_esrgan and what it calls,
// u8 RGB frame in, u8 RGB frame out, for a host without torch -- nesr_forward_nesr_u8 (one window through the 12-channel network:
// nesr12.hip's pack, the forward graph of rrdb_forward.cpp, conv_last's truncating u8 epilogue), nesr_stage_route (the dispatch),
// nesr_stage_tile_plan (the tiler's rectangles) and nesr_apply_esrgan_u8 (the stage).  The two host-only entries restate
// nesr_adapter.apply_esrgan / tile_plan in the same integer and double operations (tests/test_nesr_stage_host.py compares them).
//
// What it stands behind in the reference: nesr/nesr.py:754-813 (_apply_esrgan), :845-903 (_apply_esrgan_12channel), :905-945
// (_apply_esrgan_3channel), :311-475 (_process_with_tiling); SURVEY.md section 8(a) rows a16-a19.
#include <algorithm>
#include <vector>

#include "rrdb_ctx.h"

#pragma clang fp contract(off)      // the plan is Python's arithmetic, operation by operation

using namespace nesr;

namespace {

#define ST_CALL(expr)                     \
    do {                                  \
        const int rc__ = (expr);          \
        if (rc__ != NESR_OK) return rc__; \
    } while (0)

constexpr int NET_SCALE = 4;      // output / input size of the network these entries take (no unshuffle)
constexpr int RECT = 13;          // ints per tile of a plan

int trunc_int(double v) { return (int)v; }      // Python's int(): toward zero

int check_mode(const std::string& w, int mode) {
    if (mode != NESR_INPUT_12CH && mode != NESR_INPUT_3CH_X4) return set_error(NESR_ERR_ARG, w + ": mode must be NESR_INPUT_12CH or NESR_INPUT_3CH_X4");
    return NESR_OK;
}

// the network of nesr/nesr.py:216: RRDBNet(num_in_ch=12, num_out_ch=3, scale=4)
int check_ctx(const std::string& w, const nesr_ctx* c) {
    if (c->cin0 != 12 || c->ufac() != 1 || c->nout != 3)
        return set_error(NESR_ERR_ARG, w + " needs the network of the NESR pipeline: 12 input channels, no pixel-unshuffle, 3 output channels (this context: " +
                                           std::to_string(c->cin0) + " into conv_first, unshuffle " + std::to_string(c->ufac()) + ", " + std::to_string(c->nout) + " out)");
    return NESR_OK;
}

int check_window(const std::string& w, int H, int W) {
    if (H < 2 || W < 2)
        return set_error(NESR_ERR_ARG, w + ": a window of " + std::to_string(H) + " x " + std::to_string(W) + " (both sides must be at least 2: the 3x3 blur reflects at "
                                           "the window's edge)");
    return NESR_OK;
}

// one window of `frame` (rows stride bytes apart) -> out, rows out_row_bytes apart; every argument has been checked
int forward_window(nesr_ctx* c, const uint8_t* frame, long long stride, int y0, int x0, int h, int w, int mode, uint8_t* out, long long out_row_bytes, void* stream) {
    Pack12Args p{};
    p.src = frame;
    p.src_stride = stride;
    p.y0 = y0; p.x0 = x0; p.h = h; p.w = w;
    p.mode = mode;
    // flip on: conv_last's channels are BGR, the frame is RGB (nesr/nesr.py:901)
    return run_forward(c, nullptr, nullptr, 1, 1, 12, h, w, nullptr, out, 0, static_cast<hipStream_t>(stream), &p, out_row_bytes);
}

int plan_args(const std::string& w, int H, int W, int tile, int padding, double uf, int net_scale) {
    if (H < 1 || W < 1 || tile < 1 || padding < 0 || net_scale < 1 || !(uf > 0.0) || !(uf <= 1024.0))
        return set_error(NESR_ERR_ARG, w + ": sizes and tile at least 1, padding at least 0, 0 < upscale_factor <= 1024");
    if (H > (1 << 20) || W > (1 << 20) || tile > (1 << 20) || padding > (1 << 20) || net_scale > 64) return set_error(NESR_ERR_ARG, w + ": sizes up to 2^20, net_scale up to 64");
    return NESR_OK;
}

bool fits_one_tile(int H, int W, int tile) { return H <= tile && W <= tile; }

// nesr_adapter.tile_plan
void plan(int H, int W, int tile, int padding, double uf, int ns, std::vector<int>& r) {
    r.clear();
    if (fits_one_tile(H, W, tile)) {      // nesr.py:326-328: the processor's own output, not a canvas
        const int one[RECT] = {0, H, 0, W, 0, ns * H, 0, ns * W, 0, ns * H, 0, ns * W, 0};
        r.assign(one, one + RECT);
        return;
    }
    const int nth = (H + tile - 1) / tile, ntw = (W + tile - 1) / tile;
    const int pu = padding > 0 ? trunc_int((double)padding * uf) : 0;
    for (int i = 0; i < nth; ++i)
        for (int j = 0; j < ntw; ++j) {
            const long long ya = (long long)i * tile - padding, yb = (long long)(i + 1) * tile + padding;
            const long long xa = (long long)j * tile - padding, xb = (long long)(j + 1) * tile + padding;
            const int y0 = (int)(ya > 0 ? ya : 0), y1 = (int)(yb < H ? yb : H), x0 = (int)(xa > 0 ? xa : 0), x1 = (int)(xb < W ? xb : W);
            int oy0 = trunc_int((double)y0 * uf), oy1 = trunc_int((double)y1 * uf), ox0 = trunc_int((double)x0 * uf), ox1 = trunc_int((double)x1 * uf);
            if (padding > 0) {
                if (y0 > 0) oy0 += pu;
                if (y1 < H) oy1 -= pu;
                if (x0 > 0) ox0 += pu;
                if (x1 < W) ox1 -= pu;
            }
            const int th = ns * (y1 - y0), tw = ns * (x1 - x0);
            const double sy = (double)th / (double)(y1 - y0), sx = (double)tw / (double)(x1 - x0);
            int ty0 = y0 == 0 ? 0 : trunc_int((double)padding * sy);
            int ty1 = y1 == H ? th : trunc_int((double)th - (double)padding * sy);
            int tx0 = x0 == 0 ? 0 : trunc_int((double)padding * sx);
            int tx1 = x1 == W ? tw : trunc_int((double)tw - (double)padding * sx);
            auto mn = [](int a, int b) { return a < b ? a : b; };
            auto mx = [](int a, int b) { return a > b ? a : b; };
            ty0 = mx(0, mn(ty0, th - 1));
            ty1 = mx(ty0 + 1, mn(ty1, th));
            tx0 = mx(0, mn(tx0, tw - 1));
            tx1 = mx(tx0 + 1, mn(tx1, tw));
            const int skip = (oy1 - oy0 <= 0 || ox1 - ox0 <= 0) ? 1 : 0;
            const int t[RECT] = {y0, y1, x0, x1, ty0, ty1, tx0, tx1, oy0, oy1, ox0, ox1, skip};
            r.insert(r.end(), t, t + RECT);
        }
}

size_t tile_bytes(int H, int W, int tile, int padding) {
    const long long wh = (long long)tile + 2LL * padding, ww = wh;
    const size_t h = (size_t)(wh < H ? wh : H), w = (size_t)(ww < W ? ww : W);
    return align_up(h * NET_SCALE * w * NET_SCALE * 3, 256);
}

}  // namespace

extern "C" {

int nesr_forward_nesr_u8(nesr_ctx* c, const uint8_t* rgb_dev, int64_t src_row_bytes, int H, int W, int mode, uint8_t* out_dev, int64_t out_row_bytes,
                         void* stream) {
    const std::string w = "nesr_forward_nesr_u8";
    if (!c || !rgb_dev || !out_dev) return set_error(NESR_ERR_ARG, w + ": null argument");
    RRDB_ONLY(c);
    ST_CALL(check_mode(w, mode));
    ST_CALL(check_ctx(w, c));
    ST_CALL(check_window(w, H, W));
    if (src_row_bytes < (int64_t)W * 3 || out_row_bytes < (int64_t)W * NET_SCALE * 3) return set_error(NESR_ERR_ARG, w + ": a row stride is smaller than the row");
    return forward_window(c, rgb_dev, src_row_bytes, 0, 0, H, W, mode, out_dev, out_row_bytes, stream);
}

int nesr_stage_route(int H, int W, int enable_tiling, int force_3channel, double threshold_mp, double large_mp, int* tiled, int* mode) {
    if (!tiled || !mode) return set_error(NESR_ERR_ARG, "nesr_stage_route: null argument");
    if (H < 1 || W < 1) return set_error(NESR_ERR_ARG, "nesr_stage_route: sizes at least 1");
    const double megapixels = (double)((long long)H * W) / (double)(1024 * 1024);
    bool use_tiling = enable_tiling && megapixels > threshold_mp;
    bool use_3ch = force_3channel != 0;
    if (megapixels > large_mp) use_tiling = use_3ch = true;
    *tiled = use_tiling ? 1 : 0;
    *mode = use_3ch ? NESR_INPUT_3CH_X4 : NESR_INPUT_12CH;
    return NESR_OK;
}

int nesr_stage_tile_plan(int H, int W, int tile, int padding, double upscale_factor, int net_scale, int* rects, int cap, int* n) {
    if (!n) return set_error(NESR_ERR_ARG, "nesr_stage_tile_plan: null argument");
    ST_CALL(plan_args("nesr_stage_tile_plan", H, W, tile, padding, upscale_factor, net_scale));
    std::vector<int> r;
    plan(H, W, tile, padding, upscale_factor, net_scale, r);
    *n = (int)(r.size() / RECT);
    if (rects && cap >= *n) std::copy(r.begin(), r.end(), rects);
    return NESR_OK;
}

size_t nesr_apply_esrgan_scratch_bytes(const nesr_ctx* c, int H, int W, int tiled, int tile, int padding) {
    const std::string w = "nesr_apply_esrgan_scratch_bytes";
    if (!c) { set_error(NESR_ERR_ARG, w + ": null argument"); return 0; }
    if (rrdb_only(c, w.c_str()) || check_ctx(w, c) || plan_args(w, H, W, tile, padding, 1.0, NET_SCALE)) return 0;
    if (!tiled || fits_one_tile(H, W, tile)) return 256;      // nothing is staged: the one forward writes `out`
    return tile_bytes(H, W, tile, padding);
}

int nesr_apply_esrgan_u8(nesr_ctx* c, const uint8_t* rgb_dev, int H, int W, int mode, int tiled, int tile, int padding, double upscale_factor, void* scratch_dev,
                         size_t scratch_bytes, uint8_t* out_dev, void* stream) {
    const std::string w = "nesr_apply_esrgan_u8";
    if (!c || !rgb_dev || !out_dev) return set_error(NESR_ERR_ARG, w + ": null argument");
    RRDB_ONLY(c);
    ST_CALL(check_mode(w, mode));
    ST_CALL(check_ctx(w, c));
    ST_CALL(plan_args(w, H, W, tile, padding, upscale_factor, NET_SCALE));
    if (!tiled || fits_one_tile(H, W, tile)) {
        ST_CALL(check_window(w, H, W));
        return forward_window(c, rgb_dev, (long long)W * 3, 0, 0, H, W, mode, out_dev, (long long)W * NET_SCALE * 3, stream);
    }
    std::vector<int> r;
    plan(H, W, tile, padding, upscale_factor, NET_SCALE, r);
    const int ntiles = (int)(r.size() / RECT);
    const int out_h = trunc_int((double)H * upscale_factor), out_w = trunc_int((double)W * upscale_factor);
    if (out_h < 1 || out_w < 1) return set_error(NESR_ERR_ARG, w + ": the canvas int(H uf) x int(W uf) is empty");
    // every refusal before the first launch: a frame is evaluated whole or not at all
    for (int t = 0; t < ntiles; ++t) {
        const int* q = &r[(size_t)t * RECT];
        ST_CALL(check_window(w, q[1] - q[0], q[3] - q[2]));
        if (!q[12] && (q[8] < 0 || q[10] < 0 || q[9] > out_h || q[11] > out_w)) return set_error(NESR_ERR_ARG, w + ": a tile's rectangle leaves the canvas");
    }
    const size_t need = tile_bytes(H, W, tile, padding);
    if (!scratch_dev || scratch_bytes < need)
        return set_error(NESR_ERR_ARG, w + ": scratch of " + std::to_string(scratch_bytes) + " bytes, nesr_apply_esrgan_scratch_bytes asks for " + std::to_string(need));
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* sc = static_cast<uint8_t*>(scratch_dev);
    const long long frame_row = (long long)W * 3, canvas_row = (long long)out_w * 3;
    NESR_TRY(hipSetDevice(c->device));
    NESR_TRY(hipMemsetAsync(out_dev, 0, (size_t)out_h * canvas_row, s));      // np.zeros((out_h, out_w, c)), nesr.py:340-344
    for (int t = 0; t < ntiles; ++t) {
        const int* q = &r[(size_t)t * RECT];
        const int wh = q[1] - q[0], ww = q[3] - q[2];
        const long long tile_row = (long long)ww * NET_SCALE * 3;
        // the reference evaluates a tile before it finds its rectangle empty (nesr.py:385-395, 428-431); so does this, and its range
        // word counts
        ST_CALL(forward_window(c, rgb_dev, frame_row, q[0], q[2], wh, ww, mode, sc, tile_row, stream));
        if (q[12]) continue;
        const int ch = q[5] - q[4], cw = q[7] - q[6], oh = q[9] - q[8], ow = q[11] - q[10];
        const uint8_t* crop = sc + (size_t)q[4] * tile_row + (size_t)q[6] * 3;
        uint8_t* dst = out_dev + (size_t)q[8] * canvas_row + (size_t)q[10] * 3;
        if (ch == oh && cw == ow)
            NESR_TRY(hipMemcpy2DAsync(dst, (size_t)canvas_row, crop, (size_t)tile_row, (size_t)ow * 3, (size_t)oh, hipMemcpyDeviceToDevice, s));
        else      // cv2.resize(..., INTER_LANCZOS4), nesr.py:438-443: the crop is read in place, the rectangle written in place
            ST_CALL(nesr_resize_u8(c->device, crop, ch, cw, 3, tile_row, dst, oh, ow, canvas_row, NESR_INTER_LANCZOS4, stream));
    }
    return NESR_OK;
}

}  // extern "C"
