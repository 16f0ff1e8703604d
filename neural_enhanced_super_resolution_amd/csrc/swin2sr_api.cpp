// Swin2SR contexts (nesr_swin2sr_*): the configuration check, strict weight loading, the padded and transposed upload, the
// continuous position bias tables (computed once on the host in double), a workspace that grows with the frame, and the forward
// as a chain of launches of the three kernels of swin2sr.hip, over one frame or over a batch of images of one size: the images of
// nesr_swin2sr_forward_batch_f32, or the windows the tile plan cuts a large frame into (nesr_swin2sr_upscale_tiled_u8), or the overlapped
// windows whose f32 outputs are summed and averaged (nesr_swin2sr_upscale_overlapped_u8: the authors' --tile / --tile_overlap).  Stands behind transformers' Swin2SRForImageSuperResolution and,
// for nesr_swin2sr_upscale_u8, its Swin2SRImageProcessor and the documented post-processing.
#include <cmath>
#include <cstring>

#include "net_context.h"
#include "swin2sr_api.h"

using namespace nesr;

namespace {

// offsets in floats into the packed f32 weights; the ...h ones in halves into the f16 copy of the fp16 form
struct S2ConvW {
    size_t w = 0, b = 0, wh = 0;
    int cin = 0, cinp = 0, cout = 0, coutp = 0;
};
struct S2LayerW {
    size_t wqkv, bqkv, scale, bias, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
    size_t wqkvh = 0, woh = 0, w1h = 0, w2h = 0;
};
struct S2StageW {
    std::vector<S2LayerW> layers;
    S2ConvW conv;
    size_t wproj, bproj, wprojh = 0;
};

enum { UP_PIXELSHUFFLE = 0, UP_DIRECT = 1, UP_NEAREST = 2 };
constexpr int kFeatures = 64;      // num_features of the pixelshuffle and nearest+conv heads
constexpr int kMaxStages = 16;
constexpr int kProcessorPad = 8;   // Swin2SRImageProcessor.size_divisor
const float kMean[3] = {0.4488f, 0.4371f, 0.4040f};
const char* const kName = "Swin2SR";      // in the texts of a failed launch, workspace or weight allocation
const char* const kCreate = "nesr_swin2sr_create";

}  // namespace

struct nesr_swin2sr : NetContext {      // d_w16: the fp16 form's second copy of every GEMM weight, [n][K]
    int nin = 3, nout = 3, C = 180, cs = 192, nst = 0, ws = 8, hidden = 360, hidp = 368, heads = 6, d = 30, dp = 32, scale = 2, up = 0;
    int depth[kMaxStages];
    float eps = 1e-5f, range = 1.f, mean[4] = {0.f, 0.f, 0.f, 0.f};
    S2ConvW first, after, before, up1, up2, hr, fin, direct;
    std::vector<S2ConvW> ups;
    size_t wpe = 0, bpe = 0, peg = 0, peb = 0, lng = 0, lnb = 0, wpeh = 0;
    std::vector<S2StageW> stages;
};

namespace {

bool ends_with(const std::string& s, const char* tail) {
    const size_t n = strlen(tail);
    return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}

bool is_pow2(int v) { return v >= 1 && (v & (v - 1)) == 0; }

S2Attn attn_shape(const nesr_swin2sr* c) {
    S2Attn a;
    memset(&a, 0, sizeof(a));
    a.ws = c->ws, a.heads = c->heads, a.d = c->d, a.dp = c->dp, a.c = c->C, a.cs = c->cs;
    return a;
}

S2Conv conv_args(const nesr_swin2sr* c, const S2ConvW& w, const float* in, int H, int W, int cs_in, float* out, int cs_out) {
    S2Conv a;
    memset(&a, 0, sizeof(a));
    a.batch = 1, a.in_mode = S2_IN_ROWS, a.in = in, a.H = H, a.W = W, a.cin = w.cin, a.cinp = w.cinp, a.cs_in = cs_in;
    a.range = c->range;
    for (int i = 0; i < 4; ++i) a.mean[i] = c->mean[i];
    a.w = c->d_w + w.w, a.bias = c->d_w + w.b, a.cout = w.cout, a.coutp = w.coutp;
    a.shuffle = 1, a.out_mode = S2_OUT_ROWS, a.out = out, a.cs_out = cs_out;
    if (c->dtype == NESR_DTYPE_F16 && w.cin > 4) a.f16 = 1, a.wh = c->d_w16 + w.wh, a.status = c->d_status;      // not the frame's conv (K = 4 a tap)
    return a;
}

bool f16_form(const nesr_swin2sr* c) { return c->dtype == NESR_DTYPE_F16; }

// layer j's attention block over B images of H x W tokens
S2Attn attn_args(const nesr_swin2sr* c, const S2LayerW& L, int j, const float* in, float* out, int B, int H, int W) {
    S2Attn a = attn_shape(c);
    const float* w = c->d_w;
    a.batch = B, a.H = H, a.W = W, a.shift = j % 2 ? c->ws / 2 : 0, a.in = in, a.out = out;
    a.wqkv = w + L.wqkv, a.bqkv = w + L.bqkv, a.scale = w + L.scale, a.bias = w + L.bias, a.wo = w + L.wo, a.bo = w + L.bo;
    a.ln_g = w + L.ln1g, a.ln_b = w + L.ln1b, a.eps = c->eps;
    if (f16_form(c)) a.f16 = 1, a.wqkvh = c->d_w16 + L.wqkvh, a.woh = c->d_w16 + L.woh, a.status = c->d_status;
    return a;
}

// a row launch over M tokens: an optional product (w1 at offset w1, (size_t)-1 for none; its f16 copy at w1h), LayerNorm, residual
S2Rows rows_args(const nesr_swin2sr* c, int M, const float* in, size_t w1, size_t b1, size_t w1h, bool ln, size_t g, size_t b, float eps, const float* res,
                 float* o) {
    S2Rows a;
    memset(&a, 0, sizeof(a));
    a.m = M, a.c = c->C, a.cs = c->cs, a.in = in;
    if (w1 != (size_t)-1) {
        a.w1 = c->d_w + w1, a.b1 = c->d_w + b1, a.n1p = c->cs;
        if (f16_form(c)) a.f16 = 1, a.w1h = c->d_w16 + w1h, a.status = c->d_status;
    }
    if (ln) a.ln_g = c->d_w + g, a.ln_b = c->d_w + b, a.eps = eps;
    a.res = res, a.out = o;
    return a;
}

// layer L's MLP block, in place on X
S2Rows mlp_args(const nesr_swin2sr* c, const S2LayerW& L, int M, float* X) {
    S2Rows a = rows_args(c, M, X, L.w1, L.b1, L.w1h, true, L.ln2g, L.ln2b, c->eps, X, X);
    a.n1p = c->hidp, a.gelu = 1, a.w2 = c->d_w + L.w2, a.b2 = c->d_w + L.b2;
    if (f16_form(c)) a.w2h = c->d_w16 + L.w2h;
    return a;
}

// the fp16 form's range word, read behind a call's launches (net_range_begin clears it in front of them)
int range_end(nesr_swin2sr* c, hipStream_t s, const char* entry) {
    return net_range_end(c, s, entry, "an activation of the fp16 form was non-finite or exceeded 65504 in magnitude when it was rounded; the output is not valid "
                                      "(the f32 form carries such values)");
}

// The images of one forward: B of them, each fh x fw.  tile = 0: they lie one after the other in `frame` and in `out` (f32), or
// there is one (u8).  tile > 0 (u8 in and out): they are the tiles tile0 .. tile0 + B - 1 of the plan of an FH x FW frame.
// ov_step > 0 (u8 in, f32 out, fh = fw = t): they are the windows tile0 .. tile0 + B - 1 of the overlapped plan of the FH x FW frame
// padded to PH x PW, read from the frame's symmetric extension without any padding of their own; `out` takes them one after the other.
struct S2Batch {
    int B = 1, tile = 0, tile_pad = 0, tiles_x = 1, tile0 = 0, FH = 0, FW = 0;
    int ov_step = 0, PH = 0, PW = 0;
};

// the model's input (after the processor's symmetric padding of a u8 frame) and the conv's domain (after the reflect padding to the window)
int padded_size(const nesr_swin2sr* c, bool frame_u8, int fh, int fw, int& mh, int& mw, int& H, int& W) {
    mh = frame_u8 ? (fh / kProcessorPad + 1) * kProcessorPad : fh, mw = frame_u8 ? (fw / kProcessorPad + 1) * kProcessorPad : fw;
    H = round_up(mh, c->ws), W = round_up(mw, c->ws);
    if (H - mh > mh - 1 || W - mw > mw - 1)
        return set_error(NESR_ERR_ARG, "Swin2SR: the reflect padding to the window (" + std::to_string(c->ws) + ") is wider than the image allows");
    return NESR_OK;
}

// what forward() allocates for B images of H x W tokens: four activation buffers and the two of the upsampling head
size_t workspace_bytes(const nesr_swin2sr* c, int H, int W, size_t B, size_t& act, size_t& upb) {
    const size_t T = (size_t)H * W, cs = c->cs, sc = c->scale;
    act = align_up(B * T * cs * 4, 256), upb = c->up == UP_DIRECT ? 0 : align_up(B * T * sc * sc * kFeatures * 4, 256);
    return 4 * act + 2 * upb;
}

// frame: u8 HWC [fh][fw][3] (processor route) or f32 NCHW [nin][fh][fw] (model route); out: f32 NCHW or u8 HWC, cropped to fh s x fw s
int forward_launches(nesr_swin2sr* c, const void* frame, bool frame_u8, int fh, int fw, void* out, bool out_u8, hipStream_t s, const S2Batch& bt) {
    int mh, mw, H, W;
    int rc = padded_size(c, frame_u8 && bt.ov_step == 0, fh, fw, mh, mw, H, W);
    if (rc) return rc;
    const size_t T = (size_t)bt.B * H * W;
    if (bt.B < 1 || bt.B > 65535 || T > (size_t)S2_ROWS_MAX)
        return set_error(NESR_ERR_ARG, "Swin2SR: a batch of " + std::to_string(bt.B) + " images of " + std::to_string(H) + " x " + std::to_string(W) +
                                           " tokens: at most 65535 images and 2^31 - 33 tokens go through one launch");
    size_t act, upb;
    rc = grow(c->ws_buf, c->ws_bytes, workspace_bytes(c, H, W, bt.B, act, upb), kName);
    if (rc) return rc;
    auto conv = [&](const S2ConvW& w, const float* in, int h, int wd, int cs_in, float* o, int cs_out) {
        S2Conv a = conv_args(c, w, in, h, wd, cs_in, o, cs_out);
        a.batch = bt.B;
        return a;
    };
    auto tiled = [&](S2Conv& a) {      // where the first conv finds image b and the last one puts it
        a.tile = bt.tile, a.tile_pad = bt.tile_pad, a.tiles_x = bt.tiles_x, a.tile0 = bt.tile0, a.up = c->scale;
        a.FH = bt.tile > 0 ? bt.FH : fh, a.FW = bt.tile > 0 ? bt.FW : fw;
    };
    float* FIRST = reinterpret_cast<float*>(c->ws_buf);
    float* XS = reinterpret_cast<float*>(c->ws_buf + act);
    float* X = reinterpret_cast<float*>(c->ws_buf + 2 * act);
    float* T1 = reinterpret_cast<float*>(c->ws_buf + 3 * act);
    float* UA = reinterpret_cast<float*>(c->ws_buf + 4 * act);
    float* UB = reinterpret_cast<float*>(c->ws_buf + 4 * act + upb);
    const int M = (int)T, CS = c->cs;

    {   // first_convolution on the padded, normalised frame -> FIRST (the long residual)
        S2Conv a = conv(c->first, nullptr, H, W, 0, FIRST, CS);
        a.in_mode = frame_u8 ? S2_IN_FRAME_U8 : S2_IN_FRAME_F32, a.in = frame, a.fh = fh, a.fw = fw, a.mh = mh, a.mw = mw;
        tiled(a);
        if (bt.ov_step > 0) a.in_mode = S2_IN_WINDOW_U8, a.FH = bt.FH, a.FW = bt.FW, a.ov_step = bt.ov_step, a.PH = bt.PH, a.PW = bt.PW;
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_CONV, s, [&] { return launch_s2_conv(a, s); });
    }
    {   // patch embedding: 1x1 projection + LayerNorm (torch's default eps) -> XS
        const S2Rows a = rows_args(c, M, FIRST, c->wpe, c->bpe, c->wpeh, true, c->peg, c->peb, 1e-5f, nullptr, XS);
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_PROJ, s, [&] { return launch_s2_rows(a, s); });
    }
    for (int i = 0; i < c->nst; ++i) {
        const S2StageW& S = c->stages[i];
        for (int j = 0; j < c->depth[i]; ++j) {
            const S2LayerW& L = S.layers[j];
            {
                const S2Attn a = attn_args(c, L, j, j == 0 ? XS : X, X, bt.B, H, W);      // the stage's input stays in XS
                NESR_RUN(c->timer, kName, NESR_S2_GROUP_ATTENTION, s, [&] { return launch_s2_attn(a, s); });
            }
            {
                const S2Rows a = mlp_args(c, L, M, X);
                NESR_RUN(c->timer, kName, NESR_S2_GROUP_MLP, s, [&] { return launch_s2_rows(a, s); });
            }
        }
        {
            const S2Conv a = conv(S.conv, X, H, W, CS, T1, CS);
            NESR_RUN(c->timer, kName, NESR_S2_GROUP_CONV, s, [&] { return launch_s2_conv(a, s); });
        }
        {   // the stage's 1x1 projection + the stage's input, in place
            const S2Rows a = rows_args(c, M, T1, S.wproj, S.bproj, S.wprojh, false, 0, 0, 0.f, XS, XS);
            NESR_RUN(c->timer, kName, NESR_S2_GROUP_PROJ, s, [&] { return launch_s2_rows(a, s); });
        }
    }
    {   // the encoder's LayerNorm -> X
        const S2Rows a = rows_args(c, M, XS, (size_t)-1, 0, 0, true, c->lng, c->lnb, c->eps, nullptr, X);
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_PROJ, s, [&] { return launch_s2_rows(a, s); });
    }
    {   // conv_after_body + the long residual -> T1
        S2Conv a = conv(c->after, X, H, W, CS, T1, CS);
        a.res = FIRST, a.cs_res = CS;
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_CONV, s, [&] { return launch_s2_conv(a, s); });
    }
    auto finish = [&](S2Conv& a) {      // / img_range + mean, the crop, f32 or u8
        a.out_mode = out_u8 ? S2_OUT_U8 : S2_OUT_F32, a.out = out, a.cs_out = 0, a.oh = fh * c->scale, a.ow = fw * c->scale;
        tiled(a);
    };
    const int F = kFeatures;
    if (c->up == UP_DIRECT) {
        S2Conv a = conv(c->direct, T1, H, W, CS, nullptr, 0);
        a.shuffle = c->scale;
        finish(a);
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_UPSAMPLE, s, [&] { return launch_s2_conv(a, s); });
        return NESR_OK;
    }
    {
        S2Conv a = conv(c->before, T1, H, W, CS, UA, F);
        a.lrelu = 1, a.slope = 0.01f;
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_UPSAMPLE, s, [&] { return launch_s2_conv(a, s); });
    }
    float* cur = UA;
    float* other = UB;
    int h = H, w = W;
    if (c->up == UP_PIXELSHUFFLE) {
        const int r = c->scale == 3 ? 3 : 2;
        for (const S2ConvW& u : c->ups) {
            S2Conv a = conv(u, cur, h, w, F, other, F);
            a.shuffle = r;
            NESR_RUN(c->timer, kName, NESR_S2_GROUP_UPSAMPLE, s, [&] { return launch_s2_conv(a, s); });
            std::swap(cur, other);
            h *= r, w *= r;
        }
    } else {
        for (const S2ConvW* u : {&c->up1, &c->up2}) {
            h *= 2, w *= 2;
            S2Conv a = conv(*u, cur, h, w, F, other, F);
            a.in_mode = S2_IN_NEAREST2, a.lrelu = 1, a.slope = 0.2f;
            NESR_RUN(c->timer, kName, NESR_S2_GROUP_UPSAMPLE, s, [&] { return launch_s2_conv(a, s); });
            std::swap(cur, other);
        }
        S2Conv a = conv(c->hr, cur, h, w, F, other, F);
        a.lrelu = 1, a.slope = 0.2f;
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_UPSAMPLE, s, [&] { return launch_s2_conv(a, s); });
        std::swap(cur, other);
    }
    S2Conv a = conv(c->fin, cur, h, w, F, nullptr, 0);
    finish(a);
    NESR_RUN(c->timer, kName, NESR_S2_GROUP_UPSAMPLE, s, [&] { return launch_s2_conv(a, s); });
    return NESR_OK;
}

// the launches between the range word's reset and its check (fp16 form: the call waits for the stream and may return NESR_ERR_RANGE)
int forward(nesr_swin2sr* c, const void* frame, bool frame_u8, int fh, int fw, void* out, bool out_u8, hipStream_t s, const S2Batch& bt = S2Batch()) {
    int rc = net_range_begin(c, s);
    if (!rc) rc = forward_launches(c, frame, frame_u8, fh, fw, out, out_u8, s, bt);
    return rc ? rc : range_end(c, s, kName);
}

// The overlapped plan of an H x W frame (the authors' --tile / --tile_overlap): the frame padded once to the window, the effective
// tile t = min(tile, PH, PW), its stride and the counts of s2_overlap_axis.  The argument checks are the plan entry's, the
// workspace query's and the upscale's alike; `entry` leads the text.
struct S2OverlapPlan {
    int PH = 0, PW = 0, t = 0, step = 0, ny = 0, nx = 0;
};
int overlap_plan(const std::string& entry, int ws, int H, int W, int tile, int tile_overlap, S2OverlapPlan& p) {
    if (ws < 1 || ws > (1 << 12)) return set_error(NESR_ERR_ARG, entry + ": window_size must be 1 .. 4096, got " + std::to_string(ws));
    if (H < 1 || W < 1 || (long long)H * W > NESR_SWIN2SR_TILED_MAX_PIXELS) return set_error(NESR_ERR_ARG, entry + ": a frame (H x W) of 1 .. 2^28 pixels");
    if (tile < 1 || tile > (1 << 24)) return set_error(NESR_ERR_ARG, entry + ": tile must be 1 .. 2^24, got " + std::to_string(tile));
    p.PH = round_up(H, ws), p.PW = round_up(W, ws);
    p.t = std::min(tile, std::min(p.PH, p.PW));
    if (p.t % ws)
        return set_error(NESR_ERR_ARG, entry + ": the effective tile min(tile, padded H, padded W) = " + std::to_string(p.t) + " must be a multiple of window_size " +
                                           std::to_string(ws) + " (no window is padded on this route)");
    if (tile_overlap < 0 || tile_overlap >= p.t)
        return set_error(NESR_ERR_ARG, entry + ": tile_overlap must be 0 .. " + std::to_string(p.t - 1) + " (below the effective tile), got " + std::to_string(tile_overlap));
    p.step = p.t - tile_overlap;
    int v, f, l;
    s2_overlap_axis(p.PH, p.t, p.step, 0, 0, p.ny, v, f, l);
    s2_overlap_axis(p.PW, p.t, p.step, 0, 0, p.nx, v, f, l);
    if ((long long)p.ny * p.nx > (1ll << 26))
        return set_error(NESR_ERR_ARG, entry + ": tile and tile_overlap give " + std::to_string((long long)p.ny * p.nx) + " windows, more than 2^26");
    return NESR_OK;
}
// the staging buffer of B windows' f32 outputs, and the accumulator of the padded frame (12 bytes a padded output pixel)
size_t overlap_y_bytes(const nesr_swin2sr* c, const S2OverlapPlan& p, size_t B) { return align_up(B * 3 * (size_t)p.t * c->scale * p.t * c->scale * 4, 256); }
size_t overlap_e_bytes(const nesr_swin2sr* c, const S2OverlapPlan& p) { return align_up(3 * s2_overlap_plane(p.PH, p.PW, c->scale) * 4, 256); }

}  // namespace

extern "C" {

int nesr_swin2sr_create(nesr_swin2sr** out, int device_id, int image_size, int patch_size, int num_channels, int num_channels_out, int embed_dim,
                        int num_stages, const int* depths, const int* num_heads, int window_size, double mlp_ratio, int qkv_bias,
                        int use_absolute_embeddings, double layer_norm_eps, int upscale, double img_range, const char* resi_connection,
                        const char* upsampler) {
    if (!out) return set_error(NESR_ERR_ARG, "nesr_swin2sr_create: null out");
    *out = nullptr;
    if (!depths || !num_heads || !resi_connection || !upsampler) return set_error(NESR_ERR_ARG, "nesr_swin2sr_create: null configuration argument");
    if (num_stages < 1 || num_stages > kMaxStages) return set_error(NESR_ERR_ARG, "nesr_swin2sr_create: depths must have 1 .. 16 entries");
    if (num_channels < 1 || num_channels > 4 || num_channels_out < 1 || num_channels_out > 4)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_create: num_channels and num_channels_out must be 1 .. 4");
    if (embed_dim < 1 || embed_dim > 1024 || window_size < 1 || image_size < 1 || upscale < 1 || upscale > 8 || !(mlp_ratio > 0) || !(img_range > 0) ||
        !(layer_norm_eps >= 0))
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_create: a size of the configuration is not positive or out of range");
    for (int i = 0; i < num_stages; ++i)
        if (depths[i] < 1 || depths[i] > 64 || num_heads[i] < 1) return set_error(NESR_ERR_ARG, "nesr_swin2sr_create: depths must be 1 .. 64 and num_heads positive");
    const std::string up = upsampler, resi = resi_connection;
    if (up == "pixelshuffle_aux") return unsupported(kCreate, "upsampler", "pixelshuffle_aux (and its bicubic branch) is not supported");
    if (up != "pixelshuffle" && up != "pixelshuffledirect" && up != "nearest+conv")
        return unsupported(kCreate, "upsampler", "'" + up + "' is not one of pixelshuffle, pixelshuffledirect, nearest+conv");
    if (resi != "1conv") return unsupported(kCreate, "resi_connection", "'" + resi + "' is not supported (1conv only)");
    if (use_absolute_embeddings) return unsupported(kCreate, "use_absolute_embeddings", "absolute position embeddings are not supported");
    if (patch_size != 1) return unsupported(kCreate, "patch_size", "must be 1");
    if (!qkv_bias) return unsupported(kCreate, "qkv_bias", "must be true");
    if (image_size <= window_size) return unsupported(kCreate, "image_size", "must exceed window_size (the window and the shift are the configuration's then)");
    for (int i = 0; i < num_stages; ++i) {
        if (num_heads[i] != num_heads[0]) return unsupported(kCreate, "num_heads", "every stage must have the same number of heads");
        if (embed_dim % num_heads[i]) return unsupported(kCreate, "num_heads", "embed_dim is not a multiple of the number of heads");
    }
    if (up == "pixelshuffle" && !(upscale == 3 || is_pow2(upscale))) return unsupported(kCreate, "upscale", "pixelshuffle is built for 2^n and 3");
    if (up == "nearest+conv" && upscale != 4) return unsupported(kCreate, "upscale", "nearest+conv is built for 4 only");
    if (up == "pixelshuffledirect" && upscale * upscale * num_channels_out > 1024) return unsupported(kCreate, "upscale", "too large");

    nesr_swin2sr* c = new nesr_swin2sr();
    c->device = device_id, c->nin = num_channels, c->nout = num_channels_out, c->C = embed_dim, c->cs = round_up(embed_dim, 16), c->nst = num_stages;
    c->ws = window_size, c->hidden = (int)(mlp_ratio * embed_dim), c->hidp = round_up(std::max(c->hidden, 1), 16), c->heads = num_heads[0];
    c->d = embed_dim / c->heads, c->dp = round_up(c->d, 16), c->scale = upscale;
    c->up = up == "pixelshuffle" ? UP_PIXELSHUFFLE : (up == "pixelshuffledirect" ? UP_DIRECT : UP_NEAREST);
    c->eps = (float)layer_norm_eps, c->range = (float)img_range;
    for (int i = 0; i < num_stages; ++i) c->depth[i] = depths[i];
    if (num_channels == 3 && num_channels_out == 3)
        for (int i = 0; i < 3; ++i) c->mean[i] = kMean[i];
    {   // what the kernels keep in LDS
        S2Attn a = attn_shape(c);
        S2Rows r;
        memset(&r, 0, sizeof(r));
        r.cs = c->cs, r.n1p = c->hidp, r.w1 = reinterpret_cast<const float*>(1);
        S2Conv v;
        memset(&v, 0, sizeof(v));
        v.cinp = round_up(embed_dim, 4);
        if (c->hidden < 1 || s2_attn_lds_bytes(a) > S2_LDS_LIMIT || s2_rows_lds_bytes(r) > S2_LDS_LIMIT || s2_conv_lds_bytes(v) > S2_LDS_LIMIT) {
            delete c;
            return unsupported(kCreate, "window_size / embed_dim / mlp_ratio", "a window's tokens, a head's q, k, v and its scores (or 32 rows of the MLP) do not fit the 160 KiB of LDS");
        }
    }
    if (const int rc = check_device(device_id, NESR_SWIN2SR_NO_DEVICE)) {
        delete c;
        return rc;
    }
    StateDict& sd = c->sd;
    const int64_t C = c->C, hid = c->hidden, nf = kFeatures;
    sd.expect_wb("swin2sr.first_convolution", {C, c->nin, 3, 3});
    sd.expect_wb("swin2sr.embeddings.patch_embeddings.projection", {C, C, 1, 1});
    sd.expect_wb("swin2sr.embeddings.patch_embeddings.layernorm", {C});
    for (int i = 0; i < c->nst; ++i) {
        const std::string s = "swin2sr.encoder.stages." + std::to_string(i);
        for (int j = 0; j < c->depth[i]; ++j) {
            const std::string l = s + ".layers." + std::to_string(j), a = l + ".attention.self";
            sd.expect(a + ".logit_scale", {c->heads, 1, 1});
            sd.expect_wb(a + ".continuous_position_bias_mlp.0", {512, 2});
            sd.expect_wb(a + ".continuous_position_bias_mlp.2", {c->heads, 512}, false);
            sd.expect_wb(a + ".query", {C, C});
            sd.expect_wb(a + ".key", {C, C}, false);
            sd.expect_wb(a + ".value", {C, C});
            sd.expect_wb(l + ".attention.output.dense", {C, C});
            sd.expect_wb(l + ".layernorm_before", {C});
            sd.expect_wb(l + ".intermediate.dense", {hid, C});
            sd.expect_wb(l + ".output.dense", {C, hid});
            sd.expect_wb(l + ".layernorm_after", {C});
        }
        sd.expect_wb(s + ".conv", {C, C, 3, 3});
        sd.expect_wb(s + ".patch_embed.projection", {C, C, 1, 1});
    }
    sd.expect_wb("swin2sr.layernorm", {C});
    sd.expect_wb("swin2sr.conv_after_body", {C, C, 3, 3});
    if (c->up == UP_DIRECT) {
        sd.expect_wb("upsample.conv", {(int64_t)upscale * upscale * c->nout, C, 3, 3});
    } else {
        sd.expect_wb("upsample.conv_before_upsample", {nf, C, 3, 3});
        if (c->up == UP_PIXELSHUFFLE) {
            if (upscale == 3) {
                sd.expect_wb("upsample.upsample.convolution", {9 * nf, nf, 3, 3});
            } else {
                for (int i = 0; (1 << i) < upscale; ++i) sd.expect_wb("upsample.upsample.convolution_" + std::to_string(i), {4 * nf, nf, 3, 3});
            }
        } else {
            for (const char* n : {"conv_up1", "conv_up2", "conv_hr"}) sd.expect_wb(std::string("upsample.") + n, {nf, nf, 3, 3});
        }
        sd.expect_wb("upsample.final_convolution", {c->nout, nf, 3, 3});
    }
    *out = c;
    return NESR_OK;
}

void nesr_swin2sr_destroy(nesr_swin2sr* c) { net_destroy(c); }

int nesr_swin2sr_set_dtype(nesr_swin2sr* c, int dtype) {
    if (dtype == NESR_DTYPE_BF16)
        return set_error(NESR_ERR_UNSUPPORTED, "nesr_swin2sr_set_dtype: bf16 is not a form of Swin2SR: cosine attention multiplies a product of unit vectors by a "
                                               "temperature of up to 100, and bf16's 8 significand bits cost 0.2 to 0.4 in the logits; NESR_DTYPE_F16 is the 16-bit form");
    if (dtype != NESR_DTYPE_F32 && dtype != NESR_DTYPE_F16)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_set_dtype: dtype must be NESR_DTYPE_F32 or NESR_DTYPE_F16, got " + std::to_string(dtype));
    if (!c) return set_error(NESR_ERR_ARG, "nesr_swin2sr_set_dtype: null context");
    if (c->packed) return set_error(NESR_ERR_STATE, "nesr_swin2sr_set_dtype: the compute form is chosen between nesr_swin2sr_create and nesr_swin2sr_finalize");
    c->dtype = dtype;
    return NESR_OK;
}

int nesr_swin2sr_num_tensors(const nesr_swin2sr* c) { return net_num_tensors(c); }

int nesr_swin2sr_load_weight(nesr_swin2sr* c, const char* key, const float* data, const int64_t* shape, int ndim) {
    // buffers older checkpoints carry: recomputed here from the configuration
    return net_load_weight(c, "nesr_swin2sr_load_weight", key, data, shape, ndim, [](std::string& k) {
        return !(ends_with(k, "relative_position_index") || ends_with(k, "relative_coords_table") || ends_with(k, "attn_mask"));
    });
}

int nesr_swin2sr_finalize(nesr_swin2sr* c) {
    if (const int rc = net_begin_finalize(c, "nesr_swin2sr_finalize")) return rc;
    const StateDict& sd = c->sd;

    HostPack pk;
    auto vec = [&](const std::string& key, int padded) { return pk.vec(sd.data(key), padded); };
    // The fp16 form's second copy of a GEMM weight: hh[at + o * kp + kk] = f16(w[o][kk]), rows and columns zero padded; a lane's
    // fragment (8 k of one output) is one 16-byte load.  A value f16 cannot carry is remembered by its key.
    const bool f16 = c->dtype == NESR_DTYPE_F16;
    HalfPack hp;
    std::vector<_Float16>& hh = hp.half;
    // a Linear / 1x1 conv `name`: Wt and the bias into pk (their offsets to w and b) and, in the fp16 form, the second copy (to h)
    auto linear = [&](const std::string& name, int n, int k, size_t& w, size_t& b, size_t& h) {
        const LinW l = pk.linear(sd, name, n, k);
        w = l.w, b = l.b;
        if (f16) {
            const std::string key = name + ".weight";
            const std::vector<float>& v = sd.data(key);
            h = hp.reserve((size_t)l.np * l.kp);
            for (int o = 0; o < n; ++o)
                for (int kk = 0; kk < k; ++kk) hh[h + (size_t)o * l.kp + kk] = hp.put(key, v[(size_t)o * k + kk]);
        }
    };
    // conv weight [n][cin][3][3] -> Wt[(tap * cinp + ci)][coutp]
    auto conv = [&](const std::string& name, int n, int cin) {
        S2ConvW r;
        r.cin = cin, r.cinp = round_up(cin, 4), r.cout = n, r.coutp = round_up(n, 16);
        r.w = pk.conv_taps(sd.data(name + ".weight"), n, cin, 9, r.cinp, r.coutp);
        r.b = vec(name + ".bias", r.coutp);
        if (f16 && cin > 4) {      // [tap][coutp][cin rounded up to 16]
            const int c16 = round_up(cin, 16);
            const std::string wkey = name + ".weight";
            const std::vector<float>& w = sd.data(wkey);
            r.wh = hp.reserve((size_t)9 * r.coutp * c16);
            for (int o = 0; o < n; ++o)
                for (int ci = 0; ci < cin; ++ci)
                    for (int t = 0; t < 9; ++t) hh[r.wh + ((size_t)t * r.coutp + o) * c16 + ci] = hp.put(wkey, w[((size_t)o * cin + ci) * 9 + t]);
        }
        return r;
    };
    const int C = c->C, CS = c->cs, ws = c->ws, n = ws * ws, heads = c->heads, d = c->d, dp = c->dp;

    // the log-spaced coordinate table (float32 as transformers makes it) and the relative position index
    const int tw = 2 * ws - 1;
    std::vector<float> table((size_t)tw * tw * 2);
    auto log_coord = [&](int r) {
        float v = (float)r;
        if (ws > 1) v = v / (float)(ws - 1);
        v *= 8.0f;
        const float mag = (float)std::log2((double)(std::fabs(v) + 1.0f)) / 3.0f;
        return v > 0 ? mag : (v < 0 ? -mag : 0.0f);
    };
    for (int i = 0; i < tw; ++i)
        for (int j = 0; j < tw; ++j) table[((size_t)i * tw + j) * 2] = log_coord(i - (ws - 1)), table[((size_t)i * tw + j) * 2 + 1] = log_coord(j - (ws - 1));

    c->first = conv("swin2sr.first_convolution", C, c->nin);
    const std::string pe = "swin2sr.embeddings.patch_embeddings";
    linear(pe + ".projection", C, C, c->wpe, c->bpe, c->wpeh);
    c->peg = vec(pe + ".layernorm.weight", CS);
    c->peb = vec(pe + ".layernorm.bias", CS);
    c->stages.assign(c->nst, S2StageW());
    for (int i = 0; i < c->nst; ++i) {
        S2StageW& S = c->stages[i];
        const std::string s = "swin2sr.encoder.stages." + std::to_string(i);
        S.layers.assign(c->depth[i], S2LayerW());
        for (int j = 0; j < c->depth[i]; ++j) {
            S2LayerW& L = S.layers[j];
            const std::string l = s + ".layers." + std::to_string(j), a = l + ".attention.self";
            const int nq = heads * 3 * dp;
            L.wqkv = pk.reserve((size_t)CS * nq);
            L.bqkv = pk.reserve(nq);
            if (f16) L.wqkvh = hp.reserve((size_t)nq * CS);
            const char* parts[3] = {".query", ".key", ".value"};
            for (int p = 0; p < 3; ++p) {
                const std::string wkey = a + parts[p] + ".weight";
                const std::vector<float>& w = sd.data(wkey);
                const std::vector<float>* b = p == 1 ? nullptr : &sd.data(a + parts[p] + ".bias");
                for (int h = 0; h < heads; ++h)
                    for (int jd = 0; jd < d; ++jd) {
                        const int row = h * d + jd, col = (h * 3 + p) * dp + jd;
                        for (int k = 0; k < C; ++k) pk.host[L.wqkv + (size_t)k * nq + col] = w[(size_t)row * C + k];
                        for (int k = 0; f16 && k < C; ++k) hh[L.wqkvh + (size_t)col * CS + k] = hp.put(wkey, w[(size_t)row * C + k]);
                        if (b) pk.host[L.bqkv + col] = (*b)[row];
                    }
            }
            L.scale = pk.reserve(heads);
            {
                const std::vector<float>& ls = sd.data(a + ".logit_scale");
                for (int h = 0; h < heads; ++h) pk.host[L.scale + h] = (float)std::exp(std::min((double)ls[h], std::log(1.0 / 0.01)));
            }
            {   // 16 sigmoid(MLP(table))[index], double on the host, rounded once
                const std::vector<float>&w0 = sd.data(a + ".continuous_position_bias_mlp.0.weight"), &b0 = sd.data(a + ".continuous_position_bias_mlp.0.bias"),
                                  &w2 = sd.data(a + ".continuous_position_bias_mlp.2.weight");
                std::vector<double> tb((size_t)tw * tw * heads, 0.0);
                for (int e = 0; e < tw * tw; ++e)
                    for (int u = 0; u < 512; ++u) {
                        const double hv = (double)w0[u * 2] * table[(size_t)e * 2] + (double)w0[u * 2 + 1] * table[(size_t)e * 2 + 1] + (double)b0[u];
                        if (hv > 0)
                            for (int h = 0; h < heads; ++h) tb[(size_t)e * heads + h] += hv * (double)w2[(size_t)h * 512 + u];
                    }
                L.bias = pk.reserve((size_t)heads * n * n);
                for (int h = 0; h < heads; ++h)
                    for (int p = 0; p < n; ++p)
                        for (int q = 0; q < n; ++q) {
                            const int idx = (p / ws - q / ws + ws - 1) * tw + (p % ws - q % ws + ws - 1);
                            pk.host[L.bias + ((size_t)h * n + p) * n + q] = (float)(16.0 / (1.0 + std::exp(-tb[(size_t)idx * heads + h])));
                        }
            }
            linear(l + ".attention.output.dense", C, C, L.wo, L.bo, L.woh);
            L.ln1g = vec(l + ".layernorm_before.weight", CS);
            L.ln1b = vec(l + ".layernorm_before.bias", CS);
            linear(l + ".intermediate.dense", c->hidden, C, L.w1, L.b1, L.w1h);
            linear(l + ".output.dense", C, c->hidden, L.w2, L.b2, L.w2h);
            L.ln2g = vec(l + ".layernorm_after.weight", CS);
            L.ln2b = vec(l + ".layernorm_after.bias", CS);
        }
        S.conv = conv(s + ".conv", C, C);
        linear(s + ".patch_embed.projection", C, C, S.wproj, S.bproj, S.wprojh);
    }
    c->lng = vec("swin2sr.layernorm.weight", CS);
    c->lnb = vec("swin2sr.layernorm.bias", CS);
    c->after = conv("swin2sr.conv_after_body", C, C);
    c->ups.clear();
    if (c->up == UP_DIRECT) {
        c->direct = conv("upsample.conv", c->scale * c->scale * c->nout, C);
    } else {
        c->before = conv("upsample.conv_before_upsample", kFeatures, C);
        if (c->up == UP_PIXELSHUFFLE) {
            if (c->scale == 3) {
                c->ups.push_back(conv("upsample.upsample.convolution", 9 * kFeatures, kFeatures));
            } else {
                for (int i = 0; (1 << i) < c->scale; ++i) c->ups.push_back(conv("upsample.upsample.convolution_" + std::to_string(i), 4 * kFeatures, kFeatures));
            }
        } else {
            c->up1 = conv("upsample.conv_up1", kFeatures, kFeatures);
            c->up2 = conv("upsample.conv_up2", kFeatures, kFeatures);
            c->hr = conv("upsample.conv_hr", kFeatures, kFeatures);
        }
        c->fin = conv("upsample.final_convolution", c->nout, kFeatures);
    }
    return net_upload(c, "nesr_swin2sr_finalize", pk, &hp, kName);
}

int nesr_swin2sr_output_size(int upscale, int H, int W, int* out_h, int* out_w) {
    if (!out_h || !out_w) return set_error(NESR_ERR_ARG, "nesr_swin2sr_output_size: null pointer");
    if (upscale < 1 || upscale > 8) return set_error(NESR_ERR_ARG, "nesr_swin2sr_output_size: upscale must be 1 .. 8");
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 24)) return set_error(NESR_ERR_ARG, "nesr_swin2sr_output_size: a frame of 1 .. 2^24 pixels");
    *out_h = H * upscale, *out_w = W * upscale;
    return NESR_OK;
}

int nesr_swin2sr_forward_f32(nesr_swin2sr* c, const float* x, int N, int C, int H, int W, float* out, size_t capacity, void* stream) {
    if (!c || !x || !out) return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_f32: null pointer");
    if (!c->finalized) return set_error(NESR_ERR_STATE, "nesr_swin2sr_forward_f32: weights not finalized (nesr_swin2sr_finalize)");
    if (N != 1 || C != c->nin) return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_f32: expected [1, " + std::to_string(c->nin) + ", H, W]");
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 24)) return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_f32: a frame of 1 .. 2^24 pixels");
    if (H % c->ws || W % c->ws)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_f32: H and W must be multiples of window_size " + std::to_string(c->ws) + ", got " + std::to_string(H) +
                                           " x " + std::to_string(W) + " (nesr_swin2sr_upscale_u8 pads a frame as the image processor does)");
    const size_t need = (size_t)c->nout * H * c->scale * W * c->scale;
    if (capacity < need) return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_f32: the output needs " + std::to_string(need) + " floats, capacity is " + std::to_string(capacity));
    NESR_TRY(hipSetDevice(c->device));
    return forward(c, x, false, H, W, out, false, static_cast<hipStream_t>(stream));
}

int nesr_swin2sr_upscale_u8(nesr_swin2sr* c, const uint8_t* rgb, int H, int W, uint8_t* out, size_t capacity, void* stream) {
    if (!c || !rgb || !out) return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_u8: null pointer");
    if (!c->finalized) return set_error(NESR_ERR_STATE, "nesr_swin2sr_upscale_u8: weights not finalized (nesr_swin2sr_finalize)");
    if (c->nin != 3 || c->nout != 3) return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_u8: an RGB frame needs num_channels = num_channels_out = 3");
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 24)) return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_u8: a frame of 1 .. 2^24 pixels");
    const size_t need = (size_t)3 * H * c->scale * W * c->scale;
    if (capacity < need) return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_u8: the output needs " + std::to_string(need) + " bytes, capacity is " + std::to_string(capacity));
    NESR_TRY(hipSetDevice(c->device));
    return forward(c, rgb, true, H, W, out, true, static_cast<hipStream_t>(stream));
}

int nesr_swin2sr_forward_batch_f32(nesr_swin2sr* c, const float* x, int N, int C, int H, int W, float* out, size_t capacity, void* stream) {
    if (!c || !x || !out) return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_batch_f32: null pointer");
    if (!c->finalized) return set_error(NESR_ERR_STATE, "nesr_swin2sr_forward_batch_f32: weights not finalized (nesr_swin2sr_finalize)");
    if (N < 1 || N > 65535 || C != c->nin)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_batch_f32: expected [N, " + std::to_string(c->nin) + ", H, W] with N in 1 .. 65535, got N = " +
                                           std::to_string(N) + ", C = " + std::to_string(C));
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 24)) return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_batch_f32: images of 1 .. 2^24 pixels");
    if (H % c->ws || W % c->ws)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_batch_f32: H and W must be multiples of window_size " + std::to_string(c->ws) + ", got " +
                                           std::to_string(H) + " x " + std::to_string(W));
    if ((long long)N * H * W > S2_ROWS_MAX)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_batch_f32: N x H x W = " + std::to_string((long long)N * H * W) + " tokens do not fit one launch (2^31 - 33)");
    const size_t need = (size_t)N * c->nout * H * c->scale * W * c->scale;
    if (capacity < need)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_forward_batch_f32: the output needs " + std::to_string(need) + " floats, capacity is " + std::to_string(capacity));
    NESR_TRY(hipSetDevice(c->device));
    S2Batch bt;
    bt.B = N;
    return forward(c, x, false, H, W, out, false, static_cast<hipStream_t>(stream), bt);
}

int nesr_swin2sr_part_f32(nesr_swin2sr* c, int part, int stage, int layer, const float* in, int N, int H, int W, float* out, size_t capacity, void* stream) {
    if (!c || !in || !out) return set_error(NESR_ERR_ARG, "nesr_swin2sr_part_f32: null pointer");
    if (!c->finalized) return set_error(NESR_ERR_STATE, "nesr_swin2sr_part_f32: weights not finalized (nesr_swin2sr_finalize)");
    if (part != NESR_S2_PART_ATTENTION && part != NESR_S2_PART_MLP && part != NESR_S2_PART_STAGE_CONV)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_part_f32: part must be one of NESR_S2_PART_*, got " + std::to_string(part));
    if (stage < 0 || stage >= c->nst) return set_error(NESR_ERR_ARG, "nesr_swin2sr_part_f32: stage must be 0 .. " + std::to_string(c->nst - 1));
    if (part != NESR_S2_PART_STAGE_CONV && (layer < 0 || layer >= c->depth[stage]))
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_part_f32: layer must be 0 .. " + std::to_string(c->depth[stage] - 1));
    if (N < 1 || N > 65535 || H < 1 || W < 1 || (long long)H * W > (1ll << 24) || (long long)N * H * W > S2_ROWS_MAX)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_part_f32: tokens [N][H W][C] with N in 1 .. 65535, H W in 1 .. 2^24 and N H W below 2^31 - 33");
    if (H % c->ws || W % c->ws)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_part_f32: H and W must be multiples of window_size " + std::to_string(c->ws) + ", got " + std::to_string(H) +
                                           " x " + std::to_string(W));
    const size_t rows = (size_t)N * H * W, need = rows * c->C;
    if (capacity < need) return set_error(NESR_ERR_ARG, "nesr_swin2sr_part_f32: the output needs " + std::to_string(need) + " floats, capacity is " + std::to_string(capacity));
    NESR_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    size_t act, upb;
    int rc = grow(c->ws_buf, c->ws_bytes, workspace_bytes(c, H, W, N, act, upb), kName);
    if (rc) return rc;
    float* A = reinterpret_cast<float*>(c->ws_buf + 2 * act);
    float* B = reinterpret_cast<float*>(c->ws_buf + 3 * act);
    const size_t pitch = (size_t)c->cs * 4, dense = (size_t)c->C * 4;
    NESR_TRY(hipMemsetAsync(A, 0, rows * pitch, s));      // the columns past the real width are zero in every buffer
    NESR_TRY(hipMemcpy2DAsync(A, pitch, in, dense, dense, rows, hipMemcpyDeviceToDevice, s));
    rc = net_range_begin(c, s);
    if (rc) return rc;
    const S2StageW& S = c->stages[stage];
    if (part == NESR_S2_PART_ATTENTION) {
        const S2Attn a = attn_args(c, S.layers[layer], layer, A, B, N, H, W);
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_ATTENTION, s, [&] { return launch_s2_attn(a, s); });
    } else if (part == NESR_S2_PART_MLP) {
        S2Rows a = mlp_args(c, S.layers[layer], (int)rows, A);
        a.out = B;
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_MLP, s, [&] { return launch_s2_rows(a, s); });
    } else {
        S2Conv a = conv_args(c, S.conv, A, H, W, c->cs, B, c->cs);
        a.batch = N;
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_CONV, s, [&] { return launch_s2_conv(a, s); });
    }
    NESR_TRY(hipMemcpy2DAsync(out, dense, B, pitch, dense, rows, hipMemcpyDeviceToDevice, s));
    return range_end(c, s, "nesr_swin2sr_part_f32");
}

int nesr_swin2sr_tile_plan(int upscale, int H, int W, int tile, int tile_pad, int* tiles_y, int* tiles_x, int* win_h, int* win_w, int32_t* plan,
                           size_t capacity) {
    if (!tiles_y || !tiles_x || !win_h || !win_w) return set_error(NESR_ERR_ARG, "nesr_swin2sr_tile_plan: null pointer");
    if (upscale < 1 || upscale > 8) return set_error(NESR_ERR_ARG, "nesr_swin2sr_tile_plan: upscale must be 1 .. 8");
    if (H < 1 || W < 1 || (long long)H * W > NESR_SWIN2SR_TILED_MAX_PIXELS)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_tile_plan: a frame (H x W) of 1 .. 2^28 pixels");
    if (tile < 1 || tile > (1 << 24)) return set_error(NESR_ERR_ARG, "nesr_swin2sr_tile_plan: tile must be 1 .. 2^24, got " + std::to_string(tile));
    if (tile_pad < 0 || tile_pad > (1 << 24)) return set_error(NESR_ERR_ARG, "nesr_swin2sr_tile_plan: tile_pad must be 0 .. 2^24, got " + std::to_string(tile_pad));
    const int ny = (H + tile - 1) / tile, nx = (W + tile - 1) / tile;
    *tiles_y = ny, *tiles_x = nx, *win_h = s2_window_side(H, tile, tile_pad), *win_w = s2_window_side(W, tile, tile_pad);
    if (!plan) return NESR_OK;
    const size_t need = (size_t)ny * nx * 8;
    if (capacity < need)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_tile_plan: the plan needs " + std::to_string(need) + " integers, capacity is " + std::to_string(capacity));
    for (int ty = 0; ty < ny; ++ty)
        for (int tx = 0; tx < nx; ++tx) {
            int wy, wx, y0, y1, x0, x1;
            s2_tile_axis(H, tile, tile_pad, ty, wy, y0, y1);
            s2_tile_axis(W, tile, tile_pad, tx, wx, x0, x1);
            int32_t* r = plan + ((size_t)ty * nx + tx) * 8;
            r[0] = wy, r[1] = wx, r[2] = (y0 - wy) * upscale, r[3] = (x0 - wx) * upscale, r[4] = (y1 - y0) * upscale, r[5] = (x1 - x0) * upscale;
            r[6] = y0 * upscale, r[7] = x0 * upscale;
        }
    return NESR_OK;
}

int nesr_swin2sr_workspace_bytes(nesr_swin2sr* c, int win_h, int win_w, int batch, size_t* bytes) {
    if (!c || !bytes) return set_error(NESR_ERR_ARG, "nesr_swin2sr_workspace_bytes: null pointer");
    if (win_h < 1 || win_w < 1 || (long long)win_h * win_w > (1ll << 24)) return set_error(NESR_ERR_ARG, "nesr_swin2sr_workspace_bytes: a window (win_h x win_w) of 1 .. 2^24 pixels");
    if (batch < 1 || batch > 65535) return set_error(NESR_ERR_ARG, "nesr_swin2sr_workspace_bytes: batch must be 1 .. 65535, got " + std::to_string(batch));
    int mh, mw, H, W;
    const int rc = padded_size(c, true, win_h, win_w, mh, mw, H, W);
    if (rc) return rc;
    size_t act, upb;
    *bytes = workspace_bytes(c, H, W, batch, act, upb);
    return NESR_OK;
}

int nesr_swin2sr_upscale_tiled_u8(nesr_swin2sr* c, const uint8_t* rgb, int H, int W, int tile, int tile_pad, int max_batch, uint8_t* out, size_t capacity,
                                  void* stream) {
    if (!c || !rgb || !out) return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_tiled_u8: null pointer");
    if (!c->finalized) return set_error(NESR_ERR_STATE, "nesr_swin2sr_upscale_tiled_u8: weights not finalized (nesr_swin2sr_finalize)");
    if (c->nin != 3 || c->nout != 3) return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_tiled_u8: an RGB frame needs num_channels = num_channels_out = 3");
    if (H < 1 || W < 1 || (long long)H * W > NESR_SWIN2SR_TILED_MAX_PIXELS)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_tiled_u8: a frame (H x W) of 1 .. 2^28 pixels");
    if (tile < 1 || tile > (1 << 24)) return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_tiled_u8: tile must be 1 .. 2^24, got " + std::to_string(tile));
    if (tile_pad < 0 || tile_pad > (1 << 24))
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_tiled_u8: tile_pad must be 0 .. 2^24, got " + std::to_string(tile_pad));
    const size_t need = (size_t)3 * H * c->scale * W * c->scale;
    if (capacity < need)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_tiled_u8: the output needs " + std::to_string(need) + " bytes, capacity is " + std::to_string(capacity));
    const int sy = s2_window_side(H, tile, tile_pad), sx = s2_window_side(W, tile, tile_pad);
    if ((long long)sy * sx > (1ll << 24))
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_upscale_tiled_u8: tile + 2 tile_pad gives windows of " + std::to_string(sy) + " x " + std::to_string(sx) +
                                           ", more than 2^24 pixels");
    int mh, mw, HP, WP;
    int rc = padded_size(c, true, sy, sx, mh, mw, HP, WP);      // every window has this shape: the reflect limit holds for all or none
    if (rc) return rc;
    const long long ny = (H + tile - 1) / tile, nx = (W + tile - 1) / tile, n = ny * nx;
    // windows a batch: the caller's, or as many as the budget holds; one at least, and no more than a launch takes
    size_t act, upb;
    long long B = max_batch > 0 ? max_batch : std::max<long long>(1, (long long)(NESR_SWIN2SR_TILE_WORKSPACE_BYTES / workspace_bytes(c, HP, WP, 1, act, upb)));
    B = std::min(B, std::min<long long>(n, 65535));
    B = std::max<long long>(1, std::min(B, (long long)S2_ROWS_MAX / ((long long)HP * WP)));
    while (max_batch <= 0 && B > 1 && workspace_bytes(c, HP, WP, (size_t)B, act, upb) > NESR_SWIN2SR_TILE_WORKSPACE_BYTES) --B;
    NESR_TRY(hipSetDevice(c->device));
    S2Batch bt;
    bt.tile = tile, bt.tile_pad = tile_pad, bt.tiles_x = (int)nx, bt.FH = H, bt.FW = W;
    for (long long t0 = 0; t0 < n; t0 += B) {      // row-major, ceil(n / B) batches, the last one shorter
        bt.tile0 = (int)t0, bt.B = (int)std::min(B, n - t0);
        rc = forward(c, rgb, true, sy, sx, out, true, static_cast<hipStream_t>(stream), bt);
        if (rc) return rc;
    }
    return NESR_OK;
}

int nesr_swin2sr_overlap_plan(int upscale, int window_size, int H, int W, int tile, int tile_overlap, int* tiles_y, int* tiles_x, int* t, int* Hp, int* Wp,
                              int32_t* plan, size_t capacity) {
    if (!tiles_y || !tiles_x || !t || !Hp || !Wp) return set_error(NESR_ERR_ARG, "nesr_swin2sr_overlap_plan: null pointer");
    if (upscale < 1 || upscale > 8) return set_error(NESR_ERR_ARG, "nesr_swin2sr_overlap_plan: upscale must be 1 .. 8");
    S2OverlapPlan p;
    const int rc = overlap_plan("nesr_swin2sr_overlap_plan", window_size, H, W, tile, tile_overlap, p);
    if (rc) return rc;
    *tiles_y = p.ny, *tiles_x = p.nx, *t = p.t, *Hp = p.PH, *Wp = p.PW;
    if (!plan) return NESR_OK;
    const size_t need = (size_t)p.ny * p.nx * 4;
    if (capacity < need)
        return set_error(NESR_ERR_ARG, "nesr_swin2sr_overlap_plan: the plan needs " + std::to_string(need) + " integers, capacity is " + std::to_string(capacity));
    for (int ty = 0; ty < p.ny; ++ty)
        for (int tx = 0; tx < p.nx; ++tx) {
            int cnt, wy, wx, f, l;
            s2_overlap_axis(p.PH, p.t, p.step, ty, 0, cnt, wy, f, l);
            s2_overlap_axis(p.PW, p.t, p.step, tx, 0, cnt, wx, f, l);
            int32_t* r = plan + ((size_t)ty * p.nx + tx) * 4;
            r[0] = wy, r[1] = wx, r[2] = wy * upscale, r[3] = wx * upscale;
        }
    return NESR_OK;
}

int nesr_swin2sr_overlap_workspace_bytes(nesr_swin2sr* c, int H, int W, int tile, int tile_overlap, int batch, size_t* bytes) {
    if (!c || !bytes) return set_error(NESR_ERR_ARG, "nesr_swin2sr_overlap_workspace_bytes: null pointer");
    if (batch < 1 || batch > 65535) return set_error(NESR_ERR_ARG, "nesr_swin2sr_overlap_workspace_bytes: batch must be 1 .. 65535, got " + std::to_string(batch));
    S2OverlapPlan p;
    const int rc = overlap_plan("nesr_swin2sr_overlap_workspace_bytes", c->ws, H, W, tile, tile_overlap, p);
    if (rc) return rc;
    if ((long long)p.t * p.t > (1ll << 24)) return set_error(NESR_ERR_ARG, "nesr_swin2sr_overlap_workspace_bytes: a tile of at most 2^24 pixels");
    size_t act, upb;
    *bytes = workspace_bytes(c, p.t, p.t, batch, act, upb) + overlap_y_bytes(c, p, batch) + overlap_e_bytes(c, p);
    return NESR_OK;
}

int nesr_swin2sr_upscale_overlapped_u8(nesr_swin2sr* c, const uint8_t* rgb, int H, int W, int tile, int tile_overlap, int max_batch, uint8_t* out,
                                       size_t capacity, void* stream) {
    const char* const entry = "nesr_swin2sr_upscale_overlapped_u8";
    if (!c || !rgb || !out) return set_error(NESR_ERR_ARG, std::string(entry) + ": null pointer");
    if (!c->finalized) return set_error(NESR_ERR_STATE, std::string(entry) + ": weights not finalized (nesr_swin2sr_finalize)");
    if (c->nin != 3 || c->nout != 3) return set_error(NESR_ERR_ARG, std::string(entry) + ": an RGB frame needs num_channels = num_channels_out = 3");
    S2OverlapPlan p;
    int rc = overlap_plan(entry, c->ws, H, W, tile, tile_overlap, p);
    if (rc) return rc;
    if ((long long)p.t * p.t > (1ll << 24)) return set_error(NESR_ERR_ARG, std::string(entry) + ": a tile of at most 2^24 pixels");
    const size_t need = (size_t)3 * H * c->scale * W * c->scale;
    if (capacity < need)
        return set_error(NESR_ERR_ARG, std::string(entry) + ": the output needs " + std::to_string(need) + " bytes, capacity is " + std::to_string(capacity));
    // windows a batch: the caller's, or as many as keep the network's workspace and Y within the budget (E belongs to the frame);
    // one at least, and no more than a launch takes
    const long long n = (long long)p.ny * p.nx;
    size_t act, upb;
    auto per_batch = [&](long long b) { return workspace_bytes(c, p.t, p.t, (size_t)b, act, upb) + overlap_y_bytes(c, p, (size_t)b); };
    long long B = max_batch > 0 ? max_batch : std::max<long long>(1, (long long)(NESR_SWIN2SR_TILE_WORKSPACE_BYTES / per_batch(1)));
    B = std::min(B, std::min<long long>(n, 65535));
    B = std::max<long long>(1, std::min(B, (long long)S2_ROWS_MAX / ((long long)p.t * p.t)));
    while (max_batch <= 0 && B > 1 && per_batch(B) > NESR_SWIN2SR_TILE_WORKSPACE_BYTES) --B;
    NESR_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t net = workspace_bytes(c, p.t, p.t, (size_t)B, act, upb), yb = overlap_y_bytes(c, p, (size_t)B), eb = overlap_e_bytes(c, p);
    rc = grow(c->ws_buf, c->ws_bytes, net + yb + eb, kName);      // once: the forwards below find their part in place, E lives through them
    if (rc) return rc;
    S2Overlap o;
    memset(&o, 0, sizeof(o));
    o.PH = p.PH, o.PW = p.PW, o.t = p.t, o.step = p.step, o.up = c->scale, o.tiles_y = p.ny, o.tiles_x = p.nx;
    o.Y = reinterpret_cast<const float*>(c->ws_buf + net), o.E = reinterpret_cast<float*>(c->ws_buf + net + yb);
    o.out = out, o.oh = H * c->scale, o.ow = W * c->scale;
    NESR_TRY(hipMemsetAsync(o.E, 0, eb, s));
    rc = net_range_begin(c, s);
    if (rc) return rc;
    S2Batch bt;
    bt.tiles_x = p.nx, bt.FH = H, bt.FW = W, bt.ov_step = p.step, bt.PH = p.PH, bt.PW = p.PW;
    for (long long t0 = 0; t0 < n; t0 += B) {      // row-major, in order on the one stream: E sees the windows in ascending tile index
        bt.tile0 = (int)t0, bt.B = (int)std::min(B, n - t0);
        rc = forward_launches(c, rgb, true, p.t, p.t, const_cast<float*>(o.Y), false, s, bt);
        if (rc) return rc;
        o.tile0 = bt.tile0, o.batch = bt.B;
        NESR_RUN(c->timer, kName, NESR_S2_GROUP_UPSAMPLE, s, [&] { return launch_s2_overlap_add(o, s); });
    }
    NESR_RUN(c->timer, kName, NESR_S2_GROUP_UPSAMPLE, s, [&] { return launch_s2_overlap_finish(o, s); });
    return range_end(c, s, entry);
}

int nesr_swin2sr_set_timing(nesr_swin2sr* c, int enable) { return net_set_timing(c, "nesr_swin2sr_set_timing", enable); }

int nesr_swin2sr_kernel_time_ms(nesr_swin2sr* c, double* group_ms, int n_groups, int64_t* launches) {
    return net_kernel_time_ms(c, "nesr_swin2sr_kernel_time_ms", NESR_S2_GROUPS, group_ms, n_groups, launches);
}

}  // extern "C"
