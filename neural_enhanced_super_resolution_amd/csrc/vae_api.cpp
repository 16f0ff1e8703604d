// VAE decoder contexts (nesr_vae_*): the configuration check, strict weight loading, the padded and transposed upload, a
// workspace that grows with the frame, and the decode as a chain of launches of the kernels of vae.hip.  Stands behind diffusers'
// AutoencoderKL.decode as StableDiffusionUpscalePipeline calls it, and for nesr_vae_decode_latents_u8 the pipeline's division by the
// scaling factor in front of it and VaeImageProcessor's quantiser behind it.
#include <cmath>
#include <cstring>

#include "net_context.h"
#include "vae_api.h"

#include "sdx4_api.h"

using namespace nesr;

namespace {

// offsets in floats into the packed weights
struct VConvW {
    size_t w = 0, b = 0;
    int cin = 0, cinp = 0, cout = 0, coutp = 0;
};
struct VResW {
    NormW n1, n2;
    VConvW c1, c2;
    bool has_sc = false;
    LinW sc;
};
struct VUpW {
    std::vector<VResW> res;
    bool has_up = false;
    VConvW up;
};

constexpr int kMaxBlocks = 4, kMaxWidth = 512;
constexpr float kEps = 1e-6f;
const char* const kName = "VaeDecoder";
const char* const kCreate = "nesr_vae_create";

}  // namespace

struct nesr_vae : NetContext {
    int lat = 4, nout = 3, nb = 3, layers = 2, groups = 32;
    int width[kMaxBlocks];
    double scaling = 1.0;
    LinW pq;
    VConvW conv_in, conv_out;
    VResW mid0, mid1;
    NormW attn_norm, norm_out;
    LinW qkv, to_out;
    std::vector<VUpW> ups;
    char* tile_buf = nullptr;      // nesr_vae_decode_latents_tiled_u8: a window's latents and sample, the f32 frame
    size_t tile_bytes = 0;
};

namespace {

int top(const nesr_vae* c) { return c->width[c->nb - 1]; }

// the attention's legacy key names (diffusers' AttentionBlock) are the same tensors
std::string current_name(const std::string& key) {
    static const char* const pairs[][2] = {{".query.", ".to_q."}, {".key.", ".to_k."}, {".value.", ".to_v."}, {".proj_attn.", ".to_out.0."}};
    const std::string a = "decoder.mid_block.attentions.0";
    if (key.compare(0, a.size(), a) != 0) return key;
    for (const auto& p : pairs) {
        const size_t at = key.find(p[0], a.size());
        if (at == a.size()) return a + p[1] + key.substr(at + strlen(p[0]));
    }
    return key;
}

void expect_resnet(StateDict& sd, const std::string& r, int64_t cin, int64_t cout) {
    sd.expect_wb(r + ".norm1", {cin});
    sd.expect_wb(r + ".conv1", {cout, cin, 3, 3});
    sd.expect_wb(r + ".norm2", {cout});
    sd.expect_wb(r + ".conv2", {cout, cout, 3, 3});
    if (cin != cout) sd.expect_wb(r + ".conv_shortcut", {cout, cin, 1, 1});
}

// What a decode of h x w latents allocates: three activation buffers of the largest live tensor (the attention's q | k | v
// among them), the statistics' partial sums and one set of per-channel norms.
size_t workspace_bytes(const nesr_vae* c, int h, int w, size_t& act, size_t& part) {
    const size_t M = (size_t)h * w;
    size_t rows = M * 3 * round_up(top(c), 16), px = M;
    for (int i = c->nb - 1; i >= 0; --i) {
        rows = std::max(rows, px * round_up(c->width[i], 16));
        if (i > 0) px *= 4, rows = std::max(rows, px * round_up(c->width[i], 16));
    }
    act = align_up(rows * 4, 256);
    part = align_up(vae_stats_blocks(px) * kMaxWidth * 2 * sizeof(double), 256);
    return 3 * act + part + align_up(kMaxWidth * sizeof(VaeNorm), 256);
}

int check_latents(const nesr_vae* c, const char* entry, int h, int w) {
    if (h < 1 || w < 1 || (long long)h * w > NESR_VAE_MAX_TOKENS)
        return set_error(NESR_ERR_ARG, std::string(entry) + ": latents of 1 .. " + std::to_string(NESR_VAE_MAX_TOKENS) + " pixels (the attention's token limit), got " +
                                           std::to_string(h) + " x " + std::to_string(w));
    const long long s = 1ll << (c->nb - 1);
    if ((long long)h * s * w * s > VAE_MAX_PIXELS) return set_error(NESR_ERR_ARG, std::string(entry) + ": the output may not exceed 2^24 pixels");
    return NESR_OK;
}

int decode(nesr_vae* c, const float* z, float divisor, int h, int w, void* out, bool out_u8, hipStream_t s) {
    size_t act, part;
    int rc = grow(c->ws_buf, c->ws_bytes, workspace_bytes(c, h, w, act, part), kName);
    if (rc) return rc;
    float* cur = reinterpret_cast<float*>(c->ws_buf);
    float* t1 = reinterpret_cast<float*>(c->ws_buf + act);
    float* t2 = reinterpret_cast<float*>(c->ws_buf + 2 * act);
    double* partial = reinterpret_cast<double*>(c->ws_buf + 3 * act);
    VaeNorm* norm = reinterpret_cast<VaeNorm*>(c->ws_buf + 3 * act + part);
    const float* W = c->d_w;
    int H = h, Wd = w;

    auto stats = [&](const NormW& n, const float* in) -> int {
        VaeStats a;
        memset(&a, 0, sizeof(a));
        a.in = in, a.m = H * Wd, a.c = n.c, a.cs = round_up(n.c, 16), a.groups = c->groups, a.partial = partial;
        a.gamma = W + n.g, a.beta = W + n.b, a.eps = kEps, a.out = norm;
        NESR_RUN(c->timer, kName, NESR_VAE_GROUP_NORM, s, [&] { return launch_vae_stats_partial(a, s); });
        NESR_RUN(c->timer, kName, NESR_VAE_GROUP_NORM, s, [&] { return launch_vae_stats_finish(a, s); });
        return NESR_OK;
    };
    auto conv_args = [&](const VConvW& cw, const float* in, bool normed, float* o) {
        VaeConv a;
        memset(&a, 0, sizeof(a));
        a.in_mode = VAE_IN_ROWS, a.in = in, a.H = H, a.W = Wd, a.cin = cw.cin, a.cinp = cw.cinp, a.cs_in = round_up(cw.cin, 16);
        a.norm = normed ? norm : nullptr, a.w = W + cw.w, a.bias = W + cw.b, a.cout = cw.cout, a.coutp = cw.coutp;
        a.out_mode = VAE_OUT_ROWS, a.out = o, a.cs_out = cw.coutp;
        return a;
    };
    auto rows = [&](const LinW& l, const float* in, bool normed, const float* res, float* o) -> int {
        VaeRows a;
        memset(&a, 0, sizeof(a));
        a.m = H * Wd, a.cs_in = l.kp, a.np = l.np, a.in = in, a.norm = normed ? norm : nullptr, a.w = W + l.w, a.b = W + l.b, a.res = res, a.out = o;
        NESR_RUN(c->timer, kName, NESR_VAE_GROUP_PROJ, s, [&] { return launch_vae_rows(a, s); });
        return NESR_OK;
    };
    // cur -> cur: conv2(silu(norm2(conv1(silu(norm1(x)))))) + shortcut(x); the result replaces x in its own buffer
    auto resnet = [&](const VResW& r) -> int {
        if ((rc = stats(r.n1, cur))) return rc;
        {
            const VaeConv a = conv_args(r.c1, cur, true, t1);
            NESR_RUN(c->timer, kName, NESR_VAE_GROUP_CONV, s, [&] { return launch_vae_conv(a, s); });
        }
        if ((rc = stats(r.n2, t1))) return rc;
        if (r.has_sc && (rc = rows(r.sc, cur, false, nullptr, t2))) return rc;
        VaeConv a = conv_args(r.c2, t1, true, cur);
        a.res = r.has_sc ? t2 : cur, a.cs_res = r.c2.coutp;
        NESR_RUN(c->timer, kName, NESR_VAE_GROUP_CONV, s, [&] { return launch_vae_conv(a, s); });
        return NESR_OK;
    };

    {   // latents (/ scaling factor) as rows -> post_quant_conv -> conv_in
        VaeIn a;
        memset(&a, 0, sizeof(a));
        a.z = z, a.c = c->lat, a.m = H * Wd, a.divisor = divisor, a.out = t1;
        NESR_RUN(c->timer, kName, NESR_VAE_GROUP_PROJ, s, [&] { return launch_vae_in(a, s); });
        if ((rc = rows(c->pq, t1, false, nullptr, t2))) return rc;
        const VaeConv v = conv_args(c->conv_in, t2, false, cur);
        NESR_RUN(c->timer, kName, NESR_VAE_GROUP_CONV, s, [&] { return launch_vae_conv(v, s); });
    }
    if ((rc = resnet(c->mid0))) return rc;
    {   // x + to_out(softmax(q k^T / sqrt(C)) v) over the normalised tokens
        if ((rc = stats(c->attn_norm, cur))) return rc;
        if ((rc = rows(c->qkv, cur, true, nullptr, t1))) return rc;
        VaeAttn a;
        memset(&a, 0, sizeof(a));
        a.n = H * Wd, a.c = top(c), a.cs = round_up(top(c), 16), a.qkv = t1, a.out = t2;
        NESR_RUN(c->timer, kName, NESR_VAE_GROUP_ATTENTION, s, [&] { return launch_vae_attn(a, s); });
        if ((rc = rows(c->to_out, t2, false, cur, cur))) return rc;
    }
    if ((rc = resnet(c->mid1))) return rc;
    for (const VUpW& u : c->ups) {
        for (const VResW& r : u.res)
            if ((rc = resnet(r))) return rc;
        if (u.has_up) {
            H *= 2, Wd *= 2;
            VaeConv a = conv_args(u.up, cur, false, t1);
            a.in_mode = VAE_IN_NEAREST2;
            NESR_RUN(c->timer, kName, NESR_VAE_GROUP_UPSAMPLE, s, [&] { return launch_vae_conv(a, s); });
            std::swap(cur, t1);
        }
    }
    if ((rc = stats(c->norm_out, cur))) return rc;
    VaeConv a = conv_args(c->conv_out, cur, true, nullptr);
    a.out_mode = out_u8 ? VAE_OUT_U8 : VAE_OUT_F32, a.out = out, a.cs_out = 0;
    NESR_RUN(c->timer, kName, NESR_VAE_GROUP_CONV, s, [&] { return launch_vae_conv(a, s); });
    return NESR_OK;
}

int check_decode(const nesr_vae* c, const char* entry, const void* in, const void* out, int N, int C, int h, int w, size_t capacity, const char* unit) {
    const std::string e = entry;
    if (!c || !in || !out) return set_error(NESR_ERR_ARG, e + ": null pointer");
    if (!c->finalized) return set_error(NESR_ERR_STATE, e + ": weights not finalized (nesr_vae_finalize)");
    if (N != 1 || C != c->lat) return set_error(NESR_ERR_ARG, e + ": expected [1, " + std::to_string(c->lat) + ", h, w]");
    const int rc = check_latents(c, entry, h, w);
    if (rc) return rc;
    const size_t sc = (size_t)1 << (c->nb - 1), need = (size_t)c->nout * h * sc * w * sc;
    if (capacity < need) return set_error(NESR_ERR_ARG, e + ": the output needs " + std::to_string(need) + " " + unit + ", capacity is " + std::to_string(capacity));
    return NESR_OK;
}

}  // namespace

extern "C" {

int nesr_vae_create(nesr_vae** out, int device_id, int latent_channels, int out_channels, int num_blocks, const int* block_out_channels,
                    int layers_per_block, int norm_num_groups, double scaling_factor, const char* act_fn) {
    if (!out) return set_error(NESR_ERR_ARG, "nesr_vae_create: null out");
    *out = nullptr;
    if (!block_out_channels || !act_fn) return set_error(NESR_ERR_ARG, "nesr_vae_create: null configuration argument");
    if (num_blocks < 2 || num_blocks > kMaxBlocks) return unsupported(kCreate, "block_out_channels", "2 .. 4 entries, got " + std::to_string(num_blocks));
    if (norm_num_groups < 1) return unsupported(kCreate, "norm_num_groups", "must be positive");
    for (int i = 0; i < num_blocks; ++i) {
        const int wd = block_out_channels[i];
        if (wd < 1 || wd > kMaxWidth) return unsupported(kCreate, "block_out_channels", "every width must be 1 .. 512, got " + std::to_string(wd));
        if (wd % norm_num_groups) return unsupported(kCreate, "block_out_channels", std::to_string(wd) + " is no multiple of norm_num_groups " + std::to_string(norm_num_groups));
    }
    if (layers_per_block < 1 || layers_per_block > 4) return unsupported(kCreate, "layers_per_block", "1 .. 4, got " + std::to_string(layers_per_block));
    if (latent_channels < 1 || latent_channels > 8) return unsupported(kCreate, "latent_channels", "1 .. 8, got " + std::to_string(latent_channels));
    if (out_channels < 1 || out_channels > 4) return unsupported(kCreate, "out_channels", "1 .. 4, got " + std::to_string(out_channels));
    if (std::string(act_fn) != "silu") return unsupported(kCreate, "act_fn", "'" + std::string(act_fn) + "' is not supported (silu only)");
    if (!(scaling_factor > 0) || !std::isfinite(scaling_factor)) return unsupported(kCreate, "scaling_factor", "must be positive and finite");
    if (const int rc = check_device(device_id, NESR_VAE_NO_DEVICE)) return rc;
    nesr_vae* c = new nesr_vae();
    c->device = device_id, c->lat = latent_channels, c->nout = out_channels, c->nb = num_blocks, c->layers = layers_per_block;
    c->groups = norm_num_groups, c->scaling = scaling_factor;
    for (int i = 0; i < num_blocks; ++i) c->width[i] = block_out_channels[i];
    StateDict& sd = c->sd;
    const int64_t T = top(c), lat = c->lat;
    sd.expect_wb("post_quant_conv", {lat, lat, 1, 1});
    sd.expect_wb("decoder.conv_in", {T, lat, 3, 3});
    expect_resnet(sd, "decoder.mid_block.resnets.0", T, T);
    const std::string at = "decoder.mid_block.attentions.0";
    sd.expect_wb(at + ".group_norm", {T});
    for (const char* n : {".to_q", ".to_k", ".to_v", ".to_out.0"}) sd.expect_wb(at + n, {T, T});
    expect_resnet(sd, "decoder.mid_block.resnets.1", T, T);
    int64_t prev = T;
    for (int i = 0; i < c->nb; ++i) {
        const int64_t wd = c->width[c->nb - 1 - i];
        const std::string u = "decoder.up_blocks." + std::to_string(i);
        for (int j = 0; j <= c->layers; ++j) expect_resnet(sd, u + ".resnets." + std::to_string(j), j == 0 ? prev : wd, wd);
        if (i < c->nb - 1) sd.expect_wb(u + ".upsamplers.0.conv", {wd, wd, 3, 3});
        prev = wd;
    }
    sd.expect_wb("decoder.conv_norm_out", {prev});
    sd.expect_wb("decoder.conv_out", {c->nout, prev, 3, 3});
    *out = c;
    return NESR_OK;
}

void nesr_vae_destroy(nesr_vae* c) {
    if (c && c->tile_buf && c->device != NET_NO_DEVICE) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(c->tile_buf);
    }
    net_destroy(c);
}

int nesr_vae_num_tensors(const nesr_vae* c) { return net_num_tensors(c); }

int nesr_vae_load_weight(nesr_vae* c, const char* key, const float* data, const int64_t* shape, int ndim) {
    return net_load_weight(c, "nesr_vae_load_weight", key, data, shape, ndim, [](std::string& k) {
        k = current_name(k);
        return true;
    });
}

int nesr_vae_finalize(nesr_vae* c) {
    if (const int rc = net_begin_finalize(c, "nesr_vae_finalize")) return rc;
    const StateDict& sd = c->sd;
    HostPack pk;
    auto conv = [&](const std::string& name, int n, int cin) {
        VConvW r;
        r.cin = cin, r.cinp = round_up(cin, 4), r.cout = n, r.coutp = round_up(n, 16);
        r.w = pk.conv_taps(sd.data(name + ".weight"), n, cin, 9, r.cinp, r.coutp);
        r.b = pk.vec(sd.data(name + ".bias"), r.coutp);
        return r;
    };
    auto resnet = [&](const std::string& r, int cin, int cout) {
        VResW w;
        w.n1 = pk.norm(sd, r + ".norm1", cin), w.c1 = conv(r + ".conv1", cout, cin), w.n2 = pk.norm(sd, r + ".norm2", cout), w.c2 = conv(r + ".conv2", cout, cout);
        w.has_sc = cin != cout;
        if (w.has_sc) w.sc = pk.linear(sd, r + ".conv_shortcut", cout, cin);
        return w;
    };
    const int T = top(c);
    c->pq = pk.linear(sd, "post_quant_conv", c->lat, c->lat);
    c->conv_in = conv("decoder.conv_in", T, c->lat);
    c->mid0 = resnet("decoder.mid_block.resnets.0", T, T);
    const std::string at = "decoder.mid_block.attentions.0";
    c->attn_norm = pk.norm(sd, at + ".group_norm", T);
    c->qkv = pk.side_by_side(sd, at, {".to_q", ".to_k", ".to_v"}, T, T);      // Wt[cs][3 cs]
    c->to_out = pk.linear(sd, at + ".to_out.0", T, T);
    c->mid1 = resnet("decoder.mid_block.resnets.1", T, T);
    c->ups.assign(c->nb, VUpW());
    int prev = T;
    for (int i = 0; i < c->nb; ++i) {
        const int wd = c->width[c->nb - 1 - i];
        const std::string u = "decoder.up_blocks." + std::to_string(i);
        for (int j = 0; j <= c->layers; ++j) c->ups[i].res.push_back(resnet(u + ".resnets." + std::to_string(j), j == 0 ? prev : wd, wd));
        c->ups[i].has_up = i < c->nb - 1;
        if (c->ups[i].has_up) c->ups[i].up = conv(u + ".upsamplers.0.conv", wd, wd);
        prev = wd;
    }
    c->norm_out = pk.norm(sd, "decoder.conv_norm_out", prev);
    c->conv_out = conv("decoder.conv_out", c->nout, prev);
    return net_upload(c, "nesr_vae_finalize", pk, nullptr, kName);
}

int nesr_vae_output_size(int num_blocks, int h, int w, int* out_h, int* out_w) {
    if (!out_h || !out_w) return set_error(NESR_ERR_ARG, "nesr_vae_output_size: null pointer");
    if (num_blocks < 2 || num_blocks > kMaxBlocks) return set_error(NESR_ERR_ARG, "nesr_vae_output_size: block_out_channels has 2 .. 4 entries");
    const long long s = 1ll << (num_blocks - 1);
    if (h < 1 || w < 1 || (long long)h * w > NESR_VAE_MAX_TOKENS || (long long)h * s * w * s > VAE_MAX_PIXELS)
        return set_error(NESR_ERR_ARG, "nesr_vae_output_size: latents of 1 .. 65536 pixels (the attention's token limit) and an output of at most 2^24 pixels");
    *out_h = (int)(h * s), *out_w = (int)(w * s);
    return NESR_OK;
}

int nesr_vae_workspace_bytes(nesr_vae* c, int h, int w, size_t* bytes) {
    if (!c || !bytes) return set_error(NESR_ERR_ARG, "nesr_vae_workspace_bytes: null pointer");
    const int rc = check_latents(c, "nesr_vae_workspace_bytes", h, w);
    if (rc) return rc;
    size_t act, part;
    *bytes = workspace_bytes(c, h, w, act, part);
    return NESR_OK;
}

int nesr_vae_decode_f32(nesr_vae* c, const float* z, int N, int C, int h, int w, float* out, size_t capacity, void* stream) {
    const int rc = check_decode(c, "nesr_vae_decode_f32", z, out, N, C, h, w, capacity, "floats");
    if (rc) return rc;
    NESR_TRY(hipSetDevice(c->device));
    return decode(c, z, 1.0f, h, w, out, false, static_cast<hipStream_t>(stream));
}

int nesr_vae_decode_latents_u8(nesr_vae* c, const float* latents, int N, int C, int h, int w, uint8_t* out, size_t capacity, void* stream) {
    if (c && c->nout != 3) return set_error(NESR_ERR_ARG, "nesr_vae_decode_latents_u8: an RGB frame needs out_channels = 3");
    const int rc = check_decode(c, "nesr_vae_decode_latents_u8", latents, out, N, C, h, w, capacity, "bytes");
    if (rc) return rc;
    NESR_TRY(hipSetDevice(c->device));
    return decode(c, latents, (float)c->scaling, h, w, out, true, static_cast<hipStream_t>(stream));
}

int nesr_vae_decode_latents_tiled_u8(nesr_vae* c, const float* latents, int N, int C, int h, int w, int tile, int tile_overlap, uint8_t* out, size_t capacity, void* stream) {
    const std::string e = "nesr_vae_decode_latents_tiled_u8";
    if (!c || !latents || !out) return set_error(NESR_ERR_ARG, e + ": null pointer");
    if (c->nout != 3) return set_error(NESR_ERR_ARG, e + ": an RGB frame needs out_channels = 3");
    if (!c->finalized) return set_error(NESR_ERR_STATE, e + ": weights not finalized (nesr_vae_finalize)");
    if (N != 1 || C != c->lat) return set_error(NESR_ERR_ARG, e + ": expected [1, " + std::to_string(c->lat) + ", h, w]");
    if (h < 2 || w < 2 || h % 2 || w % 2 || (long long)h * w > SDX4_MAX_FRAME_PIXELS)
        return set_error(NESR_ERR_ARG, e + ": h and w must be positive multiples of 2 and h w at most 2^22, got " + std::to_string(h) + " x " + std::to_string(w));
    int ty = 0, tx = 0;
    const int rc = sdx4_check_windows(e.c_str(), "tile", h, w, 2, tile, tile_overlap, &ty, &tx);
    if (rc) return rc;
    const size_t sc = (size_t)1 << (c->nb - 1), need = 3 * h * sc * w * sc;
    if (capacity < need) return set_error(NESR_ERR_ARG, e + ": the output needs " + std::to_string(need) + " bytes, capacity is " + std::to_string(capacity));
    if ((reinterpret_cast<uintptr_t>(latents) & 7) || (reinterpret_cast<uintptr_t>(out) & 3))
        return set_error(NESR_ERR_ARG, e + ": the latents pointer must be 8-byte aligned, the output 4-byte");
    NESR_TRY(hipSetDevice(c->device));
    const int grc = grow(c->tile_buf, c->tile_bytes, sdx4_vae_tiled_plan(c->lat, (int)sc, h, w, ty, tx).total, kName);
    if (grc) return grc;
    return sdx4_vae_decode_tiled(c, latents, h, w, ty, tx, tile_overlap, c->tile_buf, out, nullptr, kName, Sdx4TileGroups{0, 0, 0}, static_cast<hipStream_t>(stream));
}

int nesr_vae_set_timing(nesr_vae* c, int enable) { return net_set_timing(c, "nesr_vae_set_timing", enable); }

int nesr_vae_kernel_time_ms(nesr_vae* c, double* group_ms, int n_groups, int64_t* launches) {
    return net_kernel_time_ms(c, "nesr_vae_kernel_time_ms", NESR_VAE_GROUPS, group_ms, n_groups, launches);
}

}  // extern "C"

// what the x4 pipeline (sdx4_api.cpp) asks of a context it does not own
nesr::Sdx4VaeInfo nesr::sdx4_vae_info(const nesr_vae* c) {
    return Sdx4VaeInfo{c->device, c->lat, c->nout, c->nb, c->finalized, c->timer.launches};
}

// The decode over windows (sdx4_api.h): shared by nesr_vae_decode_latents_tiled_u8 above and nesr_sdx4_upscale_tiled_u8, which
// brings its own buffer and timer.
nesr::Sdx4VaeTiledPlan nesr::sdx4_vae_tiled_plan(int lc, int scale, int h, int w, int ty, int tx) {
    Sdx4VaeTiledPlan pl;
    ScratchCarver ws;
    const size_t sc = (size_t)scale;
    pl.window = ws.take((size_t)lc * ty * tx * 4);
    pl.sample = ws.take(3 * ty * sc * tx * sc * 4);
    pl.acc = ws.take(3 * h * sc * w * sc * 4);
    pl.total = ws.total();
    return pl;
}

int nesr::sdx4_vae_decode_tiled(nesr_vae* c, const float* latents, int h, int w, int ty, int tx, int r, char* buf, uint8_t* out, GroupTimer* timer, const char* model,
                                Sdx4TileGroups groups, hipStream_t s) {
    const int sc = 1 << (c->nb - 1);
    const Sdx4VaeTiledPlan pl = sdx4_vae_tiled_plan(c->lat, sc, h, w, ty, tx);
    float* window = reinterpret_cast<float*>(buf + pl.window);
    float* sample = reinterpret_cast<float*>(buf + pl.sample);
    float* acc = reinterpret_cast<float*>(buf + pl.acc);
    {   // the decode's own workspace has its size before the first launch
        size_t act, part;
        const int rc = grow(c->ws_buf, c->ws_bytes, workspace_bytes(c, ty, tx, act, part), kName);
        if (rc) return rc;
    }
    // one window kernel: through the caller's timer, or as it is
    auto run = [&](int group, auto&& launch) -> int {
        if (timer) return timer->run(model, group, s, launch);
        const hipError_t e = launch();
        return e == hipSuccess ? NESR_OK : set_error(NESR_ERR_HIP, std::string(model) + " launch (window kernel): " + hipGetErrorString(e));
    };
    int rc;
    NESR_TRY(hipMemsetAsync(acc, 0, (size_t)3 * h * sc * w * sc * 4, s));
    const int ky = sdx4_axis_windows(h, ty, r), kx = sdx4_axis_windows(w, tx, r);
    for (int iy = 0; iy < ky; ++iy)
        for (int ix = 0; ix < kx; ++ix) {
            const int ay = sdx4_axis_origin(h, ty, r, iy), ax = sdx4_axis_origin(w, tx, r, ix);
            Sdx4Gather g;
            memset(&g, 0, sizeof(g));
            g.src = latents, g.n = 1, g.channels = c->lat, g.y = sdx4_axis(h, ty, r, ay), g.x = sdx4_axis(w, tx, r, ax), g.dst = window;
            if ((rc = run(groups.gather, [&] { return launch_sdx4_gather(g, s); }))) return rc;
            if ((rc = decode(c, window, (float)c->scaling, ty, tx, sample, false, s))) return rc;
            Sdx4BlendAdd b;
            memset(&b, 0, sizeof(b));
            b.sample = sample, b.y = sdx4_axis(h, ty, r, ay, sc), b.x = sdx4_axis(w, tx, r, ax, sc), b.acc = acc;
            if ((rc = run(groups.add, [&] { return launch_sdx4_blend_add(b, s); }))) return rc;
        }
    Sdx4BlendFinish f;
    memset(&f, 0, sizeof(f));
    f.acc = acc, f.y = sdx4_axis(h, ty, r, 0, sc), f.x = sdx4_axis(w, tx, r, 0, sc), f.out = out;
    return run(groups.finish, [&] { return launch_sdx4_blend_finish(f, s); });
}
