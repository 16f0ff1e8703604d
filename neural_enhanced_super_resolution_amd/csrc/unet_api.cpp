// UNet contexts (nesr_unet_*): the configuration check, strict weight loading, the padded and transposed upload, a workspace that
// holds the skip stack and grows with the frame, and the forward as a chain of launches of the kernels of unet.hip (in the fp16
// compute form, nesr_unet_set_dtype, the convs and the row products are unet_f16.hip's on an f16 copy of their weights).  Stands behind
// diffusers' UNet2DConditionModel.forward as StableDiffusionUpscalePipeline calls it: (sample, timestep, encoder_hidden_states,
// class_labels) -> the predicted noise.
#include <cmath>
#include <cstring>

#include "net_context.h"
#include "unet_api.h"

using namespace nesr;

namespace {

// offsets in floats into the packed weights
struct UConvW {
    size_t w = 0, b = 0;
    int cin0 = 0, cin1 = 0, cout = 0, coutp = 0;      // cin1: the skip's channels of a conv over cat(hidden, skip), or 0
};
struct UResW {
    NormW n1, n2;
    UConvW c1, c2;
    bool has_sc = false;
    LinW sc;
    size_t tw = 0, tb = 0;      // time_emb_proj
    int cin0 = 0, cin1 = 0, cout = 0, index = 0;
};
struct UAttnW {
    bool self = false;      // q | k | v in one product of the tokens; otherwise q of the tokens and k | v of the text states
    LinW q, kv, out;
};
struct UTfW {
    int dim = 0;
    NormW gn, ln1, ln2, ln3;
    LinW pin, pout, ff0, ff2;
    UAttnW a1, a2;
};
struct UBlockW {
    std::vector<UResW> res;
    std::vector<UTfW> tf;      // empty, or one a resnet
    bool has_samp = false;
    UConvW samp;
};

constexpr int kMaxLevels = 4;
constexpr float kTfNormEps = 1e-6f, kLnEps = 1e-5f;
const char* const kName = "UNet2DCondition";
const char* const kCreate = "nesr_unet_create";

}  // namespace

struct nesr_unet : NetContext {
    int cin = 7, cout = 4, levels = 4, layers = 2, heads = 8, cross = 1024, classes = 1000, groups = 32;
    float eps = 1e-5f;
    int width[kMaxLevels];
    bool attn[kMaxLevels], up_attn[kMaxLevels], only_cross[kMaxLevels];
    size_t weight_bytes = 0;         // what finalize uploaded (or would have); fp16 form: d_w does not hold what d_w16 does
    LinW t1, t2;
    size_t cls = 0;
    UConvW conv_in, conv_out;
    NormW norm_out;
    std::vector<UBlockW> down, up;
    UBlockW mid;
    std::vector<const UResW*> resnets;      // in the order of their rows of the time-embedding table
};

namespace {

// ---- the fp16 form's weight packing (unet_api.h).  Each returns whether a value was non-finite or beyond +-65504.
// rows [r0, r0 + n) of torch's weight [.][k0 + k1] -> rows [col0, col0 + n) of W16[.][K], K = round16(k0) + round16(k1): source
// 1's k start at round16(k0)
bool pack_rows_f16(_Float16* dst, const float* w, int r0, int n, int k0, int k1, int col0) {
    const int k = k0 + k1, kp0 = round_up(k0, 16), K = kp0 + (k1 ? round_up(k1, 16) : 0);
    bool bad = false;
    for (int o = 0; o < n; ++o)
        for (int kk = 0; kk < k; ++kk) {
            const float v = w[(size_t)(r0 + o) * k + kk];
            bad |= !HalfPack::carries(v);
            dst[(size_t)(col0 + o) * K + (kk < k0 ? kk : kp0 + kk - k0)] = (_Float16)v;
        }
    return bad;
}

// conv weight [n][c0 + c1][9] -> W16[round16(n)][9][round16(c0) + round16(c1)]
bool pack_conv_f16(_Float16* dst, const float* w, int n, int c0, int c1) {
    const int cin = c0 + c1, cs0 = round_up(c0, 16), ktap = cs0 + (c1 ? round_up(c1, 16) : 0);
    bool bad = false;
    for (int o = 0; o < n; ++o)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t) {
                const float v = w[((size_t)o * cin + ci) * 9 + t];
                bad |= !HalfPack::carries(v);
                dst[((size_t)o * 9 + t) * ktap + (ci < c0 ? ci : cs0 + ci - c0)] = (_Float16)v;
            }
    return bad;
}

int td_of(const nesr_unet* c) { return 4 * c->width[0]; }

void expect_resnet(StateDict& sd, const std::string& r, int64_t cin, int64_t cout, int64_t td) {
    sd.expect_wb(r + ".norm1", {cin});
    sd.expect_wb(r + ".conv1", {cout, cin, 3, 3});
    sd.expect_wb(r + ".time_emb_proj", {cout, td});
    sd.expect_wb(r + ".norm2", {cout});
    sd.expect_wb(r + ".conv2", {cout, cout, 3, 3});
    if (cin != cout) sd.expect_wb(r + ".conv_shortcut", {cout, cin, 1, 1});
}

void expect_transformer(StateDict& sd, const std::string& a, int64_t dim, int64_t cross, bool only_cross) {
    sd.expect_wb(a + ".norm", {dim});
    sd.expect_wb(a + ".proj_in", {dim, dim});
    const std::string b = a + ".transformer_blocks.0";
    for (int i = 1; i <= 2; ++i) {
        const std::string at = b + ".attn" + std::to_string(i);
        const int64_t kv = (i == 2 || only_cross) ? cross : dim;
        sd.expect_wb(b + ".norm" + std::to_string(i), {dim});
        sd.expect_wb(at + ".to_q", {dim, dim}, false);
        sd.expect_wb(at + ".to_k", {dim, kv}, false);
        sd.expect_wb(at + ".to_v", {dim, kv}, false);
        sd.expect_wb(at + ".to_out.0", {dim, dim});
    }
    sd.expect_wb(b + ".norm3", {dim});
    sd.expect_wb(b + ".ff.net.0.proj", {8 * dim, dim});
    sd.expect_wb(b + ".ff.net.2", {dim, 4 * dim});
    sd.expect_wb(a + ".proj_out", {dim, dim});
}

// The channel bookkeeping of the up blocks: resnet j of up block i takes (hidden, skip) channels and gives `out`.
struct UpShape {
    int hidden, skip, out;
};
UpShape up_shape(const nesr_unet* c, int i, int j) {
    const int L = c->levels;
    auto rev = [&](int k) { return c->width[L - 1 - k]; };
    const int out = rev(i), prev = rev(i > 0 ? i - 1 : 0), in_ch = rev(std::min(i + 1, L - 1));
    return UpShape{j == 0 ? prev : out, j == c->layers ? in_ch : out, out};
}

// Where a forward's buffers lie in the workspace (bytes from its base), and its size.
struct Plan {
    size_t x0, x1, t1, t2, h, q, a, kv, text, in, partial[2], norm[2], ln, semb, temb, total;
    std::vector<size_t> skip;
};

Plan plan(const nesr_unet* c, int n, int h, int w, int tokens) {
    const int L = c->levels;
    Plan p;
    ScratchCarver ws;
    auto px = [&](int l) { return (size_t)n * (h >> l) * (w >> l); };
    auto wp = [&](int l) { return (size_t)round_up(c->width[l], 16); };
    size_t act = 0, tf = 0, maxwp = 0, tfw = 0;
    for (int l = 0; l < L; ++l) {
        act = std::max(act, px(l) * std::max(wp(l), wp(std::min(l + 1, L - 1))));
        maxwp = std::max(maxwp, wp(l));
        if (c->attn[l] || c->up_attn[l] || l == L - 1) tf = std::max(tf, px(l) * wp(l)), tfw = std::max(tfw, wp(l));
    }
    p.x0 = ws.take(act * 4), p.x1 = ws.take(act * 4), p.t1 = ws.take(act * 4), p.t2 = ws.take(act * 4);
    p.h = ws.take(tf * 4), p.a = ws.take(tf * 4), p.q = ws.take(tf * 16);
    p.kv = ws.take((size_t)n * tokens * 2 * tfw * 4);
    p.text = ws.take((size_t)n * tokens * round_up(c->cross, 16) * 4);
    p.in = ws.take(px(0) * round_up(c->cin, 16) * 4);
    const size_t blocks = unet_gn_blocks((size_t)h * w);
    for (int s = 0; s < 2; ++s) p.partial[s] = ws.take((size_t)n * blocks * maxwp * 2 * sizeof(double));
    for (int s = 0; s < 2; ++s) p.norm[s] = ws.take((size_t)n * maxwp * sizeof(VaeNorm));
    p.ln = ws.take(px(0) * sizeof(float4));
    p.semb = ws.take((size_t)round_up(td_of(c), 16) * 4);
    p.temb = ws.take((size_t)UNET_MAX_RESNETS * UNET_MAX_WIDTH * 4);
    p.skip.push_back(ws.take(px(0) * wp(0) * 4));      // conv_in
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < c->layers; ++j) p.skip.push_back(ws.take(px(i) * wp(i) * 4));
        if (i < L - 1) p.skip.push_back(ws.take(px(i + 1) * wp(i) * 4));
    }
    p.total = ws.total();
    return p;
}

int check_frame(const nesr_unet* c, const char* entry, int n, int h, int w, int tokens) {
    const std::string e = entry;
    if (n < 1 || n > 2) return set_error(NESR_ERR_ARG, e + ": n is 1 or 2 samples, got " + std::to_string(n));
    const int div = 1 << (c->levels - 1);
    if (h < 1 || w < 1 || h % div || w % div)
        return set_error(NESR_ERR_ARG, e + ": h and w must be positive multiples of " + std::to_string(div) + " (2^(levels - 1): the skips are not resized), got " +
                                           std::to_string(h) + " x " + std::to_string(w));
    if ((long long)n * h * w > UNET_MAX_PIXELS) return set_error(NESR_ERR_ARG, e + ": n h w may not exceed 2^22 latent pixels");
    if (tokens < 1 || tokens > NESR_UNET_MAX_TEXT_TOKENS)
        return set_error(NESR_ERR_ARG, e + ": tokens must be 1 .. " + std::to_string(NESR_UNET_MAX_TEXT_TOKENS) + ", got " + std::to_string(tokens));
    for (int l = 0; l < c->levels; ++l) {
        const bool self = l == c->levels - 1 || ((c->attn[l] || c->up_attn[l]) && !c->only_cross[l]);
        if (self && (long long)(h >> l) * (w >> l) > UNET_MAX_SELF_TOKENS)
            return set_error(NESR_ERR_ARG, e + ": the self-attention of level " + std::to_string(l) + " takes at most " + std::to_string(UNET_MAX_SELF_TOKENS) +
                                               " tokens, h w gives " + std::to_string((long long)(h >> l) * (w >> l)));
    }
    return NESR_OK;
}

int forward(nesr_unet* c, const float* sample, int n, int h, int w, double timestep, int label, const float* text, int tokens, float* out, hipStream_t s) {
    const Plan p = plan(c, n, h, w, tokens);
    int rc = grow(c->ws_buf, c->ws_bytes, p.total, kName);
    if (rc) return rc;
    auto fp = [&](size_t off) { return reinterpret_cast<float*>(c->ws_buf + off); };
    float *cur = nullptr, *x0 = fp(p.x0), *x1 = fp(p.x1), *t1 = fp(p.t1), *t2 = fp(p.t2), *hb = fp(p.h), *qb = fp(p.q), *ab = fp(p.a), *kvb = fp(p.kv);
    float *textr = fp(p.text), *inr = fp(p.in), *semb = fp(p.semb), *temb = fp(p.temb);
    double* partial[2] = {reinterpret_cast<double*>(c->ws_buf + p.partial[0]), reinterpret_cast<double*>(c->ws_buf + p.partial[1])};
    VaeNorm* norm[2] = {reinterpret_cast<VaeNorm*>(c->ws_buf + p.norm[0]), reinterpret_cast<VaeNorm*>(c->ws_buf + p.norm[1])};
    float4* ln = reinterpret_cast<float4*>(c->ws_buf + p.ln);
    const float* W = c->d_w;
    const bool f16 = c->dtype == NESR_DTYPE_F16;      // a GEMM weight's offset then counts halves of d_w16
    const int L = c->levels, crossp = round_up(c->cross, 16);
    int H = h, Wd = w;

    auto src = [&](const float* ptr, int ch, const VaeNorm* nm) {
        UnetSrc u;
        u.p = ptr, u.c = ch, u.cs = ptr ? round_up(ch, 16) : 0, u.norm = nm;
        return u;
    };
    // GroupNorm statistics of in0 (| in1) into norm[0] (| norm[1])
    auto gn = [&](const NormW& nw, const float* in0, int c0, const float* in1, int c1, float eps) -> int {
        UnetGn a;
        memset(&a, 0, sizeof(a));
        a.n = n, a.m = H * Wd, a.in[0] = src(in0, c0, norm[0]), a.in[1] = src(in1, c1, in1 ? norm[1] : nullptr);
        a.partial[0] = partial[0], a.partial[1] = partial[1], a.groups = c->groups, a.gamma = W + nw.g, a.beta = W + nw.b, a.eps = eps;
        NESR_RUN(c->timer, kName, NESR_UNET_GROUP_NORM, s, [&] { return launch_unet_gn_partial(a, 0, s); });
        if (in1) NESR_RUN(c->timer, kName, NESR_UNET_GROUP_NORM, s, [&] { return launch_unet_gn_partial(a, 1, s); });
        NESR_RUN(c->timer, kName, NESR_UNET_GROUP_NORM, s, [&] { return launch_unet_gn_finish(a, s); });
        return NESR_OK;
    };
    // a conv over the current grid H x Wd (the OUTPUT grid)
    auto conv_args = [&](const UConvW& cw, const float* in0, const float* in1, bool normed, float* o) {
        UnetConv16 a;
        memset(&a, 0, sizeof(a));
        a.n = n, a.H = H, a.W = Wd, a.stride = 1;
        a.in[0] = src(in0, cw.cin0, normed ? norm[0] : nullptr), a.in[1] = src(in1, cw.cin1, normed && in1 ? norm[1] : nullptr);
        a.bias = W + cw.b, a.cout = cw.cout, a.coutp = cw.coutp, a.out = o;
        if (f16) a.w16 = c->d_w16 + cw.w, a.status = c->d_status;
        else a.w = W + cw.w;
        return a;
    };
    auto run_conv = [&](const UnetConv16& a, int group) -> int {
        if (f16) NESR_RUN(c->timer, kName, group, s, [&] { return launch_unet_conv_f16(a, s); });
        else NESR_RUN(c->timer, kName, group, s, [&] { return launch_unet_conv(a, s); });
        return NESR_OK;
    };
    auto rows_args = [&](const LinW& l, int m, const float* in0, int k0, float* o) {
        UnetRows16 a;
        memset(&a, 0, sizeof(a));
        a.m = m, a.rows_per_sample = m / n, a.in[0] = src(in0, k0, nullptr), a.b = W + l.b, a.ldw = l.np, a.np = l.np, a.out = o;
        if (f16) a.w16 = c->d_w16 + l.w, a.status = c->d_status;
        else a.w = W + l.w;
        return a;
    };
    auto run_rows = [&](const UnetRows16& a, int group) -> int {
        if (f16) NESR_RUN(c->timer, kName, group, s, [&] { return launch_unet_rows_f16(a, s); });
        else NESR_RUN(c->timer, kName, group, s, [&] { return launch_unet_rows(a, s); });
        return NESR_OK;
    };
    auto layer_norm = [&](UnetRows& a, const NormW& nw, const float* in, int m, int dim) -> int {
        UnetLnStats st;
        memset(&st, 0, sizeof(st));
        st.in = in, st.m = m, st.c = dim, st.cs = round_up(dim, 16), st.eps = kLnEps, st.out = ln;
        NESR_RUN(c->timer, kName, NESR_UNET_GROUP_NORM, s, [&] { return launch_unet_ln_stats(st, s); });
        a.prologue = UNET_PRO_LAYERNORM, a.ln = ln, a.ln_g = W + nw.g, a.ln_b = W + nw.b;
        return NESR_OK;
    };
    // in0 (| in1) -> o: conv2(silu(GN(conv1(silu(GN(x))) + temb))) + shortcut(x); o may be in0
    auto resnet = [&](const UResW& r, const float* in0, const float* in1, float* o) -> int {
        if ((rc = gn(r.n1, in0, r.cin0, in1, r.cin1, c->eps))) return rc;
        {
            UnetConv16 a = conv_args(r.c1, in0, in1, true, t1);
            a.bias = temb + (size_t)r.index * UNET_MAX_WIDTH;      // conv1.bias + time_emb_proj(silu(emb))
            if ((rc = run_conv(a, NESR_UNET_GROUP_CONV))) return rc;
        }
        if ((rc = gn(r.n2, t1, r.cout, nullptr, 0, c->eps))) return rc;
        if (r.has_sc) {
            UnetRows16 a = rows_args(r.sc, n * H * Wd, in0, r.cin0, t2);
            a.in[1] = src(in1, r.cin1, nullptr);
            if ((rc = run_rows(a, NESR_UNET_GROUP_PROJ))) return rc;
        }
        UnetConv16 a = conv_args(r.c2, t1, nullptr, true, o);
        a.res = r.has_sc ? t2 : in0;
        return run_conv(a, NESR_UNET_GROUP_CONV);
    };
    auto attention = [&](const UAttnW& at, const NormW& lnw, int dim, int m) -> int {      // hb += to_out(attn(LN(hb), context))
        const int dimp = round_up(dim, 16), tok = H * Wd;
        UnetAttn a;
        memset(&a, 0, sizeof(a));
        a.samples = n, a.nq = tok, a.heads = c->heads, a.d = dim / c->heads, a.out = ab, a.ldo = dimp;
        UnetRows16 q = rows_args(at.q, m, hb, dim, qb);
        if ((rc = layer_norm(q, lnw, hb, m, dim))) return rc;
        if ((rc = run_rows(q, NESR_UNET_GROUP_PROJ))) return rc;
        if (at.self) {
            a.nk = tok, a.q = qb, a.k = qb + dimp, a.v = qb + 2 * dimp, a.ldq = a.ldkv = 3 * dimp;
        } else {
            const UnetRows16 kv = rows_args(at.kv, n * tokens, textr, c->cross, kvb);
            if ((rc = run_rows(kv, NESR_UNET_GROUP_PROJ))) return rc;
            a.nk = tokens, a.q = qb, a.ldq = dimp, a.k = kvb, a.v = kvb + dimp, a.ldkv = 2 * dimp;
        }
        NESR_RUN(c->timer, kName, NESR_UNET_GROUP_ATTENTION, s, [&] { return launch_unet_attn(a, s); });
        UnetRows16 o = rows_args(at.out, m, ab, dim, hb);
        o.res = hb;
        return run_rows(o, NESR_UNET_GROUP_PROJ);
    };
    auto transformer = [&](const UTfW& tf, float* x) -> int {      // in place
        const int dim = tf.dim, m = n * H * Wd;
        if ((rc = gn(tf.gn, x, dim, nullptr, 0, kTfNormEps))) return rc;
        UnetRows16 pin = rows_args(tf.pin, m, x, dim, hb);
        pin.prologue = UNET_PRO_GROUPNORM, pin.in[0].norm = norm[0];
        if ((rc = run_rows(pin, NESR_UNET_GROUP_PROJ))) return rc;
        if ((rc = attention(tf.a1, tf.ln1, dim, m))) return rc;
        if ((rc = attention(tf.a2, tf.ln2, dim, m))) return rc;
        UnetRows16 f0 = rows_args(tf.ff0, m, hb, dim, qb);
        f0.geglu = 1, f0.ldw = 2 * tf.ff0.np;
        if ((rc = layer_norm(f0, tf.ln3, hb, m, dim))) return rc;
        if ((rc = run_rows(f0, NESR_UNET_GROUP_FF))) return rc;
        UnetRows16 f2 = rows_args(tf.ff2, m, qb, 4 * dim, hb);
        f2.res = hb;
        if ((rc = run_rows(f2, NESR_UNET_GROUP_FF))) return rc;
        UnetRows16 po = rows_args(tf.pout, m, hb, dim, x);
        po.res = x;
        return run_rows(po, NESR_UNET_GROUP_PROJ);
    };

    {   // the inputs as rows; silu(emb); every resnet's conv1 bias
        UnetIn a;
        memset(&a, 0, sizeof(a));
        a.src = sample, a.nchw = 1, a.c = c->cin, a.cs = round_up(c->cin, 16), a.m = H * Wd, a.rows = (long long)n * H * Wd, a.out = inr;
        NESR_RUN(c->timer, kName, NESR_UNET_GROUP_PROJ, s, [&] { return launch_unet_in(a, s); });
        UnetIn t;
        memset(&t, 0, sizeof(t));
        t.src = text, t.nchw = 0, t.c = c->cross, t.cs = crossp, t.m = tokens, t.rows = (long long)n * tokens, t.out = textr;
        NESR_RUN(c->timer, kName, NESR_UNET_GROUP_PROJ, s, [&] { return launch_unet_in(t, s); });
        const int td = td_of(c), tdp = round_up(td, 16);
        UnetEmb e;
        memset(&e, 0, sizeof(e));
        e.timestep = timestep, e.c0 = c->width[0], e.td = td, e.tdp = tdp, e.w1 = W + c->t1.w, e.b1 = W + c->t1.b, e.w2 = W + c->t2.w, e.b2 = W + c->t2.b;
        e.cls = W + c->cls + (size_t)label * tdp, e.out = semb;
        NESR_RUN(c->timer, kName, NESR_UNET_GROUP_EMBEDDING, s, [&] { return launch_unet_emb(e, s); });
        UnetTemb tb;
        memset(&tb, 0, sizeof(tb));
        tb.count = (int)c->resnets.size(), tb.td = td, tb.semb = semb, tb.weights = W, tb.out = temb;
        for (int r = 0; r < tb.count; ++r) tb.r[r].w = c->resnets[r]->tw, tb.r[r].b = c->resnets[r]->tb, tb.r[r].cb = c->resnets[r]->c1.b, tb.r[r].coutp = c->resnets[r]->c1.coutp;
        NESR_RUN(c->timer, kName, NESR_UNET_GROUP_EMBEDDING, s, [&] { return launch_unet_temb(tb, s); });
    }
    std::vector<float*> skips;
    size_t next = 0;
    auto push = [&]() {
        float* b = fp(p.skip[next++]);
        skips.push_back(b);
        return b;
    };
    {
        const UnetConv16 a = conv_args(c->conv_in, inr, nullptr, false, push());
        if ((rc = run_conv(a, NESR_UNET_GROUP_CONV))) return rc;
        cur = skips.back();
    }
    for (int i = 0; i < L; ++i) {
        const UBlockW& b = c->down[i];
        for (size_t j = 0; j < b.res.size(); ++j) {
            float* o = push();
            if ((rc = resnet(b.res[j], cur, nullptr, o))) return rc;
            if (!b.tf.empty() && (rc = transformer(b.tf[j], o))) return rc;
            cur = o;
        }
        if (b.has_samp) {
            H /= 2, Wd /= 2;
            UnetConv16 a = conv_args(b.samp, cur, nullptr, false, push());
            a.stride = 2;
            if ((rc = run_conv(a, NESR_UNET_GROUP_RESAMPLE))) return rc;
            cur = skips.back();
        }
    }
    if ((rc = resnet(c->mid.res[0], cur, nullptr, x0))) return rc;
    if ((rc = transformer(c->mid.tf[0], x0))) return rc;
    if ((rc = resnet(c->mid.res[1], x0, nullptr, x0))) return rc;
    cur = x0;
    float* other = x1;
    for (int i = 0; i < L; ++i) {
        const UBlockW& b = c->up[i];
        for (size_t j = 0; j < b.res.size(); ++j) {
            const float* skip = skips.back();
            skips.pop_back();
            if ((rc = resnet(b.res[j], cur, skip, cur))) return rc;
            if (!b.tf.empty() && (rc = transformer(b.tf[j], cur))) return rc;
        }
        if (b.has_samp) {
            H *= 2, Wd *= 2;
            UnetConv16 a = conv_args(b.samp, cur, nullptr, false, other);
            a.up = 1;
            if ((rc = run_conv(a, NESR_UNET_GROUP_RESAMPLE))) return rc;
            std::swap(cur, other);
        }
    }
    if ((rc = gn(c->norm_out, cur, c->width[0], nullptr, 0, c->eps))) return rc;
    UnetConv16 a = conv_args(c->conv_out, cur, nullptr, true, out);
    a.out_nchw = 1;
    return run_conv(a, NESR_UNET_GROUP_CONV);
}

}  // namespace

extern "C" {

int nesr_unet_create(nesr_unet** out, int device_id, int in_channels, int out_channels, int num_blocks, const int* block_out_channels,
                     const char* const* down_block_types, const char* const* up_block_types, const char* mid_block_type, const int* only_cross_attention,
                     int layers_per_block, int attention_head_dim, int cross_attention_dim, int transformer_layers_per_block, int use_linear_projection,
                     int dual_cross_attention, int num_class_embeds, int norm_num_groups, double norm_eps, int flip_sin_to_cos, double freq_shift,
                     int downsample_padding, const char* act_fn) {
    if (!out) return set_error(NESR_ERR_ARG, "nesr_unet_create: null out");
    *out = nullptr;
    if (!block_out_channels || !down_block_types || !up_block_types || !mid_block_type || !only_cross_attention || !act_fn)
        return set_error(NESR_ERR_ARG, "nesr_unet_create: null configuration argument");
    const int L = num_blocks;
    if (L < 2 || L > kMaxLevels) return unsupported(kCreate, "block_out_channels", "2 .. 4 entries, got " + std::to_string(L));
    if (layers_per_block < 1 || layers_per_block > 3) return unsupported(kCreate, "layers_per_block", "1 .. 3, got " + std::to_string(layers_per_block));
    if (norm_num_groups < 1) return unsupported(kCreate, "norm_num_groups", "must be positive");
    if (attention_head_dim < 1) return unsupported(kCreate, "attention_head_dim", "the number of heads must be positive");
    if (!use_linear_projection) return unsupported(kCreate, "use_linear_projection", "false (proj_in / proj_out as 1x1 convs around the tokens) is not supported");
    if (transformer_layers_per_block != 1) return unsupported(kCreate, "transformer_layers_per_block", "one BasicTransformerBlock a Transformer, got " + std::to_string(transformer_layers_per_block));
    if (dual_cross_attention) return unsupported(kCreate, "dual_cross_attention", "not supported");
    if (std::string(act_fn) != "silu") return unsupported(kCreate, "act_fn", "'" + std::string(act_fn) + "' is not supported (silu only)");
    if (!flip_sin_to_cos) return unsupported(kCreate, "flip_sin_to_cos", "false is not supported");
    if (freq_shift != 0.0) return unsupported(kCreate, "freq_shift", "0 only");
    if (downsample_padding != 1) return unsupported(kCreate, "downsample_padding", "1 only");
    if (!(norm_eps > 0) || !std::isfinite(norm_eps)) return unsupported(kCreate, "norm_eps", "must be positive and finite");
    if (std::string(mid_block_type) != "UNetMidBlock2DCrossAttn") return unsupported(kCreate, "mid_block_type", "'" + std::string(mid_block_type) + "' is not supported (UNetMidBlock2DCrossAttn only)");
    if (cross_attention_dim < 1 || cross_attention_dim > UNET_MAX_WIDTH) return unsupported(kCreate, "cross_attention_dim", "1 .. 1024, got " + std::to_string(cross_attention_dim));
    if (in_channels < 1 || in_channels > 16) return unsupported(kCreate, "in_channels", "1 .. 16, got " + std::to_string(in_channels));
    if (out_channels < 1 || out_channels > 16) return unsupported(kCreate, "out_channels", "1 .. 16, got " + std::to_string(out_channels));
    if (num_class_embeds < 1) return unsupported(kCreate, "num_class_embeds", "the class embedding (the pipeline's noise level) is required");
    bool attn[kMaxLevels], up_attn[kMaxLevels];
    for (int i = 0; i < L; ++i) {
        if (!down_block_types[i] || !up_block_types[i]) return set_error(NESR_ERR_ARG, "nesr_unet_create: null block type");
        const std::string d = down_block_types[i], u = up_block_types[i];
        if (d != "DownBlock2D" && d != "CrossAttnDownBlock2D") return unsupported(kCreate, "down_block_types", "'" + d + "' is not supported (DownBlock2D, CrossAttnDownBlock2D)");
        if (u != "UpBlock2D" && u != "CrossAttnUpBlock2D") return unsupported(kCreate, "up_block_types", "'" + u + "' is not supported (UpBlock2D, CrossAttnUpBlock2D)");
        attn[i] = d == "CrossAttnDownBlock2D";
        up_attn[L - 1 - i] = u == "CrossAttnUpBlock2D";      // by level
    }
    for (int i = 0; i < L; ++i) {
        const int wd = block_out_channels[i];
        if (wd < 1 || wd > UNET_MAX_WIDTH) return unsupported(kCreate, "block_out_channels", "every width must be 1 .. 1024, got " + std::to_string(wd));
        if (wd % norm_num_groups) return unsupported(kCreate, "block_out_channels", std::to_string(wd) + " is no multiple of norm_num_groups " + std::to_string(norm_num_groups));
        if (i == 0 && wd % 2) return unsupported(kCreate, "block_out_channels", "the first width (the sinusoid's) must be even, got " + std::to_string(wd));
        if (attn[i] || up_attn[i] || i == L - 1) {
            if (wd % attention_head_dim) return unsupported(kCreate, "attention_head_dim", std::to_string(wd) + " is no multiple of the " + std::to_string(attention_head_dim) + " heads");
            const int d = wd / attention_head_dim;
            if (d < 8 || d > UNET_MAX_HEAD || d % 8)
                return unsupported(kCreate, "attention_head_dim", "a head width of " + std::to_string(d) + " (width " + std::to_string(wd) + " / " + std::to_string(attention_head_dim) +
                                                             " heads): 8 .. 128 and a multiple of 8");
        }
    }
    // checked here, not only documented: every kernel's LDS fits a CU at any configuration that passed
    for (size_t bytes : {unet_conv_lds_bytes(1), unet_conv_lds_bytes(2), unet_rows_lds_bytes(), unet_attn_lds_bytes(), unet_emb_lds_bytes()})
        if (bytes > VAE_LDS_LIMIT) return unsupported(kCreate, "block_out_channels", "a kernel's LDS of " + std::to_string(bytes) + " bytes exceeds 160 KB");
    if (const int rc = check_device(device_id, NESR_UNET_NO_DEVICE)) return rc;
    nesr_unet* c = new nesr_unet();
    c->device = device_id, c->cin = in_channels, c->cout = out_channels, c->levels = L, c->layers = layers_per_block, c->heads = attention_head_dim;
    c->cross = cross_attention_dim, c->classes = num_class_embeds, c->groups = norm_num_groups, c->eps = (float)norm_eps;
    for (int i = 0; i < L; ++i) c->width[i] = block_out_channels[i], c->attn[i] = attn[i], c->up_attn[i] = up_attn[i], c->only_cross[i] = only_cross_attention[i] != 0;
    StateDict& sd = c->sd;
    const int64_t td = td_of(c), cross = c->cross;
    sd.expect_wb("conv_in", {c->width[0], c->cin, 3, 3});
    sd.expect_wb("time_embedding.linear_1", {td, c->width[0]});
    sd.expect_wb("time_embedding.linear_2", {td, td});
    sd.expect("class_embedding.weight", {c->classes, td});
    int prev = c->width[0];
    for (int i = 0; i < L; ++i) {
        const std::string d = "down_blocks." + std::to_string(i);
        for (int j = 0; j < c->layers && c->attn[i]; ++j) expect_transformer(sd, d + ".attentions." + std::to_string(j), c->width[i], cross, c->only_cross[i]);
        for (int j = 0; j < c->layers; ++j) expect_resnet(sd, d + ".resnets." + std::to_string(j), j == 0 ? prev : c->width[i], c->width[i], td);
        if (i < L - 1) sd.expect_wb(d + ".downsamplers.0.conv", {c->width[i], c->width[i], 3, 3});
        prev = c->width[i];
    }
    for (int i = 0; i < L; ++i) {
        const std::string u = "up_blocks." + std::to_string(i);
        const int l = L - 1 - i;
        for (int j = 0; j <= c->layers && c->up_attn[l]; ++j) expect_transformer(sd, u + ".attentions." + std::to_string(j), c->width[l], cross, c->only_cross[l]);
        for (int j = 0; j <= c->layers; ++j) {
            const UpShape sh = up_shape(c, i, j);
            expect_resnet(sd, u + ".resnets." + std::to_string(j), sh.hidden + sh.skip, sh.out, td);
        }
        if (i < L - 1) sd.expect_wb(u + ".upsamplers.0.conv", {c->width[l], c->width[l], 3, 3});
    }
    expect_transformer(sd, "mid_block.attentions.0", prev, cross, false);
    expect_resnet(sd, "mid_block.resnets.0", prev, prev, td);
    expect_resnet(sd, "mid_block.resnets.1", prev, prev, td);
    sd.expect_wb("conv_norm_out", {c->width[0]});
    sd.expect_wb("conv_out", {c->cout, c->width[0], 3, 3});
    *out = c;
    return NESR_OK;
}

void nesr_unet_destroy(nesr_unet* c) { net_destroy(c); }

int nesr_unet_num_tensors(const nesr_unet* c) { return net_num_tensors(c); }

int nesr_unet_set_dtype(nesr_unet* c, int dtype) {
    if (dtype == NESR_DTYPE_BF16)
        return set_error(NESR_ERR_UNSUPPORTED, "nesr_unet_set_dtype: NESR_DTYPE_BF16 (" + std::to_string(dtype) + ") is not a form of the UNet: NESR_DTYPE_F32 or NESR_DTYPE_F16");
    if (dtype != NESR_DTYPE_F32 && dtype != NESR_DTYPE_F16)
        return set_error(NESR_ERR_UNSUPPORTED, "nesr_unet_set_dtype: dtype " + std::to_string(dtype) + " is not a form of the UNet: NESR_DTYPE_F32 or NESR_DTYPE_F16");
    if (!c) return set_error(NESR_ERR_ARG, "nesr_unet_set_dtype: null context");
    if (c->packed) return set_error(NESR_ERR_STATE, "nesr_unet_set_dtype: the compute form is chosen between nesr_unet_create and nesr_unet_finalize");
    c->dtype = dtype;
    return NESR_OK;
}

int nesr_unet_dtype(const nesr_unet* c) { return c ? c->dtype : NESR_DTYPE_F32; }

int nesr_unet_weight_bytes(const nesr_unet* c, size_t* bytes) {
    if (!c || !bytes) return set_error(NESR_ERR_ARG, "nesr_unet_weight_bytes: null pointer");
    if (!c->packed) return set_error(NESR_ERR_STATE, "nesr_unet_weight_bytes: weights not finalized (nesr_unet_finalize)");
    *bytes = c->weight_bytes;
    return NESR_OK;
}

int nesr_unet_pack_linear_f16(const float* weight, int n, int k0, int k1, uint16_t* out, size_t out_halves) {
    if (!weight || !out || n < 1 || k0 < 1 || k1 < 0) return set_error(NESR_ERR_ARG, "nesr_unet_pack_linear_f16: a weight [n][k0 + k1] with n, k0 >= 1 and k1 >= 0");
    const size_t need = (size_t)round_up(n, 16) * (round_up(k0, 16) + (k1 ? round_up(k1, 16) : 0));
    if (out_halves != need) return set_error(NESR_ERR_ARG, "nesr_unet_pack_linear_f16: out_halves must be round16(n) (round16(k0) + round16(k1)) = " + std::to_string(need));
    memset(out, 0, need * sizeof(uint16_t));
    if (pack_rows_f16(reinterpret_cast<_Float16*>(out), weight, 0, n, k0, k1, 0))
        return set_error(NESR_ERR_RANGE, "nesr_unet_pack_linear_f16: the weight holds a value that is non-finite or beyond +-65504");
    return NESR_OK;
}

int nesr_unet_pack_conv_f16(const float* weight, int n, int c0, int c1, uint16_t* out, size_t out_halves) {
    if (!weight || !out || n < 1 || c0 < 1 || c1 < 0) return set_error(NESR_ERR_ARG, "nesr_unet_pack_conv_f16: a weight [n][c0 + c1][3][3] with n, c0 >= 1 and c1 >= 0");
    const size_t need = (size_t)round_up(n, 16) * 9 * (round_up(c0, 16) + (c1 ? round_up(c1, 16) : 0));
    if (out_halves != need) return set_error(NESR_ERR_ARG, "nesr_unet_pack_conv_f16: out_halves must be round16(n) 9 (round16(c0) + round16(c1)) = " + std::to_string(need));
    memset(out, 0, need * sizeof(uint16_t));
    if (pack_conv_f16(reinterpret_cast<_Float16*>(out), weight, n, c0, c1))
        return set_error(NESR_ERR_RANGE, "nesr_unet_pack_conv_f16: the weight holds a value that is non-finite or beyond +-65504");
    return NESR_OK;
}

int nesr_unet_load_weight(nesr_unet* c, const char* key, const float* data, const int64_t* shape, int ndim) {
    return net_load_weight(c, "nesr_unet_load_weight", key, data, shape, ndim, [](std::string&) { return true; });
}

int nesr_unet_finalize(nesr_unet* c) {
    if (const int rc = net_begin_finalize(c, "nesr_unet_finalize")) return rc;
    const StateDict& sd = c->sd;
    HostPack pk;
    // The fp16 form: a GEMM weight goes into `hp` alone, packed as unet_api.h states for unet_f16.hip, and its offset counts halves;
    // the f32 buffer then holds the biases, the norms, the class table and the M = 1 products' weights (embedding, time_emb_proj).
    const bool f16 = c->dtype == NESR_DTYPE_F16;
    HalfPack hp;
    const int L = c->levels, td = td_of(c), tdp = round_up(td, 16), cross = c->cross;
    // conv weight [n][cin0 + cin1][9] -> [(tap (cinp0 + cinp1) + the channel's place)][coutp]: the skip's channels start at cinp0
    auto conv = [&](const std::string& name, int n, int cin0, int cin1) {
        UConvW r;
        r.cin0 = cin0, r.cin1 = cin1, r.cout = n, r.coutp = round_up(n, 16);
        const std::vector<float>& w = sd.data(name + ".weight");
        if (f16) {
            r.w = hp.reserve((size_t)r.coutp * 9 * (round_up(cin0, 16) + (cin1 ? round_up(cin1, 16) : 0)));
            hp.note(name + ".weight", pack_conv_f16(hp.half.data() + r.w, w.data(), n, cin0, cin1));
            r.b = pk.vec(sd.data(name + ".bias"), r.coutp);
            return r;
        }
        const int cinp0 = round_up(cin0, 4), cinp = cinp0 + round_up(cin1, 4), cin = cin0 + cin1;
        r.w = pk.reserve((size_t)9 * cinp * r.coutp);
        for (int o = 0; o < n; ++o)
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < 9; ++t) pk.host[r.w + ((size_t)t * cinp + (ci < cin0 ? ci : cinp0 + ci - cin0)) * r.coutp + o] = w[((size_t)o * cin + ci) * 9 + t];
        r.b = pk.vec(sd.data(name + ".bias"), r.coutp);
        return r;
    };
    // rows [r0, r0 + n) of torch's weight [.][k0 + k1] -> columns [col0, col0 + n) of Wt[round16(k0) + round16(k1)][ld]
    // (fp16 form, a GEMM weight: rows [col0, col0 + n) of W16[ld][K] at `at` of hp)
    auto put = [&](size_t at, const std::string& key, int r0, int n, int k0, int k1, int ld, int col0, bool gemm = true) {
        const std::vector<float>& w = sd.data(key);
        if (f16 && gemm) return hp.note(key, pack_rows_f16(hp.half.data() + at, w.data(), r0, n, k0, k1, col0));
        const int k = k0 + k1, kp0 = round_up(k0, 16);
        for (int o = 0; o < n; ++o)
            for (int kk = 0; kk < k; ++kk) pk.host[at + (size_t)(kk < k0 ? kk : kp0 + kk - k0) * ld + col0 + o] = w[(size_t)(r0 + o) * k + kk];
    };
    // a matrix of K rows and ld columns: where its elements go (floats of pk, or halves of hp for a GEMM weight of the fp16 form)
    auto matrix = [&](size_t K, size_t ld, bool gemm = true) { return f16 && gemm ? hp.reserve(K * ld) : pk.reserve(K * ld); };
    // gemm false: an M = 1 product on plain FMAs (the embedding, time_emb_proj), f32 in either form
    auto linear = [&](const std::string& name, int n, int k0, int k1, bool bias, bool gemm = true) {
        LinW l;
        l.np = round_up(n, 16);
        l.w = matrix(round_up(k0, 16) + (k1 ? round_up(k1, 16) : 0), l.np, gemm);
        put(l.w, name + ".weight", 0, n, k0, k1, l.np, 0, gemm);
        l.b = bias ? pk.vec(sd.data(name + ".bias"), l.np) : pk.reserve(l.np);
        return l;
    };
    // several products of one input side by side: Wt[round16(k)][parts np], no bias
    auto fused = [&](const std::string& at, std::initializer_list<const char*> parts, int n, int k) {
        LinW l;
        const int np1 = round_up(n, 16), count = (int)parts.size();
        l.np = count * np1;
        l.w = matrix(round_up(k, 16), l.np);
        l.b = pk.reserve(l.np);
        int i = 0;
        for (const char* part : parts) put(l.w, at + part + ".weight", 0, n, k, 0, l.np, np1 * i++);
        return l;
    };
    c->resnets.clear();
    auto resnet = [&](const std::string& r, int cin0, int cin1, int cout) {
        UResW w;
        const int cin = cin0 + cin1;
        w.cin0 = cin0, w.cin1 = cin1, w.cout = cout;
        w.n1 = pk.norm(sd, r + ".norm1", cin), w.c1 = conv(r + ".conv1", cout, cin0, cin1), w.n2 = pk.norm(sd, r + ".norm2", cout), w.c2 = conv(r + ".conv2", cout, cout, 0);
        const LinW t = linear(r + ".time_emb_proj", cout, td, 0, true, false);      // Wt[td][coutp]: td = 4 width[0] is a multiple of 8, its K is not tiled
        w.tw = t.w, w.tb = t.b;
        w.has_sc = cin != cout;
        if (w.has_sc) w.sc = linear(r + ".conv_shortcut", cout, cin0, cin1, true);
        return w;
    };
    auto transformer = [&](const std::string& a, int dim, bool only_cross) {
        UTfW t;
        t.dim = dim;
        const std::string b = a + ".transformer_blocks.0";
        t.gn = pk.norm(sd, a + ".norm", dim), t.pin = linear(a + ".proj_in", dim, dim, 0, true), t.pout = linear(a + ".proj_out", dim, dim, 0, true);
        t.ln1 = pk.norm(sd, b + ".norm1", dim), t.ln2 = pk.norm(sd, b + ".norm2", dim), t.ln3 = pk.norm(sd, b + ".norm3", dim);
        for (int i = 1; i <= 2; ++i) {
            UAttnW& at = i == 1 ? t.a1 : t.a2;
            const std::string n = b + ".attn" + std::to_string(i);
            at.self = i == 1 && !only_cross;
            if (at.self) {
                at.q = fused(n, {".to_q", ".to_k", ".to_v"}, dim, dim);
            } else {
                at.q = fused(n, {".to_q"}, dim, dim);
                at.kv = fused(n, {".to_k", ".to_v"}, dim, cross);
            }
            at.out = linear(n + ".to_out.0", dim, dim, 0, true);
        }
        {   // GEGLU: value half | gate half, Wt[dimp][2 inner]
            const int inner = 4 * dim, dimp = round_up(dim, 16), np = round_up(inner, 16);
            t.ff0.np = np;
            t.ff0.w = matrix(dimp, 2 * np);
            t.ff0.b = pk.reserve(2 * np);
            const std::vector<float>& bias = sd.data(b + ".ff.net.0.proj.bias");
            for (int half = 0; half < 2; ++half) {
                put(t.ff0.w, b + ".ff.net.0.proj.weight", half * inner, inner, dim, 0, 2 * np, half * np);
                std::copy(bias.begin() + half * inner, bias.begin() + (half + 1) * inner, pk.host.begin() + t.ff0.b + (size_t)half * np);
            }
        }
        t.ff2 = linear(b + ".ff.net.2", dim, 4 * dim, 0, true);
        return t;
    };
    c->conv_in = conv("conv_in", c->width[0], c->cin, 0);
    c->t1 = linear("time_embedding.linear_1", td, c->width[0], 0, true, false);
    c->t2 = linear("time_embedding.linear_2", td, td, 0, true, false);
    {   // the class table, rows padded to tdp
        c->cls = pk.reserve((size_t)c->classes * tdp);
        const std::vector<float>& w = sd.data("class_embedding.weight");
        for (int r = 0; r < c->classes; ++r) std::copy(w.begin() + (size_t)r * td, w.begin() + (size_t)(r + 1) * td, pk.host.begin() + c->cls + (size_t)r * tdp);
    }
    c->down.assign(L, UBlockW());
    c->up.assign(L, UBlockW());
    c->mid = UBlockW();
    int prev = c->width[0];
    for (int i = 0; i < L; ++i) {
        const std::string d = "down_blocks." + std::to_string(i);
        UBlockW& b = c->down[i];
        for (int j = 0; j < c->layers; ++j) {
            b.res.push_back(resnet(d + ".resnets." + std::to_string(j), j == 0 ? prev : c->width[i], 0, c->width[i]));
            if (c->attn[i]) b.tf.push_back(transformer(d + ".attentions." + std::to_string(j), c->width[i], c->only_cross[i]));
        }
        b.has_samp = i < L - 1;
        if (b.has_samp) b.samp = conv(d + ".downsamplers.0.conv", c->width[i], c->width[i], 0);
        prev = c->width[i];
    }
    c->mid.res.push_back(resnet("mid_block.resnets.0", prev, 0, prev));
    c->mid.tf.push_back(transformer("mid_block.attentions.0", prev, false));
    c->mid.res.push_back(resnet("mid_block.resnets.1", prev, 0, prev));
    for (int i = 0; i < L; ++i) {
        const std::string u = "up_blocks." + std::to_string(i);
        const int l = L - 1 - i;
        UBlockW& b = c->up[i];
        for (int j = 0; j <= c->layers; ++j) {
            const UpShape sh = up_shape(c, i, j);
            b.res.push_back(resnet(u + ".resnets." + std::to_string(j), sh.hidden, sh.skip, sh.out));
            if (c->up_attn[l]) b.tf.push_back(transformer(u + ".attentions." + std::to_string(j), c->width[l], c->only_cross[l]));
        }
        b.has_samp = i < L - 1;
        if (b.has_samp) b.samp = conv(u + ".upsamplers.0.conv", c->width[l], c->width[l], 0);
    }
    c->norm_out = pk.norm(sd, "conv_norm_out", c->width[0]);
    c->conv_out = conv("conv_out", c->cout, c->width[0], 0);
    // the rows of the time-embedding table: the vectors above no longer move
    auto number = [&](UBlockW& b) {
        for (UResW& r : b.res) r.index = (int)c->resnets.size(), c->resnets.push_back(&r);
    };
    for (UBlockW& b : c->down) number(b);
    number(c->mid);
    for (UBlockW& b : c->up) number(b);
    if ((int)c->resnets.size() > UNET_MAX_RESNETS) return set_error(NESR_ERR_STATE, "nesr_unet_finalize: more ResnetBlocks than the embedding launch takes");
    if (hp.out_of_range().empty()) c->weight_bytes = pk.host.size() * sizeof(float) + hp.half.size() * sizeof(_Float16);      // a refused pack leaves it
    return net_upload(c, "nesr_unet_finalize", pk, &hp, kName);
}

int nesr_unet_workspace_bytes(nesr_unet* c, int n, int h, int w, int tokens, size_t* bytes) {
    if (!c || !bytes) return set_error(NESR_ERR_ARG, "nesr_unet_workspace_bytes: null pointer");
    const int rc = check_frame(c, "nesr_unet_workspace_bytes", n, h, w, tokens);
    if (rc) return rc;
    *bytes = plan(c, n, h, w, tokens).total;
    return NESR_OK;
}

}  // extern "C"

// the forward behind nesr_unet_forward_f32's checks, without the fp16 form's bracket (unet_api.h)
int unet_forward_unchecked(nesr_unet* c, const float* sample, int n, int ch, int h, int w, double timestep, int class_label, const float* text_states, int tokens,
                           float* out, size_t out_elems, hipStream_t stream) {
    const std::string e = "nesr_unet_forward_f32";
    if (!c || !sample || !text_states || !out) return set_error(NESR_ERR_ARG, e + ": null pointer");
    if (!c->finalized) return set_error(NESR_ERR_STATE, e + ": weights not finalized (nesr_unet_finalize)");
    if (ch != c->cin) return set_error(NESR_ERR_ARG, e + ": expected [n, " + std::to_string(c->cin) + ", h, w] (in_channels), got " + std::to_string(ch) + " channels");
    const int rc = check_frame(c, e.c_str(), n, h, w, tokens);
    if (rc) return rc;
    if (class_label < 0 || class_label >= c->classes)
        return set_error(NESR_ERR_ARG, e + ": class_label " + std::to_string(class_label) + " is outside the table of " + std::to_string(c->classes) + " (num_class_embeds)");
    if (!std::isfinite(timestep)) return set_error(NESR_ERR_ARG, e + ": timestep must be finite");
    const size_t need = (size_t)n * c->cout * h * w;
    if (out_elems != need) return set_error(NESR_ERR_ARG, e + ": out_elems must be n out_channels h w = " + std::to_string(need) + ", got " + std::to_string(out_elems));
    NESR_TRY(hipSetDevice(c->device));
    return forward(c, sample, n, h, w, timestep, class_label, text_states, tokens, out, stream);
}

// The fp16 form's range word around a call's launches (unet_api.h; sdx4_api.cpp brackets a whole denoising loop with them).
int unet_range_begin(nesr_unet* c, hipStream_t s) { return net_range_begin(c, s); }

int unet_range_end(nesr_unet* c, hipStream_t s, const char* entry) {
    return net_range_end(c, s, entry, "an activation of the UNet's fp16 form was non-finite or exceeded 65504 in magnitude when it was rounded to f16; the result is "
                                      "not valid (NESR_DTYPE_F32 carries such values)");
}

extern "C" {

int nesr_unet_forward_f32(nesr_unet* c, const float* sample, int n, int ch, int h, int w, double timestep, int class_label, const float* text_states, int tokens,
                          float* out, size_t out_elems, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = unet_range_begin(c, s);
    if (!rc) rc = unet_forward_unchecked(c, sample, n, ch, h, w, timestep, class_label, text_states, tokens, out, out_elems, s);
    return rc ? rc : unet_range_end(c, s, "nesr_unet_forward_f32");
}

int nesr_unet_set_timing(nesr_unet* c, int enable) { return net_set_timing(c, "nesr_unet_set_timing", enable); }

int nesr_unet_kernel_time_ms(nesr_unet* c, double* group_ms, int n_groups, int64_t* launches) {
    return net_kernel_time_ms(c, "nesr_unet_kernel_time_ms", NESR_UNET_GROUPS, group_ms, n_groups, launches);
}

}  // extern "C"

// what the x4 pipeline (sdx4_api.cpp) asks of a context it does not own
#include "sdx4_api.h"
nesr::Sdx4UnetInfo nesr::sdx4_unet_info(const nesr_unet* c) {
    return Sdx4UnetInfo{c->device, c->cin, c->cout, c->levels, c->cross, c->classes, c->finalized, c->timer.launches};
}
