// CLIP text-encoder contexts (nesr_clip_text_*): the configuration check, strict weight loading under either key generation, the
// padded and transposed upload, a workspace that grows with n tokens, and the forward as a chain of launches: the kernels of
// clip_text.hip and, for every product and every LayerNorm inside a layer, the UNet's launchers as they are.  Stands behind
// transformers' CLIPTextModel(input_ids)[0] as StableDiffusionUpscalePipeline calls it (no attention mask: padding ids are tokens).
// At the end: the single-launch test hooks nesr_clip_text_k_*.
#include <cmath>
#include <cstring>

#include "clip_text_api.h"
#include "net_context.h"

using namespace nesr;

namespace {

struct CLayerW {
    NormW ln1, ln2;
    LinW qkv, out, fc1, fc2;
};

const char* const kName = "ClipTextEncoder";
const char* const kCreate = "nesr_clip_text_create";
const char* const kPrefix = "text_model.";                       // the published files' key generation
const char* const kPositionIds = "embeddings.position_ids";      // a buffer of theirs: arange(max_position_embeddings)

}  // namespace

struct nesr_clip_text : NetContext {
    int vocab = 49408, hidden = 1024, inter = 4096, layers = 23, heads = 16, positions = 77, act = CLIP_ACT_GELU;
    float eps = 1e-5f;
    size_t tok = 0, pos = 0;
    std::vector<CLayerW> layer;
    NormW fin;
};

namespace {

// Where an encode's buffers lie in the workspace (bytes from its base), and its size.
struct Plan {
    size_t x, qkv, att, fc, ln, total;
};

Plan plan(const nesr_clip_text* c, int n, int tokens) {
    Plan p;
    ScratchCarver ws;
    const size_t m = (size_t)n * tokens, hp = round_up(c->hidden, 16), ip = round_up(c->inter, 16);
    p.x = ws.take(m * hp * 4), p.qkv = ws.take(m * 3 * hp * 4), p.att = ws.take(m * hp * 4), p.fc = ws.take(m * ip * 4), p.ln = ws.take(m * sizeof(float4));
    p.total = ws.total();
    return p;
}

int check_call(const nesr_clip_text* c, const char* entry, int n, int tokens) {
    const std::string e = entry;
    if (n < 1 || n > 2) return set_error(NESR_ERR_ARG, e + ": n is 1 or 2 samples, got " + std::to_string(n));
    const int most = std::min(c->positions, (int)NESR_UNET_MAX_TEXT_TOKENS);
    if (tokens < 1 || tokens > most)
        return set_error(NESR_ERR_ARG, e + ": tokens must be 1 .. " + std::to_string(most) + " (max_position_embeddings " + std::to_string(c->positions) +
                                           ", NESR_UNET_MAX_TEXT_TOKENS " + std::to_string(NESR_UNET_MAX_TEXT_TOKENS) + "), got " + std::to_string(tokens));
    return NESR_OK;
}

int encode(nesr_clip_text* c, const int32_t* ids, int n, int tokens, float* out, hipStream_t s) {
    const Plan p = plan(c, n, tokens);
    int rc = grow(c->ws_buf, c->ws_bytes, p.total, kName);
    if (rc) return rc;
    auto fp = [&](size_t off) { return reinterpret_cast<float*>(c->ws_buf + off); };
    float *x = fp(p.x), *qkv = fp(p.qkv), *att = fp(p.att), *fc = fp(p.fc);
    float4* ln = reinterpret_cast<float4*>(c->ws_buf + p.ln);
    const float* W = c->d_w;
    const int m = n * tokens, hp = round_up(c->hidden, 16), ip = round_up(c->inter, 16);

    auto rows_args = [&](const LinW& l, const float* in, int k, float* o) {
        UnetRows a;
        memset(&a, 0, sizeof(a));
        a.m = m, a.rows_per_sample = tokens, a.in[0].p = in, a.in[0].c = k, a.in[0].cs = round_up(k, 16), a.w = W + l.w, a.b = W + l.b, a.ldw = l.np, a.np = l.np, a.out = o;
        return a;
    };
    auto stats = [&]() -> int {      // of x, into ln
        UnetLnStats st;
        memset(&st, 0, sizeof(st));
        st.in = x, st.m = m, st.c = c->hidden, st.cs = hp, st.eps = c->eps, st.out = ln;
        NESR_RUN(c->timer, kName, NESR_CLIP_TEXT_GROUP_NORM, s, [&] { return launch_unet_ln_stats(st, s); });
        return NESR_OK;
    };
    auto normed_rows = [&](const LinW& l, const NormW& nw, float* o, int group) -> int {      // o = LN(x) w + b
        if ((rc = stats())) return rc;
        UnetRows a = rows_args(l, x, c->hidden, o);
        a.prologue = UNET_PRO_LAYERNORM, a.ln = ln, a.ln_g = W + nw.g, a.ln_b = W + nw.b;
        NESR_RUN(c->timer, kName, group, s, [&] { return launch_unet_rows(a, s); });
        return NESR_OK;
    };
    auto residual_rows = [&](const LinW& l, const float* in, int k, int group) -> int {      // x += in w + b
        UnetRows a = rows_args(l, in, k, x);
        a.res = x;
        NESR_RUN(c->timer, kName, group, s, [&] { return launch_unet_rows(a, s); });
        return NESR_OK;
    };

    {
        ClipEmbed e;
        memset(&e, 0, sizeof(e));
        e.tok = W + c->tok, e.pos = W + c->pos, e.vocab = c->vocab, e.positions = c->positions, e.rows = m, e.tokens = tokens, e.c = c->hidden, e.cs = hp, e.out = x;
        for (int r = 0; r < m; ++r) e.ids[r] = ids[r];
        NESR_RUN(c->timer, kName, NESR_CLIP_TEXT_GROUP_EMBEDDING, s, [&] { return launch_clip_embed(e, s); });
    }
    for (const CLayerW& l : c->layer) {
        if ((rc = normed_rows(l.qkv, l.ln1, qkv, NESR_CLIP_TEXT_GROUP_PROJ))) return rc;
        ClipAttn a;
        memset(&a, 0, sizeof(a));
        a.samples = n, a.tokens = tokens, a.heads = c->heads, a.d = c->hidden / c->heads;
        a.q = qkv, a.k = qkv + hp, a.v = qkv + 2 * hp, a.ldq = a.ldkv = 3 * hp, a.ldo = hp, a.out = att;
        NESR_RUN(c->timer, kName, NESR_CLIP_TEXT_GROUP_ATTENTION, s, [&] { return launch_clip_attn(a, s); });
        if ((rc = residual_rows(l.out, att, c->hidden, NESR_CLIP_TEXT_GROUP_PROJ))) return rc;
        if ((rc = normed_rows(l.fc1, l.ln2, fc, NESR_CLIP_TEXT_GROUP_FF))) return rc;
        ClipAct g;
        g.x = fc, g.count = (long long)m * ip, g.act = c->act;      // the pad columns hold 0 and act(0) = 0
        NESR_RUN(c->timer, kName, NESR_CLIP_TEXT_GROUP_FF, s, [&] { return launch_clip_act(g, s); });
        if ((rc = residual_rows(l.fc2, fc, c->inter, NESR_CLIP_TEXT_GROUP_FF))) return rc;
    }
    if ((rc = stats())) return rc;
    ClipFinal f;
    memset(&f, 0, sizeof(f));
    f.in = x, f.ln = ln, f.g = W + c->fin.g, f.b = W + c->fin.b, f.m = m, f.c = c->hidden, f.cs = hp, f.out = out;
    NESR_RUN(c->timer, kName, NESR_CLIP_TEXT_GROUP_NORM, s, [&] { return launch_clip_final(f, s); });
    return NESR_OK;
}

}  // namespace

extern "C" {

int nesr_clip_text_create(nesr_clip_text** out, int device_id, int vocab_size, int hidden_size, int intermediate_size, int num_hidden_layers,
                          int num_attention_heads, int max_position_embeddings, double layer_norm_eps, const char* hidden_act) {
    if (!out) return set_error(NESR_ERR_ARG, "nesr_clip_text_create: null out");
    *out = nullptr;
    if (!hidden_act) return set_error(NESR_ERR_ARG, "nesr_clip_text_create: null configuration argument");
    const std::string act = hidden_act;
    if (act != "gelu" && act != "quick_gelu") return unsupported(kCreate, "hidden_act", "'" + act + "' is not supported (gelu, quick_gelu)");
    if (vocab_size < 1) return unsupported(kCreate, "vocab_size", "must be positive");
    if (max_position_embeddings < 1) return unsupported(kCreate, "max_position_embeddings", "must be positive");
    if (num_hidden_layers < 1) return unsupported(kCreate, "num_hidden_layers", "must be positive");
    if (num_attention_heads < 1) return unsupported(kCreate, "num_attention_heads", "must be positive");
    if (hidden_size < 1 || hidden_size > CLIP_MAX_HIDDEN) return unsupported(kCreate, "hidden_size", "1 .. 1024, got " + std::to_string(hidden_size));
    if (hidden_size % num_attention_heads)
        return unsupported(kCreate, "num_attention_heads", std::to_string(hidden_size) + " (hidden_size) is no multiple of the " + std::to_string(num_attention_heads) + " heads");
    const int d = hidden_size / num_attention_heads;
    if (d < 8 || d > UNET_MAX_HEAD || d % 8)
        return unsupported(kCreate, "num_attention_heads", "a head width of " + std::to_string(d) + " (hidden_size " + std::to_string(hidden_size) + " / " +
                                                      std::to_string(num_attention_heads) + " heads): 8 .. 128 and a multiple of 8");
    if (intermediate_size < 1 || intermediate_size > CLIP_MAX_INTER) return unsupported(kCreate, "intermediate_size", "1 .. 4096, got " + std::to_string(intermediate_size));
    if (!(layer_norm_eps > 0) || !std::isfinite(layer_norm_eps)) return unsupported(kCreate, "layer_norm_eps", "must be positive and finite");
    for (size_t bytes : {unet_rows_lds_bytes(), clip_attn_lds_bytes()})
        if (bytes > VAE_LDS_LIMIT) return unsupported(kCreate, "hidden_size", "a kernel's LDS of " + std::to_string(bytes) + " bytes exceeds 160 KB");
    if (const int rc = check_device(device_id, NESR_CLIP_TEXT_NO_DEVICE)) return rc;
    nesr_clip_text* c = new nesr_clip_text();
    c->device = device_id, c->vocab = vocab_size, c->hidden = hidden_size, c->inter = intermediate_size, c->layers = num_hidden_layers;
    c->heads = num_attention_heads, c->positions = max_position_embeddings, c->eps = (float)layer_norm_eps;
    c->act = act == "gelu" ? CLIP_ACT_GELU : CLIP_ACT_QUICK_GELU;
    StateDict& sd = c->sd;
    const int64_t h = c->hidden, im = c->inter;
    sd.expect("embeddings.token_embedding.weight", {c->vocab, h});
    sd.expect("embeddings.position_embedding.weight", {c->positions, h});
    for (int i = 0; i < c->layers; ++i) {
        const std::string l = "encoder.layers." + std::to_string(i);
        for (const char* part : {".self_attn.k_proj", ".self_attn.v_proj", ".self_attn.q_proj", ".self_attn.out_proj"}) sd.expect_wb(l + part, {h, h});
        sd.expect_wb(l + ".layer_norm1", {h});
        sd.expect_wb(l + ".mlp.fc1", {im, h});
        sd.expect_wb(l + ".mlp.fc2", {h, im});
        sd.expect_wb(l + ".layer_norm2", {h});
    }
    sd.expect_wb("final_layer_norm", {h});
    *out = c;
    return NESR_OK;
}

void nesr_clip_text_destroy(nesr_clip_text* c) { net_destroy(c); }

int nesr_clip_text_num_tensors(const nesr_clip_text* c) { return net_num_tensors(c); }

int nesr_clip_text_load_weight(nesr_clip_text* c, const char* key, const float* data, const int64_t* shape, int ndim) {
    return net_load_weight(c, "nesr_clip_text_load_weight", key, data, shape, ndim, [](std::string& k) {
        if (k.compare(0, strlen(kPrefix), kPrefix) == 0) k = k.substr(strlen(kPrefix));
        return k != kPositionIds;      // positions count from 0 here; the buffer says nothing else
    });
}

int nesr_clip_text_finalize(nesr_clip_text* c) {
    if (const int rc = net_begin_finalize(c, "nesr_clip_text_finalize")) return rc;
    const StateDict& sd = c->sd;
    HostPack pk;
    const int h = c->hidden;
    c->tok = pk.vec(sd.data("embeddings.token_embedding.weight"));
    c->pos = pk.vec(sd.data("embeddings.position_embedding.weight"));
    c->layer.assign(c->layers, CLayerW());
    for (int i = 0; i < c->layers; ++i) {
        const std::string l = "encoder.layers." + std::to_string(i);
        CLayerW& w = c->layer[i];
        w.ln1 = pk.norm(sd, l + ".layer_norm1", h), w.ln2 = pk.norm(sd, l + ".layer_norm2", h);
        w.qkv = pk.side_by_side(sd, l, {".self_attn.q_proj", ".self_attn.k_proj", ".self_attn.v_proj"}, h, h);      // Wt[hp][3 hp]
        w.out = pk.linear(sd, l + ".self_attn.out_proj", h, h);
        w.fc1 = pk.linear(sd, l + ".mlp.fc1", c->inter, h);
        w.fc2 = pk.linear(sd, l + ".mlp.fc2", h, c->inter);
    }
    c->fin = pk.norm(sd, "final_layer_norm", h);
    return net_upload(c, "nesr_clip_text_finalize", pk, nullptr, kName);
}

int nesr_clip_text_workspace_bytes(nesr_clip_text* c, int n, int tokens, size_t* bytes) {
    if (!c || !bytes) return set_error(NESR_ERR_ARG, "nesr_clip_text_workspace_bytes: null pointer");
    const int rc = check_call(c, "nesr_clip_text_workspace_bytes", n, tokens);
    if (rc) return rc;
    *bytes = plan(c, n, tokens).total;
    return NESR_OK;
}

int nesr_clip_text_encode_f32(nesr_clip_text* c, const int32_t* ids_host, int n, int tokens, float* out_dev, size_t out_elems, void* stream) {
    const std::string e = "nesr_clip_text_encode_f32";
    if (!c || !ids_host || !out_dev) return set_error(NESR_ERR_ARG, e + ": null pointer");
    if (c->device == NESR_CLIP_TEXT_NO_DEVICE) return set_error(NESR_ERR_STATE, e + ": a context without a device launches nothing");
    if (!c->finalized) return set_error(NESR_ERR_STATE, e + ": weights not finalized (nesr_clip_text_finalize)");
    const int rc = check_call(c, e.c_str(), n, tokens);
    if (rc) return rc;
    for (int i = 0; i < n * tokens; ++i)
        if (ids_host[i] < 0 || ids_host[i] >= c->vocab)
            return set_error(NESR_ERR_ARG, e + ": id " + std::to_string(ids_host[i]) + " at position " + std::to_string(i % tokens) + " of sample " + std::to_string(i / tokens) +
                                               " is outside the table of " + std::to_string(c->vocab) + " (vocab_size)");
    const size_t need = (size_t)n * tokens * c->hidden;
    if (out_elems != need) return set_error(NESR_ERR_ARG, e + ": out_elems must be n tokens hidden_size = " + std::to_string(need) + ", got " + std::to_string(out_elems));
    NESR_TRY(hipSetDevice(c->device));
    return encode(c, ids_host, n, tokens, out_dev, static_cast<hipStream_t>(stream));
}

int nesr_clip_text_set_timing(nesr_clip_text* c, int enable) { return net_set_timing(c, "nesr_clip_text_set_timing", enable); }

int nesr_clip_text_kernel_time_ms(nesr_clip_text* c, double* group_ms, int n_groups, int64_t* launches) {
    return net_kernel_time_ms(c, "nesr_clip_text_kernel_time_ms", NESR_CLIP_TEXT_GROUPS, group_ms, n_groups, launches);
}

// ---- single-launch test hooks: device pointers in, the launcher's struct filled field for field, one launch, no context
int nesr_clip_text_k_embed(const int32_t* ids_host, int rows, int tokens, const float* tok_dev, int vocab, const float* pos_dev, int positions, int c, int cs,
                           float* out_dev, void* stream) {
    if (!ids_host || rows < 1 || rows > CLIP_MAX_IDS)
        return set_error(NESR_ERR_ARG, "nesr_clip_text_k_embed: rows must be 1 .. " + std::to_string(CLIP_MAX_IDS) + " with an id each; nothing was launched");
    ClipEmbed a;
    memset(&a, 0, sizeof(a));
    a.tok = tok_dev, a.pos = pos_dev, a.vocab = vocab, a.positions = positions, a.rows = rows, a.tokens = tokens, a.c = c, a.cs = cs, a.out = out_dev;
    for (int r = 0; r < rows; ++r) a.ids[r] = ids_host[r];
    return launch_done(launch_clip_embed(a, (hipStream_t)stream), "csrc/clip_text_api.h", "nesr_clip_text_k_embed", "launch_clip_embed");
}

int nesr_clip_text_k_attention(int samples, int tokens, int heads, int d, const float* q_dev, const float* k_dev, const float* v_dev, int ldq, int ldkv, int ldo,
                               float* out_dev, void* stream) {
    ClipAttn a{};
    a.samples = samples, a.tokens = tokens, a.heads = heads, a.d = d, a.q = q_dev, a.k = k_dev, a.v = v_dev, a.ldq = ldq, a.ldkv = ldkv, a.ldo = ldo, a.out = out_dev;
    return launch_done(launch_clip_attn(a, (hipStream_t)stream), "csrc/clip_text_api.h", "nesr_clip_text_k_attention", "launch_clip_attn");
}

}  // extern "C"

// what the x4 pipeline (sdx4_api.cpp) asks of a context it does not own
#include "sdx4_api.h"
nesr::Sdx4TextInfo nesr::sdx4_text_info(const nesr_clip_text* c) {
    return Sdx4TextInfo{c->device, c->hidden, c->positions, c->vocab, c->finalized, c->timer.launches};
}
