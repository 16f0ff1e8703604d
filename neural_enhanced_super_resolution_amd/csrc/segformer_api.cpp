// SegFormer contexts (nesr_segformer_*): strict weight loading, the BatchNorm fold and the transposed upload, the coefficient
// tables of PIL's resize, a workspace that grows on demand, and the forward as a chain of fused launches (segformer.hip,
// segformer_pre.hip).  Stands behind the reference's segmenter: AutoModelForImageSegmentation.from_pretrained and its extractor
// (nesr/nesr.py:285-301), and the part of _segment_and_enhance that runs them (nesr/nesr.py:701-716).
#include <cmath>
#include <cstring>
#include <map>
#include <tuple>

#include "net_context.h"
#include "segformer_api.h"

using namespace nesr;

namespace {

struct SegBlockW {
    size_t ln1g, ln1b, wq, bq, wsr, bsr, srg, srb, wkv, bkv, wo, bo, ln2g, ln2b, w1, b1, dww, dwb, w2, b2;
};
struct SegStageW {
    size_t wpe, bpe, peg, peb, lng, lnb, wproj, bproj;
    int kpe = 0, kpe_real = 0;
    std::vector<SegBlockW> blocks;
};

struct SegTable {
    int* d_bounds = nullptr;
    int* d_coef = nullptr;
    int ksize = 0;
};

const float kMean[3] = {0.485f, 0.456f, 0.406f};
const float kStd[3] = {0.229f, 0.224f, 0.225f};
constexpr int kModelSize = 512, kSegmentMax = 1024;
const char* const kName = "SegFormer";      // in the texts of a failed launch or workspace allocation

// ---- PIL's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) for one axis
double pil_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}
double pil_filter(int filter, double x) {
    if (filter == NESR_PIL_BILINEAR) {
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    }
    return (-3.0 <= x && x < 3.0) ? pil_sinc(x) * pil_sinc(x / 3.0) : 0.0;
}
void pil_table(int in, int out, int filter, std::vector<int>& bounds, std::vector<int>& coef, int& ksize) {
    bounds.assign((size_t)out * 2, 0);
    if (in == out) {      // the pass PIL skips, as a table: one tap of 1.0 gives the pixel back exactly
        ksize = 1;
        coef.assign(out, 1 << 22);
        for (int i = 0; i < out; ++i) bounds[2 * i] = i, bounds[2 * i + 1] = 1;
        return;
    }
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == NESR_PIL_BILINEAR ? 1.0 : 3.0) * fs;
    ksize = (int)std::ceil(support) * 2 + 1;
    coef.assign((size_t)out * ksize, 0);
    std::vector<double> w(ksize);
    const double ss = 1.0 / fs;
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = pil_filter(filter, (x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        for (int x = 0; x < n; ++x) {
            const double k = ww != 0.0 ? w[x] / ww : w[x];
            coef[(size_t)xx * ksize + x] = k < 0 ? (int)(-0.5 + k * (1 << 22)) : (int)(0.5 + k * (1 << 22));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
}

void free_table(SegTable& t) {
    if (t.d_bounds) (void)hipFree(t.d_bounds);
    if (t.d_coef) (void)hipFree(t.d_coef);
    t = SegTable();
}

int upload_table(int in, int out, int filter, SegTable& t) {
    std::vector<int> bounds, coef;
    pil_table(in, out, filter, bounds, coef, t.ksize);
    if (hipMalloc((void**)&t.d_bounds, bounds.size() * 4) != hipSuccess || hipMalloc((void**)&t.d_coef, coef.size() * 4) != hipSuccess) {
        free_table(t);
        return set_error(NESR_ERR_NOMEM, "allocating a resize table failed");
    }
    hipError_t e = hipMemcpy(t.d_bounds, bounds.data(), bounds.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t.d_coef, coef.data(), coef.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        free_table(t);
        return set_error(NESR_ERR_HIP, std::string("uploading a resize table: ") + hipGetErrorString(e));
    }
    return NESR_OK;
}

SegResample resample_args(const uint8_t* src, int h, int w, int c, int vertical, int out, const SegTable& t, uint8_t* dst, float* dst_f32) {
    SegResample a;
    memset(&a, 0, sizeof(a));
    a.src = src, a.h = h, a.w = w, a.c = c, a.vertical = vertical, a.out = out;
    a.bounds = t.d_bounds, a.coef = t.d_coef, a.ksize = t.ksize, a.dst = dst, a.dst_f32 = dst_f32;
    for (int i = 0; i < 3; ++i) a.mean[i] = kMean[i], a.stdv[i] = kStd[i];
    a.mean[3] = 0.f, a.stdv[3] = 1.f;
    return a;
}

}  // namespace

struct nesr_segformer : NetContext {
    int nin = 3, nst = 4, dec = 256, labels = 150, labels_p = 160;
    int depth[SEG_MAX_STAGES], sr[SEG_MAX_STAGES], hid[SEG_MAX_STAGES], patch[SEG_MAX_STAGES], stride[SEG_MAX_STAGES], heads[SEG_MAX_STAGES],
        mlp[SEG_MAX_STAGES];
    std::vector<SegStageW> stages;
    size_t wfuse = 0, bn_scale = 0, bn_shift = 0, wcls = 0, bcls = 0;
    char* pre = nullptr;                     // the pre-processing's images
    size_t pre_bytes = 0;
    std::map<std::tuple<int, int, int>, SegTable> tables;
};

namespace {

constexpr size_t kMaxTables = 16;      // one segment() needs at most four; a context fed many frame sizes starts over when full

int table_for(nesr_segformer* c, int in, int out, int filter, const SegTable** t) {
    const auto key = std::make_tuple(in, out, in == out ? 0 : filter);
    auto it = c->tables.find(key);
    if (it == c->tables.end()) {
        if (c->tables.size() >= kMaxTables) {      // launches that read the old tables may be in flight
            NESR_TRY(hipDeviceSynchronize());
            for (auto& kv : c->tables) free_table(kv.second);
            c->tables.clear();
        }
        SegTable nt;
        int rc = upload_table(in, out, filter, nt);
        if (rc) return rc;
        it = c->tables.emplace(key, nt).first;
    }
    *t = &it->second;
    return NESR_OK;
}

// transformers-4 checkpoint names -> transformers-5 names (transformers/conversion_mapping.py, "SegformerModel" and
// "SegformerForSemanticSegmentation"); a transformers-5 name comes back as it is
void replace_all(std::string& s, const std::string& from, const std::string& to) {
    for (size_t at = s.find(from); at != std::string::npos; at = s.find(from, at + to.size())) s.replace(at, from.size(), to);
}
// "<prefix><digits>." -> "stages.<digits>.<tail>"
void move_index(std::string& s, const std::string& prefix, const std::string& tail) {
    const size_t at = s.find(prefix);
    if (at == std::string::npos) return;
    size_t end = at + prefix.size();
    while (end < s.size() && s[end] >= '0' && s[end] <= '9') ++end;
    if (end == at + prefix.size() || end >= s.size() || s[end] != '.') return;
    const std::string digits = s.substr(at + prefix.size(), end - at - prefix.size());
    s.replace(at, end + 1 - at, "stages." + digits + "." + tail);
}
std::string seg_new_key(std::string k) {
    move_index(k, "encoder.patch_embeddings.", "patch_embeddings.");
    move_index(k, "encoder.block.", "blocks.");
    move_index(k, "encoder.layer_norm.", "layer_norm.");
    replace_all(k, "attention.self.query.", "attention.q_proj.");
    replace_all(k, "attention.self.key.", "attention.k_proj.");
    replace_all(k, "attention.self.value.", "attention.v_proj.");
    replace_all(k, "attention.self.sr.", "attention.sequence_reduction.sequence_reduction.");
    replace_all(k, "attention.self.layer_norm.", "attention.sequence_reduction.layer_norm.");
    replace_all(k, "attention.output.dense.", "attention.o_proj.");
    replace_all(k, "mlp.dense1.", "mlp.fc1.");
    replace_all(k, "mlp.dense2.", "mlp.fc2.");
    replace_all(k, ".layer_norm_1.", ".layernorm_before.");
    replace_all(k, ".layer_norm_2.", ".layernorm_after.");
    replace_all(k, "decode_head.linear_c.", "decode_head.linear_projections.");
    return k;
}

SegFused fused_zero() {
    SegFused a;
    memset(&a, 0, sizeof(a));
    return a;
}

// the token grid of every stage: a k x k conv of stride s with k / 2 padding, as torch sizes it
void stage_dims(int nst, const int* patch, const int* stride, int H, int W, int* sh, int* sw) {
    int h = H, w = W;
    for (int i = 0; i < nst; ++i) {
        const int k = patch[i], p = k / 2;
        h = (h + 2 * p - k) / stride[i] + 1;
        w = (w + 2 * p - k) / stride[i] + 1;
        sh[i] = h, sw[i] = w;
    }
}
void stage_dims(const nesr_segformer* c, int H, int W, int* sh, int* sw) { stage_dims(c->nst, c->patch, c->stride, H, W, sh, sw); }

struct SegWs {
    size_t x, xn, q, kv, h1, feat, proj[SEG_MAX_STAGES], total;
};

SegWs ws_layout(const nesr_segformer* c, const int* sh, const int* sw) {
    size_t x = 0, q = 0, kv = 0, h1 = 0;
    for (int i = 0; i < c->nst; ++i) {
        const size_t t = (size_t)sh[i] * sw[i], ch = c->hid[i];
        x = std::max(x, t * ch);
        q = std::max(q, t * ch * (c->sr[i] > 1 ? 1 : 3));
        if (c->sr[i] > 1) kv = std::max(kv, (size_t)(sh[i] / c->sr[i]) * (sw[i] / c->sr[i]) * 2 * ch);
        h1 = std::max(h1, t * ch * c->mlp[i]);
    }
    SegWs L;
    size_t off = 0;
    auto take = [&](size_t floats) {
        const size_t at = off;
        off = align_up(off + floats * 4, 256);
        return at;
    };
    L.x = take(x), L.xn = take(x), L.q = take(q), L.kv = take(std::max<size_t>(kv, 1)), L.h1 = take(h1), L.feat = take(x);
    for (int i = 0; i < c->nst; ++i) L.proj[i] = take((size_t)sh[i] * sw[i] * c->dec);
    L.total = off;
    return L;
}

// logits (NCHW f32) or class_map (u8), one of them
int forward(nesr_segformer* c, const float* x_dev, int H, int W, float* logits, uint8_t* class_map, hipStream_t s) {
    int sh[SEG_MAX_STAGES], sw[SEG_MAX_STAGES];
    stage_dims(c, H, W, sh, sw);
    const SegWs L = ws_layout(c, sh, sw);
    int rc = grow(c->ws_buf, c->ws_bytes, L.total, kName);
    if (rc) return rc;
    auto buf = [&](size_t off) { return reinterpret_cast<float*>(c->ws_buf + off); };
    auto wt = [&](size_t off) { return c->d_w + off; };
    float* X = buf(L.x);
    float* XN = buf(L.xn);
    float* Q = buf(L.q);
    float* KV = buf(L.kv);
    float* H1 = buf(L.h1);
    float* FEAT = buf(L.feat);

    for (int i = 0; i < c->nst; ++i) {
        const SegStageW& S = c->stages[i];
        const int C = c->hid[i], T = sh[i] * sw[i], sr = c->sr[i], hidden = C * c->mlp[i];
        {   // patch embed: conv + bias + LayerNorm -> X
            SegFused a = fused_zero();
            a.a_mode = SEG_A_CONV, a.m = T;
            a.in = i == 0 ? x_dev : FEAT;
            a.nchw = i == 0, a.in_h = i == 0 ? H : sh[i - 1], a.in_w = i == 0 ? W : sw[i - 1], a.in_c = i == 0 ? c->nin : c->hid[i - 1];
            a.ksz = c->patch[i], a.stride = c->stride[i], a.pad = c->patch[i] / 2, a.out_w = sw[i];
            a.k1 = S.kpe, a.k1_real = S.kpe_real, a.n1 = C;
            a.w1 = wt(S.wpe), a.bias1 = wt(S.bpe), a.ln_g = wt(S.peg), a.ln_b = wt(S.peb), a.out1 = X;
            NESR_RUN(c->timer, kName, NESR_SEG_GROUP_PATCH_EMBED, s, [&] { return launch_seg_fused(a, s); });
        }
        for (const SegBlockW& B : S.blocks) {
            {   // LayerNorm + q (sr > 1: the normalised rows go on to the reduction) | LayerNorm + q, k, v
                SegFused a = fused_zero();
                a.a_mode = SEG_A_ROWS, a.m = T, a.in = X, a.n1 = C, a.ln_g = wt(B.ln1g), a.ln_b = wt(B.ln1b);
                a.out1 = sr > 1 ? XN : nullptr;
                a.w2 = wt(B.wq), a.bias2 = wt(B.bq), a.n2 = sr > 1 ? C : 3 * C, a.ldw2 = a.n2, a.out_mode = SEG_OUT_ROWS, a.out2 = Q, a.ld_out2 = a.n2;
                NESR_RUN(c->timer, kName, NESR_SEG_GROUP_LN_PROJ, s, [&] { return launch_seg_fused(a, s); });
            }
            int keys = T;
            if (sr > 1) {   // sr x sr / stride sr conv + bias + LayerNorm, then k | v
                keys = (sh[i] / sr) * (sw[i] / sr);
                SegFused a = fused_zero();
                a.a_mode = SEG_A_CONV, a.m = keys, a.in = XN, a.nchw = 0, a.in_h = sh[i], a.in_w = sw[i], a.in_c = C;
                a.ksz = sr, a.stride = sr, a.pad = 0, a.out_w = sw[i] / sr, a.k1 = a.k1_real = C * sr * sr, a.n1 = C;
                a.w1 = wt(B.wsr), a.bias1 = wt(B.bsr), a.ln_g = wt(B.srg), a.ln_b = wt(B.srb);
                a.w2 = wt(B.wkv), a.bias2 = wt(B.bkv), a.n2 = 2 * C, a.ldw2 = 2 * C, a.out_mode = SEG_OUT_ROWS, a.out2 = KV, a.ld_out2 = 2 * C;
                NESR_RUN(c->timer, kName, NESR_SEG_GROUP_SEQ_REDUCTION, s, [&] { return launch_seg_fused(a, s); });
            }
            {   // attention + o_proj + residual, X in place
                SegAttn a;
                memset(&a, 0, sizeof(a));
                a.m = T, a.keys = keys, a.heads = c->heads[i], a.c = C;
                a.q = Q, a.q_ld = sr > 1 ? C : 3 * C;
                a.k = sr > 1 ? KV : Q + C, a.v = sr > 1 ? KV + C : Q + 2 * C, a.kv_ld = sr > 1 ? 2 * C : 3 * C;
                a.wo = wt(B.wo), a.bo = wt(B.bo), a.x = X;
                NESR_RUN(c->timer, kName, NESR_SEG_GROUP_ATTENTION, s, [&] { return launch_seg_attn(a, s); });
            }
            {   // LayerNorm + fc1 -> H1
                SegFused a = fused_zero();
                a.a_mode = SEG_A_ROWS, a.m = T, a.in = X, a.n1 = C, a.ln_g = wt(B.ln2g), a.ln_b = wt(B.ln2b);
                a.w2 = wt(B.w1), a.bias2 = wt(B.b1), a.n2 = hidden, a.ldw2 = hidden, a.out_mode = SEG_OUT_ROWS, a.out2 = H1, a.ld_out2 = hidden;
                NESR_RUN(c->timer, kName, NESR_SEG_GROUP_LN_PROJ, s, [&] { return launch_seg_fused(a, s); });
            }
            {   // gelu(dwconv3x3(H1)) x fc2 + bias + residual, X in place
                SegFused a = fused_zero();
                a.a_mode = SEG_A_DWGELU, a.m = T, a.in = H1, a.k1 = hidden, a.n1 = C, a.gh = sh[i], a.gw = sw[i];
                a.dw_w = wt(B.dww), a.dw_b = wt(B.dwb), a.w1 = wt(B.w2), a.bias1 = wt(B.b2), a.res = X, a.out1 = X;
                NESR_RUN(c->timer, kName, NESR_SEG_GROUP_MIX_FFN, s, [&] { return launch_seg_fused(a, s); });
            }
        }
        {   // the stage's LayerNorm -> FEAT (the next stage's image), and the decode head's projection of it
            SegFused a = fused_zero();
            a.a_mode = SEG_A_ROWS, a.m = T, a.in = X, a.n1 = C, a.ln_g = wt(S.lng), a.ln_b = wt(S.lnb);
            a.out1 = i + 1 < c->nst ? FEAT : nullptr;
            a.w2 = wt(S.wproj), a.bias2 = wt(S.bproj), a.n2 = c->dec, a.ldw2 = c->dec, a.out_mode = SEG_OUT_ROWS, a.out2 = buf(L.proj[i]), a.ld_out2 = c->dec;
            NESR_RUN(c->timer, kName, NESR_SEG_GROUP_DECODE_HEAD, s, [&] { return launch_seg_fused(a, s); });
        }
    }
    {   // upsample + concatenate + linear_fuse + BatchNorm + ReLU + classifier (+ argmax)
        SegFused a = fused_zero();
        a.a_mode = SEG_A_DECODE, a.m = sh[0] * sw[0], a.k1 = c->nst * c->dec, a.n1 = c->dec, a.nstage = c->nst, a.dec = c->dec;
        for (int i = 0; i < c->nst; ++i) a.proj[i] = buf(L.proj[i]), a.sh[i] = sh[i], a.sw[i] = sw[i];
        for (int i = c->nst; i < SEG_MAX_STAGES; ++i) a.proj[i] = a.proj[0], a.sh[i] = sh[0], a.sw[i] = sw[0];
        a.w1 = wt(c->wfuse), a.bn_scale = wt(c->bn_scale), a.bn_shift = wt(c->bn_shift);
        a.w2 = wt(c->wcls), a.bias2 = wt(c->bcls), a.n2 = c->labels, a.ldw2 = c->labels_p;
        a.out_mode = class_map ? SEG_OUT_ARGMAX : SEG_OUT_NCHW, a.out2 = logits, a.ld_out2 = a.m, a.out2_u8 = class_map;
        NESR_RUN(c->timer, kName, NESR_SEG_GROUP_DECODE_HEAD, s, [&] { return launch_seg_fused(a, s); });
    }
    return NESR_OK;
}

// the reference's resizes and the extractor's normalisation: rgb [H][W][3] -> pix [3][512][512]
int preprocess(nesr_segformer* c, const uint8_t* rgb, int H, int W, float* pix, hipStream_t s) {
    int h = H, w = W;
    const bool big = std::max(H, W) > kSegmentMax;
    int nh = H, nw = W;
    if (big) {
        const double scale = (double)kSegmentMax / (double)std::max(W, H);
        nw = (int)(W * scale), nh = (int)(H * scale);
        if (nw < 1 || nh < 1) return set_error(NESR_ERR_ARG, "segment: the frame's shorter side vanishes at 1024 pixels (PIL refuses that resize too)");
    }
    const size_t a_bytes = big ? align_up((size_t)H * nw * 3, 256) : 0, b_bytes = big ? align_up((size_t)nh * nw * 3, 256) : 0;
    const size_t c_bytes = align_up((size_t)nh * kModelSize * 3, 256);
    int rc = grow(c->pre, c->pre_bytes, a_bytes + b_bytes + c_bytes, kName);
    if (rc) return rc;
    uint8_t* ta = reinterpret_cast<uint8_t*>(c->pre);
    uint8_t* tb = ta + a_bytes;
    uint8_t* tc = tb + b_bytes;
    const uint8_t* cur = rgb;
    const SegTable* t = nullptr;
    if (big) {      // pil_image.resize(new_size, Image.LANCZOS), nesr/nesr.py:709
        if (nw != w) {
            if ((rc = table_for(c, w, nw, NESR_PIL_LANCZOS, &t))) return rc;
            const SegResample a = resample_args(cur, h, w, 3, 0, nw, *t, ta, nullptr);
            NESR_RUN(c->timer, kName, NESR_SEG_GROUP_PREPROCESS, s, [&] { return launch_seg_resample(a, s); });
            cur = ta, w = nw;
        }
        if (nh != h) {
            if ((rc = table_for(c, h, nh, NESR_PIL_LANCZOS, &t))) return rc;
            const SegResample a = resample_args(cur, h, w, 3, 1, nh, *t, tb, nullptr);
            NESR_RUN(c->timer, kName, NESR_SEG_GROUP_PREPROCESS, s, [&] { return launch_seg_resample(a, s); });
            cur = tb, h = nh;
        }
    }
    if (w != kModelSize) {      // the extractor's resize to 512 x 512, PIL BILINEAR
        if ((rc = table_for(c, w, kModelSize, NESR_PIL_BILINEAR, &t))) return rc;
        const SegResample a = resample_args(cur, h, w, 3, 0, kModelSize, *t, tc, nullptr);
        NESR_RUN(c->timer, kName, NESR_SEG_GROUP_PREPROCESS, s, [&] { return launch_seg_resample(a, s); });
        cur = tc, w = kModelSize;
    }
    if ((rc = table_for(c, h, kModelSize, NESR_PIL_BILINEAR, &t))) return rc;      // h == 512: the one-tap table, the normalisation alone
    const SegResample a = resample_args(cur, h, w, 3, 1, kModelSize, *t, nullptr, pix);
    NESR_RUN(c->timer, kName, NESR_SEG_GROUP_PREPROCESS, s, [&] { return launch_seg_resample(a, s); });
    return NESR_OK;
}

int check_frame(const nesr_segformer* c, const void* p, int H, int W, const void* out, const char* what) {
    if (!c || !p || !out) return set_error(NESR_ERR_ARG, std::string(what) + ": null pointer");
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 28)) return set_error(NESR_ERR_ARG, std::string(what) + ": a frame of 1 .. 2^28 pixels");
    if (!c->finalized) return set_error(NESR_ERR_STATE, std::string(what) + ": weights not finalized (nesr_segformer_finalize)");
    if (c->nin != 3) return set_error(NESR_ERR_ARG, std::string(what) + ": an RGB frame needs num_channels = 3");
    return NESR_OK;
}

}  // namespace

extern "C" {

int nesr_segformer_create(nesr_segformer** out, int device_id, int num_channels, int num_encoder_blocks, const int* depths, const int* sr_ratios,
                          const int* hidden_sizes, const int* patch_sizes, const int* strides, const int* num_attention_heads,
                          const int* mlp_ratios, int decoder_hidden_size, int num_labels) {
    if (!out) return set_error(NESR_ERR_ARG, "nesr_segformer_create: null out");
    *out = nullptr;
    if (!depths || !sr_ratios || !hidden_sizes || !patch_sizes || !strides || !num_attention_heads || !mlp_ratios)
        return set_error(NESR_ERR_ARG, "nesr_segformer_create: null configuration array");
    if (num_encoder_blocks < 1 || num_encoder_blocks > SEG_MAX_STAGES)
        return set_error(NESR_ERR_ARG, "nesr_segformer_create: num_encoder_blocks must be 1 .. " + std::to_string(SEG_MAX_STAGES));
    if (num_channels != 3) return set_error(NESR_ERR_ARG, "nesr_segformer_create: num_channels must be 3");
    if (decoder_hidden_size < 32 || decoder_hidden_size > SEG_MAX_C || decoder_hidden_size % 32)
        return set_error(NESR_ERR_ARG, "nesr_segformer_create: decoder_hidden_size must be a multiple of 32 up to 256");
    if (num_labels < 1 || num_labels > SEG_MAX_C) return set_error(NESR_ERR_ARG, "nesr_segformer_create: num_labels must be 1 .. 256");
    for (int i = 0; i < num_encoder_blocks; ++i) {
        const std::string at = " (stage " + std::to_string(i) + ")";
        if (depths[i] < 1 || depths[i] > 64 || sr_ratios[i] < 1 || sr_ratios[i] > 16 || hidden_sizes[i] < 1 || patch_sizes[i] < 1 || patch_sizes[i] > 15 ||
            strides[i] < 1 || strides[i] > 8 || num_attention_heads[i] < 1 || mlp_ratios[i] < 1 || mlp_ratios[i] > 8)
            return set_error(NESR_ERR_ARG, "nesr_segformer_create: a size of the configuration is not positive or out of range" + at);
        if (hidden_sizes[i] != 32 * num_attention_heads[i])
            return set_error(NESR_ERR_ARG, "nesr_segformer_create: the head dimension hidden_sizes / num_attention_heads must be 32 (SegFormer-B0; "
                                           "B1-B5 have 64 and are not supported)" + at);
        if (hidden_sizes[i] > SEG_MAX_C) return set_error(NESR_ERR_ARG, "nesr_segformer_create: hidden_sizes must not exceed 256" + at);
    }
    int ndev = 0;
    NESR_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return set_error(NESR_ERR_ARG, "no such device " + std::to_string(device_id));
    nesr_segformer* c = new nesr_segformer();
    c->device = device_id, c->nin = num_channels, c->nst = num_encoder_blocks, c->dec = decoder_hidden_size, c->labels = num_labels;
    c->labels_p = round_up(num_labels, 32);
    for (int i = 0; i < SEG_MAX_STAGES; ++i) {
        const int j = i < c->nst ? i : 0;
        c->depth[i] = depths[j], c->sr[i] = sr_ratios[j], c->hid[i] = hidden_sizes[j], c->patch[i] = patch_sizes[j], c->stride[i] = strides[j];
        c->heads[i] = num_attention_heads[j], c->mlp[i] = mlp_ratios[j];
    }
    StateDict& sd = c->sd;
    int cin = c->nin;
    for (int i = 0; i < c->nst; ++i) {
        const std::string s = "segformer.stages." + std::to_string(i);
        const int64_t ch = c->hid[i], k = c->patch[i], sr = c->sr[i], hidden = ch * c->mlp[i];
        sd.expect_wb(s + ".patch_embeddings.proj", {ch, cin, k, k});
        sd.expect_wb(s + ".patch_embeddings.layer_norm", {ch});
        for (int j = 0; j < c->depth[i]; ++j) {
            const std::string b = s + ".blocks." + std::to_string(j);
            sd.expect_wb(b + ".layernorm_before", {ch});
            for (const char* p : {"q_proj", "k_proj", "v_proj", "o_proj"}) sd.expect_wb(b + ".attention." + p, {ch, ch});
            if (sr > 1) {
                sd.expect_wb(b + ".attention.sequence_reduction.sequence_reduction", {ch, ch, sr, sr});
                sd.expect_wb(b + ".attention.sequence_reduction.layer_norm", {ch});
            }
            sd.expect_wb(b + ".layernorm_after", {ch});
            sd.expect_wb(b + ".mlp.fc1", {hidden, ch});
            sd.expect_wb(b + ".mlp.dwconv.dwconv", {hidden, 1, 3, 3});
            sd.expect_wb(b + ".mlp.fc2", {ch, hidden});
        }
        sd.expect_wb(s + ".layer_norm", {ch});
        cin = (int)ch;
    }
    const int64_t d = c->dec;
    for (int i = 0; i < c->nst; ++i) sd.expect_wb("decode_head.linear_projections." + std::to_string(i) + ".proj", {d, c->hid[i]});
    sd.expect("decode_head.linear_fuse.weight", {d, d * c->nst, 1, 1});
    sd.expect_wb("decode_head.batch_norm", {d});
    sd.expect("decode_head.batch_norm.running_mean", {d});
    sd.expect("decode_head.batch_norm.running_var", {d});
    sd.expect_wb("decode_head.classifier", {c->labels, d, 1, 1});
    *out = c;
    return NESR_OK;
}

void nesr_segformer_destroy(nesr_segformer* c) {
    if (c) {      // the tables and the pre-processing's images, once the device's work is done; the rest is the base's
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        for (auto& kv : c->tables) free_table(kv.second);
        if (c->pre) (void)hipFree(c->pre);
    }
    net_destroy(c);
}

int nesr_segformer_num_tensors(const nesr_segformer* c) { return net_num_tensors(c); }

int nesr_segformer_load_weight(nesr_segformer* c, const char* key, const float* data, const int64_t* shape, int ndim) {
    return net_load_weight(c, "nesr_segformer_load_weight", key, data, shape, ndim, [](std::string& k) {
        k = seg_new_key(k);
        return k != "decode_head.batch_norm.num_batches_tracked";
    });
}

int nesr_segformer_finalize(nesr_segformer* c) {
    if (const int rc = net_begin_finalize(c, "nesr_segformer_finalize")) return rc;
    const StateDict& sd = c->sd;

    HostPack pk;
    auto vec = [&](const std::string& key) { return pk.vec(sd.data(key)); };
    auto linear = [&](const std::string& name, int n, int k) {
        const size_t at = pk.reserve((size_t)k * n);
        pk.transpose_into(at, sd.data(name + ".weight"), n, k, n, 0);
        return at;
    };

    c->stages.assign(c->nst, SegStageW());
    int cin = c->nin;
    for (int i = 0; i < c->nst; ++i) {
        SegStageW& S = c->stages[i];
        const std::string s = "segformer.stages." + std::to_string(i);
        const int C = c->hid[i], ks = c->patch[i], sr = c->sr[i], hidden = C * c->mlp[i];
        S.kpe_real = cin * ks * ks;
        S.kpe = round_up(S.kpe_real, 32);
        if (i == 0) {      // the NCHW image: torch's own (c, ky, kx) order, zero rows up to a multiple of 32
            S.wpe = pk.reserve((size_t)S.kpe * C);
            pk.transpose_into(S.wpe, sd.data(s + ".patch_embeddings.proj.weight"), C, S.kpe_real, C, 0);
        } else {
            S.wpe = pk.conv_taps(sd.data(s + ".patch_embeddings.proj.weight"), C, cin, ks * ks, cin, C);      // [(ky * ks + kx) * cin + c][C]
        }
        S.bpe = vec(s + ".patch_embeddings.proj.bias");
        S.peg = vec(s + ".patch_embeddings.layer_norm.weight");
        S.peb = vec(s + ".patch_embeddings.layer_norm.bias");
        S.blocks.assign(c->depth[i], SegBlockW());
        for (int j = 0; j < c->depth[i]; ++j) {
            SegBlockW& B = S.blocks[j];
            const std::string b = s + ".blocks." + std::to_string(j), at = b + ".attention.";
            B.ln1g = vec(b + ".layernorm_before.weight");
            B.ln1b = vec(b + ".layernorm_before.bias");
            auto concat = [&](std::initializer_list<const char*> names, size_t& w_at, size_t& b_at) {
                const int n = (int)names.size() * C;
                w_at = pk.reserve((size_t)C * n);
                b_at = pk.reserve(n);
                int col = 0;
                for (const char* p : names) {
                    pk.transpose_into(w_at, sd.data(at + p + ".weight"), C, C, n, col);
                    const std::vector<float>& bias = sd.data(at + p + ".bias");
                    std::copy(bias.begin(), bias.end(), pk.host.begin() + b_at + col);
                    col += C;
                }
            };
            if (sr > 1) {
                concat({"q_proj"}, B.wq, B.bq);
                B.wsr = pk.conv_taps(sd.data(at + "sequence_reduction.sequence_reduction.weight"), C, C, sr * sr, C, C);
                B.bsr = vec(at + "sequence_reduction.sequence_reduction.bias");
                B.srg = vec(at + "sequence_reduction.layer_norm.weight");
                B.srb = vec(at + "sequence_reduction.layer_norm.bias");
                concat({"k_proj", "v_proj"}, B.wkv, B.bkv);
            } else {
                concat({"q_proj", "k_proj", "v_proj"}, B.wq, B.bq);
            }
            B.wo = linear(at + "o_proj", C, C);
            B.bo = vec(at + "o_proj.bias");
            B.ln2g = vec(b + ".layernorm_after.weight");
            B.ln2b = vec(b + ".layernorm_after.bias");
            B.w1 = linear(b + ".mlp.fc1", hidden, C);
            B.b1 = vec(b + ".mlp.fc1.bias");
            B.dww = pk.conv_taps(sd.data(b + ".mlp.dwconv.dwconv.weight"), hidden, 1, 9, 1, hidden);      // [hidden][1][3][3] -> [tap][hidden]
            B.dwb = vec(b + ".mlp.dwconv.dwconv.bias");
            B.w2 = linear(b + ".mlp.fc2", C, hidden);
            B.b2 = vec(b + ".mlp.fc2.bias");
        }
        S.lng = vec(s + ".layer_norm.weight");
        S.lnb = vec(s + ".layer_norm.bias");
        const std::string p = "decode_head.linear_projections." + std::to_string(i) + ".proj";
        S.wproj = linear(p, c->dec, C);
        S.bproj = vec(p + ".bias");
        cin = C;
    }
    const int D = c->dec;
    c->wfuse = linear("decode_head.linear_fuse", D, D * c->nst);
    c->bn_scale = pk.reserve(D);
    c->bn_shift = pk.reserve(D);
    {      // BatchNorm in eval mode: y = (x - mean) / sqrt(var + eps) * g + b = x * scale + shift
        const std::string bn = "decode_head.batch_norm.";
        const std::vector<float>&g = sd.data(bn + "weight"), &b = sd.data(bn + "bias"), &m = sd.data(bn + "running_mean"), &v = sd.data(bn + "running_var");
        for (int i = 0; i < D; ++i) {
            const double sc = (double)g[i] / std::sqrt((double)v[i] + 1e-5);
            pk.host[c->bn_scale + i] = (float)sc;
            pk.host[c->bn_shift + i] = (float)((double)b[i] - (double)m[i] * sc);
        }
    }
    c->wcls = pk.reserve((size_t)D * c->labels_p);
    pk.transpose_into(c->wcls, sd.data("decode_head.classifier.weight"), c->labels, D, c->labels_p, 0);
    c->bcls = pk.vec(sd.data("decode_head.classifier.bias"), c->labels_p);
    return net_upload(c, "nesr_segformer_finalize", pk, nullptr, nullptr);      // no model name in the allocation text
}

int nesr_segformer_output_size(int num_encoder_blocks, const int* patch_sizes, const int* strides, int H, int W, int* out_h, int* out_w) {
    if (!patch_sizes || !strides || !out_h || !out_w) return set_error(NESR_ERR_ARG, "nesr_segformer_output_size: null pointer");
    if (num_encoder_blocks < 1 || num_encoder_blocks > SEG_MAX_STAGES)
        return set_error(NESR_ERR_ARG, "nesr_segformer_output_size: num_encoder_blocks must be 1 .. " + std::to_string(SEG_MAX_STAGES));
    for (int i = 0; i < num_encoder_blocks; ++i)
        if (patch_sizes[i] < 1 || patch_sizes[i] > 15 || strides[i] < 1 || strides[i] > 8)
            return set_error(NESR_ERR_ARG, "nesr_segformer_output_size: patch_sizes must be 1 .. 15 and strides 1 .. 8");
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 26)) return set_error(NESR_ERR_ARG, "nesr_segformer_output_size: an input of 1 .. 2^26 pixels");
    int sh[SEG_MAX_STAGES], sw[SEG_MAX_STAGES];
    stage_dims(num_encoder_blocks, patch_sizes, strides, H, W, sh, sw);
    *out_h = sh[0], *out_w = sw[0];
    return NESR_OK;
}

int nesr_segformer_forward_f32(nesr_segformer* c, const float* x, int N, int C, int H, int W, float* logits, void* stream) {
    if (!c || !x || !logits) return set_error(NESR_ERR_ARG, "nesr_segformer_forward_f32: null pointer");
    if (!c->finalized) return set_error(NESR_ERR_STATE, "nesr_segformer_forward_f32: weights not finalized (nesr_segformer_finalize)");
    if (N != 1 || C != c->nin) return set_error(NESR_ERR_ARG, "nesr_segformer_forward_f32: expected [1, " + std::to_string(c->nin) + ", H, W]");
    if (H < 32 || W < 32 || H % 32 || W % 32 || (long long)H * W > (1ll << 26))
        return set_error(NESR_ERR_ARG, "nesr_segformer_forward_f32: H and W must be multiples of 32 (H W <= 2^26), got " + std::to_string(H) + " x " +
                                           std::to_string(W));
    NESR_TRY(hipSetDevice(c->device));
    return forward(c, x, H, W, logits, nullptr, static_cast<hipStream_t>(stream));
}

int nesr_segformer_preprocess_u8(nesr_segformer* c, const uint8_t* rgb, int H, int W, float* pix, void* stream) {
    int rc = check_frame(c, rgb, H, W, pix, "nesr_segformer_preprocess_u8");
    if (rc) return rc;
    NESR_TRY(hipSetDevice(c->device));
    return preprocess(c, rgb, H, W, pix, static_cast<hipStream_t>(stream));
}

int nesr_segformer_segment_u8(nesr_segformer* c, const uint8_t* rgb, int H, int W, uint8_t* class_map, size_t capacity, int* out_h, int* out_w,
                              void* stream) {
    int rc = check_frame(c, rgb, H, W, class_map, "nesr_segformer_segment_u8");
    if (rc) return rc;
    int sh[SEG_MAX_STAGES], sw[SEG_MAX_STAGES];
    stage_dims(c, kModelSize, kModelSize, sh, sw);
    if (capacity < (size_t)sh[0] * sw[0])
        return set_error(NESR_ERR_ARG, "nesr_segformer_segment_u8: the class map needs " + std::to_string(sh[0] * sw[0]) + " bytes");
    NESR_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t pix_bytes = (size_t)3 * kModelSize * kModelSize * 4;
    // the network's input lives at the head of the network's workspace region of its own: grown here, kept by forward
    static_assert(kModelSize % 32 == 0, "the model size is a legal forward size");
    const SegWs L = ws_layout(c, sh, sw);
    if ((rc = grow(c->ws_buf, c->ws_bytes, L.total + pix_bytes, kName))) return rc;
    float* pix = reinterpret_cast<float*>(c->ws_buf + L.total);
    if ((rc = preprocess(c, rgb, H, W, pix, s))) return rc;
    if ((rc = forward(c, pix, kModelSize, kModelSize, nullptr, class_map, s))) return rc;
    if (out_h) *out_h = sh[0];
    if (out_w) *out_w = sw[0];
    return NESR_OK;
}

int nesr_segformer_set_timing(nesr_segformer* c, int enable) { return net_set_timing(c, "nesr_segformer_set_timing", enable); }

int nesr_segformer_kernel_time_ms(nesr_segformer* c, double* group_ms, int n_groups, int64_t* launches) {
    return net_kernel_time_ms(c, "nesr_segformer_kernel_time_ms", NESR_SEG_GROUPS, group_ms, n_groups, launches);
}

int nesr_pil_resize_u8(int device_id, const uint8_t* src, int H, int W, int C, uint8_t* dst, int out_h, int out_w, int filter, void* stream) {
    if (!src || !dst) return set_error(NESR_ERR_ARG, "nesr_pil_resize_u8: null pointer");
    if (H < 1 || W < 1 || C < 1 || C > 4 || out_h < 1 || out_w < 1 || (long long)H * W > (1ll << 28) || (long long)out_h * out_w > (1ll << 28))
        return set_error(NESR_ERR_ARG, "nesr_pil_resize_u8: [H, W, C] with C = 1 .. 4 and sizes of 1 .. 2^28 pixels");
    if (filter != NESR_PIL_LANCZOS && filter != NESR_PIL_BILINEAR)
        return set_error(NESR_ERR_ARG, "nesr_pil_resize_u8: filter must be NESR_PIL_LANCZOS (1) or NESR_PIL_BILINEAR (2)");
    int ndev = 0;
    NESR_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return set_error(NESR_ERR_ARG, "no such device " + std::to_string(device_id));
    NESR_TRY(hipSetDevice(device_id));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (out_h == H && out_w == W) {
        NESR_TRY(hipMemcpyAsync(dst, src, (size_t)H * W * C, hipMemcpyDeviceToDevice, s));
        NESR_TRY(hipStreamSynchronize(s));      // as the resampling route: the entry returns with dst written
        return NESR_OK;
    }
    SegTable th, tv;
    uint8_t* mid = nullptr;
    int rc = NESR_OK;
    hipError_t e = hipSuccess;
    const bool hp = out_w != W, vp = out_h != H;
    if (hp) rc = upload_table(W, out_w, filter, th);
    if (!rc && vp) rc = upload_table(H, out_h, filter, tv);
    if (!rc && hp && vp && hipMalloc((void**)&mid, (size_t)H * out_w * C) != hipSuccess) rc = set_error(NESR_ERR_NOMEM, "nesr_pil_resize_u8: allocation failed");
    if (!rc && hp) e = launch_seg_resample(resample_args(src, H, W, C, 0, out_w, th, vp ? mid : dst, nullptr), s);
    if (!rc && e == hipSuccess && vp) e = launch_seg_resample(resample_args(hp ? mid : src, H, hp ? out_w : W, C, 1, out_h, tv, dst, nullptr), s);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
    free_table(th);
    free_table(tv);
    if (mid) (void)hipFree(mid);
    if (rc) return rc;
    NESR_TRY(e);
    return NESR_OK;
}

}  // extern "C"
