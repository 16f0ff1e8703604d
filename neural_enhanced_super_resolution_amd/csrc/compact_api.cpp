// SRVGGNetCompact contexts (nesr_create_compact): strict weight loading + repacking, workspace, and the forward as one launch
// per layer (srvgg_compact.hip).  Stands behind upstream realesrgan/archs/srvgg_arch.py SRVGGNetCompact.__init__ / forward and
// RealESRGANer's load_state_dict for the realesr-general-x4v3 / realesr-animevideov3 checkpoints (the reference's fetcher,
// standalone/download-x3-model.py:77-116).  The context entries of nesr_api.cpp hand a compact context's calls on to these.
#include <cmath>

#include "api_common.h"
#include "compact_api.h"

using namespace nesr;

namespace {

struct CLayer {
    int cin = 0, cout = 0, cin_p = 0, ncb = 0;
    std::vector<float> w, b;
    bool has_w = false, has_b = false;
};

}  // namespace

struct nesr_compact {
    int device = 0, nin = 3, nout = 3, nf = 64, nconv = 16, up = 4, act = NESR_ACT_PRELU, dtype = NESR_DTYPE_F32_SPLIT;
    int cus = 256;
    std::vector<CLayer> conv;                         // body.0, body.2, ..., body.2(nconv+1)
    std::vector<std::vector<float>> slope;            // PReLU slopes of body.1, body.3, ... (prelu only)
    std::vector<bool> has_slope;
    bool finalized = false;
    char* d_weights = nullptr;                        // per conv: packed weights | bias [ncb*16]; then slopes [nconv+1][64]
    std::vector<size_t> w_off, b_off;
    size_t slope_off = 0;
    char* ws = nullptr;
    size_t ws_bytes = 0;
    unsigned* d_status = nullptr;                     // [0] range word of the forward in flight, [3] latched from an unchecked earlier one
    unsigned* h_status = nullptr;
    EventTimer timer;                                 // kernel timing hook

    bool split() const { return dtype == NESR_DTYPE_F32_SPLIT; }
    bool f16() const { return dtype == NESR_DTYPE_F16; }
    bool ranged() const { return split() || f16(); }     // the forms whose values end at +-65504: they keep the range word
    int form() const { return split() ? COMPACT_SPLIT : (f16() ? COMPACT_F16 : COMPACT_BF16); }
    size_t esize() const { return split() ? 4 : 2; }
    const char* form_name() const { return f16() ? "f16 form" : "f16-pair fp32 form"; }
};

namespace {

struct CWs { size_t act0, a, b, res, total; };

CWs ws_layout(const nesr_compact* c, int N, int H, int W) {
    const size_t px = (size_t)N * H * W;
    CWs L;
    L.act0 = 0;
    L.a = align_up(px * 32 * c->esize(), 256);
    L.b = L.a + align_up(px * 64 * c->esize(), 256);
    L.res = L.b + align_up(px * 64 * c->esize(), 256);
    L.total = L.res + align_up(px * 16, 256);
    return L;
}

int ensure_ws(nesr_compact* c, size_t bytes) { return grow(c->ws, c->ws_bytes, bytes, nullptr); }

}  // namespace

namespace nesr {

int compact_create(nesr_compact** out, int device, int num_in_ch, int num_out_ch, int num_feat, int num_conv, int upscale, int act_type,
                   int dtype) {
    *out = nullptr;
    if (num_feat != 64) return set_error(NESR_ERR_ARG, "nesr_create_compact: num_feat must be 64 (realesr-general-x4v3, realesr-animevideov3)");
    if (num_in_ch != 3 || num_out_ch != 3) return set_error(NESR_ERR_ARG, "nesr_create_compact: num_in_ch and num_out_ch must be 3");
    if (upscale != 2 && upscale != 4) return set_error(NESR_ERR_ARG, "nesr_create_compact: upscale must be 2 or 4");
    if (num_conv < 1 || num_conv > 1024) return set_error(NESR_ERR_ARG, "nesr_create_compact: num_conv must be 1 .. 1024");
    if (act_type != NESR_ACT_PRELU && act_type != NESR_ACT_RELU && act_type != NESR_ACT_LEAKYRELU)
        return set_error(NESR_ERR_ARG, "nesr_create_compact: act_type must be NESR_ACT_PRELU, NESR_ACT_RELU or NESR_ACT_LEAKYRELU");
    if (dtype != NESR_DTYPE_F32_SPLIT && dtype != NESR_DTYPE_BF16 && dtype != NESR_DTYPE_F16)
        return set_error(NESR_ERR_ARG, "nesr_create_compact: dtype must be NESR_DTYPE_F32_SPLIT, NESR_DTYPE_BF16 or NESR_DTYPE_F16");
    int ndev = 0;
    NESR_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_error(NESR_ERR_ARG, "no such device " + std::to_string(device));
    NESR_TRY(hipSetDevice(device));
    nesr_compact* c = new nesr_compact();
    c->device = device;
    c->nin = num_in_ch;
    c->nout = num_out_ch;
    c->nf = num_feat;
    c->nconv = num_conv;
    c->up = upscale;
    c->act = act_type;
    c->dtype = dtype;
    (void)hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device);
    if (hipMalloc((void**)&c->d_status, 16) != hipSuccess || hipMemset(c->d_status, 0, 16) != hipSuccess ||
        hipHostMalloc((void**)&c->h_status, 16, hipHostMallocDefault) != hipSuccess) {
        compact_destroy(c);
        return set_error(NESR_ERR_HIP, "allocating the context's status words failed");
    }
    for (int i = 0; i < 4; ++i) c->h_status[i] = 0;
    auto add = [&](int cin, int cout) {
        CLayer L;
        L.cin = cin;
        L.cout = cout;
        L.cin_p = cin <= 32 ? 32 : 64;
        L.ncb = (cout + 15) / 16;
        c->conv.push_back(std::move(L));
    };
    add(num_in_ch, num_feat);
    for (int i = 0; i < num_conv; ++i) add(num_feat, num_feat);
    add(num_feat, num_out_ch * upscale * upscale);
    if (act_type == NESR_ACT_PRELU) {
        c->slope.assign(num_conv + 1, std::vector<float>());
        c->has_slope.assign(num_conv + 1, false);
    }
    *out = c;
    return NESR_OK;
}

int compact_upscale(const nesr_compact* c) { return c->up; }

void compact_destroy(nesr_compact* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    c->timer.destroy();
    if (c->ws) (void)hipFree(c->ws);
    if (c->d_weights) (void)hipFree(c->d_weights);
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->h_status) (void)hipHostFree(c->h_status);
    delete c;
}

int compact_num_tensors(const nesr_compact* c) { return (int)c->conv.size() * 2 + (int)c->slope.size(); }

int compact_load_weight(nesr_compact* c, const char* key, const float* data, const int64_t* shape, int ndim) {
    const std::string k(key);
    const std::string bad = "unexpected key in state_dict: " + k;
    if (k.rfind("body.", 0) != 0) return set_error(NESR_ERR_ARG, bad);
    const size_t dot = k.find('.', 5);
    if (dot == std::string::npos || dot == 5) return set_error(NESR_ERR_ARG, bad);
    const std::string idx = k.substr(5, dot - 5), kind = k.substr(dot + 1);
    for (char ch : idx)
        if (ch < '0' || ch > '9') return set_error(NESR_ERR_ARG, bad);
    if (idx.size() > 6 || (idx.size() > 1 && idx[0] == '0')) return set_error(NESR_ERR_ARG, bad);
    const int i = std::stoi(idx);
    if (i % 2 == 0) {
        if (i / 2 >= (int)c->conv.size() || (kind != "weight" && kind != "bias")) return set_error(NESR_ERR_ARG, bad);
        CLayer& L = c->conv[i / 2];
        if (kind == "weight") {
            if (ndim != 4 || shape[0] != L.cout || shape[1] != L.cin || shape[2] != 3 || shape[3] != 3)
                return set_error(NESR_ERR_ARG, "size mismatch for " + k + ": expected [" + std::to_string(L.cout) + "," + std::to_string(L.cin) +
                                                   ",3,3]");
            L.w.assign(data, data + (size_t)L.cout * L.cin * 9);
            L.has_w = true;
        } else {
            if (ndim != 1 || shape[0] != L.cout)
                return set_error(NESR_ERR_ARG, "size mismatch for " + k + ": expected [" + std::to_string(L.cout) + "]");
            L.b.assign(data, data + L.cout);
            L.has_b = true;
        }
    } else {
        const int a = i / 2;
        if (c->act != NESR_ACT_PRELU || a >= (int)c->slope.size() || kind != "weight") return set_error(NESR_ERR_ARG, bad);
        if (ndim != 1 || shape[0] != c->nf)
            return set_error(NESR_ERR_ARG, "size mismatch for " + k + ": expected [" + std::to_string(c->nf) + "]");
        c->slope[a].assign(data, data + c->nf);
        c->has_slope[a] = true;
    }
    c->finalized = false;
    return NESR_OK;
}

int compact_finalize(nesr_compact* c) {
    std::string missing;
    int nmiss = 0;
    auto miss = [&](const std::string& k) {
        if (nmiss++ < 4) missing += (missing.empty() ? "" : ", ") + k;
    };
    for (size_t i = 0; i < c->conv.size(); ++i) {
        if (!c->conv[i].has_w) miss("body." + std::to_string(2 * i) + ".weight");
        if (!c->conv[i].has_b) miss("body." + std::to_string(2 * i) + ".bias");
    }
    for (size_t a = 0; a < c->slope.size(); ++a)
        if (!c->has_slope[a]) miss("body." + std::to_string(2 * a + 1) + ".weight");
    if (nmiss) return set_error(NESR_ERR_STATE, "missing keys in state_dict (" + std::to_string(nmiss) + "): " + missing);
    if (c->ranged()) {   // a weight must fit the (hi, lo) pair, or the f16 value
        for (size_t i = 0; i < c->conv.size(); ++i)
            for (float v : c->conv[i].w)
                if (!(std::fabs(v) <= 65504.f))
                    return set_error(NESR_ERR_RANGE, "body." + std::to_string(2 * i) + ".weight holds a value that is non-finite or beyond "
                                                     "+-65504: it does not fit the " + c->form_name() + " (use compute_dtype bf16)");
    }
    NESR_TRY(hipSetDevice(c->device));
    const int form = c->form();
    size_t bytes = 0;
    c->w_off.clear();
    c->b_off.clear();
    for (auto& L : c->conv) {
        c->w_off.push_back(bytes);
        bytes = align_up(bytes + compact_weight_bytes(L.cin_p, L.ncb, form), 256);
        c->b_off.push_back(bytes);
        bytes = align_up(bytes + (size_t)L.ncb * 16 * 4, 256);
    }
    c->slope_off = bytes;
    bytes += (size_t)(c->nconv + 1) * 64 * 4;
    std::vector<char> host(bytes, 0);
    for (size_t i = 0; i < c->conv.size(); ++i) {
        const CLayer& L = c->conv[i];
        pack_compact_weights(L.w.data(), L.cout, L.cin, L.cin_p, L.ncb, form, reinterpret_cast<uint16_t*>(host.data() + c->w_off[i]));
        float* b = reinterpret_cast<float*>(host.data() + c->b_off[i]);
        for (int o = 0; o < L.cout; ++o) b[o] = L.b[o];
    }
    float* s = reinterpret_cast<float*>(host.data() + c->slope_off);
    for (int a = 0; a <= c->nconv; ++a)
        for (int ch = 0; ch < 64; ++ch)
            s[a * 64 + ch] = c->act == NESR_ACT_PRELU ? c->slope[a][ch] : (c->act == NESR_ACT_LEAKYRELU ? 0.1f : 0.f);
    NESR_TRY(hipDeviceSynchronize());
    if (c->d_weights) NESR_TRY(hipFree(c->d_weights));
    c->d_weights = nullptr;
    NESR_TRY(hipMalloc((void**)&c->d_weights, bytes));
    NESR_TRY(hipMemcpy(c->d_weights, host.data(), bytes, hipMemcpyHostToDevice));
    c->finalized = true;
    return NESR_OK;
}

size_t compact_workspace_bytes(const nesr_compact* c, int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return ws_layout(c, N, H, W).total;
}

int compact_reserve(nesr_compact* c, int N, int H, int W) {
    NESR_TRY(hipSetDevice(c->device));
    return ensure_ws(c, compact_workspace_bytes(c, N, H, W));
}

double compact_flops(const nesr_compact* c, int N, int H, int W) {
    const double px = (double)N * H * W;
    double macs = 0.0;
    for (const auto& L : c->conv) macs += 9.0 * L.cin * L.cout;
    return 2.0 * macs * px;
}

int compact_forward(nesr_compact* c, const float* x, const uint8_t* x_u8, int flip, int N, int C, int H, int W, float* y, uint8_t* y_u8,
                    int round_mode, hipStream_t s) {
    if (!c->finalized) return set_error(NESR_ERR_STATE, "weights not finalized (nesr_finalize_weights)");
    if (N < 1 || H < 1 || W < 1 || C != c->nin) return set_error(NESR_ERR_ARG, "forward: expected [N >= 1, " + std::to_string(c->nin) + ", H, W]");
    if ((long long)N * H * W > (1ll << 30) || (long long)H * c->up > (1 << 30) || (long long)W * c->up > (1 << 30))
        return set_error(NESR_ERR_ARG, "forward: frame too large");
    NESR_TRY(hipSetDevice(c->device));
    int rc = ensure_ws(c, ws_layout(c, N, H, W).total);
    if (rc) return rc;
    const CWs L = ws_layout(c, N, H, W);
    const int form = c->form();
    unsigned* status = c->ranged() ? c->d_status : nullptr;
    if (status) NESR_TRY(launch_status_latch(status, s));   // the range word is per forward (nesr_check_range reports a latched one once)
    CompactPack p{x, x_u8, flip, N, H, W, form, c->ws + L.act0, reinterpret_cast<float*>(c->ws + L.res), status};
    NESR_TRY(launch_compact_pack(p, s));
    auto conv = [&](int i, const void* in, void* out) {
        CompactConv a;
        a.in = in;
        a.wt = c->d_weights + c->w_off[i];
        a.bias = reinterpret_cast<const float*>(c->d_weights + c->b_off[i]);
        a.slope = reinterpret_cast<const float*>(c->d_weights + c->slope_off) + (size_t)(i < c->nconv + 1 ? i : 0) * 64;
        a.out = out;
        a.n = N;
        a.h = H;
        a.w = W;
        a.status = status;
        return a;
    };
    char* buf[2] = {c->ws + L.a, c->ws + L.b};
    NESR_TRY(launch_compact_conv(conv(0, c->ws + L.act0, buf[0]), form, 32, c->cus, s));
    NESR_TRY(c->timer.begin(s));
    int cur = 0;
    for (int i = 1; i <= c->nconv; ++i, cur ^= 1) NESR_TRY(launch_compact_conv(conv(i, buf[cur], buf[cur ^ 1]), form, 64, c->cus, s));
    NESR_TRY(c->timer.end(s));
    if (c->timer.on) {
        c->timer.launches += c->nconv;
        c->timer.flops += 2.0 * 9.0 * 64 * 64 * (double)N * H * W * c->nconv;
    }
    NESR_TRY(launch_compact_tail(conv(c->nconv + 1, buf[cur], nullptr), form, c->up, reinterpret_cast<const float*>(c->ws + L.res), y, y_u8, flip,
                               round_mode == NESR_ROUND_NEAREST ? 1 : 0, c->cus, s));
    return NESR_OK;
}

int compact_set_timing(nesr_compact* c, int enable) {
    c->timer.on = enable != 0;
    return NESR_OK;
}

int compact_kernel_time_ms(nesr_compact* c, double* total_ms, int64_t* launches, double* flops) {
    NESR_TRY(hipSetDevice(c->device));
    NESR_TRY(c->timer.collect(total_ms, launches, flops));
    return NESR_OK;
}

int compact_check_status(nesr_compact* c) {
    NESR_TRY(hipSetDevice(c->device));
    NESR_TRY(hipDeviceSynchronize());
    return compact_check_range(c, nullptr);
}

int compact_check_range(nesr_compact* c, hipStream_t s) {
    if (!c->ranged()) return NESR_OK;   // bf16 has f32's range
    const std::string path = c->f16() ? "f16 path" : "f16-pair fp32 path";
    NESR_TRY(hipSetDevice(c->device));
    NESR_TRY(hipMemcpyAsync(c->h_status, c->d_status, 16, hipMemcpyDeviceToHost, s));
    NESR_TRY(hipStreamSynchronize(s));
    const bool now = c->h_status[0] != 0, earlier = c->h_status[3] != 0;
    if (!now && !earlier) return NESR_OK;
    NESR_TRY(hipMemsetAsync(c->d_status, 0, 16, s));   // reported once; the next forward starts clean
    NESR_TRY(hipStreamSynchronize(s));
    c->h_status[0] = c->h_status[3] = 0;
    if (now)
        return set_error(NESR_ERR_RANGE, "an input or activation of the " + path + " was non-finite or exceeded 65504 in magnitude: "
                                         "the float output of that forward is NaN, an 8-bit output is invalid (use compute_dtype bf16 for "
                                         "such data)");
    return set_error(NESR_ERR_RANGE, "an EARLIER forward on this context (its result was never checked with nesr_check_range) met an input or "
                                     "activation of the " + path + " that was non-finite or exceeded 65504 in magnitude: that forward's "
                                     "output was NaN / invalid; the latest forward's output is valid");
}

}  // namespace nesr
