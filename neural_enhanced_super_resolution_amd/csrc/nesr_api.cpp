// C ABI of libnesr_hip.so (include/nesr_hip.h) for contexts: creation, strict weight loading + repacking, the forward entries,
// setters and state queries, timing, status and range checks.  A context made by nesr_create_compact is handed on to
// compact_api.cpp entry by entry; the forward graph of an RRDBNet context is rrdb_forward.cpp.  The other entries of the ABI:
// band_api.cpp (nesr_band_*), shard_api.cpp (RCCL, sharded frames), oneshot_api.cpp (no context), filters_api.cpp.
//
// What it stands behind in the reference: basicsr RRDBNet.__init__/forward and realesrgan
// RealESRGANer's load_state_dict, as called from nesr/nesr.py:216-229,887-891 and
// standalone/direct_esrgan.py:104-148.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "rrdb_ctx.h"

using namespace nesr;

namespace {
thread_local std::string g_err;
}

int nesr::set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int nesr::rrdb_only(const nesr_ctx* c, const char* entry) {
    if (c && c->compact) return set_error(NESR_ERR_ARG, std::string(entry) + ": RRDBNet contexts only (not an SRVGGNetCompact context)");
    return NESR_OK;
}

extern "C" {

const char* nesr_last_error(void) { return g_err.c_str(); }
const char* nesr_version(void) { return "nesr_hip 0.1 (gfx950)"; }

int nesr_create(nesr_ctx** out, int device_id, int conv_first_in_ch, int unshuffle, int num_feat, int num_block,
                int num_grow_ch, int num_out_ch, int dtype) {
    if (!out) return set_error(NESR_ERR_ARG, "out is null");
    *out = nullptr;
    if (unshuffle != 0 && unshuffle != 1 && unshuffle != 2 && unshuffle != 4)
        return set_error(NESR_ERR_ARG, "unshuffle must be 0, 2 or 4");
    const int u = unshuffle > 1 ? unshuffle : 1;
    if (conv_first_in_ch <= 0 || conv_first_in_ch % (u * u))
        return set_error(NESR_ERR_ARG, "conv_first_in_ch must be a positive multiple of unshuffle^2");
    if (num_feat != 32 && num_feat != 64) return set_error(NESR_ERR_ARG, "num_feat must be 32 or 64 (reference uses 64)");
    if (num_grow_ch != 32) return set_error(NESR_ERR_ARG, "num_grow_ch must be 32 (reference uses 32)");
    if (num_block < 0 || num_out_ch <= 0 || num_out_ch > 32) return set_error(NESR_ERR_ARG, "bad num_block / num_out_ch");
    if (!form_of(dtype))
        return set_error(NESR_ERR_ARG, "dtype must be 0 (f32 direct), 1 (bf16), 2 (f32 Winograd), 3 (f32 as f16 pairs) or 4 (f16)");
    int ndev = 0;
    NESR_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return set_error(NESR_ERR_ARG, "no such device " + std::to_string(device_id));
    NESR_TRY(hipSetDevice(device_id));
    // every failure from here on releases what the context holds by then
    std::unique_ptr<nesr_ctx, void (*)(nesr_ctx*)> owner(new nesr_ctx(), nesr_destroy);
    nesr_ctx* c = owner.get();
    c->device = device_id;
    constexpr size_t STATUS_BYTES = 256 + 4096 * 4;   // status words + progress words of up to 4096 tiles
    NESR_TRY(hipMalloc((void**)&c->d_status, STATUS_BYTES));
    if (hipMemset(c->d_status, 0, STATUS_BYTES) != hipSuccess || hipHostMalloc((void**)&c->h_status, 64, hipHostMallocDefault) != hipSuccess)
        return set_error(NESR_ERR_HIP, "allocating the context's status words failed");
    *c->h_status = 0;
    c->cin0 = conv_first_in_ch;
    c->unshuffle = unshuffle;
    c->nf = num_feat;
    c->nb = num_block;
    c->gc = num_grow_ch;
    c->nout = num_out_ch;
    c->winograd = dtype == NESR_DTYPE_F32_WINOGRAD;
    if (const char* e = getenv("NESR_F32_ALGO")) {   // override for A/B timing: direct | winograd
        if (dtype != NESR_DTYPE_BF16 && dtype != NESR_DTYPE_F16) {
            c->winograd = e[0] == 'w';
            dtype = e[0] == 's' ? NESR_DTYPE_F32_SPLIT : (e[0] == 'w' ? NESR_DTYPE_F32_WINOGRAD : NESR_DTYPE_F32);
        }
    }
    if (dtype == NESR_DTYPE_F32_WINOGRAD) dtype = NESR_DTYPE_F32;   // an f32 context that also holds Winograd slabs
    c->dtype = dtype;
    c->form = form_of(dtype);
    // A/B runs.  Exactly the documented values; anything else is refused, not read as the default
    if (const char* e = getenv("NESR_UPCONV")) {
        if (std::strcmp(e, "3x3") != 0 && std::strcmp(e, "2x2") != 0) return set_error(NESR_ERR_ARG, std::string("NESR_UPCONV must be 3x3 or 2x2, not '") + e + "'");
        c->upconv_2x2 = std::strcmp(e, "2x2") == 0;
    }
    if (const char* bad = bad_kernel16_override()) return set_error(NESR_ERR_ARG, std::string("NESR_BF16_KERNEL must be small or xl, not '") + bad + "'");
    if (const char* e = getenv("NESR_CONV_LAST")) {
        if (std::strcmp(e, "general") != 0 && std::strcmp(e, "narrow") != 0) return set_error(NESR_ERR_ARG, std::string("NESR_CONV_LAST must be general or narrow, not '") + e + "'");
        c->last_narrow = std::strcmp(e, "narrow") == 0;
    }
    if (const char* e = getenv("NESR_TRUNK")) c->trunk_mode = e[0] == 'l' ? 1 : (e[0] == 'p' ? 2 : 0);
    if (const char* e = getenv("NESR_RDB_FUSE")) c->rdb_mode = atoi(e);
    if (const char* e = getenv("NESR_RDB_CHAIN")) {
        if (std::strcmp(e, "0") != 0 && std::strcmp(e, "1") != 0) return set_error(NESR_ERR_ARG, std::string("NESR_RDB_CHAIN must be 0 or 1, not '") + e + "'");
        c->rdb_chain = e[0] == '1';
    }
    if (const char* e = getenv("NESR_STRIP")) c->strip_mode = atoi(e);
    c->rdb_mode_init = c->rdb_mode;
    c->strip_mode_init = c->strip_mode;
    if (const char* e = getenv("NESR_STRIP_SEG")) c->strip_seg = atoi(e);
    if (const char* e = getenv("NESR_FUSED_TIMEOUT_MS")) c->strip_timeout_ticks = (unsigned long long)atoll(e) * 100000ull;
    (void)hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device_id);
    if (const char* e = getenv("NESR_STRIP_CUS")) c->strip_cus = std::min(std::max(atoi(e), 1), std::max(c->cus, 1));
    auto add = [&](const std::string& name, int cin, int cout) {
        Layer L;
        L.name = name;
        L.cin = cin;
        L.cout = cout;
        L.cin_p = round_up(cin, c->form->kgroup);
        L.cout_p = round_up(cout, 32);
        c->index[name] = (int)c->layers.size();
        c->layers.push_back(std::move(L));
    };
    add("conv_first", c->cin0, c->nf);
    for (int b = 0; b < c->nb; ++b)
        for (int r = 1; r <= 3; ++r) {
            const std::string pre = "body." + std::to_string(b) + ".rdb" + std::to_string(r) + ".conv";
            for (int k = 1; k <= 4; ++k) add(pre + std::to_string(k), c->nf + (k - 1) * c->gc, c->gc);
            add(pre + "5", c->nf + 4 * c->gc, c->nf);
        }
    add("conv_body", c->nf, c->nf);
    add("conv_up1", c->nf, c->nf);
    add("conv_up2", c->nf, c->nf);
    add("conv_hr", c->nf, c->nf);
    add("conv_last", c->nf, c->nout);
    *out = owner.release();
    return NESR_OK;
}

int nesr_create_compact(nesr_ctx** out, int device_id, int num_in_ch, int num_out_ch, int num_feat, int num_conv, int upscale,
                        int act_type, int dtype) {
    if (!out) return set_error(NESR_ERR_ARG, "out is null");
    *out = nullptr;
    nesr_compact* k = nullptr;
    const int rc = compact_create(&k, device_id, num_in_ch, num_out_ch, num_feat, num_conv, upscale, act_type, dtype);
    if (rc) return rc;
    nesr_ctx* c = new nesr_ctx();
    c->compact = k;
    c->device = device_id;
    *out = c;
    return NESR_OK;
}

int nesr_num_tensors(const nesr_ctx* c) {
    if (c && c->compact) return compact_num_tensors(c->compact);
    return c ? (int)c->layers.size() * 2 : 0;
}

int nesr_load_weight(nesr_ctx* c, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (c && c->compact && key && data && shape) return compact_load_weight(c->compact, key, data, shape, ndim);
    if (!c || !key || !data || !shape) return set_error(NESR_ERR_ARG, "null argument");
    std::string k(key);
    const size_t dot = k.rfind('.');
    if (dot == std::string::npos) return set_error(NESR_ERR_ARG, "unexpected key in state_dict: " + k);
    const std::string lname = k.substr(0, dot), kind = k.substr(dot + 1);
    auto it = c->index.find(lname);
    if (it == c->index.end() || (kind != "weight" && kind != "bias"))
        return set_error(NESR_ERR_ARG, "unexpected key in state_dict: " + k);
    Layer& L = c->layers[it->second];
    if (kind == "weight") {
        if (ndim != 4 || shape[0] != L.cout || shape[1] != L.cin || shape[2] != 3 || shape[3] != 3)
            return set_error(NESR_ERR_ARG, "size mismatch for " + k + ": expected [" + std::to_string(L.cout) + "," +
                                               std::to_string(L.cin) + ",3,3]");
        L.w.assign(data, data + (size_t)L.cout * L.cin * 9);
        L.has_w = true;
    } else {
        if (ndim != 1 || shape[0] != L.cout)
            return set_error(NESR_ERR_ARG, "size mismatch for " + k + ": expected [" + std::to_string(L.cout) + "]");
        L.b.assign(data, data + L.cout);
        L.has_b = true;
    }
    c->finalized = false;
    return NESR_OK;
}

int nesr_finalize_weights(nesr_ctx* c) {
    if (c && c->compact) return compact_finalize(c->compact);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    std::string missing;
    int nmiss = 0;
    for (const Layer& L : c->layers) {
        if (!L.has_w && nmiss++ < 4) missing += " " + L.name + ".weight";
        if (!L.has_b && nmiss++ < 4) missing += " " + L.name + ".bias";
    }
    if (nmiss) return set_error(NESR_ERR_STATE, "Missing key(s) in state_dict (" + std::to_string(nmiss) + "):" + missing);
    // non-finite parameters are refused for every dtype; the f16-pair form (its hi half is an f16) and the f16 form also
    // need |w| <= 65504 -- never a silently clamped weight
    for (const Layer& L : c->layers) {
        const float lim = c->ranged() ? 65504.f : INFINITY;
        for (int t = 0; t < 2; ++t) {
            const std::vector<float>& v = t ? L.b : L.w;
            const float blim = t ? INFINITY : lim;   // biases are added in f32
            for (size_t i = 0; i < v.size(); ++i)
                if (!(std::fabs(v[i]) <= blim) || !std::isfinite(v[i]))
                    return set_error(NESR_ERR_RANGE, L.name + (t ? ".bias" : ".weight") + "[" + std::to_string(i) + "] = " + std::to_string(v[i]) +
                                                         (!std::isfinite(v[i]) ? ": non-finite parameter"
                                                          : c->dtype == NESR_DTYPE_F16 ? ": |w| > 65504 does not fit compute_dtype f16 (use bf16 or f32)"
                                                                                       : ": |w| > 65504 does not fit the f16-pair form of compute_dtype f32 "
                                                                                         "(use f32-winograd or f32-direct)"));
        }
    }
    NESR_TRY(hipSetDevice(c->device));
    const Form& form = *c->form;
    size_t total = 256;   // leading zero page
    std::vector<size_t> woff(c->layers.size()), boff(c->layers.size()), wwoff(c->layers.size(), 0), w2off(c->layers.size(), 0);
    // f16-pair form: conv_up1 / conv_up2 also as four folded 2x2-tap slabs (the 3x3 slabs stay: nesr_set_upconv)
    auto is_up = [&](const Layer& L) { return c->dtype == NESR_DTYPE_F32_SPLIT && (L.name == "conv_up1" || L.name == "conv_up2"); };
    for (size_t i = 0; i < c->layers.size(); ++i) {
        const Layer& L = c->layers[i];
        woff[i] = total;
        total = align_up(total + form.weight_bytes(L.cin_p, L.cout_p), 256);
        boff[i] = total;
        total = align_up(total + (size_t)L.cout_p * 4, 256);
        if (c->winograd) {   // next to the direct slab, not instead of it
            wwoff[i] = total;
            total = align_up(total + packed_weight_elems_wino_f32(L.cin_p, L.cout_p) * 4, 256);
        }
        if (is_up(L)) {
            w2off[i] = total;
            total = align_up(total + packed_upconv_elems_f16x2(L.cin_p, L.cout_p) * 2, 256);
        }
    }
    std::vector<char> host(total, 0);
    for (size_t i = 0; i < c->layers.size(); ++i) {
        const Layer& L = c->layers[i];
        form.pack(L.w.data(), L.cout, L.cin, L.cin_p, L.cout_p, host.data() + woff[i]);
        std::memcpy(host.data() + boff[i], L.b.data(), (size_t)L.cout * 4);
        if (wwoff[i]) pack_weights_wino_f32(L.w.data(), L.cout, L.cin, L.cin_p, L.cout_p, reinterpret_cast<float*>(host.data() + wwoff[i]));
        if (w2off[i]) {
            std::vector<float> folded((size_t)16 * L.cout * L.cin);
            fold_upconv_weights(L.w.data(), L.cout, L.cin, folded.data());
            for (size_t k = 0; k < folded.size(); ++k)   // a sum of up to four taps must fit the pair's hi half as every tap does
                if (!(std::fabs(folded[k]) <= 65504.f))
                    return set_error(NESR_ERR_RANGE, L.name + ".weight: a folded 2x2 tap (sum of up to four 3x3 taps) exceeds 65504 in magnitude and "
                                                              "does not fit the f16-pair form of compute_dtype f32 (use f32-winograd or f32-direct)");
            pack_upconv_weights_f16x2(folded.data(), L.cout, L.cin, L.cin_p, L.cout_p, reinterpret_cast<uint16_t*>(host.data() + w2off[i]));
        }
    }
    if (c->d_weights) {
        NESR_TRY(hipDeviceSynchronize());
        NESR_TRY(hipFree(c->d_weights));
        c->d_weights = nullptr;
    }
    void* p = nullptr;
    NESR_TRY(hipMalloc(&p, total));
    c->d_weights = static_cast<char*>(p);
    NESR_TRY(hipMemcpy(c->d_weights, host.data(), total, hipMemcpyHostToDevice));
    for (size_t i = 0; i < c->layers.size(); ++i) {
        c->layers[i].d_w = c->d_weights + woff[i];
        c->layers[i].d_b = reinterpret_cast<float*>(c->d_weights + boff[i]);
        c->layers[i].d_ww = wwoff[i] ? c->d_weights + wwoff[i] : nullptr;
        c->layers[i].d_w2 = w2off[i] ? c->d_weights + w2off[i] : nullptr;
    }
    // bf16 / f16: every dense block's weights once more as the LDS-resident kernel's stream (rdb_bf16_strip.hip), + its 192 biases
    if (c->d_strip) { NESR_TRY(hipDeviceSynchronize()); NESR_TRY(hipFree(c->d_strip)); c->d_strip = nullptr; }
    if (c->half16() && c->nf == 64 && c->gc == 32 && c->nb > 0) {
        c->strip_stride = align_up(strip_weight_bytes() + 192 * 4, 256);
        std::vector<char> hs((size_t)c->nb * 3 * c->strip_stride, 0);
        for (int b = 0; b < c->nb; ++b)
            for (int r = 0; r < 3; ++r) {
                char* blk = hs.data() + (size_t)(b * 3 + r) * c->strip_stride;
                const float* w5[5];
                float* bias = reinterpret_cast<float*>(blk + strip_weight_bytes());
                for (int k = 0; k < 5; ++k) {
                    const Layer& Ly = c->layers[layer_id(b, r, k)];
                    w5[k] = Ly.w.data();
                    std::memcpy(bias + 32 * k, Ly.b.data(), (size_t)Ly.cout * 4);
                }
                pack_strip_weights(w5, reinterpret_cast<uint16_t*>(blk), c->dtype == NESR_DTYPE_F16);
            }
        NESR_TRY(hipMalloc((void**)&c->d_strip, hs.size()));
        NESR_TRY(hipMemcpy(c->d_strip, hs.data(), hs.size(), hipMemcpyHostToDevice));
    }
    // layer table of the persistent trunk kernel (same wiring as the per-layer loop in run_forward)
    {
        std::vector<TrunkLayer> tl;
        for (int b = 0; b < c->nb; ++b)
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 5; ++k) {
                    const Layer& Ly = c->layers[layer_id(b, r, k)];
                    TrunkLayer t;
                    std::memset(&t, 0, sizeof(t));
                    t.in_buf = r;
                    t.cin = Ly.cin_p;
                    t.coutp = Ly.cout_p;
                    t.w = Ly.d_w;
                    t.bias = Ly.d_b;
                    t.res1_buf = t.res2_buf = -1;
                    t.s1 = t.s2 = 1.f;
                    if (k < 4) {
                        t.out_buf = r; t.out_coff = c->nf + k * c->gc; t.lrelu = 1;
                    } else {
                        t.out_coff = 0; t.lrelu = 0;
                        t.res1_buf = r; t.s1 = 0.2f;
                        if (r < 2) {
                            t.out_buf = r + 1;
                        } else {
                            t.out_buf = 0; t.res2_buf = 0; t.s2 = 0.2f;
                        }
                    }
                    tl.push_back(t);
                }
        if (c->d_trunk) { NESR_TRY(hipFree(c->d_trunk)); c->d_trunk = nullptr; }
        if (!tl.empty()) {
            NESR_TRY(hipMalloc((void**)&c->d_trunk, tl.size() * sizeof(TrunkLayer)));
            NESR_TRY(hipMemcpy(c->d_trunk, tl.data(), tl.size() * sizeof(TrunkLayer), hipMemcpyHostToDevice));
        }
    }
    c->finalized = true;
    return NESR_OK;
}

int nesr_forward(nesr_ctx* c, const void* x_dev, int N, int C, int H, int W, void* y_dev, void* stream) {
    if (c && c->compact && x_dev && y_dev)
        return compact_forward(c->compact, static_cast<const float*>(x_dev), nullptr, 0, N, C, H, W, static_cast<float*>(y_dev), nullptr, 0,
                               static_cast<hipStream_t>(stream));
    if (!c || !x_dev || !y_dev) return set_error(NESR_ERR_ARG, "null argument");
    return run_forward(c, static_cast<const float*>(x_dev), nullptr, 0, N, C, H, W, static_cast<float*>(y_dev), nullptr, 0,
                       static_cast<hipStream_t>(stream));
}

int nesr_forward_ragged(nesr_ctx* c, const void* x_dev, int N, int C, int H, int W, const int* hw, void* y_dev, void* stream) {
    RRDB_ONLY(c);
    if (!c || !x_dev || !y_dev || !hw) return set_error(NESR_ERR_ARG, "null argument");
    if (!c->half16()) return set_error(NESR_ERR_ARG, "nesr_forward_ragged: compute dtype bf16 or f16 only (the other forms batch equal-sized images)");
    if (N < 1 || N > nesr::RAG_MAX) return set_error(NESR_ERR_ARG, "nesr_forward_ragged: 1.." + std::to_string(nesr::RAG_MAX) + " images per call");
    const int u = c->ufac();
    if (H % u || W % u || H / u > 16383 || W / u > 16383) return set_error(NESR_ERR_ARG, "nesr_forward_ragged: slot size");
    for (int i = 0; i < N; ++i) {
        const int h = hw[2 * i], w = hw[2 * i + 1];
        if (h < 1 || w < 1 || h > H || w > W || h % u || w % u)
            return set_error(NESR_ERR_ARG, "nesr_forward_ragged: image " + std::to_string(i) + " is " + std::to_string(h) + "x" + std::to_string(w) +
                                          ", slot " + std::to_string(H) + "x" + std::to_string(W) + ", unshuffle " + std::to_string(u));
        c->rag_h[i] = (unsigned short)(h / u);
        c->rag_w[i] = (unsigned short)(w / u);
    }
    c->rag_n = N;
    c->rag_base_h = H / u;
    const int rc = run_forward(c, static_cast<const float*>(x_dev), nullptr, 0, N, C, H, W, static_cast<float*>(y_dev), nullptr, 0,
                               static_cast<hipStream_t>(stream));
    c->rag_n = 0;
    return rc;
}

int nesr_set_size_independent(nesr_ctx* c, int on) {
    if (c && c->compact) return NESR_OK;
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    c->size_independent = on ? 1 : 0;
    return NESR_OK;
}

int nesr_forward_u8(nesr_ctx* c, const uint8_t* in_hwc_dev, int H, int W, uint8_t* out_hwc_dev, int flip_rgb,
                    int round_mode, void* stream) {
    if (c && c->compact && in_hwc_dev && out_hwc_dev)
        return compact_forward(c->compact, nullptr, in_hwc_dev, flip_rgb ? 1 : 0, 1, 3, H, W, nullptr, out_hwc_dev, round_mode,
                               static_cast<hipStream_t>(stream));
    if (!c || !in_hwc_dev || !out_hwc_dev) return set_error(NESR_ERR_ARG, "null argument");
    const int u = c->ufac();
    if (c->cin0 != 3 * u * u || c->nout != 3)
        return set_error(NESR_ERR_ARG, "nesr_forward_u8 needs a 3-channel-in / 3-channel-out network");
    return run_forward(c, nullptr, in_hwc_dev, flip_rgb ? 1 : 0, 1, 3, H, W, nullptr, out_hwc_dev,
                       round_mode == NESR_ROUND_NEAREST ? 1 : 0, static_cast<hipStream_t>(stream));
}

size_t nesr_workspace_bytes(const nesr_ctx* c, int N, int H, int W) {
    if (c && c->compact) return compact_workspace_bytes(c->compact, N, H, W);
    if (!c || N <= 0 || H <= 0 || W <= 0) return 0;
    const int u = c->ufac();
    return ws_layout(c, N, (H + u - 1) / u, (W + u - 1) / u).total;
}

int nesr_reserve(nesr_ctx* c, int N, int H, int W) {
    if (c && c->compact) return compact_reserve(c->compact, N, H, W);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    NESR_TRY(hipSetDevice(c->device));
    return ensure_ws(c, nesr_workspace_bytes(c, N, H, W));
}

double nesr_forward_flops(const nesr_ctx* c, int N, int H, int W) {
    if (c && c->compact) return compact_flops(c->compact, N, H, W);
    if (!c) return 0.0;
    const int u = c->ufac();
    const double px = (double)N * (H / u) * (W / u);
    double f = 0.0;
    const int tail = 1 + c->nb * 15;
    for (int i = 0; i < (int)c->layers.size(); ++i) {
        double scale = 1.0;
        if (i == tail + 1) scale = 4.0;
        if (i >= tail + 2) scale = 16.0;
        f += conv_flops(c->layers[i], px * scale);
    }
    return f;
}

int nesr_preferred_batch(const nesr_ctx* c, int H, int W, int max_batch) {
    RRDB_ONLY(c);
    if (!c || H <= 0 || W <= 0 || max_batch <= 1) return 1;
    const int u = c->ufac();
    const int h = (H + u - 1) / u, w = (W + u - 1) / u;
    // workgroups per frame of the trunk convs (the kernel choice mirrors launch_conv3x3_bf16 / _f16)
    const bool xl = c->half16() && (long)h * w > 256L * 256L;
    static const int geo = [] { const char* e = getenv("NESR_XL_GEOMETRY"); return e ? atoi(e) : 4; }();
    const int xl_th = geo == 8 ? 32 : 16;
    const bool sp = c->dtype == NESR_DTYPE_F32_SPLIT;   // 8x32-px tiles, two workgroups per CU
    const long per = sp ? (long)((h + 7) / 8) * ((w + 31) / 32)
                        : xl ? (long)((h + xl_th - 1) / xl_th) * ((w + 31) / 32) : (long)((h + 7) / 8) * ((w + 15) / 16);
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    const long slots = (long)cus * ((xl && geo == 8) ? 1 : 2);   // co-resident workgroups
    auto eff = [&](int b) {
        const long wgs = per * b;
        return (double)wgs / (double)(((wgs + slots - 1) / slots) * slots);
    };
    double best_eff = 0.0;
    for (int b = 1; b <= max_batch; ++b) best_eff = eff(b) > best_eff ? eff(b) : best_eff;
    int best = 1;
    for (int b = 1; b <= max_batch; ++b)
        if (eff(b) >= best_eff - 0.02) best = b;   // the largest batch within 2 % of the best fill: fewest launches
    return best;
}

int nesr_set_concurrent(nesr_ctx* c, int concurrent) {
    if (c && c->compact) return NESR_OK;
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    c->shared_device = concurrent ? 1 : 0;
    return NESR_OK;
}

int nesr_set_fused(nesr_ctx* c, int on) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    c->rdb_mode = on ? c->rdb_mode_init : 0;          // on: what the context was created with (NESR_RDB_FUSE / NESR_STRIP, default auto)
    c->strip_mode = on ? c->strip_mode_init : 0;
    return NESR_OK;
}

int nesr_set_upconv(nesr_ctx* c, int mode) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (mode != NESR_UPCONV_3X3 && mode != NESR_UPCONV_2X2) return set_error(NESR_ERR_ARG, "nesr_set_upconv: mode must be NESR_UPCONV_3X3 or NESR_UPCONV_2X2");
    c->upconv_2x2 = mode == NESR_UPCONV_2X2;
    return NESR_OK;
}

int nesr_upconv_state(const nesr_ctx* c) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (c->dtype != NESR_DTYPE_F32_SPLIT || !c->upconv_2x2) return NESR_UPCONV_3X3;
    if (!c->finalized) return set_error(NESR_ERR_STATE, "nesr_upconv_state: weights not finalised");
    for (const Layer& L : c->layers)   // what the launches will really take: the folded slabs must be there
        if ((L.name == "conv_up1" || L.name == "conv_up2") && !L.d_w2) return set_error(NESR_ERR_STATE, "nesr_upconv_state: " + L.name + " has no folded weights");
    return NESR_UPCONV_2X2;
}

int nesr_set_conv_last(nesr_ctx* c, int mode) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (mode != NESR_CONV_LAST_GENERAL && mode != NESR_CONV_LAST_NARROW) return set_error(NESR_ERR_ARG, "nesr_set_conv_last: mode must be NESR_CONV_LAST_GENERAL or NESR_CONV_LAST_NARROW");
    c->last_narrow = mode == NESR_CONV_LAST_NARROW;
    return NESR_OK;
}

int nesr_fold_upconv_weights(const float* oihw, int cout, int cin, float* folded) {
    if (!oihw || !folded || cout <= 0 || cin <= 0) return set_error(NESR_ERR_ARG, "nesr_fold_upconv_weights: bad argument");
    fold_upconv_weights(oihw, cout, cin, folded);
    return NESR_OK;
}

int nesr_fused_state(const nesr_ctx* c) {
    RRDB_ONLY(c);
    if (!c) return 0;
    const int on = c->half16() ? c->strip_mode != 0 : (c->dtype == NESR_DTYPE_F32_SPLIT && c->rdb_mode != 0);
    return (on ? 1 : 0) | (c->fused_aborts << 1);
}

int nesr_rdb_chain_state(const nesr_ctx* c, int* kernel_launches, int* blocks) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (kernel_launches) *kernel_launches = c->chain_launches;
    if (blocks) *blocks = c->chain_blocks;
    return NESR_OK;
}

int nesr_rdb_chain_table(int num_block, const uint64_t* buffers, const uint64_t* layer_w, const uint64_t* layer_b, uint64_t* table) {
    if (num_block <= 0 || !buffers || !layer_w || !layer_b || !table) return set_error(NESR_ERR_ARG, "nesr_rdb_chain_table: bad argument");
    std::vector<Layer> layers((size_t)(1 + 15 * num_block));
    for (size_t i = 0; i < layers.size(); ++i) {
        layers[i].d_w = reinterpret_cast<void*>(static_cast<uintptr_t>(layer_w[i]));
        layers[i].d_b = reinterpret_cast<float*>(static_cast<uintptr_t>(layer_b[i]));
    }
    char* buf[3];
    for (int i = 0; i < 3; ++i) buf[i] = reinterpret_cast<char*>(static_cast<uintptr_t>(buffers[i]));
    static_assert(sizeof(RdbChainBlock) == 13 * sizeof(uint64_t), "13 pointers per entry");
    for (int i = 0; i < 3 * num_block; ++i) {
        RdbChainBlock e;
        rdb_block_entry(buf, layers.data(), i / 3, i % 3, e);
        std::memcpy(table + (size_t)i * 13, &e, sizeof(e));
    }
    return NESR_OK;
}

int nesr_strip_schedule(int n, const int* hw, int cus, int seg_len, int* items, int items_cap, int* wg_first, int wg_cap, int* info,
                        double* efficiency) {
    if (n <= 0 || !hw || cus <= 0 || !info) return set_error(NESR_ERR_ARG, "nesr_strip_schedule: n and cus from 1, hw and info not null");
    for (int i = 0; i < 2 * n; ++i)
        if (hw[i] <= 0) return set_error(NESR_ERR_ARG, "nesr_strip_schedule: image sizes from 1");
    const StripSchedule S = strip_schedule(n, hw, cus, seg_len);
    const int count = (int)(S.items.size() / 8);
    int walked = 0;
    const int wait = S.makespan > 0 ? strip_max_wait(S, &walked) : -1;
    info[0] = S.makespan; info[1] = S.grid; info[2] = S.smax; info[3] = S.nvimg; info[4] = count;
    info[5] = strip_plan_applies(S) ? 1 : 0;
    info[6] = wait; info[7] = walked;
    info[8] = strip_largest_pos1(S); info[9] = STRIP_MAX_POS1;
    if (efficiency) *efficiency = S.efficiency;
    if ((count > 0 && (!items || items_cap < count)) || (!S.wg_first.empty() && (!wg_first || wg_cap < (int)S.wg_first.size())))
        return set_error(NESR_ERR_ARG, "nesr_strip_schedule: the plan has " + std::to_string(count) + " items on " + std::to_string(S.grid) + " workgroups; buffers too small");
    if (count > 0) std::memcpy(items, S.items.data(), S.items.size() * sizeof(int));
    if (!S.wg_first.empty()) std::memcpy(wg_first, S.wg_first.data(), S.wg_first.size() * sizeof(int));
    return NESR_OK;
}

int nesr_debug_fault(nesr_ctx* c, int drop_workgroups) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    c->debug_drop = drop_workgroups > 0 ? drop_workgroups : 0;
    return NESR_OK;
}

int nesr_set_kernel_timing(nesr_ctx* c, int enable) {
    if (c && c->compact) return compact_set_timing(c->compact, enable);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    c->timer.on = enable != 0;
    return NESR_OK;
}

int nesr_kernel_time_ms(nesr_ctx* c, double* total_ms, int64_t* launches, double* flops) {
    if (c && c->compact) return compact_kernel_time_ms(c->compact, total_ms, launches, flops);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    NESR_TRY(hipSetDevice(c->device));
    NESR_TRY(c->timer.collect(total_ms, launches, flops));
    return NESR_OK;
}

int nesr_check_status(nesr_ctx* c) {
    if (c && c->compact) return compact_check_status(c->compact);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    NESR_TRY(hipSetDevice(c->device));
    NESR_TRY(hipDeviceSynchronize());
    if (c->last_sync) {
        unsigned flag = 0;
        NESR_TRY(hipMemcpy(&flag, c->last_sync, 4, hipMemcpyDeviceToHost));
        if (flag) return set_error(NESR_ERR_HIP, "persistent trunk kernel aborted: a neighbour wait timed out (workgroups not co-resident?)");
    }
    return nesr_check_range(c, nullptr);
}

int nesr_check_range(nesr_ctx* c, void* stream) {
    if (c && c->compact) return compact_check_range(c->compact, static_cast<hipStream_t>(stream));
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (!c->ranged() && !c->strip_used) return NESR_OK;   // the other forms compute in formats with f32's range
    NESR_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    NESR_TRY(hipMemcpyAsync(c->h_status, c->d_status, 16, hipMemcpyDeviceToHost, s));
    NESR_TRY(hipStreamSynchronize(s));
    c->strip_used = false;
    if (c->h_status[2]) {
        const unsigned code = c->h_status[2];      // 1 | layer waited for << 8 | workgroup << 16
        NESR_TRY(hipMemsetAsync(c->d_status + 2, 0, 4, s));
        NESR_TRY(hipStreamSynchronize(s));
        c->h_status[2] = 0;
        c->strip_mode = 0;       // this context runs per-layer launches from now on (valid values; not the strip kernel's bits)
        ++c->fused_aborts;
        return set_error(NESR_ERR_HIP, "the LDS-resident dense-block kernel gave up waiting for a neighbouring strip's edge column (workgroup " +
                                  std::to_string(code >> 16) + ", layer " + std::to_string((code >> 8) & 255u) +
                                  ": its workgroups were not all resident -- another process's persistent kernel shares the device?); the "
                                  "output of that forward is invalid; this context uses per-layer launches from now on (re-run the frame)");
    }
    if (!c->ranged()) return NESR_OK;
    const char* form = c->dtype == NESR_DTYPE_F16 ? "the f16 form" : "the f16-pair fp32 path";
    const char* instead = c->dtype == NESR_DTYPE_F16 ? "use compute_dtype bf16 or f32 for such data" : "use compute_dtype f32-winograd or f32-direct for such data";
    if (c->h_status[1]) {
        const unsigned code = c->h_status[1];      // 1 | chunk whose producer was waited for << 8 | tile << 16
        NESR_TRY(hipMemsetAsync(c->d_status, 0, 8, s));
        NESR_TRY(hipStreamSynchronize(s));
        c->h_status[0] = c->h_status[1] = 0;
        c->rdb_mode = 0;         // per-layer launches from now on: the same values bit for bit, no inter-workgroup waits
        ++c->fused_aborts;
        return set_error(NESR_ERR_HIP, "the fused dense-block kernel gave up waiting for a neighbouring tile's progress word (tile " +
                                  std::to_string(code >> 16) + ", input chunk " + std::to_string((code >> 8) & 255u) +
                                  ": its workgroups were not all resident -- another persistent kernel shares the device?); the "
                                  "output of that forward is invalid; this context uses per-layer launches (the same bits) from now on: re-run the frame");
    }
    if (c->h_status[3] && !*c->h_status) {
        NESR_TRY(hipMemsetAsync(c->d_status + 3, 0, 4, s));
        NESR_TRY(hipStreamSynchronize(s));
        c->h_status[3] = 0;
        return set_error(NESR_ERR_RANGE, std::string("an EARLIER forward on this context (its result was never checked with nesr_check_range) met an input or "
                                                "activation of ") + form + " that was non-finite or exceeded 65504 in magnitude: that forward's "
                                                "output was NaN / invalid; the latest forward's output is valid");
    }
    if (*c->h_status) {
        NESR_TRY(hipMemsetAsync(c->d_status, 0, 4, s));   // reported once; the next forward starts clean
        NESR_TRY(hipMemsetAsync(c->d_status + 3, 0, 4, s));
        NESR_TRY(hipStreamSynchronize(s));
        *c->h_status = 0;
        c->h_status[3] = 0;
        return set_error(NESR_ERR_RANGE, std::string("an input or activation of ") + form + " was non-finite or exceeded 65504 in magnitude: "
                                    "the float output of that forward is NaN, an 8-bit output is invalid (" + instead + ")");
    }
    return NESR_OK;
}

void nesr_destroy(nesr_ctx* c) {
    if (c && c->compact) {
        compact_destroy(c->compact);
        delete c;
        return;
    }
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    c->timer.destroy();
    band_release(c);
    if (c->ws) (void)hipFree(c->ws);
    if (c->d_weights) (void)hipFree(c->d_weights);
    if (c->d_trunk) (void)hipFree(c->d_trunk);
    if (c->d_chain) (void)hipFree(c->d_chain);
    if (c->d_strip) (void)hipFree(c->d_strip);
    if (c->shard_buf) (void)hipFree(c->shard_buf);
    if (c->comm) (void)nesr_comm_destroy(c);
    free_strip_plans(c);
    lease_forget(c);
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->h_status) (void)hipHostFree(c->h_status);
    delete c;
}

}  // extern "C"
