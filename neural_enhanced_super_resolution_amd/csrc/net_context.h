// What the five checkpoint networks' contexts share (segformer_api.cpp, swin2sr_api.cpp, vae_api.cpp, unet_api.cpp,
// clip_text_api.cpp): the head of their structs and the entries that do the same thing for each of them.  A model's struct derives
// from NetContext and keeps its own fields; its extern "C" entries hand their own name to the functions below, which put it in
// front of their texts.  On top of api_common.h (grow, upload_weights, GroupTimer) and state_dict.h (StateDict, HostPack, HalfPack).
// Not part of the public ABI.
#pragma once
#include "api_common.h"
#include "state_dict.h"

namespace nesr {

constexpr int NET_NO_DEVICE = -1;      // every model's NESR_*_NO_DEVICE: the host side alone (SegFormer refuses it at create)

struct NetContext {
    int device = 0;
    StateDict sd;                    // every expected key with its shape
    bool finalized = false;
    float* d_w = nullptr;
    char* ws_buf = nullptr;          // the network's buffers
    size_t ws_bytes = 0;
    GroupTimer timer;
    // the models with an fp16 form beside the f32 one (Swin2SR, the UNet)
    int dtype = NESR_DTYPE_F32;      // the compute form (nesr_*_set_dtype)
    bool packed = false;             // finalize has run (set for every model): the form is fixed
    _Float16* d_w16 = nullptr;       // fp16 form: the GEMM weights in halves
    unsigned* d_status = nullptr;    // fp16 form: the range word
    unsigned* h_status = nullptr;
};

inline int unsupported(const char* entry, const std::string& field, const std::string& why) {
    return set_error(NESR_ERR_UNSUPPORTED, std::string(entry) + ": " + field + ": " + why);
}

// A model frees what it owns beyond the base first (SegFormer: its tables and `pre`).
template <class Context>
void net_destroy(Context* c) {
    if (!c) return;
    if (c->device != NET_NO_DEVICE) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        c->timer.destroy();
        for (void* p : {(void*)c->ws_buf, (void*)c->d_w, (void*)c->d_w16, (void*)c->d_status})
            if (p) (void)hipFree(p);
        if (c->h_status) (void)hipHostFree(c->h_status);
    }
    delete c;
}

inline int net_num_tensors(const NetContext* c) { return c ? (int)c->sd.size() : 0; }

// `translate(k)` turns the caller's spelling of a key into the expected one in place and returns false for a buffer the model
// ignores; it runs behind the null check.
template <class Translate>
int net_load_weight(NetContext* c, const char* entry, const char* key, const float* data, const int64_t* shape, int ndim, Translate&& translate) {
    if (!c || !key || (!data && ndim > 0) || ndim < 0 || (ndim > 0 && !shape)) return set_error(NESR_ERR_ARG, std::string(entry) + ": null argument");
    std::string k = key;
    if (!translate(k)) return NESR_OK;
    const int rc = c->sd.load(k, data, shape, ndim, key);
    if (!rc) c->finalized = false;
    return rc;
}

// the head of a finalize: the null check and the missing keys
inline int net_begin_finalize(const NetContext* c, const char* entry) {
    if (!c) return set_error(NESR_ERR_ARG, std::string(entry) + ": null context");
    const std::string missing = c->sd.missing();
    return missing.empty() ? NESR_OK : set_error(NESR_ERR_STATE, missing);
}

// The tail of a finalize: `pk` goes up as d_w and, in the fp16 form, `half` as d_w16 beside a cleared range word.  A weight f16
// cannot carry is refused before any device call; a context without a device stops behind the checks.  `what` names the model in
// the allocation texts (null: none).
inline int net_upload(NetContext* c, const char* entry, const HostPack& pk, const HalfPack* half, const char* what) {
    if (half && !half->out_of_range().empty())
        return set_error(NESR_ERR_RANGE, std::string(entry) + ": " + half->out_of_range() + " holds a value that is non-finite or beyond +-65504, which the fp16 form "
                                             "cannot carry (NESR_DTYPE_F32 can)");
    c->packed = true;
    if (c->device == NET_NO_DEVICE) return NESR_OK;      // checked and packed; nothing to upload to, and no forward either
    const int rc = upload_weights(c->device, c->d_w, pk.host, what);
    if (rc) return rc;
    if (half && c->dtype == NESR_DTYPE_F16) {
        if (c->d_w16) NESR_TRY(hipFree(c->d_w16));
        c->d_w16 = nullptr;
        if (hipMalloc((void**)&c->d_w16, half->half.size() * sizeof(_Float16)) != hipSuccess) {
            c->d_w16 = nullptr;
            return set_error(NESR_ERR_NOMEM, prefix(what) + "allocating the f16 weights failed");
        }
        NESR_TRY(hipMemcpy(c->d_w16, half->half.data(), half->half.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        if (!c->d_status) {
            NESR_TRY(hipMalloc((void**)&c->d_status, sizeof(unsigned)));
            NESR_TRY(hipHostMalloc((void**)&c->h_status, sizeof(unsigned), hipHostMallocDefault));
        }
        NESR_TRY(hipMemset(c->d_status, 0, sizeof(unsigned)));
        *c->h_status = 0;
    }
    c->finalized = true;
    return NESR_OK;
}

inline int net_set_timing(NetContext* c, const char* entry, int enable) {
    if (!c) return set_error(NESR_ERR_ARG, std::string(entry) + ": null context");
    c->timer.on = enable != 0;
    return NESR_OK;
}

// group_ms[0 .. min(n_groups, model_groups)) gets each kernel group's sum since the last call; the launch count is handed out and reset
inline int net_kernel_time_ms(NetContext* c, const char* entry, int model_groups, double* group_ms, int n_groups, int64_t* launches) {
    if (!c) return set_error(NESR_ERR_ARG, std::string(entry) + ": null context");
    if (c->device == NET_NO_DEVICE) return set_error(NESR_ERR_STATE, std::string(entry) + ": a context without a device launches nothing");
    NESR_TRY(hipSetDevice(c->device));
    std::vector<double> ms(model_groups);
    const int rc = c->timer.collect(ms.data(), model_groups, launches);
    for (int i = 0; !rc && group_ms && i < n_groups && i < model_groups; ++i) group_ms[i] = ms[i];
    return rc;
}

// The fp16 form's range word: cleared in front of a call's launches, read behind them (the stream is waited for).  f32 form: nothing.
inline int net_range_begin(NetContext* c, hipStream_t s) {
    if (!c || c->dtype != NESR_DTYPE_F16 || !c->d_status) return NESR_OK;
    NESR_TRY(hipSetDevice(c->device));
    NESR_TRY(hipMemsetAsync(c->d_status, 0, sizeof(unsigned), s));
    return NESR_OK;
}
// NESR_ERR_RANGE with "<entry>: <message>" if a launch set the word
inline int net_range_end(NetContext* c, hipStream_t s, const char* entry, const char* message) {
    if (!c || c->dtype != NESR_DTYPE_F16 || !c->d_status) return NESR_OK;
    NESR_TRY(hipMemcpyAsync(c->h_status, c->d_status, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    NESR_TRY(hipStreamSynchronize(s));
    return *c->h_status ? set_error(NESR_ERR_RANGE, std::string(entry) + ": " + message) : NESR_OK;
}

}  // namespace nesr
