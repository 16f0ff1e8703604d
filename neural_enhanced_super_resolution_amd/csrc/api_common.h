// Plumbing shared by every file of the C-ABI layer (nesr_api.cpp, rrdb_forward.cpp, band_api.cpp, shard_api.cpp, oneshot_api.cpp,
// compact_api.cpp, filters_api.cpp, resize_api.cpp, frame_api.cpp, nesr_stage_api.cpp, segformer_api.cpp, swin2sr_api.cpp, vae_api.cpp,
// unet_api.cpp, clip_text_api.cpp, sdx4_api.cpp, jpeg_api.cpp, jpeg_decode_api.cpp, png_api.cpp, png_decode_api.cpp): the error string,
// the try macro, alignment, the carver of a scratch buffer's regions, a workspace that grows, the upload of a model's packed weights,
// and the kernel-timing hooks of a context (EventTimer: one bracket per forward; GroupTimer: one per launch, summed per kernel group).
// The host side of a strictly loaded state dict is state_dict.h; what the five networks that load one share around it
// (segformer_api.cpp, swin2sr_api.cpp, vae_api.cpp, unet_api.cpp, clip_text_api.cpp) is net_context.h; what the four file codecs
// share (jpeg_api.cpp, jpeg_decode_api.cpp, png_api.cpp, png_decode_api.cpp) is codec_host.h, and on the device codec_device.h.
// Not part of the public ABI (that is include/nesr_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/nesr_hip.h"

namespace nesr {

// sets nesr_last_error() (thread-local, nesr_api.cpp) and returns `code`
int set_error(int code, const std::string& msg);

#define NESR_TRY(expr)                                                                                    \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess)                                                                            \
            return nesr::set_error(NESR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));   \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

// Carves one scratch or workspace buffer into regions that each start on a 256-byte boundary: take() gives the next region's offset.
struct ScratchCarver {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += align_up(bytes, 256);
        return o;
    }
    size_t total() const { return at; }
};

// Kernel-timing hook of a context (nesr_set_kernel_timing / nesr_kernel_time_ms): one event pair around the timed part of every
// forward, summed and recycled when the caller asks.  begin / end do nothing while the hook is off.
struct EventTimer {
    using Pair = std::pair<hipEvent_t, hipEvent_t>;
    bool on = false;
    Pair cur{nullptr, nullptr};      // the pair of the forward being recorded
    std::vector<Pair> pending, spare;
    int64_t launches = 0;
    double flops = 0.0;

    hipError_t begin(hipStream_t s) {
        if (!on) return hipSuccess;
        if (!cur.first && !spare.empty()) {
            cur = spare.back();
            spare.pop_back();
        }
        hipError_t e = hipSuccess;
        if (!cur.first && (e = hipEventCreate(&cur.first)) != hipSuccess) return e;
        if (!cur.second && (e = hipEventCreate(&cur.second)) != hipSuccess) return e;
        return hipEventRecord(cur.first, s);
    }
    hipError_t end(hipStream_t s) {
        if (!on || !cur.first) return hipSuccess;
        const hipError_t e = hipEventRecord(cur.second, s);
        if (e == hipSuccess) {
            pending.push_back(cur);
            cur = Pair{nullptr, nullptr};
        }
        return e;
    }
    // waits for the recorded forwards; hands out and resets the totals
    hipError_t collect(double* total_ms, int64_t* n_launches, double* n_flops) {
        double ms = 0.0;
        for (const Pair& pr : pending) {
            hipError_t e = hipEventSynchronize(pr.second);
            float t = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&t, pr.first, pr.second);
            if (e != hipSuccess) return e;
            ms += t;
        }
        spare.insert(spare.end(), pending.begin(), pending.end());
        pending.clear();
        if (total_ms) *total_ms = ms;
        if (n_launches) *n_launches = launches;
        if (n_flops) *n_flops = flops;
        launches = 0;
        flops = 0.0;
        return hipSuccess;
    }
    void destroy() {
        pending.insert(pending.end(), spare.begin(), spare.end());
        pending.push_back(cur);
        for (const Pair& pr : pending) {
            if (pr.first) (void)hipEventDestroy(pr.first);
            if (pr.second) (void)hipEventDestroy(pr.second);
        }
        pending.clear();
        spare.clear();
        cur = Pair{nullptr, nullptr};
    }
};

// "<what>: " in front of a message, nothing for a null `what`
inline std::string prefix(const char* what) { return what ? std::string(what) + ": " : std::string(); }

// A workspace that only grows: frees and allocates anew when `bytes` exceeds what `buf` has (the device is synchronised first,
// launches that use the old buffer may be in flight).  A failed allocation leaves buf null and no sticky HIP error behind.
inline int grow(char*& buf, size_t& have, size_t bytes, const char* what) {
    if (bytes <= have) return NESR_OK;
    NESR_TRY(hipDeviceSynchronize());
    if (buf) NESR_TRY(hipFree(buf));
    buf = nullptr;
    have = 0;
    if (hipMalloc((void**)&buf, bytes) != hipSuccess) {
        buf = nullptr;
        (void)hipGetLastError();
        return set_error(NESR_ERR_NOMEM, prefix(what) + "workspace allocation of " + std::to_string(bytes) + " bytes failed" +
                                             (what ? " (the workspace grows with the frame)" : ""));
    }
    have = bytes;
    return NESR_OK;
}

// A create entry's device argument: `device_id` is `no_device` (the host side alone, no HIP call is made) or names a device.
inline int check_device(int device_id, int no_device) {
    if (device_id == no_device) return NESR_OK;
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess) return set_error(NESR_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return set_error(NESR_ERR_ARG, "no such device " + std::to_string(device_id));
    return NESR_OK;
}

// What a single-launch test hook (`entry`, nesr_vae_k_* / nesr_unet_k_*) returns for its launcher's result; `header` is the file
// that states what the launcher takes.
inline int launch_done(hipError_t e, const char* header, const char* entry, const char* launcher) {
    if (e == hipSuccess) return NESR_OK;
    if (e == hipErrorInvalidValue)
        return set_error(NESR_ERR_ARG, std::string(entry) + ": " + launcher + " refused the arguments (" + header + " states what it takes); nothing was launched");
    return set_error(NESR_ERR_HIP, std::string(entry) + ": " + launcher + ": " + hipGetErrorString(e));
}

// The one weight buffer of a model: the old one is freed (after the device's work), `host` goes up in one copy.
inline int upload_weights(int device, float*& d_w, const std::vector<float>& host, const char* what) {
    NESR_TRY(hipSetDevice(device));
    NESR_TRY(hipDeviceSynchronize());
    if (d_w) NESR_TRY(hipFree(d_w));
    d_w = nullptr;
    if (hipMalloc((void**)&d_w, host.size() * 4) != hipSuccess) {
        d_w = nullptr;
        return set_error(NESR_ERR_NOMEM, prefix(what) + "allocating the weights failed");
    }
    NESR_TRY(hipMemcpy(d_w, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    return NESR_OK;
}

// Launch counter and per-group timing of a context whose forward is a chain of launches (NetContext, net_context.h): every
// launch goes through run(), which counts it and, while `on`, brackets it with an event pair of its kernel group.
struct GroupTimer {
    struct Timed {
        int group;
        hipEvent_t a, b;
    };
    bool on = false;
    int64_t launches = 0;
    std::vector<Timed> pending;
    std::vector<hipEvent_t> spare;

    hipError_t new_event(hipEvent_t* e) {
        if (!spare.empty()) {
            *e = spare.back();
            spare.pop_back();
            return hipSuccess;
        }
        return hipEventCreate(e);
    }
    // one launch (the pair goes back to the spare list when the launch or a record fails)
    template <class F>
    int run(const char* model, int group, hipStream_t s, F&& launch) {
        Timed tm{group, nullptr, nullptr};
        hipError_t e = hipSuccess;
        if (on) {
            e = new_event(&tm.a);
            if (e == hipSuccess) e = new_event(&tm.b);
            if (e == hipSuccess) e = hipEventRecord(tm.a, s);
        }
        if (e == hipSuccess) e = launch();
        if (e == hipSuccess) ++launches;
        if (e == hipSuccess && on) e = hipEventRecord(tm.b, s);
        if (e != hipSuccess) {
            if (tm.a) spare.push_back(tm.a);
            if (tm.b) spare.push_back(tm.b);
            return set_error(NESR_ERR_HIP, std::string(model) + " launch (group " + std::to_string(group) + "): " + hipGetErrorString(e));
        }
        if (on) pending.push_back(tm);
        return NESR_OK;
    }
    // waits for the recorded launches; ms[0 .. n_groups) gets each group's sum; hands out and resets the launch count
    int collect(double* ms, int n_groups, int64_t* n_launches) {
        for (int i = 0; i < n_groups; ++i) ms[i] = 0.0;
        for (const Timed& tm : pending) {
            NESR_TRY(hipEventSynchronize(tm.b));
            float t = 0.f;
            NESR_TRY(hipEventElapsedTime(&t, tm.a, tm.b));
            if (tm.group < n_groups) ms[tm.group] += t;
        }
        for (const Timed& tm : pending) spare.insert(spare.end(), {tm.a, tm.b});
        pending.clear();
        if (n_launches) *n_launches = launches;
        launches = 0;
        return NESR_OK;
    }
    void destroy() {
        for (const Timed& tm : pending) spare.insert(spare.end(), {tm.a, tm.b});
        for (hipEvent_t e : spare) (void)hipEventDestroy(e);
        pending.clear();
        spare.clear();
    }
};

// the one way a launch of such a context is made: NESR_RUN(c->timer, "Model", group, stream, [&] { return launch_x(args, stream); })
#define NESR_RUN(timer, ...)                    \
    do {                                        \
        int rc__ = (timer).run(__VA_ARGS__);    \
        if (rc__) return rc__;                  \
    } while (0)

}  // namespace nesr
