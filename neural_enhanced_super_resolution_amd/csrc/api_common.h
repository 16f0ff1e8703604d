// Plumbing shared by every file of the C-ABI layer (nesr_api.cpp, rrdb_forward.cpp, band_api.cpp, shard_api.cpp, oneshot_api.cpp,
// compact_api.cpp, filters_api.cpp, resize_api.cpp, frame_api.cpp, nesr_stage_api.cpp, jpeg_api.cpp, jpeg_decode_api.cpp, png_api.cpp, png_decode_api.cpp): the error string, the try macro, alignment, and the kernel-timing hook of a context.
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

}  // namespace nesr
