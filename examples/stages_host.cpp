// The stages of SuperResolutionPipeline.enhance_image's loop around its networks (nesr/nesr.py:516-633) from a host with no Python
// and no torch in the process, through the C ABI of libnesr_hip.so (include/nesr_hip.h): a seeded H x W RGB frame is resized with
// each of cv2's interpolations (nesr_resize_cv_u8: nearest, linear, cubic -- the loop's no-model step, nesr/nesr.py:597-605 -- and
// Lanczos-4), up to (2H + 1) x (2W - 1) and down to (H / 2 + 1) x (W / 2 + 2); sharpened under a seeded mask
// (nesr_segment_enhance_u8: _segment_and_enhance after its argmax, nesr/nesr.py:726-747); and averaged with a second frame
// (nesr_ensemble_u8: _ensemble_results, nesr/nesr.py:1033-1054).  One line per result: its name and the FNV-1a (64 bit) checksum of
// its bytes.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/stages_host.cpp -o build/stages_host -ldl
//   build/stages_host path/to/libnesr_hip.so [H W [mask_h mask_w]]
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nesr_hip.h"

#define LOAD(name) auto p_##name = reinterpret_cast<decltype(&name)>(dlsym(lib, #name)); if (!p_##name) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s -> %s\n", #call, hipGetErrorString(e_)); return 5; } } while (0)
#define CHECK(call) do { int rc_ = (call); if (rc_ != 0) { std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, p_nesr_last_error()); return 3; } } while (0)

// bytes of a linear congruential generator (Numerical Recipes' constants): the top byte of every state
static void seeded(std::vector<uint8_t>& buf, uint32_t seed, uint8_t mask) {
    uint32_t s = seed;
    for (auto& b : buf) {
        s = s * 1664525u + 1013904223u;
        b = (uint8_t)(s >> 24) & mask;
    }
}

static uint64_t fnv1a(const std::vector<uint8_t>& buf) {
    uint64_t h = 14695981039346656037ull;
    for (uint8_t b : buf) h = (h ^ b) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so [H W [mask_h mask_w]]\n", argv[0]);
        return 1;
    }
    const int H = argc > 3 ? std::atoi(argv[2]) : 61, W = argc > 3 ? std::atoi(argv[3]) : 83;
    const int MH = argc > 5 ? std::atoi(argv[4]) : 16, MW = argc > 5 ? std::atoi(argv[5]) : 21;
    if (H < 2 || W < 2 || MH < 1 || MW < 1) { std::fprintf(stderr, "bad sizes\n"); return 1; }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_resize_cv_u8) LOAD(nesr_segment_enhance_scratch_bytes) LOAD(nesr_segment_enhance_u8)
    LOAD(nesr_ensemble_u8)
    std::printf("%s\n", p_nesr_version());

    const int UH = 2 * H + 1, UW = 2 * W - 1, DH = H / 2 + 1, DW = W / 2 + 2;
    const size_t bytes = (size_t)H * W * 3, up_bytes = (size_t)UH * UW * 3, down_bytes = (size_t)DH * DW * 3;
    std::vector<uint8_t> frame(bytes), second(bytes), mask((size_t)MH * MW), up(up_bytes), down(down_bytes), res(bytes);
    seeded(frame, 1, 255);
    seeded(mask, 2, 1);
    seeded(second, 3, 255);
    const size_t scratch_bytes = p_nesr_segment_enhance_scratch_bytes(H, W);
    uint8_t *d_frame, *d_second, *d_mask, *d_up, *d_down, *d_res;
    void* d_scratch;
    HIPCHK(hipMalloc(&d_frame, bytes)); HIPCHK(hipMalloc(&d_second, bytes)); HIPCHK(hipMalloc(&d_mask, mask.size()));
    HIPCHK(hipMalloc(&d_up, up_bytes)); HIPCHK(hipMalloc(&d_down, down_bytes)); HIPCHK(hipMalloc(&d_res, bytes));
    HIPCHK(hipMalloc(&d_scratch, scratch_bytes));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_frame, frame.data(), bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_second, second.data(), bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_mask, mask.data(), mask.size(), hipMemcpyHostToDevice, s));

    const int interps[4] = {NESR_INTER_NEAREST, NESR_INTER_LINEAR, NESR_INTER_CUBIC, NESR_INTER_LANCZOS4};
    const char* names[4] = {"nearest", "linear", "cubic", "lanczos4"};
    for (int i = 0; i < 4; ++i) {
        CHECK(p_nesr_resize_cv_u8(0, d_frame, H, W, 3, (int64_t)W * 3, d_up, UH, UW, (int64_t)UW * 3, interps[i], s));
        CHECK(p_nesr_resize_cv_u8(0, d_frame, H, W, 3, (int64_t)W * 3, d_down, DH, DW, (int64_t)DW * 3, interps[i], s));
        HIPCHK(hipMemcpyAsync(up.data(), d_up, up_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(down.data(), d_down, down_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::printf("%s_up %016llx\n%s_down %016llx\n", names[i], (unsigned long long)fnv1a(up), names[i], (unsigned long long)fnv1a(down));
    }
    CHECK(p_nesr_segment_enhance_u8(0, d_frame, H, W, d_mask, MH, MW, d_scratch, scratch_bytes, d_res, s));
    HIPCHK(hipMemcpyAsync(res.data(), d_res, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::printf("segment %016llx\n", (unsigned long long)fnv1a(res));
    const uint8_t* pair[2] = {d_frame, d_second};
    CHECK(p_nesr_ensemble_u8(0, pair, 2, H, W, 3, d_res, s));
    HIPCHK(hipMemcpyAsync(res.data(), d_res, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::printf("ensemble %016llx\n", (unsigned long long)fnv1a(res));
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_frame)); HIPCHK(hipFree(d_second)); HIPCHK(hipFree(d_mask)); HIPCHK(hipFree(d_up)); HIPCHK(hipFree(d_down));
    HIPCHK(hipFree(d_res)); HIPCHK(hipFree(d_scratch));
    return 0;
}
