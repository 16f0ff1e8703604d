// The pipeline's pre- and post-filters (SuperResolutionPipeline._preprocess_image / _postprocess_image, nesr/nesr.py:668-689,
// 1056-1084) from a host with no Python and no torch in the process, through the C ABI of libnesr_hip.so (include/nesr_hip.h):
// reads a raw H x W x 3 RGB u8 file, runs nesr_preprocess_u8 (NL-means denoise + CLAHE on L) and then nesr_postprocess_u8 (adaptive
// unsharp) on its result -- the order of one iteration of the reference, with the ESRGAN stage left out -- and writes both as raw
// RGB u8 files.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/filters_host.cpp -o build/filters_host -ldl
//   build/filters_host path/to/libnesr_hip.so in.rgb H W denoise_level pre.rgb post.rgb
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

static bool read_file(const char* path, std::vector<uint8_t>& buf) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(buf.data(), 1, buf.size(), f);
    std::fclose(f);
    return got == buf.size();
}

static bool write_file(const char* path, const std::vector<uint8_t>& buf) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const size_t put = std::fwrite(buf.data(), 1, buf.size(), f);
    return std::fclose(f) == 0 && put == buf.size();
}

int main(int argc, char** argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so in.rgb H W denoise_level pre.rgb post.rgb\n", argv[0]);
        return 1;
    }
    const int H = std::atoi(argv[3]), W = std::atoi(argv[4]);
    const double level = std::atof(argv[5]);
    if (H < 1 || W < 1) { std::fprintf(stderr, "bad size %s x %s\n", argv[3], argv[4]); return 1; }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_preprocess_scratch_bytes) LOAD(nesr_preprocess_u8) LOAD(nesr_postprocess_u8)
    std::printf("%s\n", p_nesr_version());

    const size_t bytes = (size_t)H * W * 3;
    std::vector<uint8_t> img(bytes), pre(bytes), post(bytes);
    if (!read_file(argv[2], img)) { std::fprintf(stderr, "cannot read %zu bytes from %s\n", bytes, argv[2]); return 1; }
    const size_t scratch_bytes = p_nesr_preprocess_scratch_bytes(H, W);
    uint8_t *d_img, *d_pre, *d_post;
    void* d_scratch;
    HIPCHK(hipMalloc(&d_img, bytes)); HIPCHK(hipMalloc(&d_pre, bytes)); HIPCHK(hipMalloc(&d_post, bytes));
    HIPCHK(hipMalloc(&d_scratch, scratch_bytes));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_img, img.data(), bytes, hipMemcpyHostToDevice, s));
    CHECK(p_nesr_preprocess_u8(0, d_img, H, W, level, d_scratch, scratch_bytes, d_pre, s));
    CHECK(p_nesr_postprocess_u8(0, d_pre, H, W, 1, d_post, s));
    HIPCHK(hipMemcpyAsync(pre.data(), d_pre, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(post.data(), d_post, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    size_t changed = 0;
    for (size_t i = 0; i < bytes; ++i) changed += pre[i] != img[i];
    std::printf("%d x %d, denoise level %g: pre-filter changed %zu of %zu bytes; scratch %zu bytes\n", H, W, level, changed, bytes, scratch_bytes);
    if (!write_file(argv[6], pre) || !write_file(argv[7], post)) { std::fprintf(stderr, "cannot write the outputs\n"); return 1; }
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_img)); HIPCHK(hipFree(d_pre)); HIPCHK(hipFree(d_post)); HIPCHK(hipFree(d_scratch));
    return 0;
}
