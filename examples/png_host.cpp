// cv2.imwrite(path.png, frame) -- what standalone/superres_project.py:203-206 always writes and nesr/nesr.py:619-625 saves after
// every iteration -- from a host with no Python and no torch in the process, through the C ABI of libnesr_hip.so
// (include/nesr_hip.h): reads a raw H x W x C file (C = 1, 3 or 4 in R G B (A) order; depth 8: bytes, depth 16: little-endian
// 16-bit samples), encodes it on the device with nesr_png_encode and writes the lossless .png.  The output buffer is
// nesr_png_bound, the exact worst case, so one run always fits; only the file crosses back to the host.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/png_host.cpp -o build/png_host -ldl
//   build/png_host path/to/libnesr_hip.so in.raw H W C depth out.png
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

int main(int argc, char** argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so in.raw H W C depth out.png\n", argv[0]);
        return 1;
    }
    const int H = std::atoi(argv[3]), W = std::atoi(argv[4]), C = std::atoi(argv[5]), depth = std::atoi(argv[6]);
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_png_bound) LOAD(nesr_png_scratch_bytes) LOAD(nesr_png_head) LOAD(nesr_png_encode)
    std::printf("%s\n", p_nesr_version());

    int head_bytes = 0;
    CHECK(p_nesr_png_head(H, W, C, depth, nullptr, 0, &head_bytes));              // host only; also rejects a bad shape
    const size_t bytes = (size_t)H * W * C * depth / 8;
    std::vector<uint8_t> img(bytes);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || std::fread(img.data(), 1, bytes, f) != bytes) { std::fprintf(stderr, "cannot read %zu bytes from %s\n", bytes, argv[2]); return 1; }
    std::fclose(f);

    const size_t scratch_bytes = p_nesr_png_scratch_bytes(H, W, C, depth), cap = p_nesr_png_bound(H, W, C, depth);
    uint8_t *d_img, *d_out;
    void* d_scratch;
    uint64_t* d_len;
    uint64_t len[2] = {0, 0};
    HIPCHK(hipMalloc(&d_img, bytes));
    HIPCHK(hipMalloc(&d_scratch, scratch_bytes));
    HIPCHK(hipMalloc(&d_out, cap));
    HIPCHK(hipMalloc(&d_len, sizeof(len)));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_img, img.data(), bytes, hipMemcpyHostToDevice, s));
    CHECK(p_nesr_png_encode(0, d_img, (int64_t)W * C * depth / 8, H, W, C, depth, NESR_ORDER_RGB, d_scratch, scratch_bytes, d_out, cap, d_len, s));
    HIPCHK(hipMemcpyAsync(len, d_len, sizeof(len), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::printf("out_cap %zu (the bound), the file needs %llu bytes (%d of them the head), %s\n", cap, (unsigned long long)len[0], head_bytes,
                len[1] ? "did not fit" : "fits");
    if (len[1] != 0) { std::fprintf(stderr, "the file did not fit its bound (%d)\n", (int)NESR_ERR_NOFIT); return 4; }
    std::vector<uint8_t> file(len[0]);
    HIPCHK(hipMemcpy(file.data(), d_out, len[0], hipMemcpyDeviceToHost));          // only the file crosses to the host
    f = std::fopen(argv[7], "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[7]); return 1; }
    std::printf("%d x %d x %d at %d bits: %zu bytes of %zu, scratch %zu bytes\n", H, W, C, depth, file.size(), bytes, scratch_bytes);
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_img)); HIPCHK(hipFree(d_scratch)); HIPCHK(hipFree(d_out)); HIPCHK(hipFree(d_len));
    return 0;
}
