// cv2.imwrite(path.jpg, frame) -- the last call of every entry point of the reference (standalone/direct_esrgan.py:169,
// nesr/nesr.py:646) -- from a host with no Python and no torch in the process, through the C ABI of libnesr_hip.so
// (include/nesr_hip.h): reads a raw H x W x 3 RGB u8 file (or H x W gray with C = 1), encodes it on the device with
// nesr_jpeg_encode_u8 and writes the .jpg.  The output buffer starts at H W C / 2 + 4096 bytes; when the status word says the file
// did not fit, the encode runs once more at the size the length word reported.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/jpeg_host.cpp -o build/jpeg_host -ldl
//   build/jpeg_host path/to/libnesr_hip.so in.rgb H W C quality out.jpg [first out_cap]
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
        std::fprintf(stderr, "usage: %s libnesr_hip.so in.rgb H W C quality out.jpg [first out_cap]\n", argv[0]);
        return 1;
    }
    const int H = std::atoi(argv[3]), W = std::atoi(argv[4]), C = std::atoi(argv[5]), quality = std::atoi(argv[6]);
    if (H < 1 || W < 1 || (C != 1 && C != 3)) { std::fprintf(stderr, "bad shape %s x %s x %s\n", argv[3], argv[4], argv[5]); return 1; }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_jpeg_scratch_bytes) LOAD(nesr_jpeg_header) LOAD(nesr_jpeg_encode_u8)
    std::printf("%s\n", p_nesr_version());

    const size_t bytes = (size_t)H * W * C;
    std::vector<uint8_t> img(bytes);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || std::fread(img.data(), 1, bytes, f) != bytes) { std::fprintf(stderr, "cannot read %zu bytes from %s\n", bytes, argv[2]); return 1; }
    std::fclose(f);

    int header_bytes = 0;
    CHECK(p_nesr_jpeg_header(H, W, C, quality, nullptr, 0, &header_bytes));      // host only: the size of SOI .. SOS
    const size_t scratch_bytes = p_nesr_jpeg_scratch_bytes(H, W, C);
    size_t cap = argc > 8 ? (size_t)std::atoll(argv[8]) : bytes / 2 + 4096;
    uint8_t* d_img;
    void* d_scratch;
    uint64_t* d_len;
    HIPCHK(hipMalloc(&d_img, bytes));
    HIPCHK(hipMalloc(&d_scratch, scratch_bytes));
    HIPCHK(hipMalloc(&d_len, 2 * sizeof(uint64_t)));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_img, img.data(), bytes, hipMemcpyHostToDevice, s));
    std::vector<uint8_t> file;
    for (int attempt = 0;; ++attempt) {
        uint8_t* d_out;
        uint64_t len[2] = {0, 0};
        HIPCHK(hipMalloc(&d_out, cap));
        CHECK(p_nesr_jpeg_encode_u8(0, d_img, (int64_t)W * C, H, W, C, NESR_ORDER_RGB, quality, d_scratch, scratch_bytes, d_out, cap, d_len, s));
        HIPCHK(hipMemcpyAsync(len, d_len, sizeof(len), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::printf("attempt %d: out_cap %zu, the file needs %llu bytes (%d of them the header), %s\n", attempt, cap, (unsigned long long)len[0],
                    header_bytes, len[1] ? "did not fit" : "fits");
        if (len[1] == 0) {
            file.resize(len[0]);
            HIPCHK(hipMemcpy(file.data(), d_out, len[0], hipMemcpyDeviceToHost));      // only the file crosses to the host
            HIPCHK(hipFree(d_out));
            break;
        }
        HIPCHK(hipFree(d_out));
        if (attempt == 1) { std::fprintf(stderr, "the file did not fit the size the device reported (%d)\n", (int)NESR_ERR_NOFIT); return 4; }
        cap = len[0];
    }
    f = std::fopen(argv[7], "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[7]); return 1; }
    std::printf("%d x %d x %d at quality %d: %zu bytes, scratch %zu bytes\n", H, W, C, quality, file.size(), scratch_bytes);
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_img)); HIPCHK(hipFree(d_scratch)); HIPCHK(hipFree(d_len));
    return 0;
}
