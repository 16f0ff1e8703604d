// cv2.imwrite(path.jpg, frame, [IMWRITE_JPEG_SAMPLING_FACTOR, 4:4:4, IMWRITE_JPEG_OPTIMIZE, 1, IMWRITE_JPEG_RST_INTERVAL, one MCU row])
// from a host with no Python and no torch in the process, through the C ABI of libnesr_hip.so (include/nesr_hip.h): reads a raw
// H x W x 3 RGB u8 file, encodes it on the device with nesr_jpeg_encode_ex_u8 -- full chroma resolution, Huffman tables built for the
// frame on the device, a restart marker after every row of 8 x 8 MCUs -- writes the .jpg and prints its length and FNV-1a hash.
// The header's length is the device's (the optimised DHT segments depend on the frame): the host learns the file's size from the
// length word, and runs once more at that size when the first buffer was too small.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/jpeg_options_host.cpp -o build/jpeg_options_host -ldl
//   build/jpeg_options_host path/to/libnesr_hip.so in.rgb H W quality out.jpg [first out_cap]
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
    if (argc < 7) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so in.rgb H W quality out.jpg [first out_cap]\n", argv[0]);
        return 1;
    }
    const int H = std::atoi(argv[3]), W = std::atoi(argv[4]), C = 3, quality = std::atoi(argv[5]);
    if (H < 1 || W < 1) { std::fprintf(stderr, "bad shape %s x %s\n", argv[3], argv[4]); return 1; }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_jpeg_scratch_bytes_ex) LOAD(nesr_jpeg_encode_ex_u8)
    std::printf("%s\n", p_nesr_version());

    const size_t bytes = (size_t)H * W * C;
    std::vector<uint8_t> img(bytes);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || std::fread(img.data(), 1, bytes, f) != bytes) { std::fprintf(stderr, "cannot read %zu bytes from %s\n", bytes, argv[2]); return 1; }
    std::fclose(f);

    const int mcus_per_row = (W + 7) / 8;                 // 4:4:4: an MCU is 8 x 8 pixels
    if (mcus_per_row > 65535) { std::fprintf(stderr, "a restart interval holds at most 65535 MCUs\n"); return 1; }
    const nesr_jpeg_opts opts = {quality, NESR_JPEG_444, 1, mcus_per_row};
    const size_t scratch_bytes = p_nesr_jpeg_scratch_bytes_ex(H, W, C, &opts);
    if (!scratch_bytes) { std::fprintf(stderr, "nesr_jpeg_scratch_bytes_ex rejects the shape or the options\n"); return 3; }
    size_t cap = argc > 7 ? (size_t)std::atoll(argv[7]) : bytes / 2 + 4096;
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
        CHECK(p_nesr_jpeg_encode_ex_u8(0, d_img, (int64_t)W * C, H, W, C, NESR_ORDER_RGB, &opts, d_scratch, scratch_bytes, d_out, cap, d_len, s));
        HIPCHK(hipMemcpyAsync(len, d_len, sizeof(len), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::printf("attempt %d: out_cap %zu, the file needs %llu bytes, %s\n", attempt, cap, (unsigned long long)len[0], len[1] ? "did not fit" : "fits");
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
    f = std::fopen(argv[6], "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[6]); return 1; }
    uint64_t hash = 1469598103934665603ull;               // FNV-1a, 64 bits
    for (uint8_t b : file) hash = (hash ^ b) * 1099511628211ull;
    std::printf("%d x %d at quality %d, 4:4:4, optimised, restart interval %d: %zu bytes, fnv1a %016llx, scratch %zu bytes\n", H, W, quality, mcus_per_row,
                file.size(), (unsigned long long)hash, scratch_bytes);
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_img)); HIPCHK(hipFree(d_scratch)); HIPCHK(hipFree(d_len));
    return 0;
}
