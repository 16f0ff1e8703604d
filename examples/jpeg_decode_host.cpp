// cv2.imread(path.jpg) ... cv2.imwrite(path.jpg, frame) -- the first and last call of every entry point of the reference
// (standalone/direct_esrgan.py:130 and :169) -- from a host with no Python and no torch in the process, through the C ABI of
// libnesr_hip.so (include/nesr_hip.h): the file's bytes go up, nesr_jpeg_parse reads the header on the host, nesr_jpeg_decode_u8
// decodes the frame on the device, nesr_jpeg_encode_u8 encodes it again there, and only the new file comes back.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/jpeg_decode_host.cpp -o build/jpeg_decode_host -ldl
//   build/jpeg_decode_host path/to/libnesr_hip.so in.jpg out.jpg [quality]
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
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so in.jpg out.jpg [quality]\n", argv[0]);
        return 1;
    }
    const int quality = argc > 4 ? std::atoi(argv[4]) : 95;
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_jpeg_parse) LOAD(nesr_jpeg_decode_scratch_bytes) LOAD(nesr_jpeg_decode_u8)
    LOAD(nesr_jpeg_scratch_bytes) LOAD(nesr_jpeg_encode_u8)
    std::printf("%s\n", p_nesr_version());

    std::vector<uint8_t> in;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
    for (int ch; (ch = std::fgetc(f)) != EOF;) in.push_back((uint8_t)ch);
    std::fclose(f);

    static nesr_jpeg_info info;
    CHECK(p_nesr_jpeg_parse(in.data(), in.size(), &info));                        // host only: NESR_ERR_UNSUPPORTED / NESR_ERR_BADFILE end here
    const int H = info.H, W = info.W, C = info.C;
    const size_t frame_bytes = (size_t)H * W * C;
    const size_t dec_scratch = p_nesr_jpeg_decode_scratch_bytes(&info), enc_scratch = p_nesr_jpeg_scratch_bytes(H, W, C);
    std::printf("%d x %d x %d, sampling %d x %d, restart interval %d, scan of %lld bytes\n", H, W, C, info.hs, info.vs, info.restart_interval,
                (long long)info.scan_bytes);

    uint8_t *d_file, *d_frame;
    void *d_dec, *d_enc;
    uint32_t* d_status;
    uint64_t* d_len;
    HIPCHK(hipMalloc(&d_file, in.size()));
    HIPCHK(hipMalloc(&d_frame, frame_bytes));
    HIPCHK(hipMalloc(&d_dec, dec_scratch));
    HIPCHK(hipMalloc(&d_enc, enc_scratch));
    HIPCHK(hipMalloc(&d_status, sizeof(uint32_t)));
    HIPCHK(hipMalloc(&d_len, 2 * sizeof(uint64_t)));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_file, in.data(), in.size(), hipMemcpyHostToDevice, s));      // only the file crosses to the device
    CHECK(p_nesr_jpeg_decode_u8(0, d_file, in.size(), &info, d_frame, (int64_t)W * C, NESR_ORDER_RGB, d_dec, dec_scratch, d_status, s));
    uint32_t status = 0;
    HIPCHK(hipMemcpyAsync(&status, d_status, sizeof(status), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (status != 0) { std::fprintf(stderr, "the device rejected the scan, status 0x%x (%d)\n", status, (int)NESR_ERR_BADFILE); return 4; }

    std::vector<uint8_t> file;
    size_t cap = frame_bytes / 2 + 4096;
    for (int attempt = 0;; ++attempt) {
        uint8_t* d_out;
        uint64_t len[2] = {0, 0};
        HIPCHK(hipMalloc(&d_out, cap));
        CHECK(p_nesr_jpeg_encode_u8(0, d_frame, (int64_t)W * C, H, W, C, NESR_ORDER_RGB, quality, d_enc, enc_scratch, d_out, cap, d_len, s));
        HIPCHK(hipMemcpyAsync(len, d_len, sizeof(len), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
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
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    std::printf("%zu bytes in, %zu bytes out at quality %d\n", in.size(), file.size(), quality);
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_file)); HIPCHK(hipFree(d_frame)); HIPCHK(hipFree(d_dec)); HIPCHK(hipFree(d_enc)); HIPCHK(hipFree(d_status)); HIPCHK(hipFree(d_len));
    return 0;
}
