// cv2.imread(path.png, cv2.IMREAD_UNCHANGED) ... cv2.imwrite(path.png, frame) -- what standalone/direct_esrgan.py:130 and :169 do
// around the network for a PNG input -- from a host with no Python and no torch in the process, through the C ABI of libnesr_hip.so
// (include/nesr_hip.h): the file's bytes go up, nesr_png_parse reads the chunks and plans the segments on the host, nesr_png_decode
// inflates and unfilters on the device, nesr_png_encode writes the frame as a PNG file again there, and only the new file comes back.
// A file whose deflate segments span IDAT boundaries (libpng's 8 KiB IDATs) needs the host's zlib first (imgproc.decode_png's hybrid
// route); this program takes the contiguous plans: files of nesr_png_encode, of Z_FULL_FLUSH writers, and files of one IDAT.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/png_decode_host.cpp -o build/png_decode_host -ldl
//   build/png_decode_host path/to/libnesr_hip.so in.png out.png
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
        std::fprintf(stderr, "usage: %s libnesr_hip.so in.png out.png\n", argv[0]);
        return 1;
    }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_png_parse) LOAD(nesr_png_decode_scratch_bytes) LOAD(nesr_png_decode)
    LOAD(nesr_png_bound) LOAD(nesr_png_scratch_bytes) LOAD(nesr_png_encode)
    std::printf("%s\n", p_nesr_version());

    std::vector<uint8_t> in;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
    for (int ch; (ch = std::fgetc(f)) != EOF;) in.push_back((uint8_t)ch);
    std::fclose(f);

    nesr_png_info info;
    int rc = p_nesr_png_parse(in.data(), in.size(), &info, nullptr, 0);            // host only; the first call sizes the table
    if (rc != NESR_ERR_NOFIT) { std::fprintf(stderr, "nesr_png_parse -> %d: %s\n", rc, p_nesr_last_error()); return 3; }
    std::vector<nesr_png_segment> segs((size_t)info.n_segments);
    CHECK(p_nesr_png_parse(in.data(), in.size(), &info, segs.data(), info.n_segments));
    const int H = info.H, W = info.W, C = info.C, depth = info.depth;
    std::printf("%d x %d x %d, %d bit, %d segment%s, %s\n", H, W, C, depth, info.n_segments, info.n_segments == 1 ? "" : "s",
                info.contiguous ? "contiguous" : "not contiguous");
    if (!info.contiguous) { std::fprintf(stderr, "a segment spans an IDAT boundary: inflate on the host, then nesr_png_unfilter\n"); return 4; }
    const int64_t row_bytes = (int64_t)W * C * depth / 8;
    const size_t frame_bytes = (size_t)H * row_bytes, seg_bytes = segs.size() * sizeof(nesr_png_segment);
    const size_t dec_scratch = p_nesr_png_decode_scratch_bytes(&info), enc_scratch = p_nesr_png_scratch_bytes(H, W, C, depth);
    const size_t cap = p_nesr_png_bound(H, W, C, depth);

    uint8_t *d_file, *d_frame, *d_out;
    nesr_png_segment* d_segs;
    void *d_dec, *d_enc;
    uint32_t* d_status;
    uint64_t* d_len;
    HIPCHK(hipMalloc(&d_file, in.size()));
    HIPCHK(hipMalloc(&d_segs, seg_bytes));
    HIPCHK(hipMalloc(&d_frame, frame_bytes));
    HIPCHK(hipMalloc(&d_dec, dec_scratch));
    HIPCHK(hipMalloc(&d_enc, enc_scratch));
    HIPCHK(hipMalloc(&d_out, cap));
    HIPCHK(hipMalloc(&d_status, sizeof(uint32_t)));
    HIPCHK(hipMalloc(&d_len, 2 * sizeof(uint64_t)));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_file, in.data(), in.size(), hipMemcpyHostToDevice, s));      // only the file and its plan cross to the device
    HIPCHK(hipMemcpyAsync(d_segs, segs.data(), seg_bytes, hipMemcpyHostToDevice, s));
    CHECK(p_nesr_png_decode(0, d_file, in.size(), &info, d_segs, d_frame, row_bytes, NESR_ORDER_RGB, d_dec, dec_scratch, d_status, s));
    uint32_t status = 0;
    HIPCHK(hipMemcpyAsync(&status, d_status, sizeof(status), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (status != 0) { std::fprintf(stderr, "the device rejected the file, status 0x%x (%d)\n", status, (int)NESR_ERR_BADFILE); return 4; }

    uint64_t len[2] = {0, 0};
    CHECK(p_nesr_png_encode(0, d_frame, row_bytes, H, W, C, depth, NESR_ORDER_RGB, d_enc, enc_scratch, d_out, cap, d_len, s));
    HIPCHK(hipMemcpyAsync(len, d_len, sizeof(len), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (len[1] != 0) { std::fprintf(stderr, "the file did not fit nesr_png_bound (%d)\n", (int)NESR_ERR_NOFIT); return 4; }
    std::vector<uint8_t> file(len[0]);
    HIPCHK(hipMemcpy(file.data(), d_out, len[0], hipMemcpyDeviceToHost));               // only the file crosses to the host
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    std::printf("%zu bytes in, %zu bytes out\n", in.size(), file.size());
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_file)); HIPCHK(hipFree(d_segs)); HIPCHK(hipFree(d_frame)); HIPCHK(hipFree(d_dec)); HIPCHK(hipFree(d_enc)); HIPCHK(hipFree(d_out));
    HIPCHK(hipFree(d_status)); HIPCHK(hipFree(d_len));
    return 0;
}
