// Gray, BGRA and 16-bit frames from a host with no Python and no torch in the process, through the C ABI of libnesr_hip.so
// (include/nesr_hip.h): what RealESRGANer.enhance does for a 16-bit gray scan and for an 8-bit image with alpha, each as ONE call of
// nesr_enhance_frame -- the frame is uploaded as it is, packed, evaluated (the alpha plane a second time), clamped, quantised and
// downloaded in its own sample type.  Builds a 2-block x2plus network from a file of float32 weights in state_dict order
// (conv_first.weight, conv_first.bias, body.0.rdb1.conv1.weight, ...), reads a raw uint16 H x W gray frame and a raw uint8
// H x W x 4 BGRA frame, writes the upscaled frames raw.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/frame_host.cpp -o build/frame_host -ldl
//   build/frame_host path/to/libnesr_hip.so weights.f32 gray16.raw H W gray16_out.raw bgra8.raw H W bgra8_out.raw
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "nesr_hip.h"

#define LOAD(name) auto p_##name = reinterpret_cast<decltype(&name)>(dlsym(lib, #name)); if (!p_##name) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s -> %s\n", #call, hipGetErrorString(e_)); return 5; } } while (0)
#define CHECK(call) do { int rc_ = (call); if (rc_ != 0) { std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, p_nesr_last_error()); return 3; } } while (0)

static bool read_file(const char* path, void* buf, size_t bytes) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(buf, 1, bytes, f);
    std::fclose(f);
    return got == bytes;
}

static bool write_file(const char* path, const void* buf, size_t bytes) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const size_t put = std::fwrite(buf, 1, bytes, f);
    return std::fclose(f) == 0 && put == bytes;
}

int main(int argc, char** argv) {
    if (argc < 11) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so weights.f32 gray16.raw H W gray16_out.raw bgra8.raw H W bgra8_out.raw\n", argv[0]);
        return 1;
    }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_create) LOAD(nesr_load_weight) LOAD(nesr_finalize_weights) LOAD(nesr_destroy) LOAD(nesr_last_error) LOAD(nesr_version)
    LOAD(nesr_frame_scratch_bytes) LOAD(nesr_enhance_frame) LOAD(nesr_check_range)
    std::printf("%s\n", p_nesr_version());

    const int nf = 64, gc = 32, nb = 2, scale = 2;
    nesr_ctx* ctx = nullptr;
    CHECK(p_nesr_create(&ctx, 0, 12, 2, nf, nb, gc, 3, NESR_DTYPE_F32_SPLIT));
    FILE* wf = std::fopen(argv[2], "rb");
    if (!wf) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    auto conv = [&](const std::string& name, int cin, int cout) -> int {
        std::vector<float> w((size_t)cout * cin * 9), b(cout);
        if (std::fread(w.data(), 4, w.size(), wf) != w.size() || std::fread(b.data(), 4, b.size(), wf) != b.size()) {
            std::fprintf(stderr, "%s ends before %s\n", argv[2], name.c_str());
            return 1;
        }
        const int64_t ws[4] = {cout, cin, 3, 3}, bs[1] = {cout};
        CHECK(p_nesr_load_weight(ctx, (name + ".weight").c_str(), w.data(), ws, 4));
        CHECK(p_nesr_load_weight(ctx, (name + ".bias").c_str(), b.data(), bs, 1));
        return 0;
    };
    if (conv("conv_first", 12, nf)) return 3;
    for (int b = 0; b < nb; ++b)
        for (int r = 1; r <= 3; ++r) {
            const std::string pre = "body." + std::to_string(b) + ".rdb" + std::to_string(r) + ".conv";
            for (int k = 1; k <= 4; ++k)
                if (conv(pre + std::to_string(k), nf + (k - 1) * gc, gc)) return 3;
            if (conv(pre + "5", nf + 4 * gc, nf)) return 3;
        }
    for (const char* n : {"conv_body", "conv_up1", "conv_up2", "conv_hr"})
        if (conv(n, nf, nf)) return 3;
    if (conv("conv_last", nf, 3)) return 3;
    std::fclose(wf);
    CHECK(p_nesr_finalize_weights(ctx));

    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    // one frame: upload, nesr_enhance_frame, download; the range check before the result is trusted
    auto run = [&](const char* in_path, int H, int W, int channels, int bits, int max_range, const char* out_path) -> int {
        const size_t in_bytes = (size_t)H * W * channels * (bits / 8);
        const size_t out_bytes = in_bytes * scale * scale * (max_range == 65535 ? 2 : 1) / (bits / 8);
        std::vector<uint8_t> in(in_bytes), out(out_bytes);
        if (!read_file(in_path, in.data(), in_bytes)) { std::fprintf(stderr, "cannot read %zu bytes from %s\n", in_bytes, in_path); return 1; }
        const size_t scratch_bytes = p_nesr_frame_scratch_bytes(ctx, H, W, channels, NESR_ALPHA_NETWORK);
        if (!scratch_bytes) { std::fprintf(stderr, "nesr_frame_scratch_bytes: %s\n", p_nesr_last_error()); return 3; }
        void *d_in, *d_out, *d_scratch;
        HIPCHK(hipMalloc(&d_in, in_bytes)); HIPCHK(hipMalloc(&d_out, out_bytes)); HIPCHK(hipMalloc(&d_scratch, scratch_bytes));
        HIPCHK(hipMemcpyAsync(d_in, in.data(), in_bytes, hipMemcpyHostToDevice, s));
        CHECK(p_nesr_enhance_frame(ctx, d_in, H, W, channels, bits, max_range, NESR_ALPHA_NETWORK, 0, d_scratch, scratch_bytes, d_out, s));
        HIPCHK(hipMemcpyAsync(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        CHECK(p_nesr_check_range(ctx, s));
        std::printf("%d x %d x %d, %d bits, range %d -> %d x %d: %zu bytes up, %zu bytes down, scratch %zu bytes\n", H, W, channels, bits, max_range,
                    H * scale, W * scale, in_bytes, out_bytes, scratch_bytes);
        if (!write_file(out_path, out.data(), out_bytes)) { std::fprintf(stderr, "cannot write %s\n", out_path); return 1; }
        HIPCHK(hipFree(d_in)); HIPCHK(hipFree(d_out)); HIPCHK(hipFree(d_scratch));
        return 0;
    };
    if (int rc = run(argv[3], std::atoi(argv[4]), std::atoi(argv[5]), 1, 16, 65535, argv[6])) return rc;
    if (int rc = run(argv[7], std::atoi(argv[8]), std::atoi(argv[9]), 4, 8, 255, argv[10])) return rc;
    HIPCHK(hipStreamDestroy(s));
    p_nesr_destroy(ctx);
    return 0;
}
