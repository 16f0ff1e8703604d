// A torch-free host that evaluates ONE untiled frame as row bands on two contexts of this process (include/nesr_hip.h:
// nesr_forward_banded_u8): what RealESRGANer(devices=[...], tile=0) does, from C++.  Builds a 2-block x2plus network from seeded
// weights three times -- the whole-frame context, and two band contexts on device 0, or on devices 0 and 1 when two are visible --
// runs a 96x128 BGR frame through nesr_forward_u8 and through nesr_forward_banded_u8, and compares the two byte for byte.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/banded_host.cpp -o build/nesr_banded_host -ldl && build/nesr_banded_host path/to/libnesr_hip.so
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "nesr_hip.h"

#define LOAD(name) auto p_##name = reinterpret_cast<decltype(&name)>(dlsym(lib, #name)); if (!p_##name) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s -> %s\n", #call, hipGetErrorString(e_)); return 5; } } while (0)
#define CHECK(call) do { int rc_ = (call); if (rc_ != 0) { std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, p_nesr_last_error()); return 3; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static float uniform() {   // splitmix64 -> [-1, 1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)((double)(z >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s libnesr_hip.so\n", argv[0]); return 1; }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_create) LOAD(nesr_load_weight) LOAD(nesr_finalize_weights) LOAD(nesr_forward_u8) LOAD(nesr_forward_banded_u8) LOAD(nesr_band_plan)
    LOAD(nesr_band_link_state) LOAD(nesr_check_range) LOAD(nesr_check_status) LOAD(nesr_destroy) LOAD(nesr_last_error) LOAD(nesr_version)
    std::printf("%s\n", p_nesr_version());

    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    const int nf = 64, gc = 32, nb = 2, H = 96, W = 128;
    const int devs[3] = {0, 0, ndev >= 2 ? 1 : 0};      // whole frame, upper band, lower band
    nesr_ctx* ctx[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; ++i) CHECK(p_nesr_create(&ctx[i], devs[i], 12, 2, nf, nb, gc, 3, NESR_DTYPE_F32_SPLIT));
    auto conv = [&](const std::string& name, int cin, int cout) -> int {
        std::vector<float> w((size_t)cout * cin * 9), b(cout);
        const float sc = 0.5f * std::sqrt(2.0f / (cin * 9.0f));
        for (auto& v : w) v = uniform() * sc;
        for (auto& v : b) v = uniform() * 0.01f;
        const int64_t ws[4] = {cout, cin, 3, 3}, bs[1] = {cout};
        for (nesr_ctx* c : ctx) {
            CHECK(p_nesr_load_weight(c, (name + ".weight").c_str(), w.data(), ws, 4));
            CHECK(p_nesr_load_weight(c, (name + ".bias").c_str(), b.data(), bs, 1));
        }
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
    for (nesr_ctx* c : ctx) CHECK(p_nesr_finalize_weights(c));

    int lo_hi[4];
    CHECK(p_nesr_band_plan(H / 2, 2, lo_hi, 2));
    std::printf("%d internal rows as bands [%d, %d) on device %d and [%d, %d) on device %d\n", H / 2, lo_hi[0], lo_hi[1], devs[1], lo_hi[2], lo_hi[3], devs[2]);

    std::vector<uint8_t> img((size_t)H * W * 3);
    for (auto& v : img) v = (uint8_t)((uniform() * 0.5f + 0.5f) * 255.0f);
    const size_t out_bytes = (size_t)4 * H * W * 3;
    uint8_t *dimg, *dwhole, *dband;
    HIPCHK(hipSetDevice(0));
    HIPCHK(hipMalloc(&dimg, img.size())); HIPCHK(hipMalloc(&dwhole, out_bytes)); HIPCHK(hipMalloc(&dband, out_bytes));
    HIPCHK(hipMemcpy(dimg, img.data(), img.size(), hipMemcpyHostToDevice));
    CHECK(p_nesr_forward_u8(ctx[0], dimg, H, W, dwhole, 1, NESR_ROUND_NEAREST, nullptr));
    HIPCHK(hipDeviceSynchronize());
    CHECK(p_nesr_check_status(ctx[0]));
    // two frames: the second one starts from the landing buffers and events the first one left
    for (int frame = 0; frame < 2; ++frame) {
        HIPCHK(hipSetDevice(0));
        HIPCHK(hipMemset(dband, 0, out_bytes));
        HIPCHK(hipDeviceSynchronize());
        CHECK(p_nesr_forward_banded_u8(&ctx[1], 2, dimg, H, W, 1, NESR_ROUND_NEAREST, dband, nullptr));   // streams the contexts own
        for (int d = 0; d < (ndev >= 2 ? 2 : 1); ++d) { HIPCHK(hipSetDevice(d)); HIPCHK(hipDeviceSynchronize()); }
        CHECK(p_nesr_check_range(ctx[1], nullptr));
        CHECK(p_nesr_check_range(ctx[2], nullptr));
    }
    const int st = p_nesr_band_link_state(ctx[1]);
    std::printf("link of the upper band to the lower one: %s\n", !(st & 8) ? "staged (packed, then a device-to-device copy)"
                                                                  : ((st & 32) ? "peer-written (another device)" : "local (the plain pointer)"));
    HIPCHK(hipSetDevice(0));
    std::vector<uint8_t> a(out_bytes), b(out_bytes);
    HIPCHK(hipMemcpy(a.data(), dwhole, out_bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(b.data(), dband, out_bytes, hipMemcpyDeviceToHost));
    size_t differ = 0, nonzero = 0;
    for (size_t i = 0; i < out_bytes; ++i) { differ += a[i] != b[i]; nonzero += a[i] != 0; }
    std::printf("output %dx%d, banded vs whole frame: %zu bytes differ (%zu of %zu non-zero)\n", 2 * H, 2 * W, differ, nonzero, out_bytes);
    for (nesr_ctx* c : ctx) p_nesr_destroy(c);
    HIPCHK(hipSetDevice(0));
    HIPCHK(hipFree(dimg)); HIPCHK(hipFree(dwhole)); HIPCHK(hipFree(dband));
    return (differ == 0 && nonzero > out_bytes / 2) ? 0 : 4;
}
