// One iteration of SuperResolutionPipeline.enhance_image (nesr/nesr.py:516-633, diffusion and segmentation off) from a host with no
// Python and no torch in the process, through the C ABI of libnesr_hip.so (include/nesr_hip.h), as three calls on device buffers:
//     nesr_preprocess_u8      _preprocess_image   (NL-means denoise + CLAHE on L)
//     nesr_apply_esrgan_u8    _apply_esrgan       (routed by nesr_stage_route: the 12-channel network, untiled or through the tiler)
//     nesr_postprocess_u8     _postprocess_image  (adaptive unsharp)
// and nesr_check_range before the result is trusted.  The network is the reference's RRDBNet(num_in_ch=12) (nesr/nesr.py:216) with
// one block and weights from a counter-based generator (no checkpoint ships with the reference); the frame is synthetic too.  Both
// are functions of `seed` that a test can restate (tests/test_gpu_pipeline_host.py).  The raw RGB u8 result goes to out.rgb.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/pipeline_host.cpp -o build/pipeline_host -ldl
//   build/pipeline_host path/to/libnesr_hip.so H W max_tile_size cuda_megapixel_threshold seed out.rgb
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "nesr_hip.h"

#pragma clang fp contract(off)

#define LOAD(name) auto p_##name = reinterpret_cast<decltype(&name)>(dlsym(lib, #name)); if (!p_##name) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s -> %s\n", #call, hipGetErrorString(e_)); return 5; } } while (0)
#define CHECK(call) do { int rc_ = (call); if (rc_ != 0) { std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, p_nesr_last_error()); return 3; } } while (0)

// lowbias32: a hash of the counter, so that element i of the stream is a function of (seed, i) alone
static uint32_t mix(uint32_t seed, uint32_t i) {
    uint32_t h = i + seed * 0x9E3779B9u;
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}
// uniform in [-1, 1): 24 bits, every step exact in float32
static float uniform(uint32_t seed, uint32_t i) { return (float)(mix(seed, i) >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; }

int main(int argc, char** argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so H W max_tile_size cuda_megapixel_threshold seed out.rgb\n", argv[0]);
        return 1;
    }
    const int H = std::atoi(argv[2]), W = std::atoi(argv[3]), tile = std::atoi(argv[4]);
    const double threshold_mp = std::atof(argv[5]);
    const uint32_t seed = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    if (H < 2 || W < 2 || tile < 1) { std::fprintf(stderr, "bad size %s x %s, tile %s\n", argv[2], argv[3], argv[4]); return 1; }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_create) LOAD(nesr_load_weight) LOAD(nesr_finalize_weights) LOAD(nesr_destroy) LOAD(nesr_last_error) LOAD(nesr_version)
    LOAD(nesr_preprocess_scratch_bytes) LOAD(nesr_preprocess_u8) LOAD(nesr_postprocess_u8) LOAD(nesr_stage_route) LOAD(nesr_stage_tile_plan)
    LOAD(nesr_apply_esrgan_scratch_bytes) LOAD(nesr_apply_esrgan_u8) LOAD(nesr_check_range)
    std::printf("%s\n", p_nesr_version());

    // the network: weights uniform in +-gain / sqrt(fan_in) (gain 0.7 inside the dense blocks), biases in +-0.02, conv_last's + 0.5
    const int nf = 64, gc = 32, nb = 1;
    nesr_ctx* ctx = nullptr;
    CHECK(p_nesr_create(&ctx, 0, 12, 0, nf, nb, gc, 3, NESR_DTYPE_F32_SPLIT));
    uint32_t counter = 0;
    auto conv = [&](const std::string& name, int cin, int cout, double gain, float bias_shift) -> int {
        std::vector<float> w((size_t)cout * cin * 9), b(cout);
        const float bound = (float)(gain / std::sqrt((double)(cin * 9)));
        for (float& v : w) v = uniform(seed, counter++) * bound;
        for (float& v : b) v = uniform(seed, counter++) * 0.02f + bias_shift;
        const int64_t ws[4] = {cout, cin, 3, 3}, bs[1] = {cout};
        CHECK(p_nesr_load_weight(ctx, (name + ".weight").c_str(), w.data(), ws, 4));
        CHECK(p_nesr_load_weight(ctx, (name + ".bias").c_str(), b.data(), bs, 1));
        return 0;
    };
    if (conv("conv_first", 12, nf, 1.0, 0.f)) return 3;
    for (int b = 0; b < nb; ++b)
        for (int r = 1; r <= 3; ++r) {
            const std::string pre = "body." + std::to_string(b) + ".rdb" + std::to_string(r) + ".conv";
            for (int k = 1; k <= 4; ++k)
                if (conv(pre + std::to_string(k), nf + (k - 1) * gc, gc, 0.7, 0.f)) return 3;
            if (conv(pre + "5", nf + 4 * gc, nf, 0.7, 0.f)) return 3;
        }
    for (const char* n : {"conv_body", "conv_up1", "conv_up2", "conv_hr"})
        if (conv(n, nf, nf, 1.0, 0.f)) return 3;
    if (conv("conv_last", nf, 3, 1.0, 0.5f)) return 3;
    CHECK(p_nesr_finalize_weights(ctx));

    // the frame: a colour gradient with three bits of noise
    std::vector<uint8_t> img((size_t)H * W * 3);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int c = 0; c < 3; ++c) {
                const uint32_t i = (uint32_t)((y * W + x) * 3 + c);
                img[i] = (uint8_t)((x * 5 + y * 3 + c * 61 + (int)(mix(seed + 1, i) >> 29) * 4) & 255);
            }

    // the route and the sizes of one iteration with the reference's defaults: upscale_factor 2.0, padding 16, the large-image literal 16
    const double upscale_factor = 2.0, large_mp = 16.0, denoise_level = 0.5;
    const int padding = 16;
    int tiled = 0, mode = 0, ntiles = 0;
    CHECK(p_nesr_stage_route(H, W, 1, 0, threshold_mp, large_mp, &tiled, &mode));
    CHECK(p_nesr_stage_tile_plan(H, W, tile, padding, upscale_factor, 4, nullptr, 0, &ntiles));
    const bool canvas = tiled && ntiles > 1;      // a frame that fits one tile comes back at the network's own scale
    const int Ho = canvas ? (int)(H * upscale_factor) : 4 * H, Wo = canvas ? (int)(W * upscale_factor) : 4 * W;
    const size_t in_bytes = img.size(), out_bytes = (size_t)Ho * Wo * 3;
    const size_t pre_scratch = p_nesr_preprocess_scratch_bytes(H, W), stage_scratch = p_nesr_apply_esrgan_scratch_bytes(ctx, H, W, tiled, tile, padding);
    if (!pre_scratch || !stage_scratch) { std::fprintf(stderr, "scratch sizes: %s\n", p_nesr_last_error()); return 3; }

    uint8_t *d_img, *d_pre, *d_up, *d_out;
    void *d_s0, *d_s1;
    HIPCHK(hipMalloc(&d_img, in_bytes)); HIPCHK(hipMalloc(&d_pre, in_bytes)); HIPCHK(hipMalloc(&d_up, out_bytes)); HIPCHK(hipMalloc(&d_out, out_bytes));
    HIPCHK(hipMalloc(&d_s0, pre_scratch)); HIPCHK(hipMalloc(&d_s1, stage_scratch));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_img, img.data(), in_bytes, hipMemcpyHostToDevice, s));
    CHECK(p_nesr_preprocess_u8(0, d_img, H, W, denoise_level, d_s0, pre_scratch, d_pre, s));
    CHECK(p_nesr_apply_esrgan_u8(ctx, d_pre, H, W, mode, tiled, tile, padding, upscale_factor, d_s1, stage_scratch, d_up, s));
    CHECK(p_nesr_postprocess_u8(0, d_up, Ho, Wo, 1, d_out, s));
    std::vector<uint8_t> out(out_bytes);
    HIPCHK(hipMemcpyAsync(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    CHECK(p_nesr_check_range(ctx, s));
    std::printf("%d x %d -> %d x %d: %s, %d tile%s, %s; scratch %zu + %zu bytes\n", H, W, Ho, Wo, tiled ? "tiled" : "untiled", ntiles, ntiles == 1 ? "" : "s",
                mode == NESR_INPUT_12CH ? "12-channel" : "3-channel x 4", pre_scratch, stage_scratch);
    FILE* f = std::fopen(argv[7], "wb");
    if (!f || std::fwrite(out.data(), 1, out_bytes, f) != out_bytes || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[7]); return 1; }
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_img)); HIPCHK(hipFree(d_pre)); HIPCHK(hipFree(d_up)); HIPCHK(hipFree(d_out)); HIPCHK(hipFree(d_s0)); HIPCHK(hipFree(d_s1));
    p_nesr_destroy(ctx);
    return 0;
}
