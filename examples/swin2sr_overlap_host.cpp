// Swin2SR's overlapped tiles with averaged seams (the authors' --tile / --tile_overlap) from a host with no Python and no torch in
// the process, through the C ABI of libnesr_hip.so (include/nesr_hip.h): builds the small two-stage configuration of the tests
// (embed 24, 2 x 2 layers of 2 heads, window 4, pixelshuffle x2), loads the weights from a flat float32 file that holds the state
// dict's tensors in transformers' order, asks nesr_swin2sr_overlap_plan for the plan of the frame and upscales one raw H x W x 3 RGB
// u8 frame with nesr_swin2sr_upscale_overlapped_u8: t x t windows of the frame padded once to the window, stepping by
// tile - tile_overlap, summed in float32 and divided by the number that covered each pixel; max_batch of them a launch (0: as many
// as the workspace budget holds).
//   hipcc -O2 --offload-arch=gfx950 -I include examples/swin2sr_overlap_host.cpp -o build/swin2sr_overlap_host -ldl
//   build/swin2sr_overlap_host path/to/libnesr_hip.so weights.f32 in.rgb H W tile tile_overlap out.rgb [max_batch]
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

struct Entry {
    std::string key;
    std::vector<int64_t> shape;
};

int main(int argc, char** argv) {
    if (argc < 9) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so weights.f32 in.rgb H W tile tile_overlap out.rgb [max_batch]\n", argv[0]);
        return 1;
    }
    const int H = std::atoi(argv[4]), W = std::atoi(argv[5]), tile = std::atoi(argv[6]), tile_overlap = std::atoi(argv[7]);
    const int max_batch = argc > 9 ? std::atoi(argv[9]) : 0;
    if (H < 1 || W < 1) { std::fprintf(stderr, "bad shape %s x %s\n", argv[4], argv[5]); return 1; }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_swin2sr_create) LOAD(nesr_swin2sr_destroy) LOAD(nesr_swin2sr_num_tensors)
    LOAD(nesr_swin2sr_load_weight) LOAD(nesr_swin2sr_finalize) LOAD(nesr_swin2sr_output_size) LOAD(nesr_swin2sr_overlap_plan)
    LOAD(nesr_swin2sr_overlap_workspace_bytes) LOAD(nesr_swin2sr_upscale_overlapped_u8) LOAD(nesr_swin2sr_kernel_time_ms)
    std::printf("%s\n", p_nesr_version());

    const int C = 24, heads = 2, hidden = 48, scale = 2, nf = 64, window = 4, depths[2] = {2, 2}, num_heads[2] = {heads, heads};
    nesr_swin2sr* ctx = nullptr;
    CHECK(p_nesr_swin2sr_create(&ctx, 0, /*image_size*/ 16, /*patch_size*/ 1, 3, 3, C, 2, depths, num_heads, window, /*mlp_ratio*/ 2.0,
                                /*qkv_bias*/ 1, /*use_absolute_embeddings*/ 0, /*layer_norm_eps*/ 1e-5, scale, /*img_range*/ 1.0, "1conv", "pixelshuffle"));

    // the state dict's keys and shapes, in transformers' order
    std::vector<Entry> spec;
    auto wb = [&](const std::string& name, std::vector<int64_t> w, bool bias = true) {
        const int64_t n = w[0];
        spec.push_back({name + ".weight", w});
        if (bias) spec.push_back({name + ".bias", {n}});
    };
    wb("swin2sr.first_convolution", {C, 3, 3, 3});
    wb("swin2sr.embeddings.patch_embeddings.projection", {C, C, 1, 1});
    wb("swin2sr.embeddings.patch_embeddings.layernorm", {C});
    for (int i = 0; i < 2; ++i) {
        const std::string s = "swin2sr.encoder.stages." + std::to_string(i);
        for (int j = 0; j < depths[i]; ++j) {
            const std::string l = s + ".layers." + std::to_string(j), a = l + ".attention.self";
            spec.push_back({a + ".logit_scale", {heads, 1, 1}});
            wb(a + ".continuous_position_bias_mlp.0", {512, 2});
            wb(a + ".continuous_position_bias_mlp.2", {heads, 512}, false);
            wb(a + ".query", {C, C});
            wb(a + ".key", {C, C}, false);
            wb(a + ".value", {C, C});
            wb(l + ".attention.output.dense", {C, C});
            wb(l + ".layernorm_before", {C});
            wb(l + ".intermediate.dense", {hidden, C});
            wb(l + ".output.dense", {C, hidden});
            wb(l + ".layernorm_after", {C});
        }
        wb(s + ".conv", {C, C, 3, 3});
        wb(s + ".patch_embed.projection", {C, C, 1, 1});
    }
    wb("swin2sr.layernorm", {C});
    wb("swin2sr.conv_after_body", {C, C, 3, 3});
    wb("upsample.conv_before_upsample", {nf, C, 3, 3});
    wb("upsample.upsample.convolution_0", {4 * nf, nf, 3, 3});
    wb("upsample.final_convolution", {3, nf, 3, 3});
    if ((int)spec.size() != p_nesr_swin2sr_num_tensors(ctx)) { std::fprintf(stderr, "the context waits for %d tensors, the host lists %zu\n", p_nesr_swin2sr_num_tensors(ctx), spec.size()); return 4; }

    FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    size_t total = 0;
    for (const Entry& e : spec) {
        size_t n = 1;
        for (int64_t d : e.shape) n *= (size_t)d;
        std::vector<float> w(n);
        if (std::fread(w.data(), sizeof(float), n, f) != n) { std::fprintf(stderr, "%s ends before %s\n", argv[2], e.key.c_str()); return 1; }
        CHECK(p_nesr_swin2sr_load_weight(ctx, e.key.c_str(), w.data(), e.shape.data(), (int)e.shape.size()));
        total += n;
    }
    std::fclose(f);
    CHECK(p_nesr_swin2sr_finalize(ctx));

    const size_t bytes = (size_t)H * W * 3;
    std::vector<uint8_t> img(bytes);
    f = std::fopen(argv[3], "rb");
    if (!f || std::fread(img.data(), 1, bytes, f) != bytes) { std::fprintf(stderr, "cannot read %zu bytes from %s\n", bytes, argv[3]); return 1; }
    std::fclose(f);
    int oh = 0, ow = 0;
    CHECK(p_nesr_swin2sr_output_size(scale, H, W, &oh, &ow));
    const size_t out_bytes = (size_t)oh * ow * 3;
    // the plan: the counts, the effective tile and the padded frame first, then one row per window {win_y, win_x, out_y, out_x}
    int tiles_y = 0, tiles_x = 0, t = 0, Hp = 0, Wp = 0;
    CHECK(p_nesr_swin2sr_overlap_plan(scale, window, H, W, tile, tile_overlap, &tiles_y, &tiles_x, &t, &Hp, &Wp, nullptr, 0));
    std::vector<int32_t> plan((size_t)tiles_y * tiles_x * 4);
    CHECK(p_nesr_swin2sr_overlap_plan(scale, window, H, W, tile, tile_overlap, &tiles_y, &tiles_x, &t, &Hp, &Wp, plan.data(), plan.size()));
    size_t ws_one = 0;
    CHECK(p_nesr_swin2sr_overlap_workspace_bytes(ctx, H, W, tile, tile_overlap, 1, &ws_one));
    uint8_t* d_img;
    uint8_t* d_out;
    HIPCHK(hipMalloc(&d_img, bytes));
    HIPCHK(hipMalloc(&d_out, out_bytes));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_img, img.data(), bytes, hipMemcpyHostToDevice, s));
    CHECK(p_nesr_swin2sr_upscale_overlapped_u8(ctx, d_img, H, W, tile, tile_overlap, max_batch, d_out, out_bytes, s));
    std::vector<uint8_t> out(out_bytes);
    HIPCHK(hipMemcpyAsync(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int64_t launches = 0;
    CHECK(p_nesr_swin2sr_kernel_time_ms(ctx, nullptr, 0, &launches));
    f = std::fopen(argv[8], "wb");
    if (!f || std::fwrite(out.data(), 1, out_bytes, f) != out_bytes || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[8]); return 1; }
    const int tiles = tiles_y * tiles_x, per_batch = 19 + 1;      // launches of one forward of this configuration, whatever its batch, and the accumulation
    std::printf("%zu tensors, %zu parameters; %d x %d -> %d x %d\n", spec.size(), total, H, W, oh, ow);
    std::printf("plan: %d windows (%d x %d) of %d x %d in %d x %d, %zu workspace bytes with one window a batch, %lld batches, %lld launches\n", tiles, tiles_y,
                tiles_x, t, t, Hp, Wp, ws_one, (long long)((launches - 1) / per_batch), (long long)launches);
    const int32_t* last = plan.data() + (size_t)(tiles - 1) * 4;
    std::printf("last window: at (%d, %d) -> (%d, %d)\n", last[0], last[1], last[2], last[3]);
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_img)); HIPCHK(hipFree(d_out));
    p_nesr_swin2sr_destroy(ctx);
    return 0;
}
