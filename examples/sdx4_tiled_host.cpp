// The x4 diffusion upscaler over windows from a host with no Python and no torch in the process, through the C ABI of
// libnesr_hip.so (include/nesr_hip.h): sdx4_host.cpp's contexts and inputs, then nesr_sdx4_tile_plan, nesr_sdx4_tiled_workspace_bytes
// (neither needs the device) and one nesr_sdx4_upscale_tiled_u8: the denoising loop and the VAE decode over overlapping windows, so
// the frame may exceed NESR_VAE_MAX_TOKENS low-res pixels.  Its sides must be multiples of 2^(UNet levels - 1).
//   hipcc -O2 --offload-arch=gfx950 -I include examples/sdx4_tiled_host.cpp -o build/sdx4_tiled_host -ldl
//   build/sdx4_tiled_host path/to/libnesr_hip.so weights.f32|seed:N frame.ppm ids.i32|- noise.f32|- latents.f32|- tokens noise_level steps guidance out.ppm
//                         tile tile_overlap [published|crafted [vae_tile vae_overlap]]
#include "sdx4_host_common.h"

int main(int argc, char** argv) {
    if (argc < 14) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so weights.f32|seed:N frame.ppm ids.i32|- noise.f32|- latents.f32|- tokens noise_level steps guidance out.ppm "
                             "tile tile_overlap [published|crafted [vae_tile vae_overlap]]\n", argv[0]);
        return 1;
    }
    const int tile = std::atoi(argv[12]), tile_overlap = std::atoi(argv[13]);
    const int vae_tile = argc > 16 ? std::atoi(argv[15]) : 0, vae_overlap = argc > 16 ? std::atoi(argv[16]) : -1;      // 0 and -1: the loop's plan
    const int tokens = std::atoi(argv[7]), noise_level = std::atoi(argv[8]), steps = std::atoi(argv[9]);
    const double guidance = std::atof(argv[10]);
    const bool crafted = argc > 14 && std::string(argv[14]) == "crafted";
    const bool synthetic = std::strncmp(argv[2], "seed:", 5) == 0;
    const uint64_t seed = synthetic ? std::strtoull(argv[2] + 5, nullptr, 10) : 0;
    const int n = guidance > 1.0 ? 2 : 1, lat = 4, cin = 7;

    // the frame: a binary PPM (P6, maxval 255)
    int w = 0, h = 0, maxval = 0;
    std::vector<uint8_t> frame;
    {
        FILE* f = std::fopen(argv[3], "rb");
        if (!f || std::fscanf(f, "P6 %d %d %d", &w, &h, &maxval) != 3 || maxval != 255 || w < 1 || h < 1 || std::fgetc(f) == EOF) { std::fprintf(stderr, "%s is no binary PPM of 8 bits\n", argv[3]); return 1; }
        frame.resize((size_t)h * w * 3);
        if (std::fread(frame.data(), 1, frame.size(), f) != frame.size()) { std::fprintf(stderr, "%s ends early\n", argv[3]); return 1; }
        std::fclose(f);
    }

    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_clip_text_create) LOAD(nesr_clip_text_destroy) LOAD(nesr_clip_text_num_tensors) LOAD(nesr_clip_text_load_weight)
    LOAD(nesr_clip_text_finalize) LOAD(nesr_unet_create) LOAD(nesr_unet_destroy) LOAD(nesr_unet_num_tensors) LOAD(nesr_unet_load_weight) LOAD(nesr_unet_finalize)
    LOAD(nesr_vae_create) LOAD(nesr_vae_destroy) LOAD(nesr_vae_num_tensors) LOAD(nesr_vae_load_weight) LOAD(nesr_vae_finalize) LOAD(nesr_sdx4_create) LOAD(nesr_sdx4_destroy)
    LOAD(nesr_sdx4_tile_plan) LOAD(nesr_sdx4_tiled_workspace_bytes) LOAD(nesr_sdx4_upscale_tiled_u8) LOAD(nesr_sdx4_launches)
    std::printf("%s\n", p_nesr_version());

    // the configuration
    const int vocab = crafted ? 50 : 49408, hidden = crafted ? 32 : 1024, inter = crafted ? 64 : 4096, tlayers = crafted ? 2 : 23, theads = crafted ? 4 : 16, positions = 77;
    const std::vector<int> widths = crafted ? std::vector<int>{32, 64} : std::vector<int>{256, 512, 512, 1024};
    const std::vector<int> attention = crafted ? std::vector<int>{1, 1} : std::vector<int>{0, 1, 1, 1}, only_cross = crafted ? std::vector<int>{1, 0} : std::vector<int>{1, 1, 1, 0};
    const int groups = crafted ? 8 : 32, heads = crafted ? 2 : 8, layers = crafted ? 1 : 2, cross = hidden, classes = crafted ? 32 : 1000, max_noise_level = crafted ? 31 : 350;
    const std::vector<int> vwidths = crafted ? std::vector<int>{32, 32, 64} : std::vector<int>{128, 256, 512};
    const int vlayers = crafted ? 1 : 2, L = (int)widths.size();

    nesr_clip_text* text = nullptr;
    nesr_unet* unet = nullptr;
    nesr_vae* vae = nullptr;
    CHECK(p_nesr_clip_text_create(&text, 0, vocab, hidden, inter, tlayers, theads, positions, 1e-5, "gelu"));
    std::vector<const char*> down(L), up(L);
    for (int i = 0; i < L; ++i) down[i] = attention[i] ? "CrossAttnDownBlock2D" : "DownBlock2D", up[L - 1 - i] = attention[i] ? "CrossAttnUpBlock2D" : "UpBlock2D";
    CHECK(p_nesr_unet_create(&unet, 0, cin, lat, L, widths.data(), down.data(), up.data(), "UNetMidBlock2DCrossAttn", only_cross.data(), layers, heads, cross, 1, 1, 0, classes,
                             groups, 1e-5, 1, 0.0, 1, "silu"));
    CHECK(p_nesr_vae_create(&vae, 0, lat, 3, (int)vwidths.size(), vwidths.data(), vlayers, groups, 0.08333, "silu"));

    const Spec specs[3] = {text_spec(vocab, hidden, inter, tlayers, positions), unet_spec(widths, attention, only_cross, layers, cross, classes, cin, lat),
                           vae_spec(vwidths, vlayers, lat, 3)};
    if ((int)specs[0].size() != p_nesr_clip_text_num_tensors(text) || (int)specs[1].size() != p_nesr_unet_num_tensors(unet) || (int)specs[2].size() != p_nesr_vae_num_tensors(vae)) {
        std::fprintf(stderr, "the contexts wait for %d + %d + %d tensors, the host lists %zu + %zu + %zu\n", p_nesr_clip_text_num_tensors(text), p_nesr_unet_num_tensors(unet),
                     p_nesr_vae_num_tensors(vae), specs[0].size(), specs[1].size(), specs[2].size());
        return 4;
    }
    FILE* wf = synthetic ? nullptr : std::fopen(argv[2], "rb");
    if (!synthetic && !wf) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    size_t total = 0, stream = 0;
    for (int m = 0; m < 3; ++m)
        for (const Entry& e : specs[m]) {
            size_t count = 1;
            for (int64_t d : e.shape) count *= (size_t)d;
            std::vector<float> v(count);
            if (!fill(v, e, wf, seed, stream++)) { std::fprintf(stderr, "%s ends before %s\n", argv[2], e.key.c_str()); return 1; }
            if (m == 0) CHECK(p_nesr_clip_text_load_weight(text, e.key.c_str(), v.data(), e.shape.data(), (int)e.shape.size()));
            if (m == 1) CHECK(p_nesr_unet_load_weight(unet, e.key.c_str(), v.data(), e.shape.data(), (int)e.shape.size()));
            if (m == 2) CHECK(p_nesr_vae_load_weight(vae, e.key.c_str(), v.data(), e.shape.data(), (int)e.shape.size()));
            total += count;
        }
    if (wf) std::fclose(wf);
    CHECK(p_nesr_clip_text_finalize(text));
    CHECK(p_nesr_unet_finalize(unet));
    CHECK(p_nesr_vae_finalize(vae));

    nesr_sdx4* pipe = nullptr;
    CHECK(p_nesr_sdx4_create(&pipe, text, unet, vae, 1000, 1e-4, 0.02, "scaled_linear", "v_prediction", 0, 0, 1, "leading", 0.0, 1000, "squaredcos_cap_v2", max_noise_level));

    // ids, noise, latents: files, or this host's own generator
    std::vector<int32_t> ids((size_t)n * tokens);
    std::vector<float> noise((size_t)3 * h * w), latents((size_t)lat * h * w);
    if (std::string(argv[4]) == "-") {      // begin-of-text, then end-of-text to the end: the empty prompt, for every sample
        for (size_t i = 0; i < ids.size(); ++i) ids[i] = i % tokens == 0 ? vocab - 2 : vocab - 1;
    } else if (!read_raw(argv[4], ids)) return 1;
    if (std::string(argv[5]) == "-") for (size_t i = 0; i < noise.size(); ++i) noise[i] = normal(seed, 1u << 20, i);
    else if (!read_raw(argv[5], noise)) return 1;
    if (std::string(argv[6]) == "-") for (size_t i = 0; i < latents.size(); ++i) latents[i] = normal(seed, (1u << 20) + 1, i);
    else if (!read_raw(argv[6], latents)) return 1;

    // the plan and the pipeline's own bytes: neither needs the device
    int tiles_y = 0, tiles_x = 0, ty = 0, tx = 0;
    CHECK(p_nesr_sdx4_tile_plan(h, w, 1 << (L - 1), tile, tile_overlap, &tiles_y, &tiles_x, &ty, &tx, nullptr, 0));
    std::vector<int32_t> plan((size_t)2 * tiles_y * tiles_x);
    CHECK(p_nesr_sdx4_tile_plan(h, w, 1 << (L - 1), tile, tile_overlap, &tiles_y, &tiles_x, &ty, &tx, plan.data(), plan.size()));
    size_t ws = 0;
    CHECK(p_nesr_sdx4_tiled_workspace_bytes(n, lat, hidden, 4, h, w, tokens, 1 << (L - 1), tile, tile_overlap, vae_tile, vae_overlap, &ws));
    const size_t out_bytes = (size_t)3 * 4 * h * 4 * w;
    uint8_t *d_frame, *d_out;
    float *d_noise, *d_latents;
    HIPCHK(hipMalloc(&d_frame, frame.size()));
    HIPCHK(hipMalloc(&d_out, out_bytes));
    HIPCHK(hipMalloc(&d_noise, noise.size() * sizeof(float)));
    HIPCHK(hipMalloc(&d_latents, latents.size() * sizeof(float)));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_frame, frame.data(), frame.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_noise, noise.data(), noise.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_latents, latents.data(), latents.size() * sizeof(float), hipMemcpyHostToDevice, s));
    CHECK(p_nesr_sdx4_upscale_tiled_u8(pipe, d_frame, h, w, ids.data(), tokens, d_noise, d_latents, noise_level, steps, guidance, tile, tile_overlap, vae_tile, vae_overlap, d_out,
                                       out_bytes, nullptr, s));
    std::vector<uint8_t> out(out_bytes);
    HIPCHK(hipMemcpyAsync(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int64_t launches = 0;
    CHECK(p_nesr_sdx4_launches(pipe, &launches));
    FILE* f = std::fopen(argv[11], "wb");
    if (!f || std::fprintf(f, "P6\n%d %d\n255\n", 4 * w, 4 * h) < 0 || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[11]); return 1; }
    std::printf("%zu + %zu + %zu tensors, %zu parameters; %d x %d -> %d x %d, %d x %d windows of %d x %d (last at %d, %d), %d prompt(s) of %d ids, %d steps in %lld launches, "
                "pipeline workspace %zu bytes\n", specs[0].size(), specs[1].size(), specs[2].size(), total, h, w, 4 * h, 4 * w, tiles_y, tiles_x, ty, tx, plan[plan.size() - 2],
                plan[plan.size() - 1], n, tokens, steps, (long long)launches, ws);
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_frame)); HIPCHK(hipFree(d_out)); HIPCHK(hipFree(d_noise)); HIPCHK(hipFree(d_latents));
    p_nesr_sdx4_destroy(pipe);
    p_nesr_clip_text_destroy(text);
    p_nesr_unet_destroy(unet);
    p_nesr_vae_destroy(vae);
    return 0;
}
