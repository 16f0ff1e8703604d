// The x4 upscaler's VAE decoder from a host with no Python and no torch in the process, through the C ABI of libnesr_hip.so
// (include/nesr_hip.h): builds a decoder of the given widths (default: the published (128, 256, 512), 32 groups, 2 layers a block,
// scaling factor 0.08333), loads the weights from a flat float32 file that holds the decoder's tensors in the order of
// vae.vae_state_dict_spec, and turns raw float32 latents [4][h][w] into the RGB frame with nesr_vae_decode_latents_u8 (the division
// by the scaling factor, the network and the quantiser on the device).  The frame is written as a binary PPM when the output's name
// ends in .ppm, raw H x W x 3 u8 otherwise.
//   hipcc -O2 --offload-arch=gfx950 -I include examples/vae_host.cpp -o build/vae_host -ldl
//   build/vae_host path/to/libnesr_hip.so weights.f32 latents.f32 h w out.ppm [widths, e.g. 16,32] [norm_num_groups] [layers_per_block] [scaling_factor]
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
    if (argc < 7) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so weights.f32 latents.f32 h w out.ppm|out.rgb [widths] [norm_num_groups] [layers_per_block] [scaling_factor]\n", argv[0]);
        return 1;
    }
    const int h = std::atoi(argv[4]), w = std::atoi(argv[5]);
    if (h < 1 || w < 1) { std::fprintf(stderr, "bad shape %s x %s\n", argv[4], argv[5]); return 1; }
    std::vector<int> widths;
    for (const char* p = argc > 7 ? argv[7] : "128,256,512"; *p;) {
        char* end = nullptr;
        widths.push_back((int)std::strtol(p, &end, 10));
        if (end == p) { std::fprintf(stderr, "bad widths %s\n", argv[7]); return 1; }
        p = *end == ',' ? end + 1 : end;
    }
    const int groups = argc > 8 ? std::atoi(argv[8]) : 32, layers = argc > 9 ? std::atoi(argv[9]) : 2, lat = 4, nout = 3;
    const double scaling = argc > 10 ? std::atof(argv[10]) : 0.08333;
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_vae_create) LOAD(nesr_vae_destroy) LOAD(nesr_vae_num_tensors) LOAD(nesr_vae_load_weight)
    LOAD(nesr_vae_finalize) LOAD(nesr_vae_output_size) LOAD(nesr_vae_workspace_bytes) LOAD(nesr_vae_decode_latents_u8) LOAD(nesr_vae_kernel_time_ms)
    std::printf("%s\n", p_nesr_version());

    nesr_vae* ctx = nullptr;
    CHECK(p_nesr_vae_create(&ctx, 0, lat, nout, (int)widths.size(), widths.data(), layers, groups, scaling, "silu"));

    // the decoder's keys and shapes, in the spec's order
    std::vector<Entry> spec;
    auto wb = [&](const std::string& name, std::vector<int64_t> s) {
        const int64_t n = s[0];
        spec.push_back({name + ".weight", s});
        spec.push_back({name + ".bias", {n}});
    };
    auto resnet = [&](const std::string& r, int64_t cin, int64_t cout) {
        wb(r + ".norm1", {cin});
        wb(r + ".conv1", {cout, cin, 3, 3});
        wb(r + ".norm2", {cout});
        wb(r + ".conv2", {cout, cout, 3, 3});
        if (cin != cout) wb(r + ".conv_shortcut", {cout, cin, 1, 1});
    };
    const int64_t top = widths.back();
    wb("post_quant_conv", {lat, lat, 1, 1});
    wb("decoder.conv_in", {top, lat, 3, 3});
    resnet("decoder.mid_block.resnets.0", top, top);
    const std::string at = "decoder.mid_block.attentions.0";
    wb(at + ".group_norm", {top});
    for (const char* n : {".to_q", ".to_k", ".to_v", ".to_out.0"}) wb(at + n, {top, top});
    resnet("decoder.mid_block.resnets.1", top, top);
    int64_t prev = top;
    for (size_t i = 0; i < widths.size(); ++i) {
        const int64_t wd = widths[widths.size() - 1 - i];
        const std::string u = "decoder.up_blocks." + std::to_string(i);
        for (int j = 0; j <= layers; ++j) resnet(u + ".resnets." + std::to_string(j), j == 0 ? prev : wd, wd);
        if (i + 1 < widths.size()) wb(u + ".upsamplers.0.conv", {wd, wd, 3, 3});
        prev = wd;
    }
    wb("decoder.conv_norm_out", {prev});
    wb("decoder.conv_out", {nout, prev, 3, 3});
    if ((int)spec.size() != p_nesr_vae_num_tensors(ctx)) { std::fprintf(stderr, "the context waits for %d tensors, the host lists %zu\n", p_nesr_vae_num_tensors(ctx), spec.size()); return 4; }

    FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    size_t total = 0;
    for (const Entry& e : spec) {
        size_t n = 1;
        for (int64_t d : e.shape) n *= (size_t)d;
        std::vector<float> v(n);
        if (std::fread(v.data(), sizeof(float), n, f) != n) { std::fprintf(stderr, "%s ends before %s\n", argv[2], e.key.c_str()); return 1; }
        CHECK(p_nesr_vae_load_weight(ctx, e.key.c_str(), v.data(), e.shape.data(), (int)e.shape.size()));
        total += n;
    }
    std::fclose(f);
    CHECK(p_nesr_vae_finalize(ctx));

    const size_t count = (size_t)lat * h * w;
    std::vector<float> latents(count);
    f = std::fopen(argv[3], "rb");
    if (!f || std::fread(latents.data(), sizeof(float), count, f) != count) { std::fprintf(stderr, "cannot read %zu floats from %s\n", count, argv[3]); return 1; }
    std::fclose(f);
    int oh = 0, ow = 0;
    CHECK(p_nesr_vae_output_size((int)widths.size(), h, w, &oh, &ow));
    size_t ws = 0;
    CHECK(p_nesr_vae_workspace_bytes(ctx, h, w, &ws));
    const size_t out_bytes = (size_t)oh * ow * 3;
    float* d_lat;
    uint8_t* d_out;
    HIPCHK(hipMalloc(&d_lat, count * sizeof(float)));
    HIPCHK(hipMalloc(&d_out, out_bytes));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_lat, latents.data(), count * sizeof(float), hipMemcpyHostToDevice, s));
    CHECK(p_nesr_vae_decode_latents_u8(ctx, d_lat, 1, lat, h, w, d_out, out_bytes, s));
    std::vector<uint8_t> out(out_bytes);
    HIPCHK(hipMemcpyAsync(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int64_t launches = 0;
    CHECK(p_nesr_vae_kernel_time_ms(ctx, nullptr, 0, &launches));
    const std::string name = argv[6];
    f = std::fopen(argv[6], "wb");
    if (f && name.size() > 4 && name.compare(name.size() - 4, 4, ".ppm") == 0) std::fprintf(f, "P6\n%d %d\n255\n", ow, oh);
    if (!f || std::fwrite(out.data(), 1, out_bytes, f) != out_bytes || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[6]); return 1; }
    std::printf("%zu tensors, %zu parameters; latents %d x %d -> %d x %d in %lld launches, workspace %zu bytes\n", spec.size(), total, h, w, oh, ow,
                (long long)launches, ws);
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_lat)); HIPCHK(hipFree(d_out));
    p_nesr_vae_destroy(ctx);
    return 0;
}
