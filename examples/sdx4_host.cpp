// The x4 diffusion upscaler from a host with no Python and no torch in the process, through the C ABI of libnesr_hip.so
// (include/nesr_hip.h): builds the text encoder, the UNet and the VAE decoder of a configuration, gives them weights (a flat
// float32 file that holds the tensors in the order of clip_text_state_dict_spec, unet_state_dict_spec, vae_state_dict_spec one
// after the other, or "seed:N": synthetic weights from a counter-based generator of this file), and runs one nesr_sdx4_upscale_u8:
// a binary PPM frame and the prompts' ids in, the x4 frame out as a PPM.  ids [n][tokens] int32 ([negative, prompt] when guidance >
// 1), noise [3][h][w] and latents [4][h][w] float32 come from raw files, or, for "-", from the same generator (unit normals).
//   hipcc -O2 --offload-arch=gfx950 -I include examples/sdx4_host.cpp -o build/sdx4_host -ldl
//   build/sdx4_host path/to/libnesr_hip.so weights.f32|seed:N frame.ppm ids.i32|- noise.f32|- latents.f32|- tokens noise_level steps guidance out.ppm
//                   [published|crafted]
// "published": the x4 upscaler's widths as recalled; "crafted": the small pipeline of tests/sdx4_cases.py.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
typedef std::vector<Entry> Spec;

// splitmix64 of (seed, stream, counter): a uniform in [-1, 1) with 24 bits, or a unit normal (Box-Muller)
static uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static float uniform(uint64_t seed, uint64_t stream, uint64_t i) { return (float)(mix(mix(seed) ^ mix(stream << 32 | 0xABCDu) ^ i) >> 40) * (1.0f / 8388608.0f) - 1.0f; }
static float normal(uint64_t seed, uint64_t stream, uint64_t i) {
    const double u1 = ((double)uniform(seed, stream, 2 * i) + 1.0) * 0.5, u2 = ((double)uniform(seed, stream, 2 * i + 1) + 1.0) * 0.5;
    return (float)(std::sqrt(-2.0 * std::log(u1 + 1e-12)) * std::cos(6.283185307179586 * u2));
}

static void wb(Spec& s, const std::string& name, std::vector<int64_t> shape, bool bias = true) {
    const int64_t rows = shape[0];
    s.push_back({name + ".weight", shape});
    if (bias) s.push_back({name + ".bias", {rows}});
}

static Spec text_spec(int vocab, int h, int inter, int layers, int positions) {
    Spec s;
    s.push_back({"embeddings.token_embedding.weight", {vocab, h}});
    s.push_back({"embeddings.position_embedding.weight", {positions, h}});
    for (int i = 0; i < layers; ++i) {
        const std::string l = "encoder.layers." + std::to_string(i);
        for (const char* part : {".self_attn.k_proj", ".self_attn.v_proj", ".self_attn.q_proj", ".self_attn.out_proj"}) wb(s, l + part, {h, h});
        wb(s, l + ".layer_norm1", {h});
        wb(s, l + ".mlp.fc1", {inter, h});
        wb(s, l + ".mlp.fc2", {h, inter});
        wb(s, l + ".layer_norm2", {h});
    }
    wb(s, "final_layer_norm", {h});
    return s;
}

static Spec unet_spec(const std::vector<int>& widths, const std::vector<int>& attention, const std::vector<int>& only_cross, int layers, int cross, int classes, int cin, int cout) {
    Spec s;
    const int L = (int)widths.size();
    const int64_t td = 4 * widths[0];
    auto resnet = [&](const std::string& r, int64_t ci, int64_t co) {
        wb(s, r + ".norm1", {ci});
        wb(s, r + ".conv1", {co, ci, 3, 3});
        wb(s, r + ".time_emb_proj", {co, td});
        wb(s, r + ".norm2", {co});
        wb(s, r + ".conv2", {co, co, 3, 3});
        if (ci != co) wb(s, r + ".conv_shortcut", {co, ci, 1, 1});
    };
    auto transformer = [&](const std::string& a, int64_t dim, bool oc) {
        wb(s, a + ".norm", {dim});
        wb(s, a + ".proj_in", {dim, dim});
        const std::string b = a + ".transformer_blocks.0";
        for (int i = 1; i <= 2; ++i) {
            const std::string at = b + ".attn" + std::to_string(i);
            const int64_t kv = (i == 2 || oc) ? cross : dim;
            wb(s, b + ".norm" + std::to_string(i), {dim});
            wb(s, at + ".to_q", {dim, dim}, false);
            wb(s, at + ".to_k", {dim, kv}, false);
            wb(s, at + ".to_v", {dim, kv}, false);
            wb(s, at + ".to_out.0", {dim, dim});
        }
        wb(s, b + ".norm3", {dim});
        wb(s, b + ".ff.net.0.proj", {8 * dim, dim});
        wb(s, b + ".ff.net.2", {dim, 4 * dim});
        wb(s, a + ".proj_out", {dim, dim});
    };
    wb(s, "conv_in", {widths[0], cin, 3, 3});
    wb(s, "time_embedding.linear_1", {td, widths[0]});
    wb(s, "time_embedding.linear_2", {td, td});
    s.push_back({"class_embedding.weight", {classes, td}});
    int64_t prev = widths[0];
    for (int i = 0; i < L; ++i) {
        const std::string d = "down_blocks." + std::to_string(i);
        for (int j = 0; j < layers && attention[i]; ++j) transformer(d + ".attentions." + std::to_string(j), widths[i], only_cross[i] != 0);
        for (int j = 0; j < layers; ++j) resnet(d + ".resnets." + std::to_string(j), j == 0 ? prev : widths[i], widths[i]);
        if (i < L - 1) wb(s, d + ".downsamplers.0.conv", {widths[i], widths[i], 3, 3});
        prev = widths[i];
    }
    for (int i = 0; i < L; ++i) {
        const std::string u = "up_blocks." + std::to_string(i);
        const int l = L - 1 - i;
        const int64_t out = widths[l], before = widths[L - 1 - std::max(i - 1, 0)], in_ch = widths[L - 1 - std::min(i + 1, L - 1)];
        for (int j = 0; j <= layers && attention[l]; ++j) transformer(u + ".attentions." + std::to_string(j), out, only_cross[l] != 0);
        for (int j = 0; j <= layers; ++j) resnet(u + ".resnets." + std::to_string(j), (j == 0 ? before : out) + (j == layers ? in_ch : out), out);
        if (i < L - 1) wb(s, u + ".upsamplers.0.conv", {out, out, 3, 3});
    }
    transformer("mid_block.attentions.0", prev, false);
    resnet("mid_block.resnets.0", prev, prev);
    resnet("mid_block.resnets.1", prev, prev);
    wb(s, "conv_norm_out", {widths[0]});
    wb(s, "conv_out", {cout, widths[0], 3, 3});
    return s;
}

static Spec vae_spec(const std::vector<int>& widths, int layers, int lat, int nout) {
    Spec s;
    auto resnet = [&](const std::string& r, int64_t ci, int64_t co) {
        wb(s, r + ".norm1", {ci});
        wb(s, r + ".conv1", {co, ci, 3, 3});
        wb(s, r + ".norm2", {co});
        wb(s, r + ".conv2", {co, co, 3, 3});
        if (ci != co) wb(s, r + ".conv_shortcut", {co, ci, 1, 1});
    };
    const int64_t top = widths.back();
    wb(s, "post_quant_conv", {lat, lat, 1, 1});
    wb(s, "decoder.conv_in", {top, lat, 3, 3});
    resnet("decoder.mid_block.resnets.0", top, top);
    const std::string at = "decoder.mid_block.attentions.0";
    wb(s, at + ".group_norm", {top});
    for (const char* n : {".to_q", ".to_k", ".to_v", ".to_out.0"}) wb(s, at + n, {top, top});
    resnet("decoder.mid_block.resnets.1", top, top);
    int64_t prev = top;
    for (size_t i = 0; i < widths.size(); ++i) {
        const int64_t wd = widths[widths.size() - 1 - i];
        const std::string u = "decoder.up_blocks." + std::to_string(i);
        for (int j = 0; j <= layers; ++j) resnet(u + ".resnets." + std::to_string(j), j == 0 ? prev : wd, wd);
        if (i + 1 < widths.size()) wb(s, u + ".upsamplers.0.conv", {wd, wd, 3, 3});
        prev = wd;
    }
    wb(s, "decoder.conv_norm_out", {prev});
    wb(s, "decoder.conv_out", {nout, prev, 3, 3});
    return s;
}

// one tensor: from the file, or synthetic (a norm's weight about 1, biases and tables small, products of unit gain)
static bool fill(std::vector<float>& v, const Entry& e, FILE* f, uint64_t seed, uint64_t stream) {
    if (f) return std::fread(v.data(), sizeof(float), v.size(), f) == v.size();
    const bool norm = e.key.find("norm") != std::string::npos, bias = e.key.size() > 5 && e.key.compare(e.key.size() - 5, 5, ".bias") == 0;
    size_t fan = 1;
    for (size_t d = 1; d < e.shape.size(); ++d) fan *= (size_t)e.shape[d];
    const float gain = (float)std::sqrt(3.0 / (double)fan);
    for (size_t i = 0; i < v.size(); ++i) {
        const float u = uniform(seed, stream, i);
        v[i] = norm && !bias ? 1.0f + 0.25f * u : (bias || e.key.find("embedding.weight") != std::string::npos) ? 0.25f * u : gain * u;
    }
    return true;
}

template <class T>
static bool read_raw(const char* path, std::vector<T>& v) {
    FILE* f = std::fopen(path, "rb");
    const bool ok = f && std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    if (f) std::fclose(f);
    if (!ok) std::fprintf(stderr, "cannot read %zu values from %s\n", v.size(), path);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 12) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so weights.f32|seed:N frame.ppm ids.i32|- noise.f32|- latents.f32|- tokens noise_level steps guidance out.ppm "
                             "[published|crafted]\n", argv[0]);
        return 1;
    }
    const int tokens = std::atoi(argv[7]), noise_level = std::atoi(argv[8]), steps = std::atoi(argv[9]);
    const double guidance = std::atof(argv[10]);
    const bool crafted = argc > 12 && std::string(argv[12]) == "crafted";
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
    LOAD(nesr_sdx4_workspace_bytes) LOAD(nesr_sdx4_upscale_u8) LOAD(nesr_sdx4_launches)
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

    size_t ws = 0;
    CHECK(p_nesr_sdx4_workspace_bytes(pipe, n, h, w, tokens, &ws));
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
    CHECK(p_nesr_sdx4_upscale_u8(pipe, d_frame, h, w, ids.data(), tokens, d_noise, d_latents, noise_level, steps, guidance, d_out, out_bytes, nullptr, s));
    std::vector<uint8_t> out(out_bytes);
    HIPCHK(hipMemcpyAsync(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int64_t launches = 0;
    CHECK(p_nesr_sdx4_launches(pipe, &launches));
    FILE* f = std::fopen(argv[11], "wb");
    if (!f || std::fprintf(f, "P6\n%d %d\n255\n", 4 * w, 4 * h) < 0 || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[11]); return 1; }
    std::printf("%zu + %zu + %zu tensors, %zu parameters; %d x %d -> %d x %d, %d prompt(s) of %d ids, %d steps in %lld launches, pipeline workspace %zu bytes\n", specs[0].size(),
                specs[1].size(), specs[2].size(), total, h, w, 4 * h, 4 * w, n, tokens, steps, (long long)launches, ws);
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_frame)); HIPCHK(hipFree(d_out)); HIPCHK(hipFree(d_noise)); HIPCHK(hipFree(d_latents));
    p_nesr_sdx4_destroy(pipe);
    p_nesr_clip_text_destroy(text);
    p_nesr_unet_destroy(unet);
    p_nesr_vae_destroy(vae);
    return 0;
}
