// The x4 upscaler's UNet from a host with no Python and no torch in the process, through the C ABI of libnesr_hip.so
// (include/nesr_hip.h): builds a UNet of the given configuration (default: the published one), loads the weights from a flat
// float32 file that holds the tensors in the order of unet.unet_state_dict_spec, runs one forward on a raw float32 sample
// [n][in_channels][h][w] and raw float32 text states [n][tokens][cross_attention_dim], and writes the raw float32 result
// [n][out_channels][h][w].
//   hipcc -O2 --offload-arch=gfx950 -I include examples/unet_host.cpp -o build/unet_host -ldl
//   build/unet_host path/to/libnesr_hip.so weights.f32 sample.f32 text.f32 n h w tokens timestep class_label out.f32
//                   [widths, e.g. 16,32] [attention per level, e.g. 1,1] [only_cross_attention per level, e.g. 1,0] [norm_num_groups]
//                   [heads] [layers_per_block] [cross_attention_dim] [num_class_embeds] [--dtype f32|fp16]
// --dtype (anywhere on the line; default f32) picks the compute form: nesr_unet_set_dtype between create and finalize.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
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

static std::vector<int> ints(const char* p) {
    std::vector<int> v;
    while (*p) {
        char* end = nullptr;
        v.push_back((int)std::strtol(p, &end, 10));
        if (end == p) return {};
        p = *end == ',' ? end + 1 : end;
    }
    return v;
}

static bool read_floats(const char* path, std::vector<float>& v) {
    FILE* f = std::fopen(path, "rb");
    const bool ok = f && std::fread(v.data(), sizeof(float), v.size(), f) == v.size();
    if (f) std::fclose(f);
    if (!ok) std::fprintf(stderr, "cannot read %zu floats from %s\n", v.size(), path);
    return ok;
}

int main(int argc, char** argv) {
    int dtype = NESR_DTYPE_F32;
    for (int i = 1; i < argc; ++i) {      // --dtype and its value leave the line; what stays is positional
        if (std::strcmp(argv[i], "--dtype")) continue;
        const char* v = i + 1 < argc ? argv[i + 1] : "";
        if (!std::strcmp(v, "fp16")) dtype = NESR_DTYPE_F16;
        else if (std::strcmp(v, "f32")) { std::fprintf(stderr, "--dtype takes f32 or fp16, got '%s'\n", v); return 1; }
        for (int j = i; j + 2 <= argc; ++j) argv[j] = j + 2 < argc ? argv[j + 2] : nullptr;
        argc -= 2, --i;
    }
    if (argc < 12) {
        std::fprintf(stderr, "usage: %s libnesr_hip.so weights.f32 sample.f32 text.f32 n h w tokens timestep class_label out.f32 [widths] [attention] "
                             "[only_cross_attention] [norm_num_groups] [heads] [layers_per_block] [cross_attention_dim] [num_class_embeds] [--dtype f32|fp16]\n", argv[0]);
        return 1;
    }
    const int n = std::atoi(argv[5]), h = std::atoi(argv[6]), w = std::atoi(argv[7]), tokens = std::atoi(argv[8]), label = std::atoi(argv[10]);
    const double timestep = std::atof(argv[9]);
    const std::vector<int> widths = ints(argc > 12 ? argv[12] : "256,512,512,1024"), attention = ints(argc > 13 ? argv[13] : "0,1,1,1");
    const std::vector<int> only_cross = ints(argc > 14 ? argv[14] : "1,1,1,0");
    const int groups = argc > 15 ? std::atoi(argv[15]) : 32, heads = argc > 16 ? std::atoi(argv[16]) : 8, layers = argc > 17 ? std::atoi(argv[17]) : 2;
    const int cross = argc > 18 ? std::atoi(argv[18]) : 1024, classes = argc > 19 ? std::atoi(argv[19]) : 1000, cin = 7, cout = 4;
    const int L = (int)widths.size();
    if (n < 1 || h < 1 || w < 1 || tokens < 1 || L < 1 || (int)attention.size() != L || (int)only_cross.size() != L) { std::fprintf(stderr, "bad shape or configuration\n"); return 1; }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    LOAD(nesr_last_error) LOAD(nesr_version) LOAD(nesr_unet_create) LOAD(nesr_unet_destroy) LOAD(nesr_unet_num_tensors) LOAD(nesr_unet_load_weight)
    LOAD(nesr_unet_finalize) LOAD(nesr_unet_workspace_bytes) LOAD(nesr_unet_forward_f32) LOAD(nesr_unet_kernel_time_ms) LOAD(nesr_unet_set_dtype)
    std::printf("%s\n", p_nesr_version());

    std::vector<const char*> down(L), up(L);
    for (int i = 0; i < L; ++i) down[i] = attention[i] ? "CrossAttnDownBlock2D" : "DownBlock2D", up[L - 1 - i] = attention[i] ? "CrossAttnUpBlock2D" : "UpBlock2D";
    nesr_unet* ctx = nullptr;
    CHECK(p_nesr_unet_create(&ctx, 0, cin, cout, L, widths.data(), down.data(), up.data(), "UNetMidBlock2DCrossAttn", only_cross.data(), layers, heads, cross, 1, 1, 0,
                             classes, groups, 1e-5, 1, 0.0, 1, "silu"));
    if (dtype != NESR_DTYPE_F32) {
        CHECK(p_nesr_unet_set_dtype(ctx, dtype));
        std::printf("compute form: fp16\n");
    }

    // the keys and shapes, in the spec's order
    std::vector<Entry> spec;
    const int64_t td = 4 * widths[0];
    auto wb = [&](const std::string& name, std::vector<int64_t> s, bool bias = true) {
        const int64_t rows = s[0];
        spec.push_back({name + ".weight", s});
        if (bias) spec.push_back({name + ".bias", {rows}});
    };
    auto resnet = [&](const std::string& r, int64_t ci, int64_t co) {
        wb(r + ".norm1", {ci});
        wb(r + ".conv1", {co, ci, 3, 3});
        wb(r + ".time_emb_proj", {co, td});
        wb(r + ".norm2", {co});
        wb(r + ".conv2", {co, co, 3, 3});
        if (ci != co) wb(r + ".conv_shortcut", {co, ci, 1, 1});
    };
    auto transformer = [&](const std::string& a, int64_t dim, bool oc) {
        wb(a + ".norm", {dim});
        wb(a + ".proj_in", {dim, dim});
        const std::string b = a + ".transformer_blocks.0";
        for (int i = 1; i <= 2; ++i) {
            const std::string at = b + ".attn" + std::to_string(i);
            const int64_t kv = (i == 2 || oc) ? cross : dim;
            wb(b + ".norm" + std::to_string(i), {dim});
            wb(at + ".to_q", {dim, dim}, false);
            wb(at + ".to_k", {dim, kv}, false);
            wb(at + ".to_v", {dim, kv}, false);
            wb(at + ".to_out.0", {dim, dim});
        }
        wb(b + ".norm3", {dim});
        wb(b + ".ff.net.0.proj", {8 * dim, dim});
        wb(b + ".ff.net.2", {dim, 4 * dim});
        wb(a + ".proj_out", {dim, dim});
    };
    wb("conv_in", {widths[0], cin, 3, 3});
    wb("time_embedding.linear_1", {td, widths[0]});
    wb("time_embedding.linear_2", {td, td});
    spec.push_back({"class_embedding.weight", {classes, td}});
    int64_t prev = widths[0];
    for (int i = 0; i < L; ++i) {
        const std::string d = "down_blocks." + std::to_string(i);
        for (int j = 0; j < layers && attention[i]; ++j) transformer(d + ".attentions." + std::to_string(j), widths[i], only_cross[i] != 0);
        for (int j = 0; j < layers; ++j) resnet(d + ".resnets." + std::to_string(j), j == 0 ? prev : widths[i], widths[i]);
        if (i < L - 1) wb(d + ".downsamplers.0.conv", {widths[i], widths[i], 3, 3});
        prev = widths[i];
    }
    for (int i = 0; i < L; ++i) {
        const std::string u = "up_blocks." + std::to_string(i);
        const int l = L - 1 - i;
        const int64_t out = widths[l], before = widths[L - 1 - std::max(i - 1, 0)], in_ch = widths[L - 1 - std::min(i + 1, L - 1)];
        for (int j = 0; j <= layers && attention[l]; ++j) transformer(u + ".attentions." + std::to_string(j), out, only_cross[l] != 0);
        for (int j = 0; j <= layers; ++j) resnet(u + ".resnets." + std::to_string(j), (j == 0 ? before : out) + (j == layers ? in_ch : out), out);
        if (i < L - 1) wb(u + ".upsamplers.0.conv", {out, out, 3, 3});
    }
    transformer("mid_block.attentions.0", prev, false);
    resnet("mid_block.resnets.0", prev, prev);
    resnet("mid_block.resnets.1", prev, prev);
    wb("conv_norm_out", {widths[0]});
    wb("conv_out", {cout, widths[0], 3, 3});
    if ((int)spec.size() != p_nesr_unet_num_tensors(ctx)) { std::fprintf(stderr, "the context waits for %d tensors, the host lists %zu\n", p_nesr_unet_num_tensors(ctx), spec.size()); return 4; }

    FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    size_t total = 0;
    for (const Entry& e : spec) {
        size_t count = 1;
        for (int64_t d : e.shape) count *= (size_t)d;
        std::vector<float> v(count);
        if (std::fread(v.data(), sizeof(float), count, f) != count) { std::fprintf(stderr, "%s ends before %s\n", argv[2], e.key.c_str()); return 1; }
        CHECK(p_nesr_unet_load_weight(ctx, e.key.c_str(), v.data(), e.shape.data(), (int)e.shape.size()));
        total += count;
    }
    std::fclose(f);
    CHECK(p_nesr_unet_finalize(ctx));

    std::vector<float> sample((size_t)n * cin * h * w), text((size_t)n * tokens * cross), out((size_t)n * cout * h * w);
    if (!read_floats(argv[3], sample) || !read_floats(argv[4], text)) return 1;
    size_t ws = 0;
    CHECK(p_nesr_unet_workspace_bytes(ctx, n, h, w, tokens, &ws));
    float *d_sample, *d_text, *d_out;
    HIPCHK(hipMalloc(&d_sample, sample.size() * sizeof(float)));
    HIPCHK(hipMalloc(&d_text, text.size() * sizeof(float)));
    HIPCHK(hipMalloc(&d_out, out.size() * sizeof(float)));
    hipStream_t s;
    HIPCHK(hipStreamCreate(&s));
    HIPCHK(hipMemcpyAsync(d_sample, sample.data(), sample.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_text, text.data(), text.size() * sizeof(float), hipMemcpyHostToDevice, s));
    CHECK(p_nesr_unet_forward_f32(ctx, d_sample, n, cin, h, w, timestep, label, d_text, tokens, d_out, out.size(), s));
    HIPCHK(hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int64_t launches = 0;
    CHECK(p_nesr_unet_kernel_time_ms(ctx, nullptr, 0, &launches));
    f = std::fopen(argv[11], "wb");
    if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[11]); return 1; }
    std::printf("%zu tensors, %zu parameters; %d x [%d, %d, %d] with %d text states -> [%d, %d, %d] in %lld launches, workspace %zu bytes\n", spec.size(), total, n, cin,
                h, w, tokens, cout, h, w, (long long)launches, ws);
    HIPCHK(hipStreamDestroy(s));
    HIPCHK(hipFree(d_sample)); HIPCHK(hipFree(d_text)); HIPCHK(hipFree(d_out));
    p_nesr_unet_destroy(ctx);
    return 0;
}
