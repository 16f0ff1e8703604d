// What the two hosts of the x4 diffusion upscaler share (sdx4_host.cpp, sdx4_tiled_host.cpp): the loader macros, the three networks' state
// dict specs in the order their checkpoints list the tensors, the synthetic weights of "seed:N", and the raw-file reader.
#pragma once
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
static inline uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static inline float uniform(uint64_t seed, uint64_t stream, uint64_t i) { return (float)(mix(mix(seed) ^ mix(stream << 32 | 0xABCDu) ^ i) >> 40) * (1.0f / 8388608.0f) - 1.0f; }
static inline float normal(uint64_t seed, uint64_t stream, uint64_t i) {
    const double u1 = ((double)uniform(seed, stream, 2 * i) + 1.0) * 0.5, u2 = ((double)uniform(seed, stream, 2 * i + 1) + 1.0) * 0.5;
    return (float)(std::sqrt(-2.0 * std::log(u1 + 1e-12)) * std::cos(6.283185307179586 * u2));
}

static inline void wb(Spec& s, const std::string& name, std::vector<int64_t> shape, bool bias = true) {
    const int64_t rows = shape[0];
    s.push_back({name + ".weight", shape});
    if (bias) s.push_back({name + ".bias", {rows}});
}

static inline Spec text_spec(int vocab, int h, int inter, int layers, int positions) {
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

static inline Spec unet_spec(const std::vector<int>& widths, const std::vector<int>& attention, const std::vector<int>& only_cross, int layers, int cross, int classes, int cin, int cout) {
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

static inline Spec vae_spec(const std::vector<int>& widths, int layers, int lat, int nout) {
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
static inline bool fill(std::vector<float>& v, const Entry& e, FILE* f, uint64_t seed, uint64_t stream) {
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
static inline bool read_raw(const char* path, std::vector<T>& v) {
    FILE* f = std::fopen(path, "rb");
    const bool ok = f && std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    if (f) std::fclose(f);
    if (!ok) std::fprintf(stderr, "cannot read %zu values from %s\n", v.size(), path);
    return ok;
}
