// The host side of a strictly loaded checkpoint, shared by the five models that take a transformers or diffusers state dict
// (segformer_api.cpp, swin2sr_api.cpp, vae_api.cpp, unet_api.cpp, clip_text_api.cpp; net_context.h holds the contexts' common
// part): StateDict keeps the expected keys with their shapes and the values loaded so far; HostPack is the float vector the weights
// are repacked into before their one upload, with the packers of a norm and of a padded Linear; HalfPack is the fp16 form's vector
// of halves beside it.  Host only (no HIP): tools/state_dict_check.cpp builds it alone, with its own set_error.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/nesr_hip.h"

namespace nesr {

// sets nesr_last_error() and returns `code`: nesr_api.cpp's in the library (api_common.h declares it too), the program's own elsewhere
int set_error(int code, const std::string& msg);

class StateDict {
public:
    void expect(const std::string& key, std::vector<int64_t> shape) {
        Tensor t;
        t.shape = std::move(shape);
        t_[key] = t;
        order_.push_back(key);
    }
    void expect_wb(const std::string& name, std::vector<int64_t> wshape, bool bias = true) {
        const int64_t n = wshape[0];
        expect(name + ".weight", std::move(wshape));
        if (bias) expect(name + ".bias", {n});
    }
    // strict: a key that is not expected, or another shape than the expected one, is NESR_ERR_ARG.  `given` is the caller's
    // spelling of a key it translated (the unexpected-key text names that one).
    int load(const std::string& key, const float* data, const int64_t* shape, int ndim, const char* given = nullptr) {
        auto it = t_.find(key);
        if (it == t_.end()) return set_error(NESR_ERR_ARG, std::string("unexpected key in state_dict: ") + (given ? given : key.c_str()));
        Tensor& t = it->second;
        bool same = ndim == (int)t.shape.size();
        for (int i = 0; same && i < ndim; ++i) same = shape[i] == t.shape[i];
        if (!same) {
            std::string want;
            for (int64_t d : t.shape) want += (want.empty() ? "" : ",") + std::to_string(d);
            return set_error(NESR_ERR_ARG, "size mismatch for " + key + ": expected [" + want + "]");
        }
        size_t numel = 1;
        for (int64_t d : t.shape) numel *= (size_t)d;
        t.data.assign(data, data + numel);
        t.have = true;
        return NESR_OK;
    }
    // "missing keys in state_dict (n): " and the first four of them in the expected order; empty when every key is loaded
    std::string missing() const {
        std::string names;
        int n = 0;
        for (const std::string& k : order_)
            if (!t_.at(k).have && n++ < 4) names += (names.empty() ? "" : ", ") + k;
        return n ? "missing keys in state_dict (" + std::to_string(n) + "): " + names : std::string();
    }
    const std::vector<float>& data(const std::string& key) const { return t_.at(key).data; }
    size_t size() const { return order_.size(); }

private:
    struct Tensor {
        std::vector<int64_t> shape;
        std::vector<float> data;
        bool have = false;
    };
    std::map<std::string, Tensor> t_;      // every expected key with its shape
    std::vector<std::string> order_;
};

// offsets in floats into the packed weights: a norm's gamma and beta over c channels; a product's Wt[kp][np] and bias [np]
struct NormW {
    size_t g = 0, b = 0;
    int c = 0;
};
struct LinW {
    size_t w = 0, b = 0;
    int kp = 0, np = 0;      // rows and columns of Wt (side_by_side: of all parts; the UNet's GEGLU: np of one half)
};

inline int round16(int v) { return (v + 15) / 16 * 16; }

// Every function returns or takes an offset in floats into `host`; each piece starts at a multiple of 64 floats and its padding is zero.
struct HostPack {
    std::vector<float> host;

    size_t reserve(size_t floats) {
        const size_t at = host.size();
        host.resize((at + floats + 63) / 64 * 64, 0.f);
        return at;
    }
    // a vector, zero padded to `padded`
    size_t vec(const std::vector<float>& v, size_t padded = 0) {
        const size_t at = reserve(std::max(padded, v.size()));
        std::copy(v.begin(), v.end(), host.begin() + at);
        return at;
    }
    // torch's Linear / flattened conv weight [n][k] -> host[at + kk * ld + col0 + o]
    void transpose_into(size_t at, const std::vector<float>& w, int n, int k, int ld, int col0) {
        for (int o = 0; o < n; ++o)
            for (int kk = 0; kk < k; ++kk) host[at + (size_t)kk * ld + col0 + o] = w[(size_t)o * k + kk];
    }
    // conv weight [n][cin][taps] -> [(tap * cin_padded + ci)][n_padded], the order an NHWC patch is read in
    size_t conv_taps(const std::vector<float>& w, int n, int cin, int taps, int cin_padded, int n_padded) {
        const size_t at = reserve((size_t)taps * cin_padded * n_padded);
        for (int o = 0; o < n; ++o)
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < taps; ++t) host[at + ((size_t)t * cin_padded + ci) * n_padded + o] = w[((size_t)o * cin + ci) * taps + t];
        return at;
    }
    // name.weight and name.bias of a norm over ch channels, each padded to round16(ch)
    NormW norm(const StateDict& sd, const std::string& name, int ch) {
        NormW n;
        n.c = ch, n.g = vec(sd.data(name + ".weight"), round16(ch)), n.b = vec(sd.data(name + ".bias"), round16(ch));
        return n;
    }
    // torch's Linear / 1x1 conv name.weight [n][k] -> Wt[round16(k)][round16(n)], name.bias padded (zeros without one)
    LinW linear(const StateDict& sd, const std::string& name, int n, int k, bool bias = true) {
        LinW l;
        l.kp = round16(k), l.np = round16(n);
        l.w = reserve((size_t)l.kp * l.np);
        transpose_into(l.w, sd.data(name + ".weight"), n, k, l.np, 0);
        l.b = bias ? vec(sd.data(name + ".bias"), l.np) : reserve(l.np);
        return l;
    }
    // several products [n][k] of one input side by side (q | k | v): Wt[round16(k)][parts round16(n)], part i from column i round16(n)
    LinW side_by_side(const StateDict& sd, const std::string& prefix, std::initializer_list<const char*> parts, int n, int k, bool bias = true) {
        LinW l;
        const int np1 = round16(n);
        l.kp = round16(k), l.np = (int)parts.size() * np1;
        l.w = reserve((size_t)l.kp * l.np);
        l.b = reserve(l.np);
        int col = 0;
        for (const char* part : parts) {
            transpose_into(l.w, sd.data(prefix + part + ".weight"), n, k, l.np, col);
            if (bias) {
                const std::vector<float>& b = sd.data(prefix + part + ".bias");
                std::copy(b.begin(), b.end(), host.begin() + l.b + col);
            }
            col += np1;
        }
        return l;
    }
};

// The fp16 form's copy of the GEMM weights, in halves: offsets count halves of `half`, each piece starts at a multiple of 64 and
// its padding is zero.  The first key with a value f16 cannot carry (non-finite or beyond +-65504) is kept for finalize's refusal.
struct HalfPack {
    std::vector<_Float16> half;

    static bool carries(float v) { return std::fabs(v) <= 65504.0f; }      // false for NaN
    size_t reserve(size_t halves) {
        const size_t at = half.size();
        half.resize((at + halves + 63) / 64 * 64, (_Float16)0.f);
        return at;
    }
    void note(const std::string& key, bool bad) {
        if (bad && out_of_range_.empty()) out_of_range_ = key;
    }
    // `value` of tensor `key`, rounded
    _Float16 put(const std::string& key, float value) {
        note(key, !carries(value));
        return (_Float16)value;
    }
    const std::string& out_of_range() const { return out_of_range_; }      // empty: every value so far fits

private:
    std::string out_of_range_;
};

}  // namespace nesr
