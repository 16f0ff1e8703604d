// The host side of a strictly loaded checkpoint, shared by the models that take a transformers state dict (segformer_api.cpp,
// swin2sr_api.cpp): StateDict keeps the expected keys with their shapes and the values loaded so far; HostPack is the float vector
// the weights are repacked into before their one upload.  Host only (no HIP): tools/state_dict_check.cpp builds it alone, with its
// own set_error.
#pragma once
#include <stdint.h>

#include <algorithm>
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
};

}  // namespace nesr
