// The host side of the strict loaders of SegFormer and Swin2SR (csrc/state_dict.h: StateDict, HostPack) as a stand-alone host
// program, for a sanitizer build; their C entries cannot run without a device (create needs one).  StateDict: a tiny key set, an
// unexpected key, a wrong rank and a wrong extent with their texts, a key loaded twice, and the missing-keys text with 0, 1 and 6
// keys absent.  HostPack: a 3x2 Linear transposed into a padded 16x16 and a [2][3][3][3] conv repacked with cin_padded 4 and
// n_padded 16, every element at its closed-form offset and every other float zero: the layout the kernels read, element by
// element.  Prints one line; exits 1 on a surprise.
//   c++ -std=c++17 -g -fsanitize=address,undefined -I neural_enhanced_super_resolution_amd/csrc tools/state_dict_check.cpp -o state_dict_check
#include <cstdio>
#include <set>
#include <string>

#include "state_dict.h"

namespace nesr {
static std::string g_error;
int set_error(int code, const std::string& msg) {
    g_error = msg;
    return code;
}
}  // namespace nesr

using nesr::g_error;

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, g_error.c_str()); return 1; } } while (0)

int main() {
    int checks = 0;
    {
        nesr::StateDict sd;
        sd.expect_wb("a.proj", {3, 2});
        sd.expect_wb("a.key", {2, 2}, false);
        sd.expect("a.scale", {2, 1, 1});
        sd.expect_wb("b.norm", {4});
        sd.expect("b.count", {});
        EXPECT(sd.size() == 7);
        EXPECT(sd.missing() == "missing keys in state_dict (7): a.proj.weight, a.proj.bias, a.key.weight, a.scale");

        const float v[6] = {1, 2, 3, 4, 5, 6};
        const int64_t s32[2] = {3, 2}, s23[2] = {2, 3}, s3[1] = {3}, s22[2] = {2, 2}, s211[3] = {2, 1, 1}, s4[1] = {4};
        EXPECT(sd.load("a.proj.weight", v, s32, 2) == NESR_OK);
        EXPECT(sd.data("a.proj.weight") == std::vector<float>(v, v + 6));
        EXPECT(sd.missing() == "missing keys in state_dict (6): a.proj.bias, a.key.weight, a.scale, b.norm.weight");      // six absent, four named

        EXPECT(sd.load("a.key.bias", v, s3, 1) == NESR_ERR_ARG && g_error == "unexpected key in state_dict: a.key.bias");
        EXPECT(sd.load("a.proj.bias", v, s3, 1, "old.name.bias") == NESR_OK);
        EXPECT(sd.load("nowhere", v, s3, 1, "old.nowhere") == NESR_ERR_ARG && g_error == "unexpected key in state_dict: old.nowhere");
        EXPECT(sd.load("a.key.weight", v, s3, 1) == NESR_ERR_ARG && g_error == "size mismatch for a.key.weight: expected [2,2]");        // rank
        EXPECT(sd.load("a.key.weight", v, s23, 2) == NESR_ERR_ARG && g_error == "size mismatch for a.key.weight: expected [2,2]");       // extent
        EXPECT(sd.load("a.scale", v, s22, 2) == NESR_ERR_ARG && g_error == "size mismatch for a.scale: expected [2,1,1]");
        EXPECT(sd.load("b.count", v, s3, 1) == NESR_ERR_ARG && g_error == "size mismatch for b.count: expected []");
        EXPECT(sd.data("a.key.weight").empty());      // a refused tensor leaves nothing behind

        EXPECT(sd.load("a.key.weight", v, s22, 2) == NESR_OK && sd.load("a.scale", v, s211, 3) == NESR_OK);
        EXPECT(sd.load("b.norm.weight", v, s4, 1) == NESR_OK && sd.load("b.count", v, nullptr, 0) == NESR_OK);
        EXPECT(sd.data("b.count") == std::vector<float>(1, 1.f));
        EXPECT(sd.missing() == "missing keys in state_dict (1): b.norm.bias");
        EXPECT(sd.load("b.norm.bias", v + 1, s4, 1) == NESR_OK && sd.missing().empty());

        const float again[6] = {9, 8, 7, 6, 5, 4};      // a key loaded twice: the later values, still complete
        EXPECT(sd.load("a.proj.weight", again, s32, 2) == NESR_OK && sd.data("a.proj.weight") == std::vector<float>(again, again + 6));
        EXPECT(sd.missing().empty() && sd.size() == 7);
        checks += 24;
    }
    {
        nesr::HostPack pk;
        EXPECT(pk.reserve(1) == 0 && pk.host.size() == 64 && pk.reserve(64) == 64 && pk.host.size() == 128 && pk.reserve(0) == 128 && pk.host.size() == 128);
        const size_t b = pk.vec({1.5f, 2.5f, 3.5f}, 16);
        EXPECT(b == 128 && pk.host.size() == 192 && pk.vec({4.5f}) == 192 && pk.host.size() == 256);
        for (size_t i = 0; i < pk.host.size(); ++i) {
            const float want = i == 128 ? 1.5f : i == 129 ? 2.5f : i == 130 ? 3.5f : i == 192 ? 4.5f : 0.f;
            EXPECT(pk.host[i] == want);
        }

        // Linear [n = 3][k = 2] -> Wt[16][16] at column 0 and, a second copy, at column 5 (the concatenated q | k | v)
        const int n = 3, k = 2, ld = 16;
        std::vector<float> w(n * k);
        for (int i = 0; i < n * k; ++i) w[i] = 100.f + i;
        const size_t lin = pk.reserve(16 * 16);
        EXPECT(lin == 256 && pk.host.size() == 512);
        pk.transpose_into(lin, w, n, k, ld, 0);
        pk.transpose_into(lin, w, n, k, ld, 5);
        std::set<size_t> set_at;
        for (int col0 : {0, 5})
            for (int o = 0; o < n; ++o)
                for (int kk = 0; kk < k; ++kk) {
                    const size_t at = lin + (size_t)kk * ld + col0 + o;
                    EXPECT(pk.host[at] == w[o * k + kk] && set_at.insert(at).second);
                }
        EXPECT(set_at.size() == 2 * n * k);
        for (size_t i = lin; i < pk.host.size(); ++i) EXPECT(set_at.count(i) || pk.host[i] == 0.f);

        // conv [n = 2][cin = 3][3][3] -> [(tap * 4 + ci)][16]
        const int cn = 2, cin = 3, taps = 9, cinp = 4, np = 16;
        std::vector<float> cw(cn * cin * taps);
        for (size_t i = 0; i < cw.size(); ++i) cw[i] = 1000.f + i;
        const size_t cv = pk.conv_taps(cw, cn, cin, taps, cinp, np);
        EXPECT(cv == 512 && pk.host.size() == 512 + (size_t)taps * cinp * np);      // 576 floats: a multiple of 64 already
        set_at.clear();
        for (int o = 0; o < cn; ++o)
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < taps; ++t) {
                    const size_t at = cv + ((size_t)t * cinp + ci) * np + o;
                    EXPECT(pk.host[at] == cw[(o * cin + ci) * taps + t] && set_at.insert(at).second);
                }
        EXPECT(set_at.size() == cw.size());
        for (size_t i = cv; i < pk.host.size(); ++i) EXPECT(set_at.count(i) || pk.host[i] == 0.f);

        // no padding (a k x k patch conv read NHWC, 2 x 2 here) and one input channel (depthwise taps: [tap][n])
        const size_t plain = pk.conv_taps(cw, 3, 2, 4, 2, 3), dw = pk.conv_taps(cw, 5, 1, 9, 1, 5);
        for (int o = 0; o < 3; ++o)
            for (int ci = 0; ci < 2; ++ci)
                for (int t = 0; t < 4; ++t) EXPECT(pk.host[plain + ((size_t)t * 2 + ci) * 3 + o] == cw[(o * 2 + ci) * 4 + t]);
        for (int ch = 0; ch < 5; ++ch)
            for (int t = 0; t < 9; ++t) EXPECT(pk.host[dw + (size_t)t * 5 + ch] == cw[ch * 9 + t]);
        EXPECT(plain % 64 == 0 && dw == plain + 64 && pk.host.size() == dw + 64);
        checks += 2 * n * k + (int)cw.size() + 24 + 45;
    }
    std::printf("state_dict_check: %d checks: strict loading with its texts, every repacked element at its closed-form offset, zero elsewhere\n", checks);
    return 0;
}
