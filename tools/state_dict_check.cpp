// The host side of the strict loaders of the five checkpoint networks (csrc/state_dict.h: StateDict, HostPack, HalfPack) as a
// stand-alone host program, for a sanitizer build; the library that holds their C entries is not built with one.  StateDict: a tiny
// key set, an unexpected key, a wrong rank and a wrong extent with their texts, a key loaded twice, and the missing-keys text with 0,
// 1 and 6 keys absent.  HostPack: a 3x2 Linear transposed into a padded 16x16 and a [2][3][3][3] conv repacked with cin_padded 4 and
// n_padded 16; then its packers of named tensors, norm, linear with and without a bias, and side_by_side with three parts at n = 3,
// k = 2: every element at its closed-form offset and every other float zero, the layout the kernels read, element by element.
// HalfPack: pieces of 64 halves with zero padding, 65504 passes, 65520 and NaN are noted, and the first offending key is the one
// kept.  Prints one line; exits 1 on a surprise.
// ROCm's clang++, or any compiler with _Float16 in C++ (g++ from 12):
//   clang++ -std=c++17 -g -fsanitize=address,undefined -I neural_enhanced_super_resolution_amd/csrc tools/state_dict_check.cpp -o state_dict_check
#include <cmath>
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
    {
        // the packers of named tensors: three [3][2] Linears with biases and a norm over 3 channels
        const int n = 3, k = 2, np = 16, kp = 16;
        const int64_t s32[2] = {3, 2}, s3[1] = {3};
        const char* const parts[3] = {".q", ".k", ".v"};
        nesr::StateDict sd;
        std::vector<float> w[3], b[3];
        for (int p = 0; p < 3; ++p) {
            sd.expect_wb(std::string("a") + parts[p], {3, 2});
            for (int i = 0; i < n * k; ++i) w[p].push_back(100.f * (p + 1) + i);
            for (int i = 0; i < n; ++i) b[p].push_back(-10.f * (p + 1) - i);
            EXPECT(sd.load(std::string("a") + parts[p] + ".weight", w[p].data(), s32, 2) == NESR_OK);
            EXPECT(sd.load(std::string("a") + parts[p] + ".bias", b[p].data(), s3, 1) == NESR_OK);
        }
        sd.expect_wb("a.norm", {3});
        const float g[3] = {7.f, 8.f, 9.f}, beta[3] = {-7.f, -8.f, -9.f};
        EXPECT(sd.load("a.norm.weight", g, s3, 1) == NESR_OK && sd.load("a.norm.bias", beta, s3, 1) == NESR_OK && sd.missing().empty());

        nesr::HostPack pk;
        std::set<size_t> set_at;
        auto placed = [&](size_t at, float want) { return pk.host[at] == want && set_at.insert(at).second; };

        const nesr::NormW nw = pk.norm(sd, "a.norm", 3);      // gamma and beta, a piece of 64 each (round16(3) = 16 floats asked for)
        EXPECT(nw.c == 3 && nw.g == 0 && nw.b == 64 && pk.host.size() == 128);
        for (int i = 0; i < 3; ++i) EXPECT(placed(nw.g + i, g[i]) && placed(nw.b + i, beta[i]));

        const nesr::LinW with = pk.linear(sd, "a.q", n, k);      // Wt[16][16], then the bias
        EXPECT(with.kp == kp && with.np == np && with.w == 128 && with.b == with.w + (size_t)kp * np && pk.host.size() == with.b + 64);
        const nesr::LinW without = pk.linear(sd, "a.k", n, k, false);      // the same layout, the bias piece left zero
        EXPECT(without.kp == kp && without.np == np && without.w == with.b + 64 && without.b == without.w + (size_t)kp * np && pk.host.size() == without.b + 64);
        for (int o = 0; o < n; ++o) {
            for (int kk = 0; kk < k; ++kk) EXPECT(placed(with.w + (size_t)kk * np + o, w[0][o * k + kk]) && placed(without.w + (size_t)kk * np + o, w[1][o * k + kk]));
            EXPECT(placed(with.b + o, b[0][o]));
        }

        const nesr::LinW qkv = pk.side_by_side(sd, "a", {".q", ".k", ".v"}, n, k);      // Wt[16][48]: part p from column 16 p; the bias [48]
        EXPECT(qkv.kp == kp && qkv.np == 3 * np && qkv.w == without.b + 64 && qkv.b == qkv.w + (size_t)kp * 3 * np && pk.host.size() == qkv.b + 64);
        for (int p = 0; p < 3; ++p)
            for (int o = 0; o < n; ++o) {
                for (int kk = 0; kk < k; ++kk) EXPECT(placed(qkv.w + (size_t)kk * 3 * np + p * np + o, w[p][o * k + kk]));
                EXPECT(placed(qkv.b + p * np + o, b[p][o]));
            }
        const nesr::LinW bare = pk.side_by_side(sd, "a", {".v", ".q"}, n, k, false);      // two parts, no bias: the bias piece left zero
        EXPECT(bare.np == 2 * np && bare.w == qkv.b + 64 && bare.b == bare.w + (size_t)kp * 2 * np && pk.host.size() == bare.b + 64);
        for (int p = 0; p < 2; ++p)
            for (int o = 0; o < n; ++o)
                for (int kk = 0; kk < k; ++kk) EXPECT(placed(bare.w + (size_t)kk * 2 * np + p * np + o, w[p == 0 ? 2 : 0][o * k + kk]));
        EXPECT(set_at.size() == 6 + 2 * (size_t)n * k + n + 3 * (size_t)(n * k + n) + 2 * (size_t)n * k);
        for (size_t i = 0; i < pk.host.size(); ++i) EXPECT(set_at.count(i) || pk.host[i] == 0.f);
        checks += (int)set_at.size() + 12;
    }
    {
        nesr::HalfPack hp;
        EXPECT(hp.reserve(1) == 0 && hp.half.size() == 64 && hp.reserve(64) == 64 && hp.half.size() == 128 && hp.reserve(65) == 128 && hp.half.size() == 256);
        EXPECT(hp.reserve(0) == 256 && hp.half.size() == 256);
        for (_Float16 v : hp.half) EXPECT(v == (_Float16)0.f);
        EXPECT(nesr::HalfPack::carries(65504.f) && nesr::HalfPack::carries(-65504.f) && !nesr::HalfPack::carries(65520.f) && !nesr::HalfPack::carries(NAN) &&
               !nesr::HalfPack::carries(-INFINITY));
        hp.half[0] = hp.put("first", 65504.f);      // f16's largest finite value passes, both signs
        hp.half[1] = hp.put("first", -65504.f);
        hp.half[2] = hp.put("first", 0.1f);
        EXPECT(hp.out_of_range().empty() && (float)hp.half[0] == 65504.f && (float)hp.half[1] == -65504.f && hp.half[2] == (_Float16)0.1f);
        hp.half[3] = hp.put("second", 65520.f);      // rounds to infinity: noted
        EXPECT(hp.out_of_range() == "second");
        hp.half[4] = hp.put("third", NAN);           // noted too, but the first offending key is the one kept
        hp.note("fourth", true);
        hp.note("fifth", false);
        hp.put("sixth", 1.f);
        EXPECT(hp.out_of_range() == "second");
        nesr::HalfPack nan_first;
        nan_first.note("fine", false);
        nan_first.put("nan", NAN);
        nan_first.put("large", -1e30f);
        EXPECT(nan_first.out_of_range() == "nan" && nan_first.half.empty());
        checks += 256 + 12;
    }
    std::printf("state_dict_check: %d checks: strict loading with its texts, every repacked element at its closed-form offset, zero elsewhere, the fp16 form's range notes\n", checks);
    return 0;
}
