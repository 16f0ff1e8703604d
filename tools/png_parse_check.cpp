// nesr_png_parse (csrc/png_decode_api.cpp) as a stand-alone host program, for a sanitizer build: every file named on the command line
// is parsed whole; the first two also at every prefix length; and every file with `--changes N` (default 600) seeded single-byte
// changes, each time from a heap copy of exactly that size so that a read past the end is caught.  Every accepted plan is checked: each
// segment lies inside the file, the segments ascend, and a second call with a table of n_segments entries gives the same count.
// Prints one line per file; exits 1 on an unexpected return code or a plan that breaks a bound.
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -std=c++17 -g -fsanitize=address,undefined -I neural_enhanced_super_resolution_amd/csrc \
//       tools/png_parse_check.cpp neural_enhanced_super_resolution_amd/csrc/png_decode_api.cpp -L/opt/rocm/lib -lamdhip64 -o png_parse_check
//   ./png_parse_check tests/golden/png/*.png
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.h"
#include "png_decode_kernels.h"

namespace nesr {
static std::string g_error;
int set_error(int code, const std::string& msg) {
    g_error = msg;
    return code;
}
namespace pngdec {
hipError_t launch_inflate(const InflateArgs&, hipStream_t) { return hipErrorNotSupported; }     // never reached here
hipError_t launch_unfilter(const UnfilterArgs&, hipStream_t) { return hipErrorNotSupported; }
}  // namespace pngdec
}  // namespace nesr

static long g_calls = 0, g_plans = 0;
static int g_failures = 0;

// one parse from an exact-size heap copy (table of 2 entries, then of n_segments); the plan's bounds checked when it is accepted
static int parse_copy(const uint8_t* data, size_t n) {
    uint8_t* copy = new uint8_t[n ? n : 1];
    if (n) std::memcpy(copy, data, n);
    nesr_png_info info;
    nesr_png_segment two[2];
    int rc = nesr_png_parse(copy, n, &info, two, 2);
    ++g_calls;
    if (rc == NESR_ERR_NOFIT || rc == NESR_OK) {
        std::vector<nesr_png_segment> segs((size_t)info.n_segments);
        nesr_png_info again;
        rc = nesr_png_parse(copy, n, &again, segs.data(), info.n_segments);
        ++g_calls;
        if (rc != NESR_OK || again.n_segments != info.n_segments || info.n_segments < 1) {
            ++g_failures;
        } else {
            ++g_plans;
            int64_t end = 0;
            for (const nesr_png_segment& s : segs) {
                if (s.offset < end || s.bytes < 0 || (uint64_t)s.offset > n || (uint64_t)s.bytes > n - (uint64_t)s.offset) ++g_failures;
                end = s.offset + s.bytes;
            }
            if (!segs.front().first || !segs.back().last || nesr_png_decode_scratch_bytes(&again) == 0) ++g_failures;
        }
    }
    delete[] copy;
    return rc;
}

int main(int argc, char** argv) {
    long changes = 600;
    std::vector<const char*> names;
    for (int a = 1; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--changes") && a + 1 < argc) changes = std::atol(argv[++a]);
        else names.push_back(argv[a]);
    }
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
        return seed;
    };
    for (size_t k = 0; k < names.size(); ++k) {
        std::vector<uint8_t> d;
        FILE* f = std::fopen(names[k], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", names[k]); return 2; }
        for (int ch; (ch = std::fgetc(f)) != EOF;) d.push_back((uint8_t)ch);
        std::fclose(f);
        long ok = 0, unsupported = 0, bad = 0;
        auto tally = [&](int rc) {
            if (rc == NESR_OK) ++ok;
            else if (rc == NESR_ERR_UNSUPPORTED) ++unsupported;
            else if (rc == NESR_ERR_BADFILE) ++bad;
            else ++g_failures;
        };
        const int whole = parse_copy(d.data(), d.size());
        if (whole != NESR_OK) ++g_failures;
        if (k < 2)
            for (size_t n = 0; n < d.size(); ++n) {
                const int rc = parse_copy(d.data(), n);
                if (rc == NESR_OK) ++g_failures;             // a file is whole only with its IEND
                tally(rc);
            }
        std::vector<uint8_t> m(d);
        for (long c = 0; c < changes && !m.empty(); ++c) {
            const size_t at = (size_t)(next() % m.size());
            const uint8_t keep = m[at];
            m[at] = (uint8_t)(keep ^ (1u << (next() % 8)));
            if (c % 3 == 0) m[at] = (uint8_t)next();
            tally(parse_copy(m.data(), m.size()));
            m[at] = keep;
        }
        std::printf("%s: whole %d, prefixes and changed bytes: %ld ok, %ld unsupported, %ld bad\n", names[k], whole, ok, unsupported, bad);
    }
    std::printf("%zu files, %ld calls, %ld plans accepted and bounds-checked, %d unexpected results\n", names.size(), g_calls, g_plans, g_failures);
    return g_failures ? 1 : 0;
}
