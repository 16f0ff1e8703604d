// nesr_jpeg_parse (csrc/jpeg_decode_api.cpp) as a stand-alone host program, for a sanitizer build: every file named on the command
// line is parsed whole, at every prefix length up to its scan, and with each header byte changed in turn, each time from a heap copy
// of exactly that size so that a read past the end is caught.  Prints one line per file; exits 1 on an unexpected return code.
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -std=c++17 -g -fsanitize=address,undefined -I neural_enhanced_super_resolution_amd/csrc \
//       tools/jpeg_parse_check.cpp neural_enhanced_super_resolution_amd/csrc/jpeg_decode_api.cpp -L/opt/rocm/lib -lamdhip64 -o jpeg_parse_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.h"
#include "jpeg_decode_kernels.h"

namespace nesr {
static std::string g_error;
int set_error(int code, const std::string& msg) {
    g_error = msg;
    return code;
}
namespace jpegdec {
hipError_t launch_decode(const Plan&, const DecodeArgs&, hipStream_t, int*, int*) { return hipErrorNotSupported; }   // never reached here
}  // namespace jpegdec
}  // namespace nesr

static int parse_copy(const uint8_t* data, size_t n, nesr_jpeg_info* info) {
    uint8_t* copy = new uint8_t[n ? n : 1];
    if (n) std::memcpy(copy, data, n);
    const int rc = nesr_jpeg_parse(copy, n, info);
    delete[] copy;
    return rc;
}

int main(int argc, char** argv) {
    static nesr_jpeg_info info;
    int failures = 0;
    for (int a = 1; a < argc; ++a) {
        std::vector<uint8_t> d;
        FILE* f = std::fopen(argv[a], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        for (int ch; (ch = std::fgetc(f)) != EOF;) d.push_back((uint8_t)ch);
        std::fclose(f);
        const int whole = parse_copy(d.data(), d.size(), &info);
        size_t head = d.size();
        if (whole == NESR_OK) {
            head = (size_t)info.scan_offset;
            if (info.scan_offset + info.scan_bytes > (int64_t)d.size() || nesr_jpeg_decode_scratch_bytes(&info) == 0) ++failures;
        }
        long ok = 0, unsupported = 0, bad = 0;
        auto tally = [&](int rc) {
            if (rc == NESR_OK) ++ok;
            else if (rc == NESR_ERR_UNSUPPORTED) ++unsupported;
            else if (rc == NESR_ERR_BADFILE) ++bad;
            else ++failures;
        };
        const size_t upto = head + 4 < d.size() ? head + 4 : d.size();
        for (size_t n = 0; n <= upto; ++n) tally(parse_copy(d.data(), n, &info));
        std::vector<uint8_t> m(d.begin(), d.begin() + upto);
        for (size_t at = 0; at < head && at < upto; ++at) {
            const uint8_t keep = m[at];
            for (uint8_t v : {(uint8_t)0x00, (uint8_t)0xFF, (uint8_t)(keep ^ 0x10), (uint8_t)(keep + 1)}) {
                m[at] = v;
                tally(parse_copy(m.data(), m.size(), &info));
            }
            m[at] = keep;
        }
        std::printf("%s: whole %d, prefixes and changed bytes: %ld ok, %ld unsupported, %ld bad\n", argv[a], whole, ok, unsupported, bad);
    }
    std::printf("%d files, %d unexpected results\n", argc - 1, failures);
    return failures ? 1 : 0;
}
