// Launchers of the PNG decoder (png_decode.hip) and the layout of its scratch (tests/png_decode_ref.py is the specification).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nesr_hip.h"

namespace nesr {
namespace pngdec {

// bits of the status word
constexpr uint32_t ST_TRUNC = 1;           // a segment's input ran out (or the segment lies outside the file)
constexpr uint32_t ST_BADCODE = 2;         // a code that is in no table, literal/length symbol 286 / 287, distance symbol 30 / 31
constexpr uint32_t ST_BADSTORED = 4;       // LEN != ~NLEN
constexpr uint32_t ST_BADHEADER = 8;       // BTYPE 3 or a dynamic header that breaks a rule
constexpr uint32_t ST_DEPENDENT = 16;      // a distance that reaches before the segment's first byte: not a bad file
constexpr uint32_t ST_BADEND = 32;         // BFINAL in a segment that is not the last, or bytes behind the last block
constexpr uint32_t ST_TOTAL = 64;          // the segments' sizes do not add up to N
constexpr uint32_t ST_ADLER = 128;
constexpr uint32_t ST_FILTER = 256;        // a filter type above 4

constexpr int ADLER_PIECE = 32768;         // bytes per partial Adler sum
constexpr int UNFILTER_LANES = 256;        // rows of one band of the unfilter's wavefront

// Regions of the scratch, each 256-byte aligned (png_decode_api.cpp: plan())
struct Plan {
    int H, W, C, depth, bpp;
    int64_t row;                           // 1 + W * bpp
    int64_t N;                             // H * row
    int64_t nseg, npieces;
    size_t off_filt, off_carry, off_size, off_offs, off_segst, off_adler, total;
};

struct InflateArgs {
    const uint8_t* file;
    uint64_t n;                            // bytes of the file: no load at or beyond it
    const nesr_png_segment* segs;
    int64_t nseg;
    int64_t N;
    uint64_t* size;                        // [nseg] bytes each segment inflates to
    uint64_t* offs;                        // [nseg] their exclusive scan
    uint32_t* segst;                       // [nseg] status bits of each segment
    uint8_t* filt;                         // [N] the filtered stream
    uint64_t* adler;                       // [npieces]
    int64_t npieces;
    uint32_t expect_adler;
    uint32_t* status;
};

struct UnfilterArgs {
    const uint8_t* filt;                   // [H][row]
    uint8_t* carry;                        // [H][row - 1] raw rows handed from one band of a group to the next (only those rows are written)
    int H, W, bpp, bps, C;                 // bps: bytes per sample
    int64_t row;
    int flip;                              // the frame is B G R (A)
    uint8_t* dst;
    int64_t dst_stride;
    uint32_t* status;
    int status_gate;                       // read by launch_unfilter only: 0 launches pngd_clear first (nesr_png_unfilter: nothing wrote
                                           // the word yet); the kernel itself always skips the pass on a non-zero word
};

hipError_t launch_inflate(const InflateArgs& a, hipStream_t s);
hipError_t launch_unfilter(const UnfilterArgs& a, hipStream_t s);

}  // namespace pngdec
}  // namespace nesr
