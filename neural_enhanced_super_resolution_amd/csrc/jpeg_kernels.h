// Launchers of the baseline JPEG encoder (jpeg.hip) and the layout of its scratch, shared with jpeg_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nesr {
namespace jpeg {

constexpr int MAX_HEADER = 640;            // SOI .. SOS: 623 bytes for colour, 328 for gray, 6 more with DRI
constexpr int BLOCKS_PER_GROUP = 256;      // blocks per workgroup of the length and emit passes = one chunk of the bit-offset scan
constexpr int STUFF_CHUNK = 4096;          // unstuffed bytes per chunk of the byte-stuffing passes
// Most bits one block can take: DC 11 + 11, 63 AC symbols of 16 + 10.  1660 bits = 207.5 bytes.
constexpr int MAX_BLOCK_BYTES = 208;

struct Header {
    uint8_t bytes[MAX_HEADER];
};

// Regions of the scratch, each 256-byte aligned (jpeg_api.cpp: plan())
struct Plan {
    int H, W, C;
    int mcus_x, mcus_y;                    // MCUs: 16 x 16 pixels for colour, one 8 x 8 block for gray
    int64_t nblocks;                       // blocks of the scan, dummy blocks included
    int64_t nchunks;                       // ceil(nblocks / BLOCKS_PER_GROUP)
    int64_t stream_bytes;                  // capacity of the unstuffed stream (a multiple of STUFF_CHUNK)
    int64_t stuff_chunks;                  // stream_bytes / STUFF_CHUNK
    size_t off_coef, off_len, off_chunk, off_meta, off_stream, off_ff, total;
    // the options (nesr_jpeg_opts); with the defaults every field below is 0 / empty and launch_encode runs the kernels without them
    int sampling;                          // SAMPLING_420 | 422 | 444 (gray: 420)
    int per, ny;                           // blocks per MCU (1, 3, 4, 6) and how many of them are Y
    int optimize, ri;                      // Huffman tables built on the device; MCUs per restart interval (0: none)
    int64_t nint;                          // restart intervals (1 without)
    size_t off_hist, off_luts, off_ivend, off_ivb;
};

enum { SAMPLING_420 = 0, SAMPLING_422 = 1, SAMPLING_444 = 2 };
constexpr int LUT_WORDS = 2 * 16 + 2 * 256;  // symbol -> code << 8 | length: dc[2][16], ac[2][256]
constexpr int MAX_TAIL = 24;                 // DRI and SOS, the bytes behind the DHTs the device writes
// meta words beyond EncodeArgs::meta's three: [3] bits of the scan, [4] unstuffed bytes with each interval rounded up, [5] header bytes

struct EncodeArgs {
    const uint8_t* src;
    int64_t src_stride;
    int bgr;
    uint16_t q[2][64];                     // quantisation tables, natural order
    int16_t* coef;                         // [nblocks][64] zigzag
    uint32_t* len;                         // [nblocks] bits
    uint64_t* chunk;                       // [nchunks] bits per chunk, then their exclusive scan
    uint64_t* meta;                        // [0] unstuffed bytes  [1] their chunks  [2] 0xFF bytes among them
    uint32_t* stream;                      // the unstuffed stream, zeroed
    uint64_t* ff;                          // [stuff_chunks] 0xFF bytes per chunk, then their exclusive scan
    uint8_t* out;
    uint64_t out_cap;
    uint64_t* out_len;                     // [0] bytes of the file  [1] 1 if it did not fit
    int header_bytes;
    // options only
    uint64_t* hist;                        // [4][256] symbol counts: (table 0 | 1) x (DC | AC)
    uint32_t* luts;                        // [LUT_WORDS] of the optimised tables
    uint64_t* ivend;                       // [nint] bits of the scan up to each interval's end, intervals not rounded up
    uint64_t* ivb;                         // [nint] bytes per interval, then their exclusive scan: the byte an interval starts at
    uint8_t tail[MAX_TAIL];                // optimize: header_bytes covers SOI .. SOF0, the DHTs follow on the device, then these
    int tail_bytes;
};

// default options: the kernels without them; any other: the MCU shape's transform, tables and header length from device memory,
// restart intervals
hipError_t launch_encode(const Plan& p, const EncodeArgs& a, const Header& h, hipStream_t s);

}  // namespace jpeg
}  // namespace nesr
