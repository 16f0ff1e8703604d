// Launchers of the baseline JPEG decoder (jpeg_decode.hip) and the layout of its scratch, shared with jpeg_decode_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nesr_hip.h"

namespace nesr {
namespace jpegdec {

constexpr int UNSTUFF_CHUNK = 4096;        // bytes of the scan per workgroup of the scan preparation (256 lanes of 16 bytes)
constexpr int SUBSEQ_BITS = 1024;          // bits of the unstuffed stream per lane of the self-synchronising decode
constexpr int SUBSEQ_PER_GROUP = 256;      // lanes per workgroup of that decode
constexpr int RECON_BLOCKS = 32;           // blocks per workgroup of the reconstruction: 256 lanes, one row or column of a block each
constexpr int DC_GROUP = 256;              // MCUs per workgroup of the DC prefix sum
constexpr int DRI_LANES = 64;              // restart intervals per workgroup of the restart-interval decode
constexpr int64_t MAX_SCAN_BYTES = 1 << 28;   // bit positions are 32-bit

// bits of the status word (0: the file decoded)
constexpr uint32_t ST_RST_COUNT = 1;       // not the number of restart markers the frame calls for
constexpr uint32_t ST_RST_NUMBER = 2;      // a restart marker out of sequence
constexpr uint32_t ST_BAD_CODE = 4;        // a code that is not in the table, or a DC size above 15
constexpr uint32_t ST_RUN = 8;             // a run past coefficient 63
constexpr uint32_t ST_EARLY = 16;          // the stream (or a restart interval) ends before its blocks do
constexpr uint32_t ST_EXTRA = 32;          // more blocks than the frame holds

// Regions of the scratch, each 256-byte aligned (jpeg_decode_api.cpp: plan())
struct Plan {
    int H, W, C, hs, vs, ri;
    int mcus_x, mcus_y, per;               // per: blocks per MCU
    int64_t nmcu, nblocks, nseg;           // nseg: restart intervals (1 without DRI)
    int64_t scan_bytes, nchunks;           // nchunks: ceil(scan_bytes / UNSTUFF_CHUNK)
    int64_t stream_words;                  // capacity of the unstuffed stream in 32-bit words
    int64_t nsub, ngroups;                 // upper bounds: ceil(scan bits / SUBSEQ_BITS), ceil(nsub / SUBSEQ_PER_GROUP)
    int64_t dc_groups;                     // ceil(nmcu / DC_GROUP)
    int ypitch, yrows, cpitch, crows;      // component planes, whole MCUs
    size_t off_tables, off_chunk, off_meta, off_seg, off_stream, off_rec, off_cnt, off_coef, off_dc, off_y, off_cb, off_cr, total;
};

struct DecodeArgs {
    const uint8_t* scan;                   // the scan's first byte in the file on the device
    const nesr_jpeg_huff* tables_host;     // dc[3] then ac[3], per component
    nesr_jpeg_huff* tables;                // their copy in the scratch
    uint16_t q[3][64];                     // per component, natural order
    uint64_t* chunk;                       // [nchunks] dropped bytes | restart markers << 32, then their exclusive scan
    uint32_t* meta;                        // [0] bytes of the unstuffed stream  [1] subsequences  [2] blocks decoded  [16] unsynchronised workgroups
    uint32_t* seg;                         // [nseg] byte at which each restart interval starts in the unstuffed stream
    uint32_t* stream;                      // the unstuffed stream, zero past its end
    uint64_t* rec;                         // [nsub] state at the end of each subsequence: bit | zigzag index << 32 | block in MCU << 40
    uint32_t* cnt;                         // [nsub] blocks completed in each subsequence, then their exclusive scan
    int16_t* coef;                         // [nblocks][64] natural order, blocks in scan order
    int32_t* dc;                           // [dc_groups][3] sums of DC differences, then their exclusive scan
    uint8_t *y, *cb, *cr;
    uint8_t* dst;
    int64_t dst_stride;
    int bgr;
    uint32_t* status;
};

// enqueues everything on s; without DRI it waits for s once per launch of the synchronisation sequence (a 4-byte read each).
// rounds / launches (may be null): launches of that sequence, and kernel launches in all.
hipError_t launch_decode(const Plan& p, const DecodeArgs& a, hipStream_t s, int* rounds, int* launches);

}  // namespace jpegdec
}  // namespace nesr
