// Baseline JPEG encoder for gfx950: libjpeg's compressor as cv2.imwrite runs it by default (quality-scaled Annex K tables, 4:2:0 for
// colour, islow integer FDCT, Annex K Huffman tables, no restart markers), byte for byte (tests/jpeg_ref.py is the specification).
//
// Passes, all on one stream, nothing returns to the host between them:
//   header     the SOI .. SOS bytes (a kernel argument) into out
//   transform  colour conversion, edge replication, h2v2 chroma downsampling, level shift, FDCT, quantisation; zigzag int16
//              coefficients in scan order (Y00 Y01 Y10 Y11 Cb Cr per MCU, MCUs in raster order; gray: one block per MCU)
//   lengths    bits per block (DC difference against the previous block of the component, AC run/size symbols), bits per chunk
//   scan       exclusive scan of the chunk sums, 64-bit (a 16384 x 16384 noise frame exceeds 2^32 bits)
//   zero       clears the words of the unstuffed stream the scan found to be needed
//   emit       every block writes its bits at its offset; the first and last word of a block may be shared with its neighbours and
//              are combined with atomicOr (disjoint bits: the result does not depend on the order), the words between are stored
//   count      0xFF bytes per 4096-byte chunk of the unstuffed stream;  scan: their exclusive scan
//   stuff      copies each chunk behind the header with 0x00 after each 0xFF
//   finish     FF D9, the length word and the status word
// No pass writes out[i] for i >= out_cap.
//
// The options (4:4:4 / 4:2:2, Huffman tables optimised for the frame, restart intervals; tests/jpeg_options_ref.py is their
// specification) run the same passes, with the EX = true instantiations of lengths, emit, stuff and finish, and
//   transform  jpeg_transform_row for the MCUs that are one block row high (4:4:4, 4:2:2)
//   histogram, build tables   (optimize) symbol counts, then libjpeg's jpeg_gen_optimal_table by one workgroup: BITS / HUFFVAL, the
//              code tables, and the DHT, DRI and SOS bytes of the header, whose length is then known on the device only
//   interval ends, bytes, scan   (restart interval) the byte each interval starts at; stuff inserts FF Dn between intervals
// The default options run the EX = false instantiations, which never read the options' argument.
#include "codec_device.h"
#include "jpeg_kernels.h"
#include "jpeg_tables.h"

namespace nesr {
namespace jpeg {

namespace {

// symbol -> (code << 8 | length), canonical codes from BITS / HUFFVAL; table 0 luminance, 1 chrominance
struct DevTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint8_t inv_zigzag[64];
};

constexpr void fill_codes(uint32_t* lut, const uint8_t* bits, const uint8_t* vals, int nvals) {
    uint32_t code = 0;
    int k = 0;
    for (int length = 1; length <= 16; ++length) {
        for (int i = 0; i < bits[length - 1] && k < nvals; ++i, ++k, ++code) lut[vals[k]] = (code << 8) | (uint32_t)length;
        code <<= 1;
    }
}

constexpr DevTables make_tables() {
    DevTables t{};
    const uint8_t dcv[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    fill_codes(t.dc[0], DC_LUMA_BITS, dcv, 12);
    fill_codes(t.dc[1], DC_CHROMA_BITS, dcv, 12);
    fill_codes(t.ac[0], AC_LUMA_BITS, AC_LUMA_VALS, 162);
    fill_codes(t.ac[1], AC_CHROMA_BITS, AC_CHROMA_VALS, 162);
    for (int i = 0; i < 64; ++i) t.inv_zigzag[i] = INV_ZIGZAG[i];
    return t;
}

__device__ const DevTables TABLES = make_tables();

constexpr int TRANSFORM_THREADS = 256;
constexpr int STRIP_BLOCKS = 96;           // blocks per workgroup of the transform: 16 colour MCUs, or 96 gray blocks of one block row
constexpr int WS_PITCH = 72;               // int32 per block between the FDCT passes: rows of 9 (odd: no bank conflicts either way)

// ---------------------------------------------------------------------------------------------------------------- transform
// jfdctint.c, one 8-point pass.  first: outputs 0 and 4 are << 2, the others DESCALE(., 11); second: DESCALE(., 2) and DESCALE(., 15).
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int d[8], int o[8]) {
    constexpr int N = FIRST ? 11 : 15;
    constexpr int R = 1 << (N - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        o[0] = (t10 + t11) * 4;
        o[4] = (t10 - t11) * 4;
    } else {
        o[0] = (t10 + t11 + 2) >> 2;
        o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + R) >> N;
    o[6] = (z1 - t12 * 15137 + R) >> N;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 = -z1 * 7373;
    z2 = -z2 * 20995;
    z3 = -z3 * 16069 + z5;
    z4 = -z4 * 3196 + z5;
    o[7] = (a4 + z1 + z3 + R) >> N;
    o[5] = (a5 + z2 + z4 + R) >> N;
    o[3] = (a6 + z2 + z3 + R) >> N;
    o[1] = (a7 + z1 + z4 + R) >> N;
}

struct TransformArgs {
    const uint8_t* src;
    int64_t stride;
    int H, W, bgr;
    int mcus_x;
    uint16_t q[2][64];
    int16_t* coef;
};

__device__ __forceinline__ void ycc(const uint8_t* p, int bgr, int& y, int& cb, int& cr) {
    const int r = p[bgr ? 2 : 0], g = p[1], b = p[bgr ? 0 : 2];
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// COLOR: blockIdx.x = strip of 16 MCUs, blockIdx.y = MCU row.  Gray: blockIdx.x = strip of 96 blocks, blockIdx.y = block row.
template <bool COLOR>
__global__ __launch_bounds__(TRANSFORM_THREADS) void jpeg_transform(const TransformArgs a) {
    __shared__ uint8_t smp[6144];                          // colour: Y [16][256], Cb [8][128], Cr [8][128]; gray: [8][768]
    __shared__ int ws[STRIP_BLOCKS * WS_PITCH];
    __shared__ __attribute__((aligned(16))) int16_t outb[STRIP_BLOCKS * 64];
    const int tid = threadIdx.x;
    const int strip = blockIdx.x, row = blockIdx.y;
    const int units = COLOR ? 16 : STRIP_BLOCKS;           // MCUs of a full strip
    const int u0 = strip * units;
    const int nu = min(units, a.mcus_x - u0);              // MCUs of this strip
    const int H = a.H, W = a.W;

    if (COLOR) {
        const int half_rows = (H + 1) >> 1;                // chroma rows that have source rows
        for (int q = tid; q < 8 * 128; q += TRANSFORM_THREADS) {
            const int qy = q >> 7, qx = q & 127;
            const int x0 = min(u0 * 16 + 2 * qx, W - 1), x1 = min(u0 * 16 + 2 * qx + 1, W - 1);
            const int y0 = min(row * 16 + 2 * qy, H - 1), y1 = min(row * 16 + 2 * qy + 1, H - 1);
            const uint8_t* r0 = a.src + (int64_t)y0 * a.stride;
            const uint8_t* r1 = a.src + (int64_t)y1 * a.stride;
            int y[4], cb[4], cr[4];
            ycc(r0 + (int64_t)x0 * 3, a.bgr, y[0], cb[0], cr[0]);
            ycc(r0 + (int64_t)x1 * 3, a.bgr, y[1], cb[1], cr[1]);
            ycc(r1 + (int64_t)x0 * 3, a.bgr, y[2], cb[2], cr[2]);
            ycc(r1 + (int64_t)x1 * 3, a.bgr, y[3], cb[3], cr[3]);
            smp[(2 * qy) * 256 + 2 * qx] = (uint8_t)y[0];
            smp[(2 * qy) * 256 + 2 * qx + 1] = (uint8_t)y[1];
            smp[(2 * qy + 1) * 256 + 2 * qx] = (uint8_t)y[2];
            smp[(2 * qy + 1) * 256 + 2 * qx + 1] = (uint8_t)y[3];
            // chroma rows past the last downsampled row repeat THAT row (the source is padded to even height only); this differs
            // from the Y rows exactly when H = 8 mod 16
            const int cy = row * 8 + qy;
            if (cy >= half_rows) {
                const int e0 = min(2 * (half_rows - 1), H - 1), e1 = min(2 * (half_rows - 1) + 1, H - 1);
                const uint8_t* s0 = a.src + (int64_t)e0 * a.stride;
                const uint8_t* s1 = a.src + (int64_t)e1 * a.stride;
                int t;
                ycc(s0 + (int64_t)x0 * 3, a.bgr, t, cb[0], cr[0]);
                ycc(s0 + (int64_t)x1 * 3, a.bgr, t, cb[1], cr[1]);
                ycc(s1 + (int64_t)x0 * 3, a.bgr, t, cb[2], cr[2]);
                ycc(s1 + (int64_t)x1 * 3, a.bgr, t, cb[3], cr[3]);
            }
            const int bias = 1 + (qx & 1);                 // strips start at even chroma columns
            smp[4096 + qy * 128 + qx] = (uint8_t)((cb[0] + cb[1] + cb[2] + cb[3] + bias) >> 2);
            smp[5120 + qy * 128 + qx] = (uint8_t)((cr[0] + cr[1] + cr[2] + cr[3] + bias) >> 2);
        }
    } else {
        for (int q = tid; q < 8 * 768; q += TRANSFORM_THREADS) {
            const int qy = q / 768, qx = q - qy * 768;
            const int x = min(u0 * 8 + qx, W - 1), y = min(row * 8 + qy, H - 1);
            smp[q] = a.src[(int64_t)y * a.stride + x];
        }
    }
    __syncthreads();

    // row pass: task t = (block, row)
    for (int t = tid; t < STRIP_BLOCKS * 8; t += TRANSFORM_THREADS) {
        const int b = t >> 3, r = t & 7;
        const uint8_t* s;
        if (COLOR) {
            const int m = b / 6, k = b - m * 6;
            s = k < 4 ? smp + ((k >> 1) * 8 + r) * 256 + m * 16 + (k & 1) * 8 : smp + 4096 + (k - 4) * 1024 + r * 128 + m * 8;
        } else {
            s = smp + r * 768 + b * 8;
        }
        int d[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (int)s[i] - 128;
        fdct8<true>(d, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[t * 9 + i] = o[i];
    }
    __syncthreads();

    // column pass and quantisation: task t = (block, column)
    const int blocks_w = (W + 7) >> 3, blocks_h = (H + 7) >> 3;
    for (int t = tid; t < STRIP_BLOCKS * 8; t += TRANSFORM_THREADS) {
        const int b = t >> 3, c = t & 7;
        int comp = 0;
        bool dummy = false;
        if (COLOR) {
            const int m = b / 6, k = b - m * 6;
            comp = k < 4 ? 0 : 1;
            dummy = k < 4 && ((u0 + m) * 2 + (k & 1) >= blocks_w || row * 2 + (k >> 1) >= blocks_h);
        }
        int d[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = ws[b * WS_PITCH + r * 9 + c];
        fdct8<false>(d, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n = r * 8 + c;
            const unsigned Q = a.q[comp][n];
            const unsigned mag = ((unsigned)abs(o[r]) + 4u * Q) / (8u * Q);      // exact integer division
            outb[b * 64 + TABLES.inv_zigzag[n]] = dummy ? (int16_t)0 : (int16_t)(o[r] < 0 ? -(int)mag : (int)mag);
        }
    }
    __syncthreads();
    if (COLOR) {
        // dummy Y blocks: no AC, the DC of the block coded just before them in the MCU (which may itself be a dummy)
        if (tid < 16) {
            for (int k = 1; k < 4; ++k)
                if ((u0 + tid) * 2 + (k & 1) >= blocks_w || row * 2 + (k >> 1) >= blocks_h) outb[(tid * 6 + k) * 64] = outb[(tid * 6 + k - 1) * 64];
        }
        __syncthreads();
    }
    const int per = COLOR ? 6 : 1;
    const int64_t first = ((int64_t)row * a.mcus_x + u0) * per;       // first block of the strip in scan order
    uint4* dst = reinterpret_cast<uint4*>(a.coef + first * 64);
    const uint4* from = reinterpret_cast<const uint4*>(outb);
    for (int i = tid; i < nu * per * 8; i += TRANSFORM_THREADS) dst[i] = from[i];
}

// The MCUs that are one block row high: HS = 1 is 4:4:4 (Y Cb Cr, 8 x 8 pixels, a strip of 32 MCUs), HS = 2 is 4:2:2 (Y0 Y1 Cb Cr,
// 16 x 8 pixels, a strip of 24 MCUs); both strips are STRIP_BLOCKS blocks.  blockIdx.x = strip, blockIdx.y = MCU row.
// h2v1: source columns are replicated to the MCU width, chroma is (a + b + bias) >> 1 with bias 0, 1, 0, 1 along the row; rows past
// the last are copies of it (no vertical mixing, so replicating source rows and replicating downsampled rows are the same).
template <int HS>
__global__ __launch_bounds__(TRANSFORM_THREADS) void jpeg_transform_row(const TransformArgs a) {
    constexpr int PER = HS + 2;                            // blocks per MCU
    constexpr int UNITS = STRIP_BLOCKS / PER;              // MCUs of a full strip
    constexpr int CW = UNITS * 8, YW = CW * HS;            // chroma and Y samples per row of the strip
    static_assert(8 * YW + 16 * CW == 6144, "the strip's samples fill smp");
    __shared__ uint8_t smp[6144];                          // Y [8][YW], Cb [8][CW], Cr [8][CW]
    __shared__ int ws[STRIP_BLOCKS * WS_PITCH];
    __shared__ __attribute__((aligned(16))) int16_t outb[STRIP_BLOCKS * 64];
    const int tid = threadIdx.x;
    const int strip = blockIdx.x, row = blockIdx.y;
    const int u0 = strip * UNITS;
    const int nu = min(UNITS, a.mcus_x - u0);
    const int H = a.H, W = a.W;
    for (int q = tid; q < 8 * CW; q += TRANSFORM_THREADS) {
        const int qy = q / CW, qx = q - qy * CW;
        const uint8_t* r0 = a.src + (int64_t)min(row * 8 + qy, H - 1) * a.stride;
        int y, cb, cr;
        if (HS == 1) {
            ycc(r0 + (int64_t)min(u0 * 8 + qx, W - 1) * 3, a.bgr, y, cb, cr);
            smp[qy * YW + qx] = (uint8_t)y;
        } else {
            int y1, cb1, cr1;
            ycc(r0 + (int64_t)min(u0 * 16 + 2 * qx, W - 1) * 3, a.bgr, y, cb, cr);
            ycc(r0 + (int64_t)min(u0 * 16 + 2 * qx + 1, W - 1) * 3, a.bgr, y1, cb1, cr1);
            smp[qy * YW + 2 * qx] = (uint8_t)y;
            smp[qy * YW + 2 * qx + 1] = (uint8_t)y1;
            const int bias = qx & 1;                       // strips start at even chroma columns
            cb = (cb + cb1 + bias) >> 1;
            cr = (cr + cr1 + bias) >> 1;
        }
        smp[8 * YW + qy * CW + qx] = (uint8_t)cb;
        smp[8 * YW + 8 * CW + qy * CW + qx] = (uint8_t)cr;
    }
    __syncthreads();
    for (int t = tid; t < STRIP_BLOCKS * 8; t += TRANSFORM_THREADS) {
        const int b = t >> 3, r = t & 7;
        const int m = b / PER, k = b - m * PER;
        const uint8_t* s = k < HS ? smp + r * YW + m * 8 * HS + k * 8 : smp + 8 * YW + (k - HS) * 8 * CW + r * CW + m * 8;
        int d[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (int)s[i] - 128;
        fdct8<true>(d, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[t * 9 + i] = o[i];
    }
    __syncthreads();
    const int blocks_w = (W + 7) >> 3;
    for (int t = tid; t < STRIP_BLOCKS * 8; t += TRANSFORM_THREADS) {
        const int b = t >> 3, c = t & 7;
        const int m = b / PER, k = b - m * PER;
        const int comp = k < HS ? 0 : 1;
        const bool dummy = HS == 2 && k == 1 && (u0 + m) * 2 + 1 >= blocks_w;
        int d[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = ws[b * WS_PITCH + r * 9 + c];
        fdct8<false>(d, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n = r * 8 + c;
            const unsigned Q = a.q[comp][n];
            const unsigned mag = ((unsigned)abs(o[r]) + 4u * Q) / (8u * Q);
            outb[b * 64 + TABLES.inv_zigzag[n]] = dummy ? (int16_t)0 : (int16_t)(o[r] < 0 ? -(int)mag : (int)mag);
        }
    }
    __syncthreads();
    if (HS == 2) {
        // the dummy second Y block: no AC, the DC of the block coded just before it
        if (tid < UNITS && (u0 + tid) * 2 + 1 >= blocks_w) outb[(tid * PER + 1) * 64] = outb[tid * PER * 64];
        __syncthreads();
    }
    const int64_t first = ((int64_t)row * a.mcus_x + u0) * PER;
    uint4* dst = reinterpret_cast<uint4*>(a.coef + first * 64);
    const uint4* from = reinterpret_cast<const uint4*>(outb);
    for (int i = tid; i < nu * PER * 8; i += TRANSFORM_THREADS) dst[i] = from[i];
}

// ---------------------------------------------------------------------------------------------------------------- entropy coding
__device__ __forceinline__ int bit_length(int v) { return 32 - __clz(v); }      // v >= 0

// The symbols of one block in coding order: sink(code, length) for each Huffman code and each run of extra bits.
template <typename Sink>
__device__ __forceinline__ void code_block(const int16_t* coef, int prev_dc, const uint32_t* dc_lut, const uint32_t* ac_lut, Sink&& sink) {
    const uint4* p = reinterpret_cast<const uint4*>(coef);
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 v = p[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (int)(int16_t)(w[j >> 1] >> ((j & 1) * 16));
            if (g == 0 && j == 0) {
                const int d = c - prev_dc;
                const int cat = bit_length(abs(d));
                const uint32_t e = dc_lut[cat];
                sink(e >> 8, (int)(e & 255));
                if (cat) sink((uint32_t)(d < 0 ? d - 1 : d) & ((1u << cat) - 1u), cat);
                continue;
            }
            if (c == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                const uint32_t e = ac_lut[0xF0];
                sink(e >> 8, (int)(e & 255));
                run -= 16;
            }
            const int size = bit_length(abs(c));
            const uint32_t e = ac_lut[(run << 4) | size];
            sink(e >> 8, (int)(e & 255));
            sink((uint32_t)(c < 0 ? c - 1 : c) & ((1u << size) - 1u), size);
            run = 0;
        }
    }
    if (run) {
        const uint32_t e = ac_lut[0];
        sink(e >> 8, (int)(e & 255));
    }
}

// block n of the scan: its Huffman table and the block that holds the DC predictor (-1: the predictor is 0)
__device__ __forceinline__ void block_kind(int64_t n, bool color, int& table, int64_t& prev) {
    if (!color) {
        table = 0;
        prev = n - 1;
        return;
    }
    const int k = (int)(n % 6);
    table = k < 4 ? 0 : 1;
    prev = k == 0 ? n - 3 : (k < 4 ? n - 1 : n - 6);      // Y00 follows the last MCU's Y11; Cb and Cr their own
}

__device__ __forceinline__ void load_luts(uint32_t* dc, uint32_t* ac) {
    for (int i = threadIdx.x; i < 32; i += blockDim.x) dc[i] = TABLES.dc[i >> 4][i & 15];
    for (int i = threadIdx.x; i < 512; i += blockDim.x) ac[i] = TABLES.ac[i >> 8][i & 255];
}

// What the kernels of the options need beyond the defaults' arguments.  The EX = false instantiations are the default file's: they
// get an empty one and never read it.
struct ScanEx {
    int per, ny, ri;               // blocks per MCU, the Y blocks among them, MCUs per restart interval (0: none)
    const uint32_t* luts;          // [LUT_WORDS] built on the device, or null: the compile-time tables
    const uint64_t* ivend;         // [nint] bits of the scan up to each interval's end
    const uint64_t* ivb;           // [nint] the unstuffed byte each interval starts at
    int64_t nint;
    const uint64_t* header_dev;    // the header's length when only the device knows it, or null
};

// block_kind for any MCU shape, with the predictors back at 0 in the first MCU of a restart interval
__device__ __forceinline__ void block_kind_ex(int64_t n, const ScanEx& x, int& table, int64_t& prev) {
    const int64_t mcu = n / x.per;
    const int k = (int)(n - mcu * x.per);
    table = k < x.ny ? 0 : 1;
    prev = k == 0 ? n - (x.per - x.ny + 1) : (k < x.ny ? n - 1 : n - x.per);
    if (x.ri && (k == 0 || k >= x.ny) && mcu % x.ri == 0) prev = -1;
}

__device__ __forceinline__ void load_luts_ex(uint32_t* dc, uint32_t* ac, const uint32_t* luts) {
    if (!luts) return load_luts(dc, ac);
    for (int i = threadIdx.x; i < 32; i += blockDim.x) dc[i] = luts[i];
    for (int i = threadIdx.x; i < 512; i += blockDim.x) ac[i] = luts[32 + i];
}

// code_block's walk with the symbols counted instead of coded: h[0 .. 256) DC categories, h[256 .. 512) AC symbols (LDS)
__device__ __forceinline__ void count_block(const int16_t* coef, int prev_dc, uint32_t* h) {
    const uint4* p = reinterpret_cast<const uint4*>(coef);
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 v = p[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (int)(int16_t)(w[j >> 1] >> ((j & 1) * 16));
            if (g == 0 && j == 0) {
                atomicAdd(h + bit_length(abs(c - prev_dc)), 1u);
                continue;
            }
            if (c == 0) {
                ++run;
                continue;
            }
            if (run > 15) {
                atomicAdd(h + 256 + 0xF0, (uint32_t)(run >> 4));
                run &= 15;
            }
            atomicAdd(h + 256 + ((run << 4) | bit_length(abs(c))), 1u);
            run = 0;
        }
    }
    if (run) atomicAdd(h + 256, 1u);
}

// optimize, pass 1: the four histograms, private to the workgroup in LDS (at most 256 x 64 per bin), merged into 64-bit bins (one
// symbol of a 65535 x 65535 frame can pass 2^32).  hist is zero on entry.
__global__ __launch_bounds__(BLOCKS_PER_GROUP) void jpeg_histogram(const int16_t* coef, int64_t nblocks, const ScanEx x, uint64_t* hist) {
    __shared__ uint32_t h[4 * 256];
    for (int i = threadIdx.x; i < 4 * 256; i += BLOCKS_PER_GROUP) h[i] = 0;
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * BLOCKS_PER_GROUP + threadIdx.x;
    if (n < nblocks) {
        int table;
        int64_t prev;
        block_kind_ex(n, x, table, prev);
        count_block(coef + n * 64, prev >= 0 ? (int)coef[prev * 64] : 0, h + table * 512);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * 256; i += BLOCKS_PER_GROUP)
        if (h[i]) atomicAdd(reinterpret_cast<unsigned long long*>(hist) + i, (unsigned long long)h[i]);
}

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return b < a ? b : a; }

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = umin64(v, o);
    }
    return v;
}

struct Tail {
    uint8_t bytes[MAX_TAIL];
};

// optimize, pass 2: libjpeg's jpeg_gen_optimal_table on each histogram, one wavefront per table (DC0 AC0 DC1 AC1; gray: the first
// two).  Lane l holds the symbols l, l + 64, .. l + 256 in registers (256 is the reserved symbol of frequency 1, which keeps the
// code of all 1-bits unused).  A merge step takes the two least frequent symbols -- among equals the larger index, hence the key
// frequency << 9 | 511 - symbol under a minimum -- and lengthens the code of every leaf below either (libjpeg walks its `others`
// chains for that; `root` names the tree a leaf is in, which marks the same leaves).  Then, one lane per table as 257 symbols are
// few: BITS with the lengths beyond 16 moved up pairwise, the reserved code dropped from the longest length; HUFFVAL by length,
// then symbol (each symbol's rank, in parallel); the codes; and the DHT segment behind the header's first `prefix` bytes, followed
// by `tail` (DRI, SOS).  meta[5] = the header's length.  A frame whose unlimited lengths pass 32 stops libjpeg with an error; here
// such lengths count as 32, which keeps every index in range.
__global__ __launch_bounds__(256) void jpeg_build_tables(const uint64_t* hist, int ntables, uint32_t* luts, uint8_t* out, uint64_t out_cap, int prefix,
                                                         const Tail tail, int tail_bytes, uint64_t* meta) {
    __shared__ int cs[4][257];
    __shared__ int bits[4][33];
    __shared__ uint8_t vals[4][256];
    __shared__ int nvals[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool active = w < ntables;
    constexpr uint64_t NONE = ~0ull;
    if (active) {
        uint64_t f[5];
        int size[5], root[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int s = lane + 64 * j;
            f[j] = s < 256 ? hist[w * 256 + s] : (s == 256 ? 1 : 0);
            size[j] = 0;
            root[j] = s;
        }
        for (int step = 0; step < 256; ++step) {
            uint64_t k1 = NONE;
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if (f[j]) k1 = umin64(k1, (f[j] << 9) | (uint64_t)(511 - (lane + 64 * j)));
            k1 = wave_min(k1);
            const int c1 = 511 - (int)(k1 & 511);
            uint64_t k2 = NONE;
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if (f[j] && lane + 64 * j != c1) k2 = umin64(k2, (f[j] << 9) | (uint64_t)(511 - (lane + 64 * j)));
            k2 = wave_min(k2);
            if (k2 == NONE) break;
            const int c2 = 511 - (int)(k2 & 511);
            const uint64_t sum = (k1 >> 9) + (k2 >> 9);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int s = lane + 64 * j;
                if (s == c1) f[j] = sum;
                if (s == c2) f[j] = 0;
                if (root[j] == c1 || root[j] == c2) {
                    ++size[j];
                    root[j] = c1;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (lane + 64 * j <= 256) cs[w][lane + 64 * j] = min(size[j], 32);
    }
    __syncthreads();
    if (active && lane == 0) {
        int* b = bits[w];
        for (int i = 0; i <= 32; ++i) b[i] = 0;
        for (int s = 0; s <= 256; ++s)
            if (cs[w][s]) ++b[cs[w][s]];
        for (int i = 32; i > 16; --i) {
            while (b[i] > 0) {
                int j = i - 2;
                while (j > 0 && b[j] == 0) --j;
                if (j == 0) break;
                b[i] -= 2;
                ++b[i - 1];
                b[j + 1] += 2;
                --b[j];
            }
        }
        int i = 16;
        while (i > 0 && b[i] == 0) --i;
        if (i > 0) --b[i];
        int n = 0;
        for (i = 1; i <= 16; ++i) n += b[i];
        nvals[w] = min(n, 256);
    }
    __syncthreads();
    if (active) {
        for (int s = lane; s < 256; s += 64) {
            const int mine = cs[w][s];
            if (!mine) continue;
            int rank = 0;
            for (int k = 0; k < 256; ++k) {
                const int o = cs[w][k];
                rank += (int)(o && (o < mine || (o == mine && k < s)));
            }
            vals[w][rank] = (uint8_t)s;
        }
    }
    __syncthreads();
    if (active) {
        const int nv = nvals[w];
        if (lane == 0) {
            uint32_t* lut = (w & 1) ? luts + 32 + (w >> 1) * 256 : luts + (w >> 1) * 16;
            const int limit = (w & 1) ? 256 : 16;
            uint32_t code = 0;
            int k = 0;
            for (int length = 1; length <= 16; ++length) {
                for (int i = 0; i < bits[w][length] && k < nv; ++i, ++k, ++code)
                    if (vals[w][k] < limit) lut[vals[w][k]] = (code << 8) | (uint32_t)length;
                code <<= 1;
            }
        }
        uint64_t at = (uint64_t)prefix;
        for (int u = 0; u < w; ++u) at += 21 + nvals[u];
        for (int i = lane; i < 21 + nv; i += 64) {
            const int length = 19 + nv;
            const uint8_t v = i == 0 ? 0xFF : i == 1 ? 0xC4 : i == 2 ? (uint8_t)(length >> 8) : i == 3 ? (uint8_t)length
                            : i == 4 ? (uint8_t)(((w & 1) << 4) | (w >> 1)) : i < 21 ? (uint8_t)bits[w][i - 4] : vals[w][i - 21];
            if (at + i < out_cap) out[at + i] = v;
        }
    }
    if (threadIdx.x < tail_bytes + 1) {
        uint64_t at = (uint64_t)prefix;
        for (int u = 0; u < ntables; ++u) at += 21 + nvals[u];
        if ((int)threadIdx.x < tail_bytes) {
            if (at + threadIdx.x < out_cap) out[at + threadIdx.x] = tail.bytes[threadIdx.x];
        } else {
            meta[5] = at + tail_bytes;
        }
    }
}

template <bool EX>
__global__ __launch_bounds__(BLOCKS_PER_GROUP) void jpeg_lengths(const int16_t* coef, int64_t nblocks, int color, uint32_t* len, uint64_t* chunk, const ScanEx x) {
    __shared__ uint32_t dc[32], ac[512];
    __shared__ uint32_t total;
    if (EX) load_luts_ex(dc, ac, x.luts);
    else load_luts(dc, ac);
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * BLOCKS_PER_GROUP + threadIdx.x;
    if (n < nblocks) {
        int table;
        int64_t prev;
        if (EX) block_kind_ex(n, x, table, prev);
        else block_kind(n, color != 0, table, prev);
        const int prev_dc = prev >= 0 ? (int)coef[prev * 64] : 0;
        uint32_t bits = 0;
        code_block(coef + n * 64, prev_dc, dc + table * 16, ac + table * 256, [&](uint32_t, int l) { bits += (uint32_t)l; });
        len[n] = bits;
        atomicAdd(&total, bits);                           // integers: any order gives the same sum
    }
    __syncthreads();
    if (threadIdx.x == 0) chunk[blockIdx.x] = total;
}

// Exclusive scan of data[0 .. n) in place by one workgroup of 1024; n = *n_dev when n_dev is given.  *total_out = the sum.
__global__ __launch_bounds__(1024) void jpeg_scan64(uint64_t* data, int64_t n_host, const uint64_t* n_dev, uint64_t* total_out) {
    __shared__ uint64_t buf[2][1024];
    const int64_t n = n_dev ? (int64_t)*n_dev : n_host;
    const uint64_t total = codec::group_scan_1024<uint64_t>(n, buf, [&](int64_t i) { return data[i]; }, [&](int64_t i, uint64_t x) { data[i] = x; });
    if (threadIdx.x == 0) *total_out = total;
}

// restart intervals: bits up to the end of each interval (len's inclusive scan at the interval's last block), whether an interval is
// a fraction of a workgroup or spans many.  span = blocks per interval.
__global__ __launch_bounds__(BLOCKS_PER_GROUP) void jpeg_interval_ends(const uint32_t* len, const uint64_t* chunk, int64_t nblocks, int64_t span, uint64_t* ivend) {
    __shared__ uint32_t sc[2][BLOCKS_PER_GROUP];
    const int tid = threadIdx.x;
    const int64_t n = (int64_t)blockIdx.x * BLOCKS_PER_GROUP + tid;
    int cur = 0;
    sc[0][tid] = n < nblocks ? len[n] : 0;
    __syncthreads();
    for (int d = 1; d < BLOCKS_PER_GROUP; d <<= 1) {
        const uint32_t x = sc[cur][tid] + (tid >= d ? sc[cur][tid - d] : 0);
        sc[cur ^ 1][tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    if (n < nblocks && ((n + 1) % span == 0 || n == nblocks - 1)) ivend[n / span] = chunk[blockIdx.x] + sc[cur][tid];
}

// bytes of each interval, rounded up; their exclusive scan (jpeg_scan64) is the byte each interval starts at
__global__ __launch_bounds__(256) void jpeg_interval_bytes(const uint64_t* ivend, int64_t nint, uint64_t* ivb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nint) ivb[i] = (ivend[i] - (i ? ivend[i - 1] : 0) + 7) >> 3;
}

// how many of v[0 .. n) (increasing) are below x
__device__ __forceinline__ int64_t count_below(const uint64_t* v, int64_t n, uint64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// clears the words of the stream that hold total_bits (rounded up to a whole chunk of the stuffing passes, within the capacity)
// BYTES: *total counts bytes (restart intervals, each rounded up), not bits
template <bool BYTES>
__global__ __launch_bounds__(256) void jpeg_zero(uint4* stream, const uint64_t* total_bits, int64_t cap_bytes) {
    int64_t bytes = BYTES ? (int64_t)*total_bits : (int64_t)((*total_bits + 7) >> 3);
    bytes = (bytes + STUFF_CHUNK - 1) / STUFF_CHUNK * STUFF_CHUNK;
    if (bytes > cap_bytes) bytes = cap_bytes;
    const int64_t n = bytes >> 4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) stream[i] = make_uint4(0, 0, 0, 0);
}

struct BitWriter {
    uint32_t* stream;
    int64_t word, words;       // next word, capacity
    uint64_t acc;              // the low `n` bits are pending
    int n;
    bool shared;               // the next word to leave may hold bits of the block before

    __device__ __forceinline__ void put(uint32_t code, int length) {
        acc = (acc << length) | code;
        n += length;
        if (n >= 32) {
            const uint32_t w = (uint32_t)(acc >> (n - 32));
            n -= 32;
            acc &= (1ull << n) - 1ull;
            if (word < words) {
                if (shared) atomicOr(stream + word, __builtin_bswap32(w));
                else stream[word] = __builtin_bswap32(w);
            }
            shared = false;
            ++word;
        }
    }
    __device__ __forceinline__ void finish() {            // the last, partial word: shared with the block after
        if (n > 0 && word < words) atomicOr(stream + word, __builtin_bswap32((uint32_t)(acc << (32 - n))));
    }
};

template <bool EX>
__global__ __launch_bounds__(BLOCKS_PER_GROUP) void jpeg_emit(const int16_t* coef, int64_t nblocks, int color, const uint32_t* len, const uint64_t* chunk,
                                                               uint32_t* stream, int64_t stream_words, uint64_t* meta, const ScanEx x) {
    __shared__ uint32_t dc[32], ac[512];
    __shared__ uint32_t sc[2][BLOCKS_PER_GROUP];
    if (EX) load_luts_ex(dc, ac, x.luts);
    else load_luts(dc, ac);
    const int tid = threadIdx.x;
    const int64_t n = (int64_t)blockIdx.x * BLOCKS_PER_GROUP + tid;
    const uint32_t mine = n < nblocks ? len[n] : 0;
    int cur = 0;
    sc[0][tid] = mine;
    __syncthreads();
    for (int d = 1; d < BLOCKS_PER_GROUP; d <<= 1) {
        const uint32_t x = sc[cur][tid] + (tid >= d ? sc[cur][tid - d] : 0);
        sc[cur ^ 1][tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    if (n >= nblocks) return;
    uint64_t pos = chunk[blockIdx.x] + (uint64_t)(sc[cur][tid] - mine);
    bool last = n == nblocks - 1;                         // of the scan, or of a restart interval: both end on a byte
    int table;
    int64_t prev;
    if (EX) {
        block_kind_ex(n, x, table, prev);
        if (x.ri) {                                       // the interval starts on its byte; within it the blocks follow each other
            const int64_t span = (int64_t)x.ri * x.per, i = n / span;
            pos = 8 * x.ivb[i] + (pos - (i ? x.ivend[i - 1] : 0));
            last = last || (n + 1) % span == 0;
        }
    } else {
        block_kind(n, color != 0, table, prev);
    }
    const int prev_dc = prev >= 0 ? (int)coef[prev * 64] : 0;
    BitWriter bw{stream, (int64_t)(pos >> 5), stream_words, 0, (int)(pos & 31), true};
    code_block(coef + n * 64, prev_dc, dc + table * 16, ac + table * 256, [&](uint32_t c, int l) { bw.put(c, l); });
    if (last) {                                           // pad the last byte with 1-bits
        const uint64_t end = pos + mine;
        const int pad = (int)((8 - (end & 7)) & 7);
        if (pad) bw.put((1u << pad) - 1u, pad);
        if (n == nblocks - 1) {
            const uint64_t bytes = (end + 7) >> 3;
            meta[0] = bytes;
            meta[1] = (bytes + STUFF_CHUNK - 1) / STUFF_CHUNK;
        }
    }
    bw.finish();
}

// ---------------------------------------------------------------------------------------------------------------- byte stuffing
__device__ __forceinline__ int count_ff(uint32_t w) {
    return (int)((w & 255) == 255) + (int)(((w >> 8) & 255) == 255) + (int)(((w >> 16) & 255) == 255) + (int)((w >> 24) == 255);
}

// bytes of the stream past meta[0] are zero (jpeg_zero clears whole chunks), so a chunk is counted without looking at its end
__global__ __launch_bounds__(256) void jpeg_count_ff(const uint4* stream, const uint64_t* meta, uint64_t* ff) {
    __shared__ uint32_t total;
    const int64_t chunks = (int64_t)meta[1];
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        if (threadIdx.x == 0) total = 0;
        __syncthreads();
        const uint4 v = stream[c * (STUFF_CHUNK / 16) + threadIdx.x];
        const int k = count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);
        if (k) atomicAdd(&total, (uint32_t)k);
        __syncthreads();
        if (threadIdx.x == 0) ff[c] = total;
        __syncthreads();
    }
}

// EX: FF Dn (n counting mod 8, not stuffed) goes in front of the byte every restart interval but the first starts at, so a byte's
// place in the file is header + bytes before + FFs before + 2 * boundaries before.  An interval is at least one byte, so its start
// bytes are distinct and a byte of the stream becomes at most four of the file (FF Dn FF 00: an interval may begin with FF, the
// standard luminance DC code of category 11 is 1 1111 1110).  The staging holds four times the chunk, which no chunk can pass.
template <bool EX>
__global__ __launch_bounds__(256) void jpeg_stuff(const uint4* stream, const uint64_t* meta, const uint64_t* ff, uint8_t* out, uint64_t out_cap, int header_bytes,
                                                  const ScanEx x) {
    constexpr int STAGED = (EX ? 4 : 2) * STUFF_CHUNK;
    __shared__ uint32_t sc[2][256];
    __shared__ uint8_t staged[STAGED];
    const int tid = threadIdx.x;
    const int64_t bytes = (int64_t)meta[0], chunks = (int64_t)meta[1];
    const uint64_t header = EX && x.header_dev ? *x.header_dev : (uint64_t)header_bytes;
    const uint64_t* starts = EX && x.ri ? x.ivb + 1 : nullptr;      // of the intervals a marker precedes
    const int64_t nmark = EX && x.ri ? x.nint - 1 : 0;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint4 v = stream[c * (STUFF_CHUNK / 16) + tid];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const int64_t at = c * STUFF_CHUNK + tid * 16;
        const int valid = (int)max((int64_t)0, min((int64_t)16, bytes - at));
        int k = count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);     // bytes past `bytes` are zero
        int64_t mark = 0;                                 // the next marker at or behind this thread's first byte
        if (EX && nmark && valid) {
            mark = count_below(starts, nmark, (uint64_t)at);
            k += 2 * (int)(count_below(starts, nmark, (uint64_t)(at + valid)) - mark);
        }
        int cur = 0;
        sc[0][tid] = (uint32_t)k;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t y = sc[cur][tid] + (tid >= d ? sc[cur][tid - d] : 0);
            sc[cur ^ 1][tid] = y;
            cur ^= 1;
            __syncthreads();
        }
        int o = tid * 16 + (int)sc[cur][tid] - k;
        const int chunk_out = (int)min((int64_t)STUFF_CHUNK, bytes - c * STUFF_CHUNK) + (int)sc[cur][255];
        uint64_t next = EX && nmark && valid && mark < nmark ? starts[mark] : ~0ull;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < valid) {
                if (EX && next == (uint64_t)(at + j)) {
                    staged[o] = 0xFF;
                    staged[o + 1] = (uint8_t)(0xD0 | (mark & 7));
                    o += 2;
                    ++mark;
                    next = mark < nmark ? starts[mark] : ~0ull;
                }
                const uint8_t b = (uint8_t)(w[j >> 2] >> ((j & 3) * 8));
                staged[o] = b;
                if (b == 255) staged[o + 1] = 0;
                o += b == 255 ? 2 : 1;
            }
        }
        __syncthreads();
        uint64_t base = header + (uint64_t)(c * STUFF_CHUNK) + ff[c];
        if (EX && nmark) base += 2 * (uint64_t)count_below(starts, nmark, (uint64_t)(c * STUFF_CHUNK));
        for (int i = tid; i < chunk_out; i += 256)
            if (base + (uint64_t)i < out_cap) out[base + i] = staged[i];
        __syncthreads();
    }
}

__global__ void jpeg_header(const Header h, int n, uint8_t* out, uint64_t out_cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (uint64_t)i < out_cap) out[i] = h.bytes[i];
}

template <bool EX>
__global__ void jpeg_finish(const uint64_t* meta, uint8_t* out, uint64_t out_cap, int header_bytes, uint64_t* out_len, const ScanEx x) {
    uint64_t end = (uint64_t)header_bytes + meta[0] + meta[2];
    if (EX) end = (x.header_dev ? *x.header_dev : (uint64_t)header_bytes) + meta[0] + meta[2] + (x.ri ? 2 * (uint64_t)(x.nint - 1) : 0);
    if (end < out_cap) out[end] = 0xFF;
    if (end + 1 < out_cap) out[end + 1] = 0xD9;
    out_len[0] = end + 2;
    out_len[1] = end + 2 > out_cap ? 1 : 0;
}

}  // namespace

namespace {

TransformArgs transform_args(const Plan& p, const EncodeArgs& a) {
    TransformArgs t{};
    t.src = a.src;
    t.stride = a.src_stride;
    t.H = p.H;
    t.W = p.W;
    t.bgr = a.bgr;
    t.mcus_x = p.mcus_x;
    for (int i = 0; i < 64; ++i) {
        t.q[0][i] = a.q[0][i];
        t.q[1][i] = a.q[1][i];
    }
    t.coef = a.coef;
    return t;
}

// The passes behind the transform.  EX = false is the file cv2.imwrite writes by default (4:2:0 or gray, standard tables, no restart
// interval): the kernels without the options, an empty ScanEx.  EX = true takes the scan's layout from the plan; optimize adds the
// histogram and the table builder in front of lengths (the header's DHTs, DRI and SOS then come from the builder, and its length from
// meta[5]); a restart interval adds the second scan level (interval ends, their bytes, the scan of those) between the chunk scan and zero.
template <bool EX>
hipError_t launch_passes(const Plan& p, const EncodeArgs& a, hipStream_t s) {
    const int color = EX ? 0 : (int)(p.C == 3);              // with EX the layout is x.per / x.ny
    ScanEx x{};
    if (EX) {
        x.per = p.per;
        x.ny = p.ny;
        x.ri = p.ri;
        x.nint = p.nint;
    }
    const unsigned groups = (unsigned)p.nchunks;
    if (p.optimize) {
        hipError_t e = hipMemsetAsync(a.hist, 0, 4 * 256 * sizeof(uint64_t), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(jpeg_histogram, dim3(groups), dim3(BLOCKS_PER_GROUP), 0, s, a.coef, p.nblocks, x, a.hist);
        Tail tail{};
        for (int i = 0; i < a.tail_bytes; ++i) tail.bytes[i] = a.tail[i];
        hipLaunchKernelGGL(jpeg_build_tables, dim3(1), dim3(256), 0, s, a.hist, p.C == 3 ? 4 : 2, a.luts, a.out, a.out_cap, a.header_bytes, tail, a.tail_bytes, a.meta);
        x.luts = a.luts;
        x.header_dev = a.meta + 5;
    }
    hipLaunchKernelGGL(jpeg_lengths<EX>, dim3(groups), dim3(BLOCKS_PER_GROUP), 0, s, a.coef, p.nblocks, color, a.len, a.chunk, x);
    hipLaunchKernelGGL(jpeg_scan64, dim3(1), dim3(1024), 0, s, a.chunk, p.nchunks, (const uint64_t*)nullptr, a.meta + 3);
    const unsigned wide = (unsigned)(p.stuff_chunks < 4096 ? p.stuff_chunks : 4096);
    if (p.ri) {
        hipLaunchKernelGGL(jpeg_interval_ends, dim3(groups), dim3(BLOCKS_PER_GROUP), 0, s, a.len, a.chunk, p.nblocks, (int64_t)p.ri * p.per, a.ivend);
        hipLaunchKernelGGL(jpeg_interval_bytes, dim3((unsigned)((p.nint + 255) / 256)), dim3(256), 0, s, a.ivend, p.nint, a.ivb);
        hipLaunchKernelGGL(jpeg_scan64, dim3(1), dim3(1024), 0, s, a.ivb, p.nint, (const uint64_t*)nullptr, a.meta + 4);
        x.ivend = a.ivend;
        x.ivb = a.ivb;
        hipLaunchKernelGGL(jpeg_zero<true>, dim3(wide), dim3(256), 0, s, reinterpret_cast<uint4*>(a.stream), a.meta + 4, p.stream_bytes);
    } else {
        hipLaunchKernelGGL(jpeg_zero<false>, dim3(wide), dim3(256), 0, s, reinterpret_cast<uint4*>(a.stream), a.meta + 3, p.stream_bytes);
    }
    hipLaunchKernelGGL(jpeg_emit<EX>, dim3(groups), dim3(BLOCKS_PER_GROUP), 0, s, a.coef, p.nblocks, color, a.len, a.chunk, a.stream, p.stream_bytes / 4, a.meta, x);
    hipLaunchKernelGGL(jpeg_count_ff, dim3(wide), dim3(256), 0, s, reinterpret_cast<const uint4*>(a.stream), a.meta, a.ff);
    hipLaunchKernelGGL(jpeg_scan64, dim3(1), dim3(1024), 0, s, a.ff, (int64_t)0, a.meta + 1, a.meta + 2);
    hipLaunchKernelGGL(jpeg_stuff<EX>, dim3(wide), dim3(256), 0, s, reinterpret_cast<const uint4*>(a.stream), a.meta, a.ff, a.out, a.out_cap, a.header_bytes, x);
    hipLaunchKernelGGL(jpeg_finish<EX>, dim3(1), dim3(1), 0, s, a.meta, a.out, a.out_cap, a.header_bytes, a.out_len, x);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_encode(const Plan& p, const EncodeArgs& a, const Header& h, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_header, dim3((a.header_bytes + 255) / 256), dim3(256), 0, s, h, a.header_bytes, a.out, a.out_cap);
    const TransformArgs t = transform_args(p, a);
    // blockIdx.y carries the MCU row: at most 65535 / 8 + 1 rows, within the grid limit
    if (p.C != 3) hipLaunchKernelGGL(jpeg_transform<false>, dim3((p.mcus_x + STRIP_BLOCKS - 1) / STRIP_BLOCKS, p.mcus_y), dim3(TRANSFORM_THREADS), 0, s, t);
    else if (p.sampling == SAMPLING_420) hipLaunchKernelGGL(jpeg_transform<true>, dim3((p.mcus_x + 15) / 16, p.mcus_y), dim3(TRANSFORM_THREADS), 0, s, t);
    else if (p.sampling == SAMPLING_422) hipLaunchKernelGGL(jpeg_transform_row<2>, dim3((p.mcus_x + 23) / 24, p.mcus_y), dim3(TRANSFORM_THREADS), 0, s, t);
    else hipLaunchKernelGGL(jpeg_transform_row<1>, dim3((p.mcus_x + 31) / 32, p.mcus_y), dim3(TRANSFORM_THREADS), 0, s, t);
    const bool defaults = p.sampling == SAMPLING_420 && !p.optimize && !p.ri;
    return defaults ? launch_passes<false>(p, a, s) : launch_passes<true>(p, a, s);
}

}  // namespace jpeg
}  // namespace nesr
