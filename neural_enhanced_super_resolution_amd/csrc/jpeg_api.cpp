// C-ABI entries of the baseline JPEG encoder (include/nesr_hip.h): nesr_jpeg_scratch_bytes, nesr_jpeg_header (host only) and
// nesr_jpeg_encode_u8 (kernels of jpeg.hip).  The file a caller of the reference gets from cv2.imwrite(path.jpg, frame)
// (standalone/direct_esrgan.py:169, nesr/nesr.py:646): quality 95 by default, 4:2:0, baseline, standard Huffman tables.
#include "api_common.h"
#include "jpeg_kernels.h"
#include "jpeg_tables.h"

using namespace nesr;
using namespace nesr::jpeg;

namespace {

bool plan(int H, int W, int C, Plan* p) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3)) return false;
    p->H = H;
    p->W = W;
    p->C = C;
    const int unit = C == 3 ? 16 : 8;
    p->mcus_x = (W + unit - 1) / unit;
    p->mcus_y = (H + unit - 1) / unit;
    p->nblocks = (int64_t)p->mcus_x * p->mcus_y * (C == 3 ? 6 : 1);
    p->nchunks = (p->nblocks + BLOCKS_PER_GROUP - 1) / BLOCKS_PER_GROUP;
    p->stream_bytes = (int64_t)align_up((size_t)p->nblocks * MAX_BLOCK_BYTES + 8, STUFF_CHUNK);
    p->stuff_chunks = p->stream_bytes / STUFF_CHUNK;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += align_up(bytes, 256);
        return o;
    };
    p->off_coef = take((size_t)p->nblocks * 128);
    p->off_len = take((size_t)p->nblocks * 4);
    p->off_chunk = take((size_t)p->nchunks * 8);
    p->off_meta = take(256);
    p->off_stream = take((size_t)p->stream_bytes);
    p->off_ff = take((size_t)p->stuff_chunks * 8);
    p->total = at;
    return true;
}

// jpeg_quality_scaling and jpeg_add_quant_table(force_baseline): natural order
void quant_table(const uint8_t* base, int quality, uint16_t* q) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int v = (base[i] * s + 50) / 100;
        q[i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

struct Writer {
    uint8_t* p;
    int n = 0;
    void u8(int v) { p[n++] = (uint8_t)v; }
    void u16(int v) {
        u8(v >> 8);
        u8(v & 255);
    }
    void raw(const uint8_t* s, int k) {
        for (int i = 0; i < k; ++i) u8(s[i]);
    }
};

void dht(Writer& w, int tc_th, const uint8_t* bits, const uint8_t* vals, int nvals) {
    w.u16(0xFFC4);
    w.u16(19 + nvals);
    w.u8(tc_th);
    w.raw(bits, 16);
    w.raw(vals, nvals);
}

// SOI, JFIF 1.01 APP0 (no unit, density 1:1), DQT per table, SOF0, DHT per table, SOS: as libjpeg writes them
int write_header(int H, int W, int C, const uint16_t q[2][64], uint8_t* out) {
    static const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    Writer w{out};
    w.raw(app0, (int)sizeof(app0));
    for (int t = 0; t < (C == 3 ? 2 : 1); ++t) {
        w.u16(0xFFDB);
        w.u16(67);
        w.u8(t);
        for (int k = 0; k < 64; ++k) w.u8(q[t][ZIGZAG[k]]);
    }
    w.u16(0xFFC0);
    w.u16(8 + 3 * C);
    w.u8(8);
    w.u16(H);
    w.u16(W);
    w.u8(C);
    for (int c = 0; c < C; ++c) {
        w.u8(c + 1);
        w.u8(C == 3 && c == 0 ? 0x22 : 0x11);
        w.u8(c == 0 ? 0 : 1);
    }
    dht(w, 0x00, DC_LUMA_BITS, dc_vals, 12);
    dht(w, 0x10, AC_LUMA_BITS, AC_LUMA_VALS, 162);
    if (C == 3) {
        dht(w, 0x01, DC_CHROMA_BITS, dc_vals, 12);
        dht(w, 0x11, AC_CHROMA_BITS, AC_CHROMA_VALS, 162);
    }
    w.u16(0xFFDA);
    w.u16(6 + 2 * C);
    w.u8(C);
    for (int c = 0; c < C; ++c) {
        w.u8(c + 1);
        w.u8(c == 0 ? 0x00 : 0x11);
    }
    w.u8(0);
    w.u8(63);
    w.u8(0);
    return w.n;
}

int check_shape(const char* who, int H, int W, int C, int quality) {
    const std::string w(who);
    if (H < 1 || W < 1) return set_error(NESR_ERR_ARG, w + ": H and W must be at least 1");
    if (H > 65535 || W > 65535) return set_error(NESR_ERR_ARG, w + ": a JPEG file holds at most 65535 x 65535 pixels");
    if (C != 1 && C != 3) return set_error(NESR_ERR_ARG, w + ": " + std::to_string(C) + " channels (1 or 3)");
    if (quality < 1 || quality > 100) return set_error(NESR_ERR_ARG, w + ": quality " + std::to_string(quality) + " outside 1..100");
    return NESR_OK;
}

}  // namespace

size_t nesr_jpeg_scratch_bytes(int H, int W, int C) {
    Plan p;
    return plan(H, W, C, &p) ? p.total : 0;
}

int nesr_jpeg_header(int H, int W, int C, int quality, uint8_t* buf, int cap, int* n) {
    if (!n) return set_error(NESR_ERR_ARG, "nesr_jpeg_header: null argument");
    const int rc = check_shape("nesr_jpeg_header", H, W, C, quality);
    if (rc != NESR_OK) return rc;
    uint16_t q[2][64];
    quant_table(LUMA_Q, quality, q[0]);
    quant_table(CHROMA_Q, quality, q[1]);
    Header h;
    *n = write_header(H, W, C, q, h.bytes);
    if (buf && cap >= *n)
        for (int i = 0; i < *n; ++i) buf[i] = h.bytes[i];
    return NESR_OK;
}

int nesr_jpeg_encode_u8(int device_id, const uint8_t* src_dev, int64_t src_row_bytes, int H, int W, int C, int order, int quality, void* scratch_dev,
                        size_t scratch_bytes, uint8_t* out_dev, size_t out_cap, uint64_t* out_len_dev, void* stream) {
    if (!src_dev || !scratch_dev || !out_dev || !out_len_dev) return set_error(NESR_ERR_ARG, "nesr_jpeg_encode_u8: null argument");
    const int rc = check_shape("nesr_jpeg_encode_u8", H, W, C, quality);
    if (rc != NESR_OK) return rc;
    if (order != NESR_ORDER_RGB && order != NESR_ORDER_BGR) return set_error(NESR_ERR_ARG, "nesr_jpeg_encode_u8: order must be NESR_ORDER_RGB or NESR_ORDER_BGR");
    if (src_row_bytes < (int64_t)W * C) return set_error(NESR_ERR_ARG, "nesr_jpeg_encode_u8: the row stride is smaller than a row");
    Plan p;
    plan(H, W, C, &p);
    if (scratch_bytes < p.total)
        return set_error(NESR_ERR_ARG, "nesr_jpeg_encode_u8: scratch of " + std::to_string(scratch_bytes) + " bytes, " + std::to_string(p.total) + " needed");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15) return set_error(NESR_ERR_ARG, "nesr_jpeg_encode_u8: the scratch must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(out_len_dev) & 7) return set_error(NESR_ERR_ARG, "nesr_jpeg_encode_u8: out_len_dev must be 8-byte aligned");
    EncodeArgs a{};
    a.src = src_dev;
    a.src_stride = src_row_bytes;
    a.bgr = order == NESR_ORDER_BGR;
    quant_table(LUMA_Q, quality, a.q[0]);
    quant_table(CHROMA_Q, quality, a.q[1]);
    uint8_t* s = static_cast<uint8_t*>(scratch_dev);
    a.coef = reinterpret_cast<int16_t*>(s + p.off_coef);
    a.len = reinterpret_cast<uint32_t*>(s + p.off_len);
    a.chunk = reinterpret_cast<uint64_t*>(s + p.off_chunk);
    a.meta = reinterpret_cast<uint64_t*>(s + p.off_meta);
    a.stream = reinterpret_cast<uint32_t*>(s + p.off_stream);
    a.ff = reinterpret_cast<uint64_t*>(s + p.off_ff);
    a.out = out_dev;
    a.out_cap = out_cap;
    a.out_len = out_len_dev;
    Header h;
    a.header_bytes = write_header(H, W, C, a.q, h.bytes);
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_encode(p, a, h, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}
