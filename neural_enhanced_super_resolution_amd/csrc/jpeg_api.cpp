// C-ABI entries of the baseline JPEG encoder (include/nesr_hip.h): nesr_jpeg_scratch_bytes, nesr_jpeg_header (host only) and
// nesr_jpeg_encode_u8 (kernels of jpeg.hip).  The file a caller of the reference gets from cv2.imwrite(path.jpg, frame)
// (standalone/direct_esrgan.py:169, nesr/nesr.py:646): quality 95 by default, 4:2:0, baseline, standard Huffman tables.
// The _ex entries take a nesr_jpeg_opts (sampling, optimize, restart interval: cv2.imwrite's other JPEG flags); the three entries
// without it forward with {quality, NESR_JPEG_420, 0, 0}, which plans the same scratch and runs the same launches as before.
#include "codec_host.h"
#include "jpeg_kernels.h"
#include "jpeg_tables.h"

using namespace nesr;
using namespace nesr::jpeg;

namespace {

const nesr_jpeg_opts DEFAULTS_95 = {95, NESR_JPEG_420, 0, 0};

// the one statement of which options are valid (quality is checked with the shape)
int check_opts(const char* who, const nesr_jpeg_opts* o) {
    const std::string w(who);
    if (!o) return set_error(NESR_ERR_ARG, w + ": null options");
    if (o->sampling != NESR_JPEG_420 && o->sampling != NESR_JPEG_422 && o->sampling != NESR_JPEG_444)
        return set_error(NESR_ERR_ARG, w + ": sampling " + std::to_string(o->sampling) + " (NESR_JPEG_420, NESR_JPEG_422 or NESR_JPEG_444; 4:4:0 and 4:1:1 are not encoded)");
    if (o->restart_interval < 0 || o->restart_interval > 65535)
        return set_error(NESR_ERR_ARG, w + ": restart interval " + std::to_string(o->restart_interval) + " outside 0..65535 MCUs");
    return NESR_OK;
}

// With the default options the regions and the total are what they were before the options existed.
bool plan(int H, int W, int C, const nesr_jpeg_opts& o, Plan* p) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3) || check_opts("nesr_jpeg_scratch_bytes", &o) != NESR_OK) return false;
    *p = Plan{};
    p->H = H;
    p->W = W;
    p->C = C;
    p->sampling = C == 1 ? SAMPLING_420 : (o.sampling == NESR_JPEG_444 ? SAMPLING_444 : o.sampling == NESR_JPEG_422 ? SAMPLING_422 : SAMPLING_420);
    p->optimize = o.optimize != 0;
    p->ri = o.restart_interval;
    const int unit_x = C == 1 || p->sampling == SAMPLING_444 ? 8 : 16;
    const int unit_y = C == 3 && p->sampling == SAMPLING_420 ? 16 : 8;
    p->ny = (unit_x / 8) * (unit_y / 8);
    p->per = C == 1 ? 1 : p->ny + 2;
    p->mcus_x = (W + unit_x - 1) / unit_x;
    p->mcus_y = (H + unit_y - 1) / unit_y;
    const int64_t mcus = (int64_t)p->mcus_x * p->mcus_y;
    p->nint = p->ri ? (mcus + p->ri - 1) / p->ri : 1;
    p->nblocks = mcus * p->per;
    p->nchunks = (p->nblocks + BLOCKS_PER_GROUP - 1) / BLOCKS_PER_GROUP;
    // every restart interval but the last is rounded up to a byte: at most one more byte each (the markers are not in this stream)
    p->stream_bytes = (int64_t)align_up((size_t)p->nblocks * MAX_BLOCK_BYTES + 8 + (p->ri ? (size_t)p->nint : 0), STUFF_CHUNK);
    p->stuff_chunks = p->stream_bytes / STUFF_CHUNK;
    ScratchCarver ws;
    p->off_coef = ws.take((size_t)p->nblocks * 128);
    p->off_len = ws.take((size_t)p->nblocks * 4);
    p->off_chunk = ws.take((size_t)p->nchunks * 8);
    p->off_meta = ws.take(256);
    p->off_stream = ws.take((size_t)p->stream_bytes);
    p->off_ff = ws.take((size_t)p->stuff_chunks * 8);
    p->off_hist = ws.take(p->optimize ? 4 * 256 * 8 : 0);
    p->off_luts = ws.take(p->optimize ? LUT_WORDS * 4 : 0);
    p->off_ivend = ws.take(p->ri ? (size_t)p->nint * 8 : 0);
    p->off_ivb = ws.take(p->ri ? (size_t)p->nint * 8 : 0);
    p->total = ws.total();
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

// DRI (with a restart interval) and SOS: what follows the DHTs
void write_tail(Writer& w, int C, int ri) {
    if (ri) {
        w.u16(0xFFDD);
        w.u16(4);
        w.u16(ri);
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
}

// SOI, JFIF 1.01 APP0 (no unit, density 1:1), DQT per table, SOF0, DHT per table, DRI, SOS: as libjpeg writes them.  tables = false
// stops behind SOF0: the device writes the optimised DHTs and the tail.
int write_header(int H, int W, int C, const uint16_t q[2][64], uint8_t* out, int sampling = SAMPLING_420, int ri = 0, bool tables = true) {
    static const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    const int y_factors = sampling == SAMPLING_444 ? 0x11 : (sampling == SAMPLING_422 ? 0x21 : 0x22);
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
        w.u8(C == 3 && c == 0 ? y_factors : 0x11);
        w.u8(c == 0 ? 0 : 1);
    }
    if (!tables) return w.n;
    dht(w, 0x00, DC_LUMA_BITS, dc_vals, 12);
    dht(w, 0x10, AC_LUMA_BITS, AC_LUMA_VALS, 162);
    if (C == 3) {
        dht(w, 0x01, DC_CHROMA_BITS, dc_vals, 12);
        dht(w, 0x11, AC_CHROMA_BITS, AC_CHROMA_VALS, 162);
    }
    write_tail(w, C, ri);
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

size_t nesr_jpeg_scratch_bytes_ex(int H, int W, int C, const nesr_jpeg_opts* opts) {
    Plan p;
    return opts && plan(H, W, C, *opts, &p) ? p.total : 0;
}

size_t nesr_jpeg_scratch_bytes(int H, int W, int C) { return nesr_jpeg_scratch_bytes_ex(H, W, C, &DEFAULTS_95); }

int nesr_jpeg_header_ex(int H, int W, int C, const nesr_jpeg_opts* opts, uint8_t* buf, int cap, int* n) {
    if (!n) return set_error(NESR_ERR_ARG, "nesr_jpeg_header: null argument");
    int rc = check_opts("nesr_jpeg_header", opts);
    if (rc != NESR_OK) return rc;
    rc = check_shape("nesr_jpeg_header", H, W, C, opts->quality);
    if (rc != NESR_OK) return rc;
    if (opts->optimize) return set_error(NESR_ERR_ARG, "nesr_jpeg_header: with optimize the Huffman tables, and so the header, exist on the device only");
    Plan p;
    plan(H, W, C, *opts, &p);
    uint16_t q[2][64];
    quant_table(LUMA_Q, opts->quality, q[0]);
    quant_table(CHROMA_Q, opts->quality, q[1]);
    Header h;
    *n = write_header(H, W, C, q, h.bytes, p.sampling, p.ri);
    if (buf && cap >= *n)
        for (int i = 0; i < *n; ++i) buf[i] = h.bytes[i];
    return NESR_OK;
}

int nesr_jpeg_header(int H, int W, int C, int quality, uint8_t* buf, int cap, int* n) {
    const nesr_jpeg_opts o = {quality, NESR_JPEG_420, 0, 0};
    return nesr_jpeg_header_ex(H, W, C, &o, buf, cap, n);
}

int nesr_jpeg_encode_ex_u8(int device_id, const uint8_t* src_dev, int64_t src_row_bytes, int H, int W, int C, int order, const nesr_jpeg_opts* opts,
                           void* scratch_dev, size_t scratch_bytes, uint8_t* out_dev, size_t out_cap, uint64_t* out_len_dev, void* stream) {
    if (!src_dev || !scratch_dev || !out_dev || !out_len_dev) return set_error(NESR_ERR_ARG, "nesr_jpeg_encode_u8: null argument");
    const char* who = "nesr_jpeg_encode_u8";
    int rc = check_opts(who, opts);
    if (rc == NESR_OK) rc = check_shape(who, H, W, C, opts->quality);
    if (rc == NESR_OK) rc = codec::check_order(who, order);
    if (rc == NESR_OK) rc = codec::check_row_stride(who, src_row_bytes, (int64_t)W * C);
    if (rc != NESR_OK) return rc;
    Plan p;
    plan(H, W, C, *opts, &p);
    rc = codec::check_scratch(who, scratch_dev, scratch_bytes, p.total);
    if (rc == NESR_OK) rc = codec::check_word_alignment(who, "out_len_dev", out_len_dev, 8);
    if (rc != NESR_OK) return rc;
    EncodeArgs a{};
    a.src = src_dev;
    a.src_stride = src_row_bytes;
    a.bgr = order == NESR_ORDER_BGR;
    quant_table(LUMA_Q, opts->quality, a.q[0]);
    quant_table(CHROMA_Q, opts->quality, a.q[1]);
    uint8_t* s = static_cast<uint8_t*>(scratch_dev);
    a.coef = reinterpret_cast<int16_t*>(s + p.off_coef);
    a.len = reinterpret_cast<uint32_t*>(s + p.off_len);
    a.chunk = reinterpret_cast<uint64_t*>(s + p.off_chunk);
    a.meta = reinterpret_cast<uint64_t*>(s + p.off_meta);
    a.stream = reinterpret_cast<uint32_t*>(s + p.off_stream);
    a.ff = reinterpret_cast<uint64_t*>(s + p.off_ff);
    a.hist = reinterpret_cast<uint64_t*>(s + p.off_hist);
    a.luts = reinterpret_cast<uint32_t*>(s + p.off_luts);
    a.ivend = reinterpret_cast<uint64_t*>(s + p.off_ivend);
    a.ivb = reinterpret_cast<uint64_t*>(s + p.off_ivb);
    a.out = out_dev;
    a.out_cap = out_cap;
    a.out_len = out_len_dev;
    Header h;
    a.header_bytes = write_header(H, W, C, a.q, h.bytes, p.sampling, p.ri, !p.optimize);
    if (p.optimize) {
        Writer tail{a.tail};
        write_tail(tail, C, p.ri);
        a.tail_bytes = tail.n;
    }
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_encode(p, a, h, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_jpeg_encode_u8(int device_id, const uint8_t* src_dev, int64_t src_row_bytes, int H, int W, int C, int order, int quality, void* scratch_dev,
                        size_t scratch_bytes, uint8_t* out_dev, size_t out_cap, uint64_t* out_len_dev, void* stream) {
    const nesr_jpeg_opts o = {quality, NESR_JPEG_420, 0, 0};
    return nesr_jpeg_encode_ex_u8(device_id, src_dev, src_row_bytes, H, W, C, order, &o, scratch_dev, scratch_bytes, out_dev, out_cap, out_len_dev, stream);
}
