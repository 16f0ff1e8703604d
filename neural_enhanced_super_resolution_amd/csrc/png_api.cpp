// C-ABI entries of the PNG encoder (include/nesr_hip.h): nesr_png_bound, nesr_png_scratch_bytes, nesr_png_head and
// nesr_png_code_lengths (host only) and nesr_png_encode (kernels of png.hip).  The lossless file a caller of the reference keeps:
// standalone/superres_project.py:203-206 always writes .png, nesr/nesr.py:619-625 saves intermediate_iter{n}.png, and
// standalone/direct_esrgan.py:130,169 writes a PNG input (alpha, gray, 16 bit) back as PNG.
#include "codec_host.h"
#include "png_kernels.h"

using namespace nesr;
using namespace nesr::png;
using codec::be32;
using codec::crc32;

namespace {

bool plan(int H, int W, int C, int depth, Plan* p) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3 && C != 4) || (depth != 8 && depth != 16)) return false;
    p->H = H;
    p->W = W;
    p->C = C;
    p->depth = depth;
    p->bpp = C * depth / 8;
    p->row = 1 + (int64_t)W * p->bpp;
    p->N = (int64_t)H * p->row;
    p->nchunks = (p->N + CHUNK - 1) / CHUNK;
    ScratchCarver ws;
    p->off_filt = ws.take((size_t)p->N);
    p->off_slot = ws.take((size_t)p->nchunks * SLOT);
    p->off_size = ws.take((size_t)p->nchunks * 8);
    p->off_offs = ws.take((size_t)p->nchunks * 8);
    p->off_adler = ws.take((size_t)p->nchunks * 8);
    p->off_meta = ws.take(256);
    p->total = ws.total();
    return true;
}

// signature, IHDR, IDAT[78 01]
void write_head(int H, int W, int C, int depth, uint8_t* o) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    for (int i = 0; i < 8; ++i) o[i] = sig[i];
    be32(o + 8, 13);
    o[12] = 'I', o[13] = 'H', o[14] = 'D', o[15] = 'R';
    be32(o + 16, (uint32_t)W);
    be32(o + 20, (uint32_t)H);
    o[24] = (uint8_t)depth;
    o[25] = C == 1 ? 0 : (C == 3 ? 2 : 6);
    o[26] = o[27] = o[28] = 0;
    be32(o + 29, crc32(o + 12, 17));
    be32(o + 33, 2);
    o[37] = 'I', o[38] = 'D', o[39] = 'A', o[40] = 'T';
    o[41] = 0x78, o[42] = 0x01;                        // zlib: deflate, 32 KiB window, no preset dictionary, fastest
    be32(o + 43, crc32(o + 37, 6));
}

int check_shape(const char* who, int H, int W, int C, int depth) {
    const std::string w(who);
    if (H < 1 || W < 1) return set_error(NESR_ERR_ARG, w + ": H and W must be at least 1");
    if (H > 65535 || W > 65535) return set_error(NESR_ERR_ARG, w + ": at most 65535 x 65535 pixels");
    if (C != 1 && C != 3 && C != 4) return set_error(NESR_ERR_ARG, w + ": " + std::to_string(C) + " channels (1, 3 or 4)");
    if (depth != 8 && depth != 16) return set_error(NESR_ERR_ARG, w + ": depth " + std::to_string(depth) + " (8 or 16)");
    return NESR_OK;
}

}  // namespace

size_t nesr_png_bound(int H, int W, int C, int depth) {
    Plan p;
    return plan(H, W, C, depth, &p) ? (size_t)(HEAD_BYTES + TAIL_BYTES + p.N + CHUNK_OVERHEAD * p.nchunks) : 0;
}

size_t nesr_png_scratch_bytes(int H, int W, int C, int depth) {
    Plan p;
    return plan(H, W, C, depth, &p) ? p.total : 0;
}

int nesr_png_head(int H, int W, int C, int depth, uint8_t* buf, int cap, int* n) {
    if (!n) return set_error(NESR_ERR_ARG, "nesr_png_head: null argument");
    const int rc = check_shape("nesr_png_head", H, W, C, depth);
    if (rc != NESR_OK) return rc;
    *n = HEAD_BYTES;
    if (buf && cap >= HEAD_BYTES) write_head(H, W, C, depth, buf);
    return NESR_OK;
}

int nesr_png_code_lengths(const uint32_t* counts, int n, int limit, uint8_t* lengths) {
    if (!counts || !lengths) return set_error(NESR_ERR_ARG, "nesr_png_code_lengths: null argument");
    if (n < 2 || n > NLIT || limit < 1 || limit > 15 || n > (1 << limit))
        return set_error(NESR_ERR_ARG, "nesr_png_code_lengths: 2 <= n <= 286, 1 <= limit <= 15, n <= 2^limit");
    uint64_t sum = 0;
    for (int i = 0; i < n; ++i) sum += counts[i];
    if (sum >> 32) return set_error(NESR_ERR_ARG, "nesr_png_code_lengths: the counts must sum to less than 2^32");
    HuffWork w;
    const int m = sort_used(counts, n, w);
    code_lengths_sorted(counts, m, n, limit, lengths, w);
    return NESR_OK;
}

int nesr_png_encode(int device_id, const void* src_dev, int64_t src_row_bytes, int H, int W, int C, int depth, int order, void* scratch_dev,
                    size_t scratch_bytes, uint8_t* out_dev, size_t out_cap, uint64_t* out_len_dev, void* stream) {
    if (!src_dev || !scratch_dev || !out_dev || !out_len_dev) return set_error(NESR_ERR_ARG, "nesr_png_encode: null argument");
    const char* who = "nesr_png_encode";
    int rc = check_shape(who, H, W, C, depth);
    if (rc == NESR_OK) rc = codec::check_order(who, order);
    if (rc != NESR_OK) return rc;
    Plan p;
    plan(H, W, C, depth, &p);
    rc = codec::check_row_stride(who, src_row_bytes, (int64_t)W * p.bpp);
    if (rc == NESR_OK) rc = codec::check_scratch(who, scratch_dev, scratch_bytes, p.total);
    if (rc == NESR_OK) rc = codec::check_word_alignment(who, "out_len_dev", out_len_dev, 8);
    if (rc != NESR_OK) return rc;
    EncodeArgs a{};
    a.src = static_cast<const uint8_t*>(src_dev);
    a.src_stride = src_row_bytes;
    a.flip = order == NESR_ORDER_BGR;
    uint8_t* s = static_cast<uint8_t*>(scratch_dev);
    a.filt = s + p.off_filt;
    a.slot = s + p.off_slot;
    a.size = reinterpret_cast<uint64_t*>(s + p.off_size);
    a.offs = reinterpret_cast<uint64_t*>(s + p.off_offs);
    a.adler = reinterpret_cast<uint64_t*>(s + p.off_adler);
    a.meta = reinterpret_cast<uint64_t*>(s + p.off_meta);
    a.out = out_dev;
    a.out_cap = out_cap;
    a.out_len = out_len_dev;
    Head h{};
    write_head(H, W, C, depth, h.bytes);
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_encode(p, a, h, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}
