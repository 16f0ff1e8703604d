// C-ABI entries of the PNG decoder (include/nesr_hip.h): nesr_png_parse (host only), nesr_png_decode_scratch_bytes, nesr_png_decode
// and nesr_png_unfilter (kernels of png_decode.hip).  What a caller of the reference gets from cv2.imread(path.png,
// cv2.IMREAD_UNCHANGED) (standalone/direct_esrgan.py:130): gray, colour or colour + alpha, 8 or 16 bit.  tests/png_decode_ref.py is
// the specification of the parser and of the segment plan.
#include "codec_host.h"
#include "png_decode_kernels.h"

using namespace nesr;
using namespace nesr::pngdec;
using codec::be32;
using codec::crc32;

namespace {

int bad(const char* what) { return set_error(NESR_ERR_BADFILE, std::string("nesr_png_parse: ") + what); }

bool is(const uint8_t* p, const char* kind) { return p[0] == (uint8_t)kind[0] && p[1] == (uint8_t)kind[1] && p[2] == (uint8_t)kind[2] && p[3] == (uint8_t)kind[3]; }

// Walks the chunks of file[0 .. n) from `at` = 8 on and calls idat(payload offset, length) for every IDAT, in order.  Every read is
// behind a check against n.  NESR_OK when IEND closes the file.
template <typename F>
int walk(const uint8_t* file, size_t n, F&& idat) {
    size_t at = 8;
    int state = 0;                                       // 0: before the IDATs, 1: inside them, 2: behind them
    bool first = true;
    for (;;) {
        if (n - at < 12) return bad("the file ends before IEND");
        const uint32_t length = be32(file + at);
        const uint8_t* kind = file + at + 4;
        if (length > 0x7FFFFFFFu || (size_t)length > n - at - 12) return bad("a chunk length past the end");
        if (first) {
            first = false;                               // IHDR: checked by the caller before the walk
        } else if (is(kind, "IHDR")) {
            return bad("two IHDR chunks");
        } else if (is(kind, "IDAT")) {
            if (state == 2) return bad("IDAT chunks that are not consecutive");
            state = 1;
            idat(at + 8, (size_t)length);
        } else if (is(kind, "IEND")) {
            if (length != 0 || at + 12 != n) return bad("IEND is not the end of the file");
            return NESR_OK;
        } else {
            if (!(kind[0] & 0x20) && !is(kind, "PLTE")) return bad("an unknown critical chunk");
            state = state ? 2 : 0;
        }
        at += 12 + (size_t)length;
    }
}

bool plan(const nesr_png_info* info, Plan* p) {
    if (info->H < 1 || info->W < 1 || info->H > 65535 || info->W > 65535) return false;
    if ((info->C != 1 && info->C != 3 && info->C != 4) || (info->depth != 8 && info->depth != 16)) return false;
    p->H = info->H;
    p->W = info->W;
    p->C = info->C;
    p->depth = info->depth;
    p->bpp = info->C * info->depth / 8;
    p->row = 1 + (int64_t)info->W * p->bpp;
    p->N = (int64_t)info->H * p->row;
    if (info->stream_bytes != p->N) return false;
    if (info->n_segments < 1) return false;
    p->nseg = info->n_segments;
    p->npieces = (p->N + ADLER_PIECE - 1) / ADLER_PIECE;
    ScratchCarver ws;
    p->off_filt = ws.take((size_t)p->N);
    p->off_carry = ws.take((size_t)info->H * (size_t)(p->row - 1));
    p->off_size = ws.take((size_t)p->nseg * 8);
    p->off_offs = ws.take((size_t)p->nseg * 8);
    p->off_segst = ws.take((size_t)p->nseg * 4);
    p->off_adler = ws.take((size_t)p->npieces * 8);
    p->total = ws.total();
    return true;
}

int check_dst(const char* who, const Plan& p, int64_t dst_row_bytes, int order, const void* scratch, size_t scratch_bytes, size_t need, const uint32_t* status) {
    int rc = codec::check_order(who, order);
    if (rc == NESR_OK) rc = codec::check_row_stride(who, dst_row_bytes, (int64_t)p.W * p.bpp);
    if (rc == NESR_OK) rc = codec::check_scratch(who, scratch, scratch_bytes, need);
    if (rc == NESR_OK) rc = codec::check_word_alignment(who, "status_dev", status, 4);
    return rc;
}

UnfilterArgs unfilter_args(const Plan& p, const uint8_t* filt, uint8_t* carry, void* dst, int64_t dst_row_bytes, int order, uint32_t* status, int gate) {
    UnfilterArgs u{};
    u.filt = filt;
    u.carry = carry;
    u.H = p.H;
    u.W = p.W;
    u.bpp = p.bpp;
    u.bps = p.depth / 8;
    u.C = p.C;
    u.row = p.row;
    u.flip = order == NESR_ORDER_BGR && p.C >= 3;
    u.dst = static_cast<uint8_t*>(dst);
    u.dst_stride = dst_row_bytes;
    u.status = status;
    u.status_gate = gate;
    return u;
}

}  // namespace

int nesr_png_parse(const uint8_t* file, size_t n, nesr_png_info* info, nesr_png_segment* segs, int cap) {
    if (!file || !info || cap < 0 || (cap > 0 && !segs)) return set_error(NESR_ERR_ARG, "nesr_png_parse: null argument");
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    if (n < 8) return bad("no PNG signature");
    for (int i = 0; i < 8; ++i)
        if (file[i] != sig[i]) return bad("no PNG signature");
    if (n - 8 < 12) return bad("the file ends before IEND");
    if (be32(file + 8) > 0x7FFFFFFFu || (size_t)be32(file + 8) > n - 20) return bad("a chunk length past the end");
    if (!is(file + 12, "IHDR") || be32(file + 8) != 13) return bad("the first chunk is not IHDR");
    if (be32(file + 29) != crc32(file + 12, 17)) return bad("IHDR's CRC");
    const uint32_t W = be32(file + 16), H = be32(file + 20);
    const int depth = file[24], ctype = file[25], comp = file[26], flt = file[27], lace = file[28];
    bool legal = false;
    switch (ctype) {
        case 0: legal = depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16; break;
        case 3: legal = depth == 1 || depth == 2 || depth == 4 || depth == 8; break;
        case 2: case 4: case 6: legal = depth == 8 || depth == 16; break;
        default: break;
    }
    if (W == 0 || H == 0 || W > 0x7FFFFFFFu || H > 0x7FFFFFFFu || comp || flt || lace > 1 || !legal) return bad("IHDR's fields");
    if (lace || (ctype != 0 && ctype != 2 && ctype != 6) || depth < 8 || W > 65535 || H > 65535)
        return set_error(NESR_ERR_UNSUPPORTED, "nesr_png_parse: colour type " + std::to_string(ctype) + ", depth " + std::to_string(depth) + ", interlace " +
                                                   std::to_string(lace) + ", " + std::to_string(W) + " x " + std::to_string(H));
    // first walk: the structure, the length of Z (the IDAT payloads joined), its first two and its last four bytes
    uint64_t zlen = 0;
    uint8_t zhead[2] = {0, 0}, ztail[4] = {0, 0, 0, 0};
    int rc = walk(file, n, [&](size_t off, size_t length) {
        for (size_t i = 0; i < length && zlen + i < 2; ++i) zhead[zlen + i] = file[off + i];
        for (size_t i = length < 4 ? 0 : length - 4; i < length; ++i) {
            ztail[0] = ztail[1], ztail[1] = ztail[2], ztail[2] = ztail[3];
            ztail[3] = file[off + i];
        }
        zlen += length;
    });
    if (rc != NESR_OK) return rc;
    if (zlen < 7) return bad("no deflate stream in the IDATs");
    if ((zhead[0] & 15) != 8 || (zhead[0] >> 4) > 7 || (zhead[1] & 0x20) || (zhead[0] * 256 + zhead[1]) % 31) return bad("the zlib header");
    *info = nesr_png_info{};
    info->H = (int32_t)H;
    info->W = (int32_t)W;
    info->C = ctype == 0 ? 1 : (ctype == 2 ? 3 : 4);
    info->depth = depth;
    info->stream_bytes = (int64_t)H * (1 + (int64_t)W * (info->C * depth / 8));
    info->adler = be32(ztail);
    // second walk: the pieces of D = Z[2 : zlen - 4) and the cuts between them
    const uint64_t dend = zlen - 4;
    uint64_t zpos = 0, seg_at = 0;
    int64_t seg_off = -1;
    uint32_t tail = 0;                                   // the last four bytes of D seen so far
    uint64_t tail_n = 0;
    bool spans = false, contiguous = true;
    int64_t count = 0;
    auto emit = [&](uint64_t bytes, bool last) {
        if (count < cap) segs[count] = nesr_png_segment{seg_off, (int64_t)bytes, seg_at == 0 ? 1 : 0, last ? 1 : 0};
        ++count;
        contiguous = contiguous && !spans;
    };
    walk(file, n, [&](size_t off, size_t length) {
        const uint64_t lo = zpos < 2 ? 2 : zpos, hi = zpos + length < dend ? zpos + length : dend;
        if (hi > lo) {
            const size_t poff = off + (size_t)(lo - zpos);
            const uint64_t dpos = lo - 2, plen = hi - lo;
            if (seg_off < 0) seg_off = (int64_t)poff;
            if (dpos > 0) {
                if (lo == zpos && tail_n >= 4 && tail == 0x0000FFFFu) {
                    emit(dpos - seg_at, false);
                    seg_off = (int64_t)poff;
                    seg_at = dpos;
                    spans = false;
                } else if (dpos > seg_at) {
                    spans = true;
                }
            }
            for (uint64_t i = plen < 4 ? 0 : plen - 4; i < plen; ++i) tail = (tail << 8) | file[poff + i];
            tail_n += plen;
        }
        zpos += length;
    });
    emit(zlen - 6 - seg_at, true);
    info->contiguous = contiguous ? 1 : 0;
    if (count > 0x7FFFFFFF) return set_error(NESR_ERR_UNSUPPORTED, "nesr_png_parse: more than 2^31 segments");
    info->n_segments = (int32_t)count;
    if (count > cap) return set_error(NESR_ERR_NOFIT, "nesr_png_parse: " + std::to_string(count) + " segments, the table holds " + std::to_string(cap));
    return NESR_OK;
}

size_t nesr_png_decode_scratch_bytes(const nesr_png_info* info) {
    Plan p;
    return info && plan(info, &p) ? p.total : 0;
}

int nesr_png_decode(int device_id, const uint8_t* file_dev, size_t n, const nesr_png_info* info, const nesr_png_segment* segs_dev, void* dst_dev,
                    int64_t dst_row_bytes, int order, void* scratch_dev, size_t scratch_bytes, uint32_t* status_dev, void* stream) {
    if (!file_dev || !info || !segs_dev || !dst_dev || !scratch_dev || !status_dev) return set_error(NESR_ERR_ARG, "nesr_png_decode: null argument");
    Plan p;
    if (!plan(info, &p)) return set_error(NESR_ERR_ARG, "nesr_png_decode: the info does not describe a supported frame (fill it with nesr_png_parse)");
    if (!info->contiguous) return set_error(NESR_ERR_ARG, "nesr_png_decode: a segment spans an IDAT boundary (inflate on the host, then nesr_png_unfilter)");
    int rc = check_dst("nesr_png_decode", p, dst_row_bytes, order, scratch_dev, scratch_bytes, p.total, status_dev);
    if (rc == NESR_OK) rc = codec::check_word_alignment("nesr_png_decode", "segs_dev", segs_dev, 8);
    if (rc != NESR_OK) return rc;
    uint8_t* s = static_cast<uint8_t*>(scratch_dev);
    InflateArgs a{};
    a.file = file_dev;
    a.n = n;
    a.segs = segs_dev;
    a.nseg = p.nseg;
    a.N = p.N;
    a.size = reinterpret_cast<uint64_t*>(s + p.off_size);
    a.offs = reinterpret_cast<uint64_t*>(s + p.off_offs);
    a.segst = reinterpret_cast<uint32_t*>(s + p.off_segst);
    a.filt = s + p.off_filt;
    a.adler = reinterpret_cast<uint64_t*>(s + p.off_adler);
    a.npieces = p.npieces;
    a.expect_adler = info->adler;
    a.status = status_dev;
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_inflate(a, static_cast<hipStream_t>(stream)));
    NESR_TRY(launch_unfilter(unfilter_args(p, a.filt, s + p.off_carry, dst_dev, dst_row_bytes, order, status_dev, 1), static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_png_unfilter(int device_id, const uint8_t* filtered_dev, int H, int W, int C, int depth, void* dst_dev, int64_t dst_row_bytes, int order,
                      void* scratch_dev, size_t scratch_bytes, uint32_t* status_dev, void* stream) {
    if (!filtered_dev || !dst_dev || !scratch_dev || !status_dev) return set_error(NESR_ERR_ARG, "nesr_png_unfilter: null argument");
    nesr_png_info info{};
    info.H = H;
    info.W = W;
    info.C = C;
    info.depth = depth;
    info.n_segments = 1;
    info.stream_bytes = (C == 1 || C == 3 || C == 4) && (depth == 8 || depth == 16) ? (int64_t)H * (1 + (int64_t)W * (C * depth / 8)) : -1;
    Plan p;
    if (!plan(&info, &p)) return set_error(NESR_ERR_ARG, "nesr_png_unfilter: 1 .. 65535 rows and columns, 1, 3 or 4 channels, depth 8 or 16");
    const size_t need = align_up((size_t)H * (size_t)(p.row - 1), 256);
    const int rc = check_dst("nesr_png_unfilter", p, dst_row_bytes, order, scratch_dev, scratch_bytes, need, status_dev);
    if (rc != NESR_OK) return rc;
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_unfilter(unfilter_args(p, filtered_dev, static_cast<uint8_t*>(scratch_dev), dst_dev, dst_row_bytes, order, status_dev, 0),
                             static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

size_t nesr_png_unfilter_scratch_bytes(int H, int W, int C, int depth) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3 && C != 4) || (depth != 8 && depth != 16)) return 0;
    return align_up((size_t)H * (size_t)W * (size_t)(C * depth / 8), 256);
}
