// C-ABI entries of the baseline JPEG decoder (include/nesr_hip.h): nesr_jpeg_parse (host only), nesr_jpeg_decode_scratch_bytes and
// nesr_jpeg_decode_u8 (kernels of jpeg_decode.hip).  What a caller of the reference gets from cv2.imread(path.jpg)
// (nesr/nesr.py:661-666, standalone/direct_esrgan.py:130), without the EXIF rotation: cv2.IMREAD_UNCHANGED's reading.
#include <cstddef>

#include "codec_host.h"
#include "jpeg_decode_kernels.h"
#include "jpeg_tables.h"

using namespace nesr;
using namespace nesr::jpegdec;

namespace {

struct RawHuff {
    bool set = false;
    uint8_t bits[16];
    uint8_t vals[256];
    int nvals = 0;
};

// jdhuff.c jpeg_make_d_derived_tbl: canonical codes, a look-ahead table for the short ones, maxcode / valoff for the rest
void derive(const RawHuff& r, nesr_jpeg_huff* h) {
    for (int i = 0; i < 512; ++i) h->look[i] = 0;
    for (int i = 0; i < 256; ++i) h->vals[i] = i < r.nvals ? r.vals[i] : 0;
    int code = 0, k = 0;
    h->maxcode[0] = -1;
    h->valoff[0] = 0;
    for (int length = 1; length <= 16; ++length) {
        const int count = r.bits[length - 1];
        h->valoff[length] = k - code;
        if (count == 0) {
            h->maxcode[length] = -1;
        } else {
            if (length <= 9)
                for (int i = 0; i < count; ++i) {
                    const int lo = (code + i) << (9 - length);
                    for (int j = 0; j < (1 << (9 - length)); ++j) h->look[lo + j] = (uint16_t)((length << 8) | r.vals[k + i]);
                }
            code += count;
            k += count;
            h->maxcode[length] = code - 1;
        }
        code <<= 1;
    }
    h->maxcode[17] = 0x7FFFFFFF;
}

struct Frame {
    bool set = false;
    int H = 0, W = 0, C = 0;
    int id[4], hs[4], vs[4], tq[4];
};

thread_local int last_rounds = 0, last_launches = 0;     // of this thread's last nesr_jpeg_decode_u8

int bad(const char* what) { return set_error(NESR_ERR_BADFILE, std::string("nesr_jpeg_parse: ") + what); }
int unsupported(const std::string& what) { return set_error(NESR_ERR_UNSUPPORTED, "nesr_jpeg_parse: " + what); }

bool plan(const nesr_jpeg_info* info, Plan* p) {
    if (info->H < 1 || info->W < 1 || info->H > 65535 || info->W > 65535) return false;
    if (info->C != 1 && info->C != 3) return false;
    const bool gray = info->C == 1;
    if (gray ? (info->hs != 1 || info->vs != 1) : !((info->hs == 1 && info->vs == 1) || (info->hs == 2 && (info->vs == 1 || info->vs == 2)))) return false;
    if (info->restart_interval < 0 || info->restart_interval > 65535) return false;
    if (info->scan_offset < 0 || info->scan_bytes < 1 || info->scan_bytes > MAX_SCAN_BYTES) return false;
    p->H = info->H;
    p->W = info->W;
    p->C = info->C;
    p->hs = info->hs;
    p->vs = info->vs;
    p->ri = info->restart_interval;
    p->mcus_x = (info->W + 8 * info->hs - 1) / (8 * info->hs);
    p->mcus_y = (info->H + 8 * info->vs - 1) / (8 * info->vs);
    if (info->mcus_x != p->mcus_x || info->mcus_y != p->mcus_y) return false;
    p->per = gray ? 1 : info->hs * info->vs + 2;
    p->nmcu = (int64_t)p->mcus_x * p->mcus_y;
    p->nblocks = p->nmcu * p->per;
    p->nseg = p->ri ? (p->nmcu + p->ri - 1) / p->ri : 1;
    p->scan_bytes = info->scan_bytes;
    p->nchunks = (p->scan_bytes + UNSTUFF_CHUNK - 1) / UNSTUFF_CHUNK;
    p->stream_words = (int64_t)align_up((size_t)p->scan_bytes + 16, 256) / 4;
    p->nsub = (p->scan_bytes * 8 + SUBSEQ_BITS - 1) / SUBSEQ_BITS;
    p->ngroups = (p->nsub + SUBSEQ_PER_GROUP - 1) / SUBSEQ_PER_GROUP;
    p->dc_groups = (p->nmcu + DC_GROUP - 1) / DC_GROUP;
    p->ypitch = p->mcus_x * info->hs * 8;
    p->yrows = p->mcus_y * info->vs * 8;
    p->cpitch = p->mcus_x * 8;
    p->crows = p->mcus_y * 8;
    ScratchCarver ws;
    p->off_tables = ws.take(6 * sizeof(nesr_jpeg_huff));
    p->off_chunk = ws.take((size_t)p->nchunks * 8);
    p->off_meta = ws.take(256);
    p->off_seg = ws.take((size_t)p->nseg * 4);
    p->off_stream = ws.take((size_t)p->stream_words * 4);
    p->off_rec = ws.take((size_t)p->nsub * 8);
    p->off_cnt = ws.take((size_t)p->nsub * 4);
    p->off_coef = ws.take((size_t)p->nblocks * 128);
    p->off_dc = ws.take((size_t)p->dc_groups * 12);
    p->off_y = ws.take((size_t)p->ypitch * p->yrows);
    p->off_cb = ws.take(gray ? 0 : (size_t)p->cpitch * p->crows);
    p->off_cr = ws.take(gray ? 0 : (size_t)p->cpitch * p->crows);
    p->total = ws.total();
    return true;
}

}  // namespace

int nesr_jpeg_parse(const uint8_t* file, size_t n, nesr_jpeg_info* info) {
    if (!file || !info) return set_error(NESR_ERR_ARG, "nesr_jpeg_parse: null argument");
    if (n < 4 || file[0] != 0xFF || file[1] != 0xD8) return bad("no SOI");
    size_t pos = 2;
    uint16_t qt[4][64];
    bool qt_set[4] = {false, false, false, false};
    RawHuff huff[2][4];
    Frame f;
    int ri = 0, adobe = -1;
    for (;;) {
        if (pos + 2 > n) return bad("the header ends before SOS");
        if (file[pos] != 0xFF) return bad("a byte that is no marker between the segments");
        while (pos + 1 < n && file[pos + 1] == 0xFF) ++pos;              // fill bytes
        if (pos + 2 > n) return bad("the header ends before SOS");
        const int m = file[pos + 1];
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9) return bad("EOI before SOS");
        if (pos + 2 > n) return bad("a segment length past the end");
        const size_t seg_len = ((size_t)file[pos] << 8) | file[pos + 1];
        if (seg_len < 2 || pos + seg_len > n) return bad("a segment length past the end");
        const uint8_t* seg = file + pos + 2;
        const size_t len = seg_len - 2;
        if (m == 0xC0 || m == 0xC1) {
            if (f.set) return bad("two frame headers");
            if (len < 6) return bad("short SOF");
            const int prec = seg[0], C = seg[5];
            if (len < 6 + 3 * (size_t)C) return bad("short SOF");
            if (prec != 8) return unsupported(std::to_string(prec) + "-bit precision");
            if (C != 1 && C != 3) return unsupported(std::to_string(C) + " components");
            f.H = (seg[1] << 8) | seg[2];
            f.W = (seg[3] << 8) | seg[4];
            f.C = C;
            if (f.H == 0 || f.W == 0) return bad("an empty frame");
            for (int i = 0; i < C; ++i) {
                f.id[i] = seg[6 + 3 * i];
                f.hs[i] = seg[7 + 3 * i] >> 4;
                f.vs[i] = seg[7 + 3 * i] & 15;
                f.tq[i] = seg[8 + 3 * i];
            }
            f.set = true;
        } else if (m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF)) {
            return unsupported("SOF" + std::to_string(m - 0xC0) + ": progressive, lossless, hierarchical or arithmetic coding");
        } else if (m == 0xC4) {
            size_t at = 0;
            while (at < len) {
                if (at + 17 > len) return bad("short DHT");
                const int tc = seg[at] >> 4, th = seg[at] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += seg[at + 1 + i];
                if (tc > 1 || th > 3 || cnt > 256 || at + 17 + (size_t)cnt > len) return bad("bad DHT");
                int code = 0;
                for (int length = 1; length <= 16; ++length) {           // the codes of a length must fit that length
                    code += seg[at + length];
                    if (code > (1 << length)) return bad("bad DHT");
                    code <<= 1;
                }
                RawHuff& r = huff[tc][th];
                r.set = true;
                for (int i = 0; i < 16; ++i) r.bits[i] = seg[at + 1 + i];
                r.nvals = cnt;
                for (int i = 0; i < cnt; ++i) r.vals[i] = seg[at + 17 + i];
                at += 17 + (size_t)cnt;
            }
        } else if (m == 0xDB) {
            size_t at = 0;
            while (at < len) {
                const int pq = seg[at] >> 4, tq = seg[at] & 15;
                if (pq == 1) return unsupported("16-bit DQT");
                if (pq != 0 || tq > 3 || at + 65 > len) return bad("bad DQT");
                for (int k = 0; k < 64; ++k) qt[tq][jpeg::ZIGZAG[k]] = seg[at + 1 + k];
                qt_set[tq] = true;
                at += 65;
            }
        } else if (m == 0xDD) {
            if (len < 2) return bad("short DRI");
            ri = (seg[0] << 8) | seg[1];
        } else if (m == 0xEE) {
            if (len >= 12 && seg[0] == 'A' && seg[1] == 'd' && seg[2] == 'o' && seg[3] == 'b' && seg[4] == 'e') adobe = seg[11];
        } else if (m == 0xDA) {
            if (!f.set) return bad("SOS before SOF");
            if (len < 1 || len < 4 + 2 * (size_t)seg[0]) return bad("short SOS");
            const int ns = seg[0];
            if (ns != f.C) return unsupported("more than one scan");
            for (int i = 0; i < ns; ++i)
                if (seg[1 + 2 * i] != f.id[i]) return unsupported("the scan's components are not the frame's in order");
            if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) return unsupported("a spectral selection or successive approximation");
            int hs = 1, vs = 1;
            if (f.C == 3) {
                if (adobe == 0) return unsupported("Adobe transform 0 (RGB)");
                if (f.id[0] == 'R' && f.id[1] == 'G' && f.id[2] == 'B' && adobe < 0) return unsupported("RGB component ids");
                hs = f.hs[0];
                vs = f.vs[0];
                const bool ok = f.hs[1] == 1 && f.vs[1] == 1 && f.hs[2] == 1 && f.vs[2] == 1 && ((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)));
                if (!ok) return unsupported("sampling factors other than 4:4:4, 4:2:2, 4:2:0");
            }
            *info = nesr_jpeg_info{};
            info->H = f.H;
            info->W = f.W;
            info->C = f.C;
            info->hs = hs;
            info->vs = vs;
            info->restart_interval = ri;
            info->mcus_x = (f.W + 8 * hs - 1) / (8 * hs);
            info->mcus_y = (f.H + 8 * vs - 1) / (8 * vs);
            for (int c = 0; c < f.C; ++c) {
                const int td = seg[2 + 2 * c] >> 4, ta = seg[2 + 2 * c] & 15;
                if (f.tq[c] > 3 || td > 3 || ta > 3 || !qt_set[f.tq[c]] || !huff[0][td].set || !huff[1][ta].set) return bad("a table the scan names is missing");
                for (int i = 0; i < 64; ++i) info->q[c][i] = qt[f.tq[c]][i];
                derive(huff[0][td], &info->dc[c]);
                derive(huff[1][ta], &info->ac[c]);
            }
            for (int c = f.C; c < 3; ++c) {                                // gray: the unused slots repeat component 0
                for (int i = 0; i < 64; ++i) info->q[c][i] = info->q[0][i];
                info->dc[c] = info->dc[0];
                info->ac[c] = info->ac[0];
            }
            info->scan_offset = (int64_t)(pos + seg_len);
            const size_t start = pos + seg_len;
            const size_t end = (n >= start + 2 && file[n - 2] == 0xFF && file[n - 1] == 0xD9) ? n - 2 : n;
            info->scan_bytes = (int64_t)(end - start);
            if (info->scan_bytes < 1) return bad("an empty scan");
            if (info->scan_bytes > MAX_SCAN_BYTES) return unsupported("a scan of more than 2^28 bytes");
            return NESR_OK;
        }
        pos += seg_len;
    }
}

size_t nesr_jpeg_decode_scratch_bytes(const nesr_jpeg_info* info) {
    Plan p;
    return info && plan(info, &p) ? p.total : 0;
}

int nesr_jpeg_decode_u8(int device_id, const uint8_t* file_dev, size_t n, const nesr_jpeg_info* info, uint8_t* dst_dev, int64_t dst_row_bytes, int order,
                        void* scratch_dev, size_t scratch_bytes, uint32_t* status_dev, void* stream) {
    if (!file_dev || !info || !dst_dev || !scratch_dev || !status_dev) return set_error(NESR_ERR_ARG, "nesr_jpeg_decode_u8: null argument");
    Plan p;
    if (!plan(info, &p)) return set_error(NESR_ERR_ARG, "nesr_jpeg_decode_u8: the info does not describe a supported frame (fill it with nesr_jpeg_parse)");
    if ((uint64_t)info->scan_offset + (uint64_t)info->scan_bytes > (uint64_t)n) return set_error(NESR_ERR_ARG, "nesr_jpeg_decode_u8: the scan lies outside the file");
    const char* who = "nesr_jpeg_decode_u8";
    int rc = codec::check_order(who, order);
    if (rc == NESR_OK) rc = codec::check_row_stride(who, dst_row_bytes, (int64_t)p.W * p.C);
    if (rc == NESR_OK) rc = codec::check_scratch(who, scratch_dev, scratch_bytes, p.total);
    if (rc == NESR_OK) rc = codec::check_word_alignment(who, "status_dev", status_dev, 4);
    if (rc != NESR_OK) return rc;
    DecodeArgs a{};
    uint8_t* s = static_cast<uint8_t*>(scratch_dev);
    a.scan = file_dev + info->scan_offset;
    a.tables_host = info->dc;                               // dc[3] and ac[3] are adjacent in nesr_jpeg_info
    static_assert(offsetof(nesr_jpeg_info, ac) == offsetof(nesr_jpeg_info, dc) + 3 * sizeof(nesr_jpeg_huff), "dc and ac tables must be adjacent");
    a.tables = reinterpret_cast<nesr_jpeg_huff*>(s + p.off_tables);
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) a.q[c][i] = info->q[c][i];
    a.chunk = reinterpret_cast<uint64_t*>(s + p.off_chunk);
    a.meta = reinterpret_cast<uint32_t*>(s + p.off_meta);
    a.seg = reinterpret_cast<uint32_t*>(s + p.off_seg);
    a.stream = reinterpret_cast<uint32_t*>(s + p.off_stream);
    a.rec = reinterpret_cast<uint64_t*>(s + p.off_rec);
    a.cnt = reinterpret_cast<uint32_t*>(s + p.off_cnt);
    a.coef = reinterpret_cast<int16_t*>(s + p.off_coef);
    a.dc = reinterpret_cast<int32_t*>(s + p.off_dc);
    a.y = s + p.off_y;
    a.cb = s + p.off_cb;
    a.cr = s + p.off_cr;
    a.dst = dst_dev;
    a.dst_stride = dst_row_bytes;
    a.bgr = order == NESR_ORDER_BGR;
    a.status = status_dev;
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_decode(p, a, static_cast<hipStream_t>(stream), &last_rounds, &last_launches));
    return NESR_OK;
}

int nesr_jpeg_decode_last_launches(int* sync_rounds, int* launches) {
    if (!sync_rounds || !launches) return set_error(NESR_ERR_ARG, "nesr_jpeg_decode_last_launches: null argument");
    *sync_rounds = last_rounds;
    *launches = last_launches;
    return NESR_OK;
}
