// C ABI of the banded evaluation (exact multi-GPU mode: one row band of the frame per rank, SURVEY.md section 8(e) mode 2).
// The caller runs the stages of the forward graph (rrdb_forward.cpp) in order and refreshes the apron rows of the feature map each
// stage reads (nesr_band_rows) with its neighbours' band rows in between; banded.py holds that protocol.
#include "rrdb_ctx.h"

using namespace nesr;

namespace {

int band_ready(const nesr_ctx* c) {
    if (!c->band_valid) return set_error(NESR_ERR_STATE, "nesr_band_begin has not run (or a whole-frame forward reused the workspace)");
    return NESR_OK;
}

}  // namespace

extern "C" {

int nesr_band_begin(nesr_ctx* c, const void* x_dev, int C, int H, int W, void* stream) {
    RRDB_ONLY(c);
    if (!c || !x_dev) return set_error(NESR_ERR_ARG, "null argument");
    c->band_valid = false;
    int rc = fw_setup(c, 1, C, H, W, c->band);
    if (rc) return rc;
    if ((rc = fw_first(c, c->band, static_cast<const float*>(x_dev), nullptr, 0, C, H, W, static_cast<hipStream_t>(stream)))) return rc;
    c->band_valid = true;
    return NESR_OK;
}

int nesr_band_rdb(nesr_ctx* c, int index, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = band_ready(c)) return rc;
    if (index < 0 || index >= 3 * c->nb) return set_error(NESR_ERR_ARG, "RDB index out of range");
    NESR_TRY(hipSetDevice(c->device));
    return fw_rdb(c, c->band, index / 3, index % 3, static_cast<hipStream_t>(stream));
}

int nesr_band_rdb_phase(nesr_ctx* c, int index, int phase, int top, int bottom, int edge_rows, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = band_ready(c)) return rc;
    if (index < 0 || index >= 3 * c->nb) return set_error(NESR_ERR_ARG, "RDB index out of range");
    if ((phase != 0 && phase != 1) || top < 0 || bottom < 0 || edge_rows < 0 || top + bottom > c->band.h)
        return set_error(NESR_ERR_ARG, "bad phase / apron / edge rows");
    NESR_TRY(hipSetDevice(c->device));
    return fw_rdb(c, c->band, index / 3, index % 3, static_cast<hipStream_t>(stream), phase, top, bottom, edge_rows);
}

int nesr_band_pack_edges(nesr_ctx* c, int buffer, int top, int bottom, int nrows, void* top_dst, void* bottom_dst, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = band_ready(c)) return rc;
    const int h = c->band.h;
    if (top < 0 || bottom < 0 || nrows < 0 || top + bottom + nrows > h) return set_error(NESR_ERR_ARG, "bad apron / row count");
    int rc = NESR_OK;
    if (top_dst && (rc = nesr_band_rows(c, buffer, top, nrows, top_dst, 0, stream))) return rc;
    if (bottom_dst && (rc = nesr_band_rows(c, buffer, h - bottom - nrows, nrows, bottom_dst, 0, stream))) return rc;
    return NESR_OK;
}

int nesr_band_unpack_aprons(nesr_ctx* c, int buffer, int top, int bottom, int nrows, const void* top_src, const void* bottom_src, void* stream) {
    RRDB_ONLY(c);
    if (!c) return set_error(NESR_ERR_ARG, "null ctx");
    if (int rc = band_ready(c)) return rc;
    const int h = c->band.h;
    if ((top_src && nrows > top) || (bottom_src && nrows > bottom) || nrows < 0) return set_error(NESR_ERR_ARG, "more rows than the apron holds");
    int rc = NESR_OK;
    if (top_src && (rc = nesr_band_rows(c, buffer, top - nrows, nrows, const_cast<void*>(top_src), 1, stream))) return rc;
    if (bottom_src && (rc = nesr_band_rows(c, buffer, h - bottom, nrows, const_cast<void*>(bottom_src), 1, stream))) return rc;
    return NESR_OK;
}

int nesr_band_tail(nesr_ctx* c, void* y_dev, void* stream) {
    RRDB_ONLY(c);
    if (!c || !y_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (int rc = band_ready(c)) return rc;
    NESR_TRY(hipSetDevice(c->device));
    return fw_tail(c, c->band, static_cast<float*>(y_dev), nullptr, 0, 0, static_cast<hipStream_t>(stream));
}

size_t nesr_band_row_bytes(const nesr_ctx* c) {
    if (rrdb_only(c, __func__)) return 0;   // the error is set; a size cannot carry the code
    if (!c || !c->band_valid) return 0;
    return (size_t)c->band.w * c->nf * c->esize();
}

int nesr_band_rows(nesr_ctx* c, int buffer, int row0, int nrows, void* staging_dev, int write, void* stream) {
    RRDB_ONLY(c);
    if (!c || !staging_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (int rc = band_ready(c)) return rc;
    const FwState& F = c->band;
    if (buffer < 0 || buffer > 3 || row0 < 0 || nrows < 0 || row0 + nrows > F.h) return set_error(NESR_ERR_ARG, "bad buffer / row range");
    if (nrows == 0) return NESR_OK;
    NESR_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = buffer < 3 ? F.buf[buffer] : c->ws + F.L.f;
    const Map& m = buffer < 3 ? F.m_t : F.m_f;
    char* stg = static_cast<char*>(staging_dev);
    const int kind = c->kind();
    if (kind == 0) {
        // NHWC f32: channels [0, nf) of every pixel of the rows; the dense-block buffers have ct channels per pixel
        const size_t spitch = (size_t)m.pix * 4, width = (size_t)c->nf * 4, rows = (size_t)nrows * F.w;
        char* src = base + (size_t)row0 * F.w * spitch;
        if (write) NESR_TRY(hipMemcpy2DAsync(src, spitch, stg, width, width, rows, hipMemcpyDeviceToDevice, s));
        else NESR_TRY(hipMemcpy2DAsync(stg, width, src, spitch, width, rows, hipMemcpyDeviceToDevice, s));
        return NESR_OK;
    }
    // channel-blocked: the rows of one 16-channel chunk are one contiguous span; staging = [chunk][rows][w][pixel bytes]
    const size_t pixbytes = (size_t)m.pix * 2, span = (size_t)nrows * F.w * pixbytes;
    for (int ch = 0; ch < c->nf / 16; ++ch) {
        char* src = base + (size_t)ch * (size_t)m.chunk * 2 + (size_t)row0 * F.w * pixbytes;
        char* dst = stg + (size_t)ch * span;
        if (write) NESR_TRY(hipMemcpyAsync(src, dst, span, hipMemcpyDeviceToDevice, s));
        else NESR_TRY(hipMemcpyAsync(dst, src, span, hipMemcpyDeviceToDevice, s));
    }
    return NESR_OK;
}

}  // extern "C"
