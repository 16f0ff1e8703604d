// C-ABI entries for gray, BGRA and 16-bit frames (include/nesr_hip.h): nesr_pack_frame / nesr_unpack_frame (kernels of frame_io.hip,
// no context) and nesr_enhance_frame, RealESRGANer.enhance for one untiled frame on a context: pack, nesr_forward, the alpha channel
// through the network again or through nesr_resize_f32, unpack.  Every argument is checked before a device is touched.
#include "rrdb_ctx.h"

using namespace nesr;

namespace {

#define FR_CALL(expr)                     \
    do {                                  \
        const int rc__ = (expr);          \
        if (rc__ != NESR_OK) return rc__; \
    } while (0)

// what every entry shares: the kind of frame
int check_kind(const std::string& w, int H, int W, int channels, int bits, int max_range, int alpha_mode) {
    if (H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24)) return set_error(NESR_ERR_ARG, w + ": sizes from 1 to 2^24");
    if (channels != 1 && channels != 3 && channels != 4)
        return set_error(NESR_ERR_ARG, w + ": " + std::to_string(channels) + " channels (a frame is gray = 1, BGR = 3 or BGRA = 4)");
    if (bits != 8 && bits != 16) return set_error(NESR_ERR_ARG, w + ": " + std::to_string(bits) + " bits (uint8 = 8 or uint16 = 16)");
    if (max_range != 255 && max_range != 65535) return set_error(NESR_ERR_ARG, w + ": max_range " + std::to_string(max_range) + " (255 or 65535)");
    if (max_range == 65535 && bits == 8) return set_error(NESR_ERR_ARG, w + ": max_range 65535 needs 16 bits");
    if (alpha_mode != NESR_ALPHA_NETWORK && alpha_mode != NESR_ALPHA_LINEAR)
        return set_error(NESR_ERR_ARG, w + ": alpha_mode " + std::to_string(alpha_mode) + " (NESR_ALPHA_NETWORK or NESR_ALPHA_LINEAR)");
    return NESR_OK;
}

int check_rows(const std::string& w, const void* p, int W, int channels, int bits, int64_t row_bytes) {
    const int S = bits / 8;
    if (row_bytes < (int64_t)W * channels * S) return set_error(NESR_ERR_ARG, w + ": a row pitch is smaller than the row");
    if (S > 1 && ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)row_bytes) & 1)) return set_error(NESR_ERR_ARG, w + ": uint16 pointers and pitches must be even");
    return NESR_OK;
}

// network properties of a context: output / input size and the unshuffle factor; false: not a 3-in 3-out network
bool net_of(const nesr_ctx* c, int* scale, int* ufac) {
    if (c->compact) {
        *scale = compact_upscale(c->compact);
        *ufac = 1;
        return true;       // nesr_create_compact takes 3 channels in and out only
    }
    *ufac = c->ufac();
    *scale = 4 / *ufac;
    return c->cin0 == 3 * *ufac * *ufac && c->nout == 3;
}

struct Scratch { size_t x, y, a, ya, total; };
Scratch scratch_layout(int H, int W, int scale, int channels, int alpha_mode) {
    const size_t in = (size_t)H * W * 4, out = in * scale * scale;
    Scratch L;
    L.x = 0;
    L.y = L.x + align_up(3 * in, 256);
    L.a = L.y + align_up(3 * out, 256);
    L.ya = L.a;
    L.total = L.a;
    if (channels == 4) {
        const size_t planes = alpha_mode == NESR_ALPHA_NETWORK ? 3 : 1;
        L.ya = L.a + align_up(planes * in, 256);
        L.total = L.ya + align_up(planes * out, 256);
    }
    return L;
}

int check_enhance(const nesr_ctx* c, int H, int W, int channels, int bits, int max_range, int alpha_mode, int* scale) {
    const std::string w = "nesr_enhance_frame";
    FR_CALL(check_kind(w, H, W, channels, bits, max_range, alpha_mode));
    int u = 1;
    if (!net_of(c, scale, &u)) return set_error(NESR_ERR_ARG, w + " needs a 3-channel-in / 3-channel-out network");
    if (H % u || W % u)
        return set_error(NESR_ERR_ARG, w + ": " + std::to_string(H) + " x " + std::to_string(W) + " is not a multiple of the unshuffle factor " + std::to_string(u) +
                                       " (pad the frame first, as RealESRGANer.pre_process does)");
    if ((long long)H * *scale > (1 << 24) || (long long)W * *scale > (1 << 24)) return set_error(NESR_ERR_ARG, w + ": frame too large");
    return NESR_OK;
}

}  // namespace

extern "C" {

int nesr_pack_frame(int device_id, const void* src_dev, int H, int W, int channels, int bits, int64_t src_row_bytes, int max_range, int through_fp16,
                    float* image_dev, int alpha_mode, float* alpha_dev, void* stream) {
    const std::string w = "nesr_pack_frame";
    if (!src_dev || !image_dev) return set_error(NESR_ERR_ARG, w + ": null argument");
    FR_CALL(check_kind(w, H, W, channels, bits, max_range, alpha_mode));
    FR_CALL(check_rows(w, src_dev, W, channels, bits, src_row_bytes));
    FramePack p{};
    p.src = static_cast<const unsigned char*>(src_dev);
    p.src_pitch = src_row_bytes;
    p.H = H; p.W = W; p.C = channels; p.bytes = bits / 8;
    p.max_range = (float)max_range;
    p.through_fp16 = through_fp16 ? 1 : 0;
    p.image = image_dev;
    p.alpha = channels == 4 ? alpha_dev : nullptr;
    p.alpha_form = alpha_mode == NESR_ALPHA_LINEAR ? FRAME_ALPHA_PLANE : FRAME_ALPHA_RGB;
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_pack_frame(p, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_unpack_frame(int device_id, const float* image_dev, int Ho, int Wo, int64_t image_plane, int64_t image_row, int through_fp16, int alpha_mode,
                      const float* alpha_dev, int64_t alpha_plane, int64_t alpha_row, int channels, int bits, int max_range, void* dst_dev,
                      int64_t dst_row_bytes, void* stream) {
    const std::string w = "nesr_unpack_frame";
    if (!image_dev || !dst_dev || (channels == 4 && !alpha_dev)) return set_error(NESR_ERR_ARG, w + ": null argument");
    FR_CALL(check_kind(w, Ho, Wo, channels, bits, max_range, alpha_mode));
    FR_CALL(check_rows(w, dst_dev, Wo, channels, bits, dst_row_bytes));
    if (image_row < Wo || image_plane < (int64_t)(Ho - 1) * image_row + Wo) return set_error(NESR_ERR_ARG, w + ": an image pitch is smaller than what it spans");
    if (channels == 4 && (alpha_row < Wo || (alpha_mode == NESR_ALPHA_NETWORK && alpha_plane < (int64_t)(Ho - 1) * alpha_row + Wo)))
        return set_error(NESR_ERR_ARG, w + ": an alpha pitch is smaller than what it spans");
    FrameUnpack u{};
    u.image = image_dev;
    u.image_plane = image_plane; u.image_row = image_row;
    u.alpha = channels == 4 ? alpha_dev : nullptr;
    u.alpha_plane = alpha_plane; u.alpha_row = alpha_row;
    u.alpha_form = alpha_mode == NESR_ALPHA_LINEAR ? FRAME_ALPHA_PLANE : FRAME_ALPHA_RGB;
    u.H = Ho; u.W = Wo; u.C = channels; u.bytes = bits / 8;
    u.max_range = (float)max_range;
    u.through_fp16 = through_fp16 ? 1 : 0;
    u.dst = static_cast<unsigned char*>(dst_dev);
    u.dst_pitch = dst_row_bytes;
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_unpack_frame(u, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

size_t nesr_frame_scratch_bytes(const nesr_ctx* c, int H, int W, int channels, int alpha_mode) {
    int scale = 0;
    if (!c || check_enhance(c, H, W, channels, 16, 65535, alpha_mode, &scale) != NESR_OK) return 0;
    return scratch_layout(H, W, scale, channels, alpha_mode).total;
}

int nesr_enhance_frame(nesr_ctx* c, const void* src_dev, int H, int W, int channels, int bits, int max_range, int alpha_mode, int through_fp16,
                       void* scratch_dev, size_t scratch_bytes, void* dst_dev, void* stream) {
    const std::string w = "nesr_enhance_frame";
    if (!c || !src_dev || !scratch_dev || !dst_dev) return set_error(NESR_ERR_ARG, w + ": null argument");
    // the kind of frame first: nothing of the context is read for a frame no context could take
    FR_CALL(check_kind(w, H, W, channels, bits, max_range, alpha_mode));
    FR_CALL(check_rows(w, src_dev, W, channels, bits, (int64_t)W * channels * (bits / 8)));
    int scale = 0;
    FR_CALL(check_enhance(c, H, W, channels, bits, max_range, alpha_mode, &scale));
    const Scratch L = scratch_layout(H, W, scale, channels, alpha_mode);
    if (scratch_bytes < L.total)
        return set_error(NESR_ERR_ARG, w + ": scratch of " + std::to_string(scratch_bytes) + " bytes, nesr_frame_scratch_bytes asks for " + std::to_string(L.total));
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 255) return set_error(NESR_ERR_ARG, w + ": scratch must be 256-byte aligned");
    const int out_bits = max_range == 65535 ? 16 : 8;
    if (out_bits == 16 && (reinterpret_cast<uintptr_t>(dst_dev) & 1)) return set_error(NESR_ERR_ARG, w + ": uint16 pointers and pitches must be even");
    const int device = c->device, Ho = H * scale, Wo = W * scale;
    char* sc = static_cast<char*>(scratch_dev);
    float *x = reinterpret_cast<float*>(sc + L.x), *y = reinterpret_cast<float*>(sc + L.y);
    float *a = reinterpret_cast<float*>(sc + L.a), *ya = reinterpret_cast<float*>(sc + L.ya);
    FR_CALL(nesr_pack_frame(device, src_dev, H, W, channels, bits, (int64_t)W * channels * (bits / 8), max_range, through_fp16, x, alpha_mode,
                            channels == 4 ? a : nullptr, stream));
    FR_CALL(nesr_forward(c, x, 1, 3, H, W, y, stream));
    if (channels == 4) {
        if (alpha_mode == NESR_ALPHA_NETWORK) FR_CALL(nesr_forward(c, a, 1, 3, H, W, ya, stream));
        else FR_CALL(nesr_resize_f32(device, a, H, W, 1, (int64_t)W * 4, ya, Ho, Wo, (int64_t)Wo * 4, NESR_INTER_LINEAR, stream));
    }
    return nesr_unpack_frame(device, y, Ho, Wo, (int64_t)Ho * Wo, Wo, through_fp16, alpha_mode, channels == 4 ? ya : nullptr, (int64_t)Ho * Wo, Wo, channels,
                             out_bits, max_range, dst_dev, (int64_t)Wo * channels * (out_bits / 8), stream);
}

}  // extern "C"
