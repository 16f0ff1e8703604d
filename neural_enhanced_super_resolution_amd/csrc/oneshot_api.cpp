// C-ABI entries that need no context (include/nesr_hip.h): tile cut / paste, NL-means and CLAHE on device buffers, and the
// single-layer test hooks nesr_conv3x3 / nesr_conv3x3_up, which run one conv of any compute form with scratch of their own.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rrdb_ctx.h"

using namespace nesr;

namespace {
thread_local int t_noted_kernel = CONV_KERNEL_NONE;   // what the launcher running on this thread chose last
thread_local int t_hook_kernel = CONV_KERNEL_NONE;    // ... as of the last single-layer hook call on this thread
}  // namespace

void nesr::note_conv_kernel(int family) { t_noted_kernel = family; }

extern "C" {

int nesr_cut_tiles_u8(int device_id, const uint8_t* frame_hwc_dev, int H, int W, int flip_rgb, int through_fp16, const int* windows, int n, int Hs, int Ws,
                      float* tiles_nchw_dev, void* stream) {
    if (!frame_hwc_dev || !windows || !tiles_nchw_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (n < 1 || n > TILE_IO_MAX || Hs < 1 || Ws < 1) return set_error(NESR_ERR_ARG, "nesr_cut_tiles_u8: 1.." + std::to_string(TILE_IO_MAX) + " tiles per call");
    TileIo t;
    std::memset(&t, 0, sizeof(t));
    for (int i = 0; i < n; ++i) {
        const int y0 = windows[4 * i], x0 = windows[4 * i + 1], h = windows[4 * i + 2], w = windows[4 * i + 3];
        if (y0 < 0 || x0 < 0 || h < 1 || w < 1 || y0 + h > H || x0 + w > W || h > Hs || w > Ws)
            return set_error(NESR_ERR_ARG, "nesr_cut_tiles_u8: window " + std::to_string(i) + " outside the frame or larger than a slot");
        t.desc[8 * i] = y0; t.desc[8 * i + 1] = x0; t.desc[8 * i + 2] = h; t.desc[8 * i + 3] = w;
    }
    t.frame = const_cast<uint8_t*>(frame_hwc_dev); t.frame_w = W; t.tiles = tiles_nchw_dev; t.Hs = Hs; t.Ws = Ws; t.flip = flip_rgb ? 1 : 0;
    t.round = through_fp16 ? 1 : 0;
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_cut_tiles(t, n, Hs, Ws, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_paste_tiles_u8(int device_id, const float* tiles_nchw_dev, int n, int Hs, int Ws, const int64_t* desc, uint8_t* dst_dev, size_t dst_bytes,
                        int flip_rgb, int round_mode, int through_fp16, void* stream) {
    if (!tiles_nchw_dev || !desc || !dst_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (n < 1 || n > TILE_IO_MAX || Hs < 1 || Ws < 1) return set_error(NESR_ERR_ARG, "nesr_paste_tiles_u8: 1.." + std::to_string(TILE_IO_MAX) + " tiles per call");
    TileIo t;
    std::memset(&t, 0, sizeof(t));
    int maxh = 0, maxw = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* d = desc + 6 * i;      // crop y, crop x, h, w, destination offset (bytes), row pitch (bytes)
        if (d[0] < 0 || d[1] < 0 || d[2] < 1 || d[3] < 1 || d[0] + d[2] > Hs || d[1] + d[3] > Ws || d[4] < 0 || d[5] < d[3] * 3 ||
            (uint64_t)d[4] + (uint64_t)(d[2] - 1) * (uint64_t)d[5] + (uint64_t)d[3] * 3 > dst_bytes)
            return set_error(NESR_ERR_ARG, "nesr_paste_tiles_u8: tile " + std::to_string(i) + ": crop outside its slot or destination outside the buffer");
        int* o = t.desc + 8 * i;
        o[0] = (int)d[0]; o[1] = (int)d[1]; o[2] = (int)d[2]; o[3] = (int)d[3]; o[4] = (int)d[5];
        o[5] = (int)(uint32_t)((uint64_t)d[4] & 0xffffffffull); o[6] = (int)(uint32_t)((uint64_t)d[4] >> 32);
        maxh = std::max(maxh, (int)d[2]); maxw = std::max(maxw, (int)d[3]);
    }
    t.frame = dst_dev; t.tiles = const_cast<float*>(tiles_nchw_dev); t.Hs = Hs; t.Ws = Ws; t.flip = flip_rgb ? 1 : 0;
    t.round = (round_mode == NESR_ROUND_NEAREST ? 1 : 0) | (through_fp16 ? 2 : 0);
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_paste_tiles(t, n, maxh, maxw, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_nl_means_u8(int device_id, const uint8_t* planes_dev, int C, int H, int W, int template_size, int search_size, const int* weights_dev, int nbins,
                     uint8_t* out_dev, void* stream) {
    if (!planes_dev || !weights_dev || !out_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (template_size != 7 || search_size != 21) return set_error(NESR_ERR_ARG, "nesr_nl_means_u8: template 7 / search 21 (what nesr/nesr.py:674 passes)");
    if (C < 1 || C > 3 || H < 1 || W < 1 || nbins < 1) return set_error(NESR_ERR_ARG, "nesr_nl_means_u8: 1..3 planes, a non-empty image and table");
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_nl_means(planes_dev, C, H, W, weights_dev, nbins, 6 /* 49 template pixels -> next power of two 64 */, out_dev, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_clahe_u8(int device_id, const uint8_t* gray_dev, int H, int W, double clip_limit, int grid_x, int grid_y, float* lut_dev, uint8_t* out_dev, void* stream) {
    if (!gray_dev || !lut_dev || !out_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (H < 1 || W < 1 || grid_x < 1 || grid_y < 1 || grid_x * grid_y > 4096 || !(clip_limit > 0.0)) return set_error(NESR_ERR_ARG, "nesr_clahe_u8: non-empty image, grid and clip limit");
    // clahe.cpp: the image is used as it is only when BOTH sides divide by the grid; otherwise both are padded
    const int ph = (H % grid_y || W % grid_x) ? grid_y - H % grid_y : 0, pw = (H % grid_y || W % grid_x) ? grid_x - W % grid_x : 0;
    const int th = (H + ph) / grid_y, tw = (W + pw) / grid_x;
    const long long area = (long long)th * tw;
    if (area > (1ll << 30)) return set_error(NESR_ERR_ARG, "nesr_clahe_u8: tile too large");
    int clip = (int)(clip_limit * (double)area / 256.0);
    clip = clip < 1 ? 1 : clip;
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_clahe(gray_dev, H, W, grid_x, grid_y, th, tw, clip, (float)(255.0 / (double)area), 1.0f / (float)th, 1.0f / (float)tw, lut_dev, out_dev,
                         static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_conv3x3(int device_id, int dtype, const void* x_dev, int N, int Cin, int H, int W, const float* w_host,
                 const float* b_host, int Cout, int lrelu, int upsample, void* y_dev, void* stream) {
    // the default of new contexts, read once per process
    static const int mode = [] {
        const char* e = getenv("NESR_UPCONV");
        return !e ? NESR_UPCONV_2X2 : (std::strcmp(e, "3x3") == 0 ? NESR_UPCONV_3X3 : (std::strcmp(e, "2x2") == 0 ? NESR_UPCONV_2X2 : -1));
    }();
    if (mode < 0) {
        t_hook_kernel = CONV_KERNEL_NONE;
        return set_error(NESR_ERR_ARG, "NESR_UPCONV must be 3x3 or 2x2");
    }
    return nesr_conv3x3_up(device_id, dtype, x_dev, N, Cin, H, W, w_host, b_host, Cout, lrelu, upsample, y_dev, stream, mode);
}

int nesr_conv3x3_up(int device_id, int dtype, const void* x_dev, int N, int Cin, int H, int W, const float* w_host,
                    const float* b_host, int Cout, int lrelu, int upsample, void* y_dev, void* stream, int upconv_mode) {
    t_hook_kernel = t_noted_kernel = CONV_KERNEL_NONE;   // a call that fails before its launch reports no kernel
    if (const char* bad = bad_kernel16_override()) return set_error(NESR_ERR_ARG, std::string("NESR_BF16_KERNEL must be small or xl, not '") + bad + "'");
    if (!x_dev || !w_host || !b_host || !y_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout > 64) return set_error(NESR_ERR_ARG, "bad shape (Cout <= 64)");
    const Form* form = form_of(dtype);   // F32_WINOGRAD: the Winograd slab and kernel alone
    if (!form) return set_error(NESR_ERR_ARG, "bad dtype");
    const bool sp = dtype == NESR_DTYPE_F32_SPLIT;
    const bool hf = dtype == NESR_DTYPE_F16;
    if (upconv_mode != NESR_UPCONV_3X3 && upconv_mode != NESR_UPCONV_2X2) return set_error(NESR_ERR_ARG, "bad upconv_mode");
    const bool up2x2 = sp && upsample && upconv_mode == NESR_UPCONV_2X2;   // the folded form exists for the f16-pair form
    const int kind = form->kind;
    if (hf)
        for (size_t i = 0; i < (size_t)Cout * Cin * 9; ++i)
            if (!(std::fabs(w_host[i]) <= 65504.f)) return set_error(NESR_ERR_RANGE, "weight does not fit the f16 form (|w| > 65504 or non-finite)");
    NESR_TRY(hipSetDevice(device_id));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t es = form->esize;
    const int cin_p = round_up(Cin, form->kgroup), cout_p = round_up(Cout, 32);
    const int up = upsample ? 1 : 0;
    const int ho = H << up, wo = W << up;
    std::vector<char> hw(up2x2 ? packed_upconv_elems_f16x2(cin_p, cout_p) * 2 : form->weight_bytes(cin_p, cout_p));
    if (up2x2) {
        std::vector<float> folded((size_t)16 * Cout * Cin);
        fold_upconv_weights(w_host, Cout, Cin, folded.data());
        for (size_t i = 0; i < folded.size(); ++i)
            if (!(std::fabs(folded[i]) <= 65504.f)) return set_error(NESR_ERR_RANGE, "a folded 2x2 tap does not fit the f16-pair form (|w| > 65504 or non-finite)");
        pack_upconv_weights_f16x2(folded.data(), Cout, Cin, cin_p, cout_p, reinterpret_cast<uint16_t*>(hw.data()));
    } else {
        form->pack(w_host, Cout, Cin, cin_p, cout_p, hw.data());
    }
    std::vector<float> hb(cout_p, 0.f);
    std::memcpy(hb.data(), b_host, (size_t)Cout * 4);
    // device scratch of this one call; freed on every return path
    struct Scratch {
        std::vector<void*> ptrs;
        ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
        hipError_t take(void** p, size_t bytes) {
            const hipError_t e = hipMalloc(p, bytes);
            if (e == hipSuccess) ptrs.push_back(*p);
            return e;
        }
    } scratch;
    char *d_w = nullptr, *d_in = nullptr, *d_out = nullptr, *d_zero = nullptr;
    float* d_b = nullptr;
    const size_t in_bytes = (size_t)N * H * W * cin_p * es, out_bytes = (size_t)N * ho * wo * cout_p * es;
    NESR_TRY(scratch.take((void**)&d_w, hw.size()));
    NESR_TRY(scratch.take((void**)&d_b, hb.size() * 4));
    NESR_TRY(scratch.take((void**)&d_in, in_bytes));
    NESR_TRY(scratch.take((void**)&d_out, out_bytes));
    NESR_TRY(scratch.take((void**)&d_zero, 256));
    NESR_TRY(hipMemset(d_zero, 0, 256));
    unsigned* d_status = reinterpret_cast<unsigned*>(d_zero + 128);   // the upper half of the zero page is never a DMA source (>= 16 B needed)
    NESR_TRY(hipMemcpy(d_w, hw.data(), hw.size(), hipMemcpyHostToDevice));
    NESR_TRY(hipMemcpy(d_b, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
    PackArgs p;
    std::memset(&p, 0, sizeof(p));
    const Map mi = make_map(kind, cin_p, (size_t)N * H * W), mo = make_map(kind, cout_p, (size_t)N * ho * wo);
    p.src = x_dev; p.n = N; p.c = Cin; p.hin = H; p.win = W; p.unshuffle = 1; p.dst = d_in; p.dst_map = mi; p.cp = cin_p; p.bf16 = kind;
    p.status = form->ranged ? d_status : nullptr;
    NESR_TRY(launch_pack_input(p, s));
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = d_in; a.in_map = mi; a.in_h = H; a.in_w = W; a.up = up; a.cin = cin_p;
    a.w = d_w; a.bias = d_b; a.coutp = cout_p;
    a.n = N; a.h = ho; a.w_ = wo;
    a.out = d_out; a.out_map = mo; a.out_coff = 0;
    a.lrelu = lrelu ? 1 : 0; a.s1 = a.s2 = 1.f;
    a.zeros = d_zero;
    a.status = form->ranged ? d_status : nullptr;
    NESR_TRY(up2x2 ? launch_upconv2x2_f16x2(a, s) : form->launch(a, s));
    t_hook_kernel = t_noted_kernel;
    NESR_TRY(launch_nhwc_to_nchw(d_out, kind, mo, N, Cout, ho, wo, static_cast<float*>(y_dev), s));
    NESR_TRY(hipStreamSynchronize(s));
    if (hf) {
        unsigned flag = 0;
        NESR_TRY(hipMemcpy(&flag, d_status, 4, hipMemcpyDeviceToHost));
        if (flag) return set_error(NESR_ERR_RANGE, "input or output of the layer was non-finite or exceeded 65504 in magnitude (f16 form)");
    }
    if (sp) {
        unsigned flag = 0;
        NESR_TRY(hipMemcpy(&flag, d_status, 4, hipMemcpyDeviceToHost));
        if (flag) return set_error(NESR_ERR_RANGE, "input or output of the layer was non-finite or exceeded 65504 in magnitude (f16-pair form)");
        for (size_t i = 0; i < (size_t)Cout * Cin * 9; ++i)
            if (!(std::fabs(w_host[i]) <= 65504.f)) return set_error(NESR_ERR_RANGE, "weight does not fit the f16-pair form (|w| > 65504 or non-finite)");
    }
    return NESR_OK;
}

int nesr_debug_last_conv_kernel(void) { return t_hook_kernel; }

}  // extern "C"
