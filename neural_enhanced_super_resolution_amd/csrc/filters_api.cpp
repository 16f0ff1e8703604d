// C-ABI entries of the pipeline's filters (include/nesr_hip.h): nesr_lab_u8, nesr_gaussian_u8, nesr_postprocess_u8,
// nesr_segment_enhance_u8, nesr_ensemble_u8 (kernels of filters.hip), nesr_preprocess_u8 (those and the NL-means / CLAHE kernels of imgproc.hip as one stream-ordered sequence), and the
// host-side tables the reference's OpenCV calls build internally (nesr_gaussian_taps, nesr_nl_means_weights).  The tables restate
// imgproc.gaussian_kernel_u8 and imgproc.nl_means_weights in the same double operations (tests/test_filters_host.py compares them).
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>

#include "api_common.h"
#include "nesr_kernels.h"

#pragma clang fp contract(off)      // the host tables are Python's double arithmetic, operation by operation

using namespace nesr;

namespace {

#define FT_CALL(expr)                     \
    do {                                  \
        const int rc__ = (expr);          \
        if (rc__ != NESR_OK) return rc__; \
    } while (0)

constexpr int CLAHE_GRID = 8;
constexpr size_t CLAHE_LUT_BYTES = (size_t)CLAHE_GRID * CLAHE_GRID * 256 * sizeof(float);

// imgproc.gaussian_kernel_u8
int gaussian_taps(double sigma, int ksize, std::vector<int>& q, const char* who) {
    if (!std::isfinite(sigma)) return set_error(NESR_ERR_ARG, std::string(who) + ": sigma must be finite");
    if (ksize <= 0) {
        const double k = std::nearbyint(sigma * 6 + 1);          // Python's round(): half to even
        if (!(k < 2.0 * GAUSS_MAX_RADIUS + 2)) return set_error(NESR_ERR_ARG, std::string(who) + ": sigma too large (at most 31 taps)");
        if (!(k >= 0.0)) return set_error(NESR_ERR_ARG, std::string(who) + ": sigma too negative (no kernel of at least one tap)");
        ksize = (int)k | 1;
    }
    if (ksize % 2 == 0) return set_error(NESR_ERR_ARG, std::string(who) + ": ksize must be odd");
    if (ksize > 2 * GAUSS_MAX_RADIUS + 1) return set_error(NESR_ERR_ARG, std::string(who) + ": ksize must be at most 31");
    const int r = ksize / 2;
    static const double small[4][7] = {{1.0},
                                       {0.25, 0.5, 0.25},
                                       {0.0625, 0.25, 0.375, 0.25, 0.0625},
                                       {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125}};
    std::vector<double> k(ksize);
    if (sigma <= 0 && ksize <= 7) {                               // OpenCV's tabulated small kernels
        for (int i = 0; i < ksize; ++i) k[i] = small[r][i];
    } else {
        if (sigma <= 0) sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8;
        const double den = 2.0 * sigma * sigma;
        double sum = 0;
        for (int i = 0; i < ksize; ++i) {
            const double x = (double)(i - r);
            k[i] = std::exp(-(x * x) / den);
            sum += k[i];
        }
        for (int i = 0; i < ksize; ++i) k[i] = k[i] / sum;
    }
    q.assign(ksize, 0);
    int total = 0;
    for (int i = 0; i < ksize; ++i) {
        q[i] = (int)std::nearbyint(k[i] * 256.0);
        total += q[i];
    }
    q[r] += 256 - total;
    return NESR_OK;
}

// imgproc.nl_means_weights
int nl_means_weights(int C, double h, int tmpl, int search, std::vector<int>* table, int* nbins, int* shift) {
    if (C < 1 || C > 3) return set_error(NESR_ERR_ARG, "nesr_nl_means_weights: 1..3 channels");
    if (!(h > 0) || !std::isfinite(h)) return set_error(NESR_ERR_ARG, "nesr_nl_means_weights: h must be positive and finite");
    if (tmpl < 1 || tmpl > 35 || search < 1 || search > 255) return set_error(NESR_ERR_ARG, "nesr_nl_means_weights: template 1..35, search 1..255");
    const int tsq = tmpl * tmpl;
    int s = 0;
    while ((1 << s) < tsq) ++s;
    const double mult = (double)(1 << s) / tsq;                    // almost_dist -> actual dist
    const long long M = 2147483647ll / ((long long)search * search * 255);
    const long long n = (((long long)255 * 255 * C * tsq) >> s) + 1;
    *nbins = (int)n;
    *shift = s;
    if (!table) return NESR_OK;
    table->resize((size_t)n);
    const double den = h * h * C, floor_w = 0.001 * (double)M;
    for (long long i = 0; i < n; ++i) {
        const double d = (double)i * mult;
        const double w = std::nearbyint((double)M * std::exp(-d / den));
        (*table)[(size_t)i] = w < floor_w ? 0 : (int)w;
    }
    return NESR_OK;
}

// NL-means weight tables on the device, per (device, channels, h): built and uploaded by the first nesr_preprocess_u8 that needs them
std::mutex g_wmu;
std::map<std::tuple<int, int, double>, std::pair<int*, int>> g_weights;

int device_weights(int device, int C, double h, const int** dev, int* nbins) {
    std::lock_guard<std::mutex> lock(g_wmu);
    const auto key = std::make_tuple(device, C, h);
    auto it = g_weights.find(key);
    if (it == g_weights.end()) {
        std::vector<int> t;
        int n = 0, shift = 0;
        FT_CALL(nl_means_weights(C, h, 7, 21, &t, &n, &shift));
        int nz = 0;
        while (nz < n && t[nz] != 0) ++nz;                             // the weights fall monotonically to 0: a short table is enough
        const int len = nz + 1 < n ? nz + 1 : n;
        int* d = nullptr;
        NESR_TRY(hipMalloc(&d, (size_t)len * sizeof(int)));
        const hipError_t e = hipMemcpy(d, t.data(), (size_t)len * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return set_error(NESR_ERR_HIP, std::string("uploading the NL-means weights: ") + hipGetErrorString(e));
        }
        it = g_weights.emplace(key, std::make_pair(d, len)).first;
    }
    *dev = it->second.first;
    *nbins = it->second.second;
    return NESR_OK;
}

// src / dst: HWC (one pointer, step 3) or planar (three planes, step 1)
LabArgs lab_args(const uint8_t* s0, const uint8_t* s1, const uint8_t* s2, int src_step, uint8_t* d0, uint8_t* d1, uint8_t* d2, int dst_step,
                 size_t n, int mode0, int mode1) {
    LabArgs a{};
    a.src[0] = s0; a.src[1] = s1; a.src[2] = s2;
    a.dst[0] = d0; a.dst[1] = d1; a.dst[2] = d2;
    a.n = n; a.src_step = src_step; a.dst_step = dst_step; a.mode0 = mode0; a.mode1 = mode1;
    return a;
}
LabArgs lab_hwc_to_planes(const uint8_t* hwc, uint8_t* p, size_t n, int mode) { return lab_args(hwc, hwc + 1, hwc + 2, 3, p, p + n, p + 2 * n, 1, n, mode, -1); }

}  // namespace

int nesr_lab_u8(int device_id, const uint8_t* src_dev, int H, int W, int mode, uint8_t* dst_dev, void* stream) {
    if (!src_dev || !dst_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (H < 1 || W < 1) return set_error(NESR_ERR_ARG, "nesr_lab_u8: H and W must be at least 1");
    if (mode & ~(NESR_LAB_FROM_LAB | NESR_LAB_LINEAR | NESR_LAB_FIRST_IS_BLUE | NESR_LAB_PLANAR))
        return set_error(NESR_ERR_ARG, "nesr_lab_u8: mode must be a combination of NESR_LAB_* bits");
    const bool planar = mode & NESR_LAB_PLANAR;
    if (planar && src_dev == dst_dev) return set_error(NESR_ERR_ARG, "nesr_lab_u8: the planar form cannot run in place");
    const size_t n = (size_t)H * W;
    const int m = mode & ~NESR_LAB_PLANAR;
    const LabArgs a = !planar ? lab_args(src_dev, src_dev + 1, src_dev + 2, 3, dst_dev, dst_dev + 1, dst_dev + 2, 3, n, m, -1)
                      : (mode & NESR_LAB_FROM_LAB) ? lab_args(src_dev, src_dev + n, src_dev + 2 * n, 1, dst_dev, dst_dev + 1, dst_dev + 2, 3, n, m, -1)
                                                   : lab_hwc_to_planes(src_dev, dst_dev, n, m);
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_lab(a, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_gaussian_taps(double sigma, int ksize, int* taps, int cap, int* n) {
    if (!n) return set_error(NESR_ERR_ARG, "null argument");
    std::vector<int> q;
    FT_CALL(gaussian_taps(sigma, ksize, q, "nesr_gaussian_taps"));
    *n = (int)q.size();
    if (taps && cap >= *n)
        for (int i = 0; i < *n; ++i) taps[i] = q[i];
    return NESR_OK;
}

int nesr_gaussian_u8(int device_id, const uint8_t* src_dev, int H, int W, int C, double sigma, int ksize, uint8_t* dst_dev, void* stream) {
    if (!src_dev || !dst_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (H < 1 || W < 1 || (C != 1 && C != 3)) return set_error(NESR_ERR_ARG, "nesr_gaussian_u8: H, W >= 1 and C = 1 or 3");
    if (src_dev == dst_dev) return set_error(NESR_ERR_ARG, "nesr_gaussian_u8: cannot run in place (src == dst)");
    std::vector<int> q;
    FT_CALL(gaussian_taps(sigma, ksize, q, "nesr_gaussian_u8"));
    GaussTaps t{};
    t.r = (int)q.size() / 2;
    for (size_t i = 0; i < q.size(); ++i) t.k[i] = q[i];
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_gaussian(src_dev, H, W, C, t, dst_dev, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_nl_means_weights(int C, double h, int template_size, int search_size, int* table, int cap, int* nbins, int* shift) {
    if (!nbins || !shift) return set_error(NESR_ERR_ARG, "null argument");
    int n = 0, s = 0;
    FT_CALL(nl_means_weights(C, h, template_size, search_size, nullptr, &n, &s));
    *nbins = n;
    *shift = s;
    if (table && cap >= n) {
        std::vector<int> t;
        FT_CALL(nl_means_weights(C, h, template_size, search_size, &t, &n, &s));
        for (int i = 0; i < n; ++i) table[i] = t[i];
    }
    return NESR_OK;
}

size_t nesr_preprocess_scratch_bytes(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return 2 * align_up((size_t)3 * H * W, 256) + CLAHE_LUT_BYTES;
}

int nesr_preprocess_u8(int device_id, const uint8_t* rgb_dev, int H, int W, double denoise_level, void* scratch_dev, size_t scratch_bytes,
                       uint8_t* out_dev, void* stream) {
    if (!rgb_dev || !scratch_dev || !out_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (H < 1 || W < 1) return set_error(NESR_ERR_ARG, "nesr_preprocess_u8: H and W must be at least 1");
    if (!std::isfinite(denoise_level)) return set_error(NESR_ERR_ARG, "nesr_preprocess_u8: denoise_level must be finite");
    const size_t need = nesr_preprocess_scratch_bytes(H, W);
    if (scratch_bytes < need)
        return set_error(NESR_ERR_ARG, "nesr_preprocess_u8: scratch of " + std::to_string(scratch_bytes) + " bytes, " + std::to_string(need) + " needed");
    const size_t n = (size_t)H * W;
    uint8_t* P = static_cast<uint8_t*>(scratch_dev);                // Lab planes [3][H][W]
    uint8_t* Q = P + align_up(3 * n, 256);                                // second set of planes
    float* lut = reinterpret_cast<float*>(Q + align_up(3 * n, 256));     // CLAHE tables
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int lbgr = NESR_LAB_LINEAR | NESR_LAB_FIRST_IS_BLUE;
    if (denoise_level > 0) {                                         // fastNlMeansDenoisingColored(img, None, h, h, 7, 21), h = 10 denoise_level
        const double h = denoise_level * 10;
        const int* wl = nullptr;
        const int* wab = nullptr;
        int nl = 0, nab = 0;
        NESR_TRY(hipSetDevice(device_id));
        FT_CALL(device_weights(device_id, 1, h, &wl, &nl));
        FT_CALL(device_weights(device_id, 2, h, &wab, &nab));
        NESR_TRY(launch_lab(lab_hwc_to_planes(rgb_dev, P, n, lbgr), s));
        FT_CALL(nesr_nl_means_u8(device_id, P, 1, H, W, 7, 21, wl, nl, Q, stream));
        FT_CALL(nesr_nl_means_u8(device_id, P + n, 2, H, W, 7, 21, wab, nab, Q + n, stream));
        NESR_TRY(launch_lab(lab_args(Q, Q + n, Q + 2 * n, 1, P, P + n, P + 2 * n, 1, n, NESR_LAB_FROM_LAB | lbgr, 0), s));   // Lab -> LBGR -> Lab (sRGB)
    } else {
        NESR_TRY(hipSetDevice(device_id));
        NESR_TRY(launch_lab(lab_hwc_to_planes(rgb_dev, P, n, 0), s));
    }
    FT_CALL(nesr_clahe_u8(device_id, P, H, W, 2.0, CLAHE_GRID, CLAHE_GRID, lut, Q, stream));           // CLAHE on L -> Q[0]
    NESR_TRY(launch_lab(lab_args(Q, P + n, P + 2 * n, 1, out_dev, out_dev + 1, out_dev + 2, 3, n, NESR_LAB_FROM_LAB, -1), s));   // (L', a, b) -> RGB
    return NESR_OK;
}

namespace {
// the taps of _postprocess_image's two blurs; the sigma 3 one is also _segment_and_enhance's
int sharpen_taps(SharpenTaps& t, const char* who) {
    std::vector<int> k2, k3;
    FT_CALL(gaussian_taps(2.0, 0, k2, who));
    FT_CALL(gaussian_taps(3.0, 0, k3, who));
    if (k2.size() != 13 || k3.size() != 19) return set_error(NESR_ERR_ARG, std::string(who) + ": unexpected blur sizes");
    for (int i = 0; i < 13; ++i) t.k2[i] = k2[i];
    for (int i = 0; i < 19; ++i) t.k3[i] = k3[i];
    return NESR_OK;
}
}  // namespace

size_t nesr_segment_enhance_scratch_bytes(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return align_up((size_t)H * W, 256);
}

int nesr_segment_enhance_u8(int device_id, const uint8_t* rgb_dev, int H, int W, const uint8_t* mask_dev, int mask_h, int mask_w, void* scratch_dev,
                            size_t scratch_bytes, uint8_t* out_dev, void* stream) {
    if (!rgb_dev || !mask_dev || !scratch_dev || !out_dev) return set_error(NESR_ERR_ARG, "nesr_segment_enhance_u8: null argument");
    if (H < 1 || W < 1 || mask_h < 1 || mask_w < 1) return set_error(NESR_ERR_ARG, "nesr_segment_enhance_u8: H, W, mask_h and mask_w must be at least 1");
    if (rgb_dev == out_dev) return set_error(NESR_ERR_ARG, "nesr_segment_enhance_u8: cannot run in place (rgb == out)");
    const size_t need = nesr_segment_enhance_scratch_bytes(H, W);
    if (scratch_bytes < need)
        return set_error(NESR_ERR_ARG, "nesr_segment_enhance_u8: scratch of " + std::to_string(scratch_bytes) + " bytes, " + std::to_string(need) + " needed");
    SharpenTaps t{};
    FT_CALL(sharpen_taps(t, "nesr_segment_enhance_u8"));
    const uint8_t* mask = mask_dev;
    if (mask_h != H || mask_w != W) {          // cv2.resize(object_mask, (w, h)): the default interpolation, INTER_LINEAR
        uint8_t* m = static_cast<uint8_t*>(scratch_dev);
        if (m == mask_dev) return set_error(NESR_ERR_ARG, "nesr_segment_enhance_u8: the mask cannot be the scratch");
        FT_CALL(nesr_resize_cv_u8(device_id, mask_dev, mask_h, mask_w, 1, mask_w, m, H, W, W, NESR_INTER_LINEAR, stream));
        mask = m;
    }
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_segment_sharpen(rgb_dev, H, W, t, mask, out_dev, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

int nesr_ensemble_u8(int device_id, const uint8_t* const* images_dev, int n, int H, int W, int C, uint8_t* out_dev, void* stream) {
    if (!images_dev || !out_dev) return set_error(NESR_ERR_ARG, "nesr_ensemble_u8: null argument");
    if (n < 1 || n > ENSEMBLE_MAX) return set_error(NESR_ERR_ARG, "nesr_ensemble_u8: " + std::to_string(n) + " images (1 to 8)");
    if (H < 1 || W < 1 || C < 1) return set_error(NESR_ERR_ARG, "nesr_ensemble_u8: H, W and C must be at least 1");
    EnsembleArgs a{};
    for (int k = 0; k < n; ++k) {
        if (!images_dev[k]) return set_error(NESR_ERR_ARG, "nesr_ensemble_u8: null image");
        a.img[k] = images_dev[k];
    }
    a.out = out_dev;
    a.total = (size_t)H * W * C;
    a.n = n;
    a.w = (float)(1.0 / (double)n);            // numpy 1.x: the float64 weight takes the array's float32 (value-based casting)
    hipStream_t s = static_cast<hipStream_t>(stream);
    NESR_TRY(hipSetDevice(device_id));
    if (n == 1) {                              // _ensemble_results returns the one image as it is
        if (images_dev[0] != out_dev) NESR_TRY(hipMemcpyAsync(out_dev, images_dev[0], a.total, hipMemcpyDeviceToDevice, s));
        return NESR_OK;
    }
    NESR_TRY(launch_ensemble(a, s));
    return NESR_OK;
}

int nesr_postprocess_u8(int device_id, const uint8_t* rgb_dev, int H, int W, int adaptive_sharpening, uint8_t* out_dev, void* stream) {
    if (!rgb_dev || !out_dev) return set_error(NESR_ERR_ARG, "null argument");
    if (H < 1 || W < 1) return set_error(NESR_ERR_ARG, "nesr_postprocess_u8: H and W must be at least 1");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!adaptive_sharpening) {
        if (rgb_dev == out_dev) return NESR_OK;
        NESR_TRY(hipSetDevice(device_id));
        NESR_TRY(hipMemcpyAsync(out_dev, rgb_dev, (size_t)H * W * 3, hipMemcpyDeviceToDevice, s));
        return NESR_OK;
    }
    if (rgb_dev == out_dev) return set_error(NESR_ERR_ARG, "nesr_postprocess_u8: cannot sharpen in place (rgb == out)");
    SharpenTaps t{};
    FT_CALL(sharpen_taps(t, "nesr_postprocess_u8"));
    NESR_TRY(hipSetDevice(device_id));
    NESR_TRY(launch_postprocess(rgb_dev, H, W, t, out_dev, s));
    return NESR_OK;
}
