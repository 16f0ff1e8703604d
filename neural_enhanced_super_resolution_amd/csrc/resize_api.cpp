// C-ABI entries of cv2.resize (include/nesr_hip.h): nesr_resize_u8 / _u16 / _f32 / nesr_resize_cv_u8 (kernels of resize.hip) and the
// host-side coefficient tables (nesr_resize_taps, nesr_resize_cv_taps).  The tables restate imgproc._axis_taps / _lanczos4_coeffs / linear_resize_f32's axis() and
// oracle/cv2_ref.py's _lanczos_weights in the same double and float operations, in plain C++ (tests/test_resize_host.py compares
// them), so a host without torch can resize.  Device copies of the tables are kept per (device, kind, n_in, n_out).
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>

#include "api_common.h"
#include "nesr_kernels.h"

#pragma clang fp contract(off)      // the host tables are Python's arithmetic, operation by operation

using namespace nesr;

namespace {

#define RS_CALL(expr)                     \
    do {                                  \
        const int rc__ = (expr);          \
        if (rc__ != NESR_OK) return rc__; \
    } while (0)

enum TableKind { LANCZOS_FIXED = 0, LANCZOS_FLOAT = 1, LINEAR = 2, CUBIC_FIXED = 3, LINEAR_FIXED = 4, NEAREST = 5 };

// position d of an axis resized n_in -> n_out: cv2's sampling position (d + 0.5) n_in / n_out - 0.5 in double, cast to float
void axis_position(int n_in, int n_out, int d, int* i0, float* frac) {
    const double scale = (double)n_in / (double)n_out;
    const float pos = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = std::floor(pos);
    *i0 = (int)fl;
    *frac = pos - fl;
}

// cv2 interpolateLanczos4, twice, because the two restatements this project checks against evaluate it in different precisions and
// each form must equal its own bit for bit:
//   lanczos4_coeffs_f64  imgproc._lanczos4_coeffs (the u8 form's 11-bit coefficients): the fraction widened to double first,
//                        angles, sines and quotient in double, rounded to float32 once, float32 sum in order, float32 scale.
//   lanczos4_coeffs_f32  oracle/cv2_ref.py _lanczos_weights (the u16 form's float32 coefficients): the fraction is a numpy float32
//                        and Python's scalars do not widen it, so x + 3, the angle y, y * y and the quotient are float32 (only sin,
//                        cos and the numerator are double); numpy sums the 8 floats pairwise.
const double S45 = 0.70710678118654752440084436210485;
const double CS[8][2] = {{1, 0}, {-S45, -S45}, {0, 1}, {S45, -S45}, {-1, 0}, {S45, S45}, {0, -1}, {-S45, S45}};

bool lanczos4_exact(float frac, float co[8]) {
    if (!(frac < 1.1920929e-07f)) return false;
    for (int i = 0; i < 8; ++i) co[i] = i == 3 ? 1.0f : 0.0f;
    return true;
}

void lanczos4_coeffs_f64(float frac, float co[8]) {
    if (lanczos4_exact(frac, co)) return;
    const double x = (double)frac, q = M_PI * 0.25;
    const double y0 = -(x + 3) * q;
    const double s0 = std::sin(y0), c0 = std::cos(y0);
    float sum = 0.0f;
    for (int i = 0; i < 8; ++i) {
        const double y = -(x + 3 - (double)i) * q;
        co[i] = (float)((CS[i][0] * s0 + CS[i][1] * c0) / (y * y));
        sum = sum + co[i];
    }
    const float inv = 1.0f / sum;
    for (int i = 0; i < 8; ++i) co[i] = co[i] * inv;
}

void lanczos4_coeffs_f32(float frac, float co[8]) {
    if (lanczos4_exact(frac, co)) return;
    const float pi = (float)M_PI, t = frac + 3.0f;
    const float y0 = (-t * pi) * 0.25f;
    const double s0 = std::sin((double)y0), c0 = std::cos((double)y0);
    for (int i = 0; i < 8; ++i) {
        const float y = (-(t - (float)i) * pi) * 0.25f;
        co[i] = (float)(CS[i][0] * s0 + CS[i][1] * c0) / (y * y);
    }
    const float sum = ((co[0] + co[1]) + (co[2] + co[3])) + ((co[4] + co[5]) + (co[6] + co[7]));
    const float inv = 1.0f / sum;
    for (int i = 0; i < 8; ++i) co[i] = co[i] * inv;
}

int fixed11(float c) {           // saturate_cast<short>(c * INTER_RESIZE_COEF_SCALE)
    const float v = std::nearbyint(c * 2048.0f);
    return (int)(v < -32768.f ? -32768.f : (v > 32767.f ? 32767.f : v));
}

// cv2 interpolateCubic (A = -0.75) in float32, operation by operation (imgproc._cubic_coeffs; the fraction is NOT zeroed at the ends)
void cubic_coeffs(float x, float co[4]) {
    const float A = -0.75f;
    co[0] = ((A * (x + 1.0f) - 5.0f * A) * (x + 1.0f) + 8.0f * A) * (x + 1.0f) - 4.0f * A;
    co[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    co[2] = ((A + 2.0f) * (1.0f - x) - (A + 3.0f)) * (1.0f - x) * (1.0f - x) + 1.0f;
    co[3] = 1.0f - co[0] - co[1] - co[2];
}

// INTER_NEAREST: min(floor(d scale), n_in - 1), the scale in double as axis_position takes it
int nearest_index(int n_in, int n_out, int d) {
    const double scale = (double)n_in / (double)n_out;
    const int i = (int)std::floor((double)d * scale);
    return i < n_in - 1 ? i : n_in - 1;
}

// INTER_LINEAR, 8 bit: the clamped first tap and short(rint((1 - f) 2048)), short(rint(f 2048)), f = 0 at the clamped ends
void linear_fixed(int n_in, int n_out, int d, int* i0, int co[2]) {
    float f;
    axis_position(n_in, n_out, d, i0, &f);
    const bool lo = *i0 < 0, hi = *i0 >= n_in - 1;
    if (lo || hi) f = 0.0f;
    *i0 = lo ? 0 : (hi ? n_in - 1 : *i0);
    co[0] = fixed11(1.0f - f);
    co[1] = fixed11(f);
}

// the device image of a table (nesr_kernels.h, ResizeArgs): n_out first indices, then the coefficients
void build_table(TableKind kind, int n_in, int n_out, std::vector<int>& t) {
    union { float f; int i; } u;
    if (kind == LINEAR) {
        t.assign((size_t)n_out * 3, 0);
        for (int d = 0; d < n_out; ++d) {
            int i0;
            float f;
            axis_position(n_in, n_out, d, &i0, &f);
            const bool lo = i0 < 0, hi = i0 >= n_in - 1;
            if (lo || hi) f = 0.0f;
            i0 = lo ? 0 : (hi ? n_in - 1 : i0);
            t[d] = i0;
            t[(size_t)n_out + d] = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
            u.f = f;
            t[(size_t)2 * n_out + d] = u.i;
        }
        return;
    }
    if (kind == NEAREST) {
        t.assign((size_t)n_out, 0);
        for (int d = 0; d < n_out; ++d) t[d] = nearest_index(n_in, n_out, d);
        return;
    }
    if (kind == LINEAR_FIXED) {
        t.assign((size_t)n_out * 3, 0);
        for (int d = 0; d < n_out; ++d) linear_fixed(n_in, n_out, d, &t[d], &t[(size_t)n_out + (size_t)d * 2]);
        return;
    }
    if (kind == CUBIC_FIXED) {
        t.assign((size_t)n_out * 5, 0);
        for (int d = 0; d < n_out; ++d) {
            int i0;
            float f, co[4];
            axis_position(n_in, n_out, d, &i0, &f);
            cubic_coeffs(f, co);
            t[d] = i0 - 1;
            for (int k = 0; k < 4; ++k) t[(size_t)n_out + (size_t)d * 4 + k] = fixed11(co[k]);
        }
        return;
    }
    t.assign((size_t)n_out * 9, 0);
    for (int d = 0; d < n_out; ++d) {
        int i0;
        float f, co[8];
        axis_position(n_in, n_out, d, &i0, &f);
        if (kind == LANCZOS_FIXED) lanczos4_coeffs_f64(f, co);
        else lanczos4_coeffs_f32(f, co);
        t[d] = i0 - 3;
        for (int k = 0; k < 8; ++k) {
            if (kind == LANCZOS_FIXED) {
                t[(size_t)n_out + (size_t)d * 8 + k] = fixed11(co[k]);
            } else {
                u.f = co[k];
                t[(size_t)n_out + (size_t)d * 8 + k] = u.i;
            }
        }
    }
}

// Device tables per (device, kind, n_in, n_out): built and uploaded by the first call that needs them, kept for the process.  The
// lock is held from the lookup until the kernel that reads the tables is enqueued, so dropping the cache (hipFree waits for the
// device) never takes a table from a launch.
struct HostDev {
    std::vector<int> host;
    int* dev = nullptr;
};
std::mutex g_mu;
std::map<std::tuple<int, int, int, int>, HostDev> g_tables;
constexpr size_t MAX_TABLES = 1024;

void make_room() {               // before a call's lookups, never between them
    if (g_tables.size() + 2 <= MAX_TABLES) return;
    for (auto& e : g_tables) (void)hipFree(e.second.dev);
    g_tables.clear();
}

int device_table(int device, TableKind kind, int n_in, int n_out, const HostDev** out) {
    const auto key = std::make_tuple(device, (int)kind, n_in, n_out);
    auto it = g_tables.find(key);
    if (it == g_tables.end()) {
        HostDev t;
        build_table(kind, n_in, n_out, t.host);
        const size_t bytes = t.host.size() * sizeof(int);
        NESR_TRY(hipMalloc(&t.dev, bytes));
        const hipError_t e = hipMemcpy(t.dev, t.host.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(t.dev);
            return set_error(NESR_ERR_HIP, std::string("uploading the resize table: ") + hipGetErrorString(e));
        }
        it = g_tables.emplace(key, std::move(t)).first;
    }
    *out = &it->second;
    return NESR_OK;
}

// source positions a tile of t outputs reads at most (tiles start at multiples of t; first[] is monotone)
int max_span(const int* first, int n_out, int n_in, int t, int taps) {
    int m = 1;
    for (int d0 = 0; d0 < n_out; d0 += t) {
        const int d1 = d0 + t < n_out ? d0 + t : n_out;
        const int s = first[d1 - 1] + taps - 1 - first[d0] + 1;
        m = s > m ? s : m;
    }
    return m < n_in ? m : n_in;
}

int pow2_at_least(int v, int cap) {
    int p = 1;
    while (p < v && p < cap) p <<= 1;
    return p;
}

// tile shape: the widest, then the tallest power of two whose LDS need fits RESIZE_LDS_BUDGET (1 x 1 needs 8 x 8 samples: always fits)
void plan_tile(ResizeArgs& a, int S, const int* xfirst, const int* yfirst, int taps = 8) {
    auto need = [&](int tx, int ty) {
        const int cols = max_span(xfirst, a.dst_w, a.src_w, tx, taps), rows = max_span(yfirst, a.dst_h, a.src_h, ty, taps);
        a.tx = tx;
        a.ty = ty;
        a.max_rows = rows;
        a.stage_pitch = round_up(cols * a.C * S + 3, 4);
        a.out_pitch = round_up(tx * a.C * S + 3, 4);
        const size_t stage = (size_t)rows * a.stage_pitch, tile = (size_t)ty * a.out_pitch;
        const size_t r0 = align_up(stage > tile ? stage : tile, 16);
        const size_t total = r0 + (size_t)rows * a.C * tx * 4;
        a.region0 = (int)(r0 < (1u << 30) ? r0 : (1u << 30));
        a.lds_bytes = (int)(total < (1u << 30) ? total : (1u << 30));
        return total;
    };
    int tx = pow2_at_least(a.dst_w, a.C == 1 ? 256 : 64), ty = pow2_at_least(a.dst_h, 64);
    while (tx > 1 && need(tx, 1) > (size_t)RESIZE_LDS_BUDGET) tx >>= 1;
    while (need(tx, ty) > (size_t)RESIZE_LDS_BUDGET && ty > 1) ty >>= 1;
}

const char* interp_name(int interp) {
    return interp == NESR_INTER_LANCZOS4 ? "NESR_INTER_LANCZOS4" : interp == NESR_INTER_LINEAR ? "NESR_INTER_LINEAR" : "an unknown interpolation";
}

// the checks every form shares; S = bytes per sample
int check_args(const char* who, const char* type, int S, int want_interp, const void* src, int src_h, int src_w, int C, int64_t src_row_bytes,
               const void* dst, int dst_h, int dst_w, int64_t dst_row_bytes, int interp, bool c2) {
    const std::string w(who);
    if (!src || !dst) return set_error(NESR_ERR_ARG, w + ": null argument");
    if (interp != want_interp)
        return set_error(NESR_ERR_ARG, w + ": " + type + " with " + interp_name(interp) + " (" + std::to_string(interp) + ") is not supported (u8 and u16 take "
                                       "NESR_INTER_LANCZOS4, f32 takes NESR_INTER_LINEAR)");
    if (src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1) return set_error(NESR_ERR_ARG, w + ": every size must be at least 1");
    if (src_h > (1 << 24) || src_w > (1 << 24) || dst_h > (1 << 24) || dst_w > (1 << 24)) return set_error(NESR_ERR_ARG, w + ": sizes up to 2^24");
    if (c2 ? (C < 1 || C > 4) : (C != 1 && C != 3 && C != 4))
        return set_error(NESR_ERR_ARG, w + ": " + std::to_string(C) + " channels (" + type + " takes " + (c2 ? "1 to 4" : "1, 3 or 4") + ")");
    if (src_row_bytes < (long long)src_w * C * S || dst_row_bytes < (long long)dst_w * C * S)
        return set_error(NESR_ERR_ARG, w + ": a row stride is smaller than the row");
    if (src == dst) return set_error(NESR_ERR_ARG, w + ": cannot run in place (src == dst)");
    if (S > 1 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)src_row_bytes | (uintptr_t)dst_row_bytes) & (uintptr_t)(S - 1)))
        return set_error(NESR_ERR_ARG, w + ": pointers and row strides must be multiples of the sample size");
    return NESR_OK;
}

ResizeArgs base_args(const void* src, int src_h, int src_w, int C, int64_t src_row_bytes, void* dst, int dst_h, int dst_w, int64_t dst_row_bytes) {
    ResizeArgs a{};
    a.src = static_cast<const unsigned char*>(src);
    a.dst = static_cast<unsigned char*>(dst);
    a.src_stride = src_row_bytes;
    a.dst_stride = dst_row_bytes;
    a.src_h = src_h; a.src_w = src_w; a.dst_h = dst_h; a.dst_w = dst_w; a.C = C;
    return a;
}

int lanczos4(int device, int S, ResizeArgs a, void* stream) {
    NESR_TRY(hipSetDevice(device));
    std::lock_guard<std::mutex> lock(g_mu);
    const TableKind kind = S == 1 ? LANCZOS_FIXED : LANCZOS_FLOAT;
    const HostDev *tx = nullptr, *ty = nullptr;
    make_room();
    RS_CALL(device_table(device, kind, a.src_w, a.dst_w, &tx));
    RS_CALL(device_table(device, kind, a.src_h, a.dst_h, &ty));
    a.xtab = tx->dev;
    a.ytab = ty->dev;
    plan_tile(a, S, tx->host.data(), ty->host.data());
    NESR_TRY(launch_resize_lanczos4(a, S, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}

// nesr_resize_cv_u8's nearest, linear and cubic forms: the two tables, then one launch
int cv_resize(int device, TableKind kind, ResizeArgs a, void* stream) {
    NESR_TRY(hipSetDevice(device));
    std::lock_guard<std::mutex> lock(g_mu);
    const HostDev *tx = nullptr, *ty = nullptr;
    make_room();
    RS_CALL(device_table(device, kind, a.src_w, a.dst_w, &tx));
    RS_CALL(device_table(device, kind, a.src_h, a.dst_h, &ty));
    a.xtab = tx->dev;
    a.ytab = ty->dev;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (kind == CUBIC_FIXED) {
        plan_tile(a, 1, tx->host.data(), ty->host.data(), 4);
        NESR_TRY(launch_resize_cubic_u8(a, s));
    } else if (kind == LINEAR_FIXED) {
        NESR_TRY(launch_resize_linear_u8(a, s));
    } else {
        NESR_TRY(launch_resize_nearest_u8(a, s));
    }
    return NESR_OK;
}

bool cv_interp_known(int interp) {
    return interp == NESR_INTER_NEAREST || interp == NESR_INTER_LINEAR || interp == NESR_INTER_CUBIC || interp == NESR_INTER_LANCZOS4;
}

}  // namespace

int nesr_resize_cv_taps(int n_in, int n_out, int interp, int* first_out, int* coef_out, int cap, int* n_out_written) {
    if (!n_out_written) return set_error(NESR_ERR_ARG, "nesr_resize_cv_taps: null argument");
    if (n_in < 1 || n_out < 1 || n_in > (1 << 24) || n_out > (1 << 24)) return set_error(NESR_ERR_ARG, "nesr_resize_cv_taps: sizes from 1 to 2^24");
    if (!cv_interp_known(interp))
        return set_error(NESR_ERR_ARG, "nesr_resize_cv_taps: interp must be NESR_INTER_NEAREST, NESR_INTER_LINEAR, NESR_INTER_CUBIC or NESR_INTER_LANCZOS4");
    *n_out_written = n_out;
    if (!first_out || !coef_out || cap < n_out) return NESR_OK;
    const TableKind kind = interp == NESR_INTER_NEAREST ? NEAREST : interp == NESR_INTER_LINEAR ? LINEAR_FIXED : interp == NESR_INTER_CUBIC ? CUBIC_FIXED : LANCZOS_FIXED;
    const int per = interp == NESR_INTER_NEAREST ? 1 : interp == NESR_INTER_LINEAR ? 2 : interp == NESR_INTER_CUBIC ? 4 : 8;
    std::vector<int> t;
    build_table(kind, n_in, n_out, t);          // the image the kernels read
    for (int d = 0; d < n_out; ++d) {
        first_out[d] = t[d];
        for (int k = 0; k < per; ++k) coef_out[(size_t)d * per + k] = kind == NEAREST ? 1 : t[(size_t)n_out + (size_t)d * per + k];
    }
    return NESR_OK;
}

int nesr_resize_cv_u8(int device_id, const uint8_t* src_dev, int src_h, int src_w, int C, int64_t src_row_bytes, uint8_t* dst_dev, int dst_h, int dst_w,
                      int64_t dst_row_bytes, int interp, void* stream) {
    if (!cv_interp_known(interp))
        return set_error(NESR_ERR_ARG, "nesr_resize_cv_u8: interpolation " + std::to_string(interp) + " is not supported (NESR_INTER_NEAREST, NESR_INTER_LINEAR, "
                                       "NESR_INTER_CUBIC or NESR_INTER_LANCZOS4)");
    RS_CALL(check_args("nesr_resize_cv_u8", "u8", 1, interp, src_dev, src_h, src_w, C, src_row_bytes, dst_dev, dst_h, dst_w, dst_row_bytes, interp, false));
    const ResizeArgs a = base_args(src_dev, src_h, src_w, C, src_row_bytes, dst_dev, dst_h, dst_w, dst_row_bytes);
    if (interp == NESR_INTER_LANCZOS4) return lanczos4(device_id, 1, a, stream);
    return cv_resize(device_id, interp == NESR_INTER_NEAREST ? NEAREST : interp == NESR_INTER_LINEAR ? LINEAR_FIXED : CUBIC_FIXED, a, stream);
}

int nesr_resize_taps(int n_in, int n_out, int interp, int* first_out, float* coef_out, int cap, int* n_out_written) {
    if (!n_out_written) return set_error(NESR_ERR_ARG, "nesr_resize_taps: null argument");
    if (n_in < 1 || n_out < 1 || n_in > (1 << 24) || n_out > (1 << 24)) return set_error(NESR_ERR_ARG, "nesr_resize_taps: sizes from 1 to 2^24");
    if (interp != NESR_INTER_LANCZOS4 && interp != NESR_INTER_LINEAR)
        return set_error(NESR_ERR_ARG, "nesr_resize_taps: interp must be NESR_INTER_LANCZOS4 or NESR_INTER_LINEAR");
    *n_out_written = n_out;
    if (!first_out || !coef_out || cap < n_out) return NESR_OK;
    for (int d = 0; d < n_out; ++d) {
        int i0;
        float f;
        axis_position(n_in, n_out, d, &i0, &f);
        if (interp == NESR_INTER_LANCZOS4) {
            float co[8], cq[8];
            lanczos4_coeffs_f32(f, co);
            lanczos4_coeffs_f64(f, cq);
            first_out[d] = i0 - 3;
            for (int k = 0; k < 8; ++k) {
                coef_out[(size_t)d * 16 + k] = co[k];
                coef_out[(size_t)d * 16 + 8 + k] = (float)fixed11(cq[k]);
            }
        } else {
            const bool lo = i0 < 0, hi = i0 >= n_in - 1;
            if (lo || hi) f = 0.0f;
            i0 = lo ? 0 : (hi ? n_in - 1 : i0);
            first_out[d] = i0;
            coef_out[(size_t)d * 2] = f;
            coef_out[(size_t)d * 2 + 1] = i0 + 1 < n_in ? 1.0f : 0.0f;
        }
    }
    return NESR_OK;
}

int nesr_resize_u8(int device_id, const uint8_t* src_dev, int src_h, int src_w, int C, int64_t src_row_bytes, uint8_t* dst_dev, int dst_h, int dst_w,
                   int64_t dst_row_bytes, int interp, void* stream) {
    RS_CALL(check_args("nesr_resize_u8", "u8", 1, NESR_INTER_LANCZOS4, src_dev, src_h, src_w, C, src_row_bytes, dst_dev, dst_h, dst_w, dst_row_bytes, interp, false));
    return lanczos4(device_id, 1, base_args(src_dev, src_h, src_w, C, src_row_bytes, dst_dev, dst_h, dst_w, dst_row_bytes), stream);
}

int nesr_resize_u16(int device_id, const uint16_t* src_dev, int src_h, int src_w, int C, int64_t src_row_bytes, uint16_t* dst_dev, int dst_h, int dst_w,
                    int64_t dst_row_bytes, int interp, void* stream) {
    RS_CALL(check_args("nesr_resize_u16", "u16", 2, NESR_INTER_LANCZOS4, src_dev, src_h, src_w, C, src_row_bytes, dst_dev, dst_h, dst_w, dst_row_bytes, interp, false));
    return lanczos4(device_id, 2, base_args(src_dev, src_h, src_w, C, src_row_bytes, dst_dev, dst_h, dst_w, dst_row_bytes), stream);
}

int nesr_resize_f32(int device_id, const float* src_dev, int src_h, int src_w, int C, int64_t src_row_bytes, float* dst_dev, int dst_h, int dst_w,
                    int64_t dst_row_bytes, int interp, void* stream) {
    RS_CALL(check_args("nesr_resize_f32", "f32", 4, NESR_INTER_LINEAR, src_dev, src_h, src_w, C, src_row_bytes, dst_dev, dst_h, dst_w, dst_row_bytes, interp, true));
    ResizeArgs a = base_args(src_dev, src_h, src_w, C, src_row_bytes, dst_dev, dst_h, dst_w, dst_row_bytes);
    NESR_TRY(hipSetDevice(device_id));
    std::lock_guard<std::mutex> lock(g_mu);
    const HostDev *tx = nullptr, *ty = nullptr;
    make_room();
    RS_CALL(device_table(device_id, LINEAR, src_w, dst_w, &tx));
    RS_CALL(device_table(device_id, LINEAR, src_h, dst_h, &ty));
    a.xtab = tx->dev;
    a.ytab = ty->dev;
    NESR_TRY(launch_resize_linear_f32(a, static_cast<hipStream_t>(stream)));
    return NESR_OK;
}
