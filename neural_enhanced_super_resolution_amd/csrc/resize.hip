// cv2.resize as HIP kernels (nesr/nesr.py:437-446 and upstream's RealESRGANer.enhance(outscale=...,
// alpha_upsampler=...)): INTER_LANCZOS4 on 8-bit (OpenCV's fixed point) and 16-bit (float32) images, INTER_LINEAR on float32; and
// the 8-bit INTER_NEAREST, INTER_LINEAR and INTER_CUBIC of the rest of enhance_image's loop (nesr/nesr.py:597-605, 720-724, 732;
// nesr_resize_cv_u8).  Each kernel restates the torch chain of imgproc.py (lanczos4_resize, linear_resize_f32, resize_u8) / the
// loops of oracle/cv2_ref.py operation by operation; parity against cv2 itself is unpinned (cv2 is not installed).
//
// The Lanczos forms (and the 8-bit bicubic: the same kernel with 4 taps) run both passes in one launch and keep nothing in HBM between them.  A workgroup owns TY output rows x TX output
// columns.  It copies the source rectangle those outputs read (8 taps per axis, indices clamped = BORDER_REPLICATE) into LDS with
// aligned 4-byte loads, runs the horizontal pass for every staged source row into LDS planes (int32 for u8, float for u16), runs
// the vertical pass from those planes, collects the output tile in LDS and stores it as whole aligned 4-byte words (single bytes
// only at a row's unaligned ends, so a destination that is a rectangle of a larger canvas keeps every byte around it).  TX and TY
// come from the host (resize_api.cpp): the largest powers of two whose LDS need stays within RESIZE_LDS_BUDGET, so two workgroups
// fit a CU at every ratio; one output row needs 8 source rows, which always fits.
//
// Images are addressed as base pointer + row stride in bytes (pixels of a row contiguous): a sub-rectangle of a frame is an offset
// pointer with the frame's stride, and is its own image (the border is the rectangle's edge).
#include "../../include/nesr_hip.h"
#include "nesr_kernels.h"

namespace nesr {
namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename T> struct Acc;
template <> struct Acc<uint8_t> { using type = int; };
template <> struct Acc<uint16_t> { using type = float; };

// u8: coefficient x sample in int32 (|sum| < 2^20 x 2048 per product; the vertical sum is kept in int64, as the torch chain does:
// an adversarial image can pass 2^31 before the saturation).  u16: acc = acc + w * x with the product and the sum rounded
// separately, k ascending (oracle/cv2_ref.py's order).
__device__ __forceinline__ int hstep(int acc, int w, int x) { return acc + w * x; }
__device__ __forceinline__ float hstep(float acc, float w, float x) { return add_rn(acc, mul_rn(w, x)); }

__device__ __forceinline__ uint8_t finish(long long v, uint8_t) {
    v = (v + (1ll << 21)) >> 22;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
__device__ __forceinline__ uint16_t finish(float v, uint16_t) {
    v = rintf(v);
    return (uint16_t)(v < 0.f ? 0.f : (v > 65535.f ? 65535.f : v));
}

// NT taps per axis: 8 = Lanczos-4 (first tap floor - 3), 4 = bicubic (first tap floor - 1; u8 only)
template <typename T, int C, int NT>
__global__ __launch_bounds__(256) void lanczos4_kernel(ResizeArgs a) {
    using A = typename Acc<T>::type;
    using V = typename std::conditional<sizeof(T) == 1, long long, float>::type;      // vertical accumulator
    extern __shared__ __align__(16) unsigned char lds[];
    constexpr int S = (int)sizeof(T);
    const int tid = threadIdx.x;
    const int TX = a.tx, TY = a.ty;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int nx = min(TX, a.dst_w - x0), ny = min(TY, a.dst_h - y0);
    const int* __restrict__ xfirst = a.xtab;
    const int* __restrict__ yfirst = a.ytab;
    const A* __restrict__ xcoef = reinterpret_cast<const A*>(a.xtab + a.dst_w);
    const A* __restrict__ ycoef = reinterpret_cast<const A*>(a.ytab + a.dst_h);
    // the source rectangle of this tile: first tap of the first output .. last tap of the last one, clamped (the tables are monotone)
    const int clo = clampi(xfirst[x0], 0, a.src_w - 1), chi = clampi(xfirst[x0 + nx - 1] + NT - 1, 0, a.src_w - 1);
    const int rlo = clampi(yfirst[y0], 0, a.src_h - 1), rhi = clampi(yfirst[y0 + ny - 1] + NT - 1, 0, a.src_h - 1);
    const int nr = rhi - rlo + 1;                       // <= a.max_rows
    const int seg = (chi - clo + 1) * C * S;            // bytes of a staged row segment; <= a.stage_pitch - 4
    unsigned char* stage = lds;                         // [nr][stage_pitch] source bytes, then reused as the output tile
    A* hbuf = reinterpret_cast<A*>(lds + a.region0);    // [nr][C][TX] horizontal sums

    // 1. stage: row r's segment lands at stage + r * pitch + (its global address & 3), so aligned words map to aligned words
    const int wpr = a.stage_pitch >> 2;
    const long long row_bytes = (long long)a.src_w * C * S;
    for (int i = tid; i < nr * wpr; i += 256) {
        const int r = i / wpr, wd = i - r * wpr;
        const unsigned char* row = a.src + (size_t)(rlo + r) * a.src_stride;
        const long long b0 = (long long)clo * C * S;
        const int sh = (int)((reinterpret_cast<uintptr_t>(row) + (uintptr_t)b0) & 3);
        const long long off = b0 - sh + 4ll * wd;       // byte offset of this word from the row's start
        if (off >= b0 + seg) continue;
        unsigned v = 0;
        if (off >= 0 && off + 4 <= row_bytes) {
            v = *reinterpret_cast<const unsigned*>(row + off);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (off + b >= 0 && off + b < row_bytes) v |= (unsigned)row[off + b] << (8 * b);
        }
        *reinterpret_cast<unsigned*>(stage + (size_t)r * a.stage_pitch + 4 * wd) = v;
    }
    __syncthreads();

    // 2. horizontal pass: a thread keeps one output column (its taps and coefficients in registers) and walks the staged rows
    const int lx = tid & (TX - 1), rstep = 256 / TX;
    if (lx < nx) {
        const int first = xfirst[x0 + lx];
        int o[NT];
        A w[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            o[k] = (clampi(first + k, 0, a.src_w - 1) - clo) * C * S;
            w[k] = xcoef[(size_t)(x0 + lx) * NT + k];
        }
        for (int r = tid / TX; r < nr; r += rstep) {
            const unsigned char* row = a.src + (size_t)(rlo + r) * a.src_stride;
            const int sh = (int)((reinterpret_cast<uintptr_t>(row) + (uintptr_t)((long long)clo * C * S)) & 3);
            const unsigned char* p = stage + (size_t)r * a.stage_pitch + sh;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                A acc = 0;
#pragma unroll
                for (int k = 0; k < NT; ++k) acc = hstep(acc, w[k], (A)*reinterpret_cast<const T*>(p + o[k] + c * S));
                hbuf[((size_t)r * C + c) * TX + lx] = acc;
            }
        }
    }
    __syncthreads();

    // 3. vertical pass into the output tile (LDS, over the stage): row oy at otile + oy * out_pitch + (its global address & 3)
    unsigned char* otile = lds;
    const size_t dx0 = (size_t)x0 * C * S;
    if (lx < nx) {
        for (int oy = tid / TX; oy < ny; oy += rstep) {
            const int first = yfirst[y0 + oy];
            int rr[NT];
            A w[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                rr[k] = clampi(first + k, 0, a.src_h - 1) - rlo;
                w[k] = ycoef[(size_t)(y0 + oy) * NT + k];
            }
            const int sh = (int)((reinterpret_cast<uintptr_t>(a.dst + (size_t)(y0 + oy) * a.dst_stride) + dx0) & 3);
            T* q = reinterpret_cast<T*>(otile + (size_t)oy * a.out_pitch + sh) + lx * C;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                V acc = 0;
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const A h = hbuf[((size_t)rr[k] * C + c) * TX + lx];
                    if constexpr (sizeof(T) == 1) acc += (long long)w[k] * h;
                    else acc = hstep(acc, w[k], h);
                }
                q[c] = finish(acc, T());
            }
        }
    }
    __syncthreads();

    // 4. store: aligned 4-byte words; the bytes of a word that lie outside the row's run are never written
    const int run = nx * C * S, opw = a.out_pitch >> 2;
    for (int i = tid; i < ny * opw; i += 256) {
        const int oy = i / opw, wd = i - oy * opw;
        unsigned char* g = a.dst + (size_t)(y0 + oy) * a.dst_stride + dx0;            // first byte of the run
        const int sh = (int)(reinterpret_cast<uintptr_t>(g) & 3);
        const int off = 4 * wd - sh;                                                   // of this word from g
        if (off >= run) continue;
        const unsigned v = *reinterpret_cast<const unsigned*>(otile + (size_t)oy * a.out_pitch + 4 * wd);
        if (off >= 0 && off + 4 <= run) {
            *reinterpret_cast<unsigned*>(g + off) = v;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (off + b >= 0 && off + b < run) g[off + b] = (unsigned char)(v >> (8 * b));
        }
    }
}

// imgproc.linear_resize_f32: a (1 - f) + b f per pass, every product and sum rounded by itself; one output pixel per thread
template <int C>
__global__ __launch_bounds__(256) void linear_f32_kernel(ResizeArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.dst_w || y >= a.dst_h) return;
    const int* xt = a.xtab;
    const int* yt = a.ytab;
    const int xa = xt[x], xb = xt[a.dst_w + x], ya = yt[y], yb = yt[a.dst_h + y];
    const float fx = __int_as_float(xt[2 * a.dst_w + x]), fy = __int_as_float(yt[2 * a.dst_h + y]);
    const float gx = sub_rn(1.0f, fx), gy = sub_rn(1.0f, fy);
    const float* r0 = reinterpret_cast<const float*>(a.src + (size_t)ya * a.src_stride);
    const float* r1 = reinterpret_cast<const float*>(a.src + (size_t)yb * a.src_stride);
    float* q = reinterpret_cast<float*>(a.dst + (size_t)y * a.dst_stride) + (size_t)x * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float top = add_rn(mul_rn(r0[(size_t)xa * C + c], gx), mul_rn(r0[(size_t)xb * C + c], fx));
        const float bot = add_rn(mul_rn(r1[(size_t)xa * C + c], gx), mul_rn(r1[(size_t)xb * C + c], fx));
        q[c] = add_rn(mul_rn(top, gy), mul_rn(bot, fy));
    }
}

// cv2's other 8-bit interpolations, one output pixel per thread, both passes in registers (nothing between them anywhere):
//   PT_NEAREST  xtab / ytab = the source index of every position; the samples are copied
//   PT_LINEAR   tables = first index s (clamped), then 2 coefficients per position (11-bit, non-negative); the second tap is
//               min(s + 1, n - 1).  OpenCV's 8-bit form: t = S[s] a0 + S[s + 1] a1, then
//               (((b0 (t0 >> 4)) >> 16) + ((b1 (t1 >> 4)) >> 16) + 2) >> 2 -- at most 255, nothing to saturate
//   PT_AREA2    both axes shrink by exactly 2 (cv2 switches INTER_LINEAR to its area filter): (a + b + c + d + 2) >> 2, no tables
enum { PT_NEAREST = 0, PT_LINEAR = 1, PT_AREA2 = 2 };

template <int C, int MODE>
__global__ __launch_bounds__(256) void point_u8_kernel(ResizeArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.dst_w || y >= a.dst_h) return;
    uint8_t* q = a.dst + (size_t)y * a.dst_stride + (size_t)x * C;
    if constexpr (MODE == PT_NEAREST) {
        const uint8_t* p = a.src + (size_t)a.ytab[y] * a.src_stride + (size_t)a.xtab[x] * C;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c];
    } else if constexpr (MODE == PT_AREA2) {
        const uint8_t* r0 = a.src + (size_t)(2 * y) * a.src_stride + (size_t)(2 * x) * C;
        const uint8_t* r1 = r0 + a.src_stride;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = (uint8_t)(((int)r0[c] + (int)r0[C + c] + (int)r1[c] + (int)r1[C + c] + 2) >> 2);
    } else {
        const int xa = a.xtab[x], ya = a.ytab[y];
        const int xb = min(xa + 1, a.src_w - 1), yb = min(ya + 1, a.src_h - 1);
        const int a0 = a.xtab[a.dst_w + 2 * x], a1 = a.xtab[a.dst_w + 2 * x + 1];
        const int b0 = a.ytab[a.dst_h + 2 * y], b1 = a.ytab[a.dst_h + 2 * y + 1];
        const uint8_t* r0 = a.src + (size_t)ya * a.src_stride;
        const uint8_t* r1 = a.src + (size_t)yb * a.src_stride;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int t0 = (int)r0[(size_t)xa * C + c] * a0 + (int)r0[(size_t)xb * C + c] * a1;
            const int t1 = (int)r1[(size_t)xa * C + c] * a0 + (int)r1[(size_t)xb * C + c] * a1;
            q[c] = (uint8_t)((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2);
        }
    }
}

template <int MODE>
hipError_t launch_point_u8_t(const ResizeArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.dst_w + 63) / 64), (unsigned)((a.dst_h + 3) / 4));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (a.C == 1) hipLaunchKernelGGL((point_u8_kernel<1, MODE>), grid, dim3(256), 0, s, a);
    else if (a.C == 3) hipLaunchKernelGGL((point_u8_kernel<3, MODE>), grid, dim3(256), 0, s, a);
    else if (a.C == 4) hipLaunchKernelGGL((point_u8_kernel<4, MODE>), grid, dim3(256), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename T, int NT>
hipError_t launch_lanczos4_t(const ResizeArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.dst_w + a.tx - 1) / a.tx), (unsigned)((a.dst_h + a.ty - 1) / a.ty));
    const size_t lds = (size_t)a.lds_bytes;
    if (a.C == 1) hipLaunchKernelGGL((lanczos4_kernel<T, 1, NT>), grid, dim3(256), lds, s, a);
    else if (a.C == 3) hipLaunchKernelGGL((lanczos4_kernel<T, 3, NT>), grid, dim3(256), lds, s, a);
    else if (a.C == 4) hipLaunchKernelGGL((lanczos4_kernel<T, 4, NT>), grid, dim3(256), lds, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

namespace {
bool tile_plan_ok(const ResizeArgs& a) {
    if (a.tx < 1 || a.tx > 256 || (a.tx & (a.tx - 1)) || a.ty < 1 || a.lds_bytes > RESIZE_LDS_BUDGET || (a.stage_pitch & 3) || (a.out_pitch & 3) ||
        (a.region0 & 15))
        return false;
    return a.dst_h <= 65535 * a.ty;
}
}  // namespace

hipError_t launch_resize_lanczos4(const ResizeArgs& a, int elem_bytes, hipStream_t s) {
    if (!tile_plan_ok(a)) return hipErrorInvalidValue;
    return elem_bytes == 1 ? launch_lanczos4_t<uint8_t, 8>(a, s) : elem_bytes == 2 ? launch_lanczos4_t<uint16_t, 8>(a, s) : hipErrorInvalidValue;
}

hipError_t launch_resize_cubic_u8(const ResizeArgs& a, hipStream_t s) {
    if (!tile_plan_ok(a)) return hipErrorInvalidValue;
    return launch_lanczos4_t<uint8_t, 4>(a, s);
}

hipError_t launch_resize_nearest_u8(const ResizeArgs& a, hipStream_t s) { return launch_point_u8_t<PT_NEAREST>(a, s); }

hipError_t launch_resize_linear_u8(const ResizeArgs& a, hipStream_t s) {
    if (a.src_w == 2 * a.dst_w && a.src_h == 2 * a.dst_h) return launch_point_u8_t<PT_AREA2>(a, s);
    return launch_point_u8_t<PT_LINEAR>(a, s);
}

hipError_t launch_resize_linear_f32(const ResizeArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.dst_w + 63) / 64), (unsigned)((a.dst_h + 3) / 4));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    switch (a.C) {
        case 1: hipLaunchKernelGGL(linear_f32_kernel<1>, grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL(linear_f32_kernel<2>, grid, dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(linear_f32_kernel<3>, grid, dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL(linear_f32_kernel<4>, grid, dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nesr
