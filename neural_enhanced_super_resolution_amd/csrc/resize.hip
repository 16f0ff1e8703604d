// cv2.resize as HIP kernels (nesr/nesr.py:437-446 and upstream's RealESRGANer.enhance(outscale=...,
// alpha_upsampler=...)): INTER_LANCZOS4 on 8-bit (OpenCV's fixed point) and 16-bit (float32) images, INTER_LINEAR on float32.  Each
// kernel restates the torch chain of imgproc.py (lanczos4_resize, linear_resize_f32) / the loops of oracle/cv2_ref.py operation by
// operation; parity against cv2 itself is unpinned (cv2 is not installed).
//
// The Lanczos forms run both passes in one launch and keep nothing in HBM between them.  A workgroup owns TY output rows x TX output
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

template <typename T, int C>
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
    const int clo = clampi(xfirst[x0], 0, a.src_w - 1), chi = clampi(xfirst[x0 + nx - 1] + 7, 0, a.src_w - 1);
    const int rlo = clampi(yfirst[y0], 0, a.src_h - 1), rhi = clampi(yfirst[y0 + ny - 1] + 7, 0, a.src_h - 1);
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
        int o[8];
        A w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            o[k] = (clampi(first + k, 0, a.src_w - 1) - clo) * C * S;
            w[k] = xcoef[(size_t)(x0 + lx) * 8 + k];
        }
        for (int r = tid / TX; r < nr; r += rstep) {
            const unsigned char* row = a.src + (size_t)(rlo + r) * a.src_stride;
            const int sh = (int)((reinterpret_cast<uintptr_t>(row) + (uintptr_t)((long long)clo * C * S)) & 3);
            const unsigned char* p = stage + (size_t)r * a.stage_pitch + sh;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                A acc = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc = hstep(acc, w[k], (A)*reinterpret_cast<const T*>(p + o[k] + c * S));
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
            int rr[8];
            A w[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                rr[k] = clampi(first + k, 0, a.src_h - 1) - rlo;
                w[k] = ycoef[(size_t)(y0 + oy) * 8 + k];
            }
            const int sh = (int)((reinterpret_cast<uintptr_t>(a.dst + (size_t)(y0 + oy) * a.dst_stride) + dx0) & 3);
            T* q = reinterpret_cast<T*>(otile + (size_t)oy * a.out_pitch + sh) + lx * C;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                V acc = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
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

template <typename T>
hipError_t launch_lanczos4_t(const ResizeArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.dst_w + a.tx - 1) / a.tx), (unsigned)((a.dst_h + a.ty - 1) / a.ty));
    const size_t lds = (size_t)a.lds_bytes;
    if (a.C == 1) hipLaunchKernelGGL((lanczos4_kernel<T, 1>), grid, dim3(256), lds, s, a);
    else if (a.C == 3) hipLaunchKernelGGL((lanczos4_kernel<T, 3>), grid, dim3(256), lds, s, a);
    else if (a.C == 4) hipLaunchKernelGGL((lanczos4_kernel<T, 4>), grid, dim3(256), lds, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

hipError_t launch_resize_lanczos4(const ResizeArgs& a, int elem_bytes, hipStream_t s) {
    if (a.tx < 1 || a.tx > 256 || (a.tx & (a.tx - 1)) || a.ty < 1 || a.lds_bytes > RESIZE_LDS_BUDGET || (a.stage_pitch & 3) || (a.out_pitch & 3) ||
        (a.region0 & 15))
        return hipErrorInvalidValue;
    if (a.dst_h > 65535 * a.ty) return hipErrorInvalidValue;
    return elem_bytes == 1 ? launch_lanczos4_t<uint8_t>(a, s) : elem_bytes == 2 ? launch_lanczos4_t<uint16_t>(a, s) : hipErrorInvalidValue;
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
