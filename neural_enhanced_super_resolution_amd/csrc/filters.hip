// The rest of the pipeline's filters -- everything of SuperResolutionPipeline._preprocess_image
// (nesr/nesr.py:668-689) and _postprocess_image (nesr/nesr.py:1056-1084) that is not the non-local means or the CLAHE of
// imgproc.hip: the Lab conversions around them, OpenCV's fixed-point Gaussian blur and the adaptive unsharp mask.  Each kernel
// restates the torch function of imgproc.py that specifies it (rgb2lab_u8 / lab2rgb_u8, gaussian_blur_u8, postprocess_image)
// operation by operation, so the two agree bit for bit (tests/test_gpu_filters_hip.py); parity against cv2 is unpinned (cv2 is
// not installed; oracle/cv2_ref.py restates the same algorithms).
#include "../../include/nesr_hip.h"
#include "nesr_kernels.h"

namespace nesr {
namespace {

// The Lab conversions in float, as the torch chain evaluates them on the device: every operation rounds by itself (the torch
// operations are separate kernels, so nothing is ever contracted into an fma -- hence mul_rn / add_rn / sub_rn of
// nesr_kernels.h), a Python constant is the float nearest to its double (ATen casts a scalar operand to the tensor's type), a
// division of a tensor by a scalar is a multiplication by the reciprocal (ATen's div_true on the device; the reciprocal is
// taken in double and rounded to float -- for 1.055 and 1.088754 that differs from 1.0f / float(x), found by the exhaustive
// test), torch.pow is the device library's powf and torch.round is round half to even.
#define F32(x) ((float)(x))                  // a Python float operand of a float tensor
#define RCP(x) ((float)(1.0 / (x)))          // `tensor / x`: ATen multiplies by the reciprocal, taken in double and rounded to float

__device__ __forceinline__ float lab_f(float t) {
    return t > F32(0.008856) ? powf(fmaxf(t, F32(1e-12)), F32(1.0 / 3.0)) : add_rn(mul_rn(F32(7.787), t), F32(16.0 / 116.0));
}

__device__ __forceinline__ int to_u8(float v) {
    v = rintf(v);
    return (int)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
}

// imgproc.rgb2lab_u8
__device__ __forceinline__ void rgb2lab(const int in[3], bool linear, bool blue, int out[3]) {
    float c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[i] = mul_rn((float)in[i], RCP(255.0));
        if (!linear)
            c[i] = c[i] <= F32(0.04045) ? mul_rn(c[i], RCP(12.92)) : powf(mul_rn(add_rn(c[i], F32(0.055)), RCP(1.055)), F32(2.4));
    }
    const float r = blue ? c[2] : c[0], g = c[1], b = blue ? c[0] : c[2];
    const float X = mul_rn(add_rn(add_rn(mul_rn(F32(0.412453), r), mul_rn(F32(0.357580), g)), mul_rn(F32(0.180423), b)), RCP(0.950456));
    const float Y = add_rn(add_rn(mul_rn(F32(0.212671), r), mul_rn(F32(0.715160), g)), mul_rn(F32(0.072169), b));
    const float Z = mul_rn(add_rn(add_rn(mul_rn(F32(0.019334), r), mul_rn(F32(0.119193), g)), mul_rn(F32(0.950227), b)), RCP(1.088754));
    const float fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
    const float L = Y > F32(0.008856) ? sub_rn(mul_rn(116.0f, fy), 16.0f) : mul_rn(F32(903.3), Y);
    out[0] = to_u8(mul_rn(mul_rn(L, 255.0f), RCP(100.0)));
    out[1] = to_u8(add_rn(mul_rn(500.0f, sub_rn(fx, fy)), 128.0f));
    out[2] = to_u8(add_rn(mul_rn(200.0f, sub_rn(fy, fz)), 128.0f));
}

__device__ __forceinline__ float lab_inv(float f) {
    return f <= F32(6.0 / 29.0) ? mul_rn(sub_rn(f, F32(16.0 / 116.0)), RCP(7.787)) : mul_rn(mul_rn(f, f), f);
}

// imgproc.lab2rgb_u8
__device__ __forceinline__ void lab2rgb(const int in[3], bool linear, bool blue, int out[3]) {
    const float L = mul_rn(mul_rn((float)in[0], 100.0f), RCP(255.0));
    const float a = sub_rn((float)in[1], 128.0f), b = sub_rn((float)in[2], 128.0f);
    float fy = mul_rn(add_rn(L, 16.0f), RCP(116.0));
    const float Y = L <= 8.0f ? mul_rn(L, RCP(903.3)) : mul_rn(mul_rn(fy, fy), fy);
    fy = L <= 8.0f ? add_rn(mul_rn(F32(7.787), Y), F32(16.0 / 116.0)) : fy;
    const float fx = add_rn(fy, mul_rn(a, RCP(500.0))), fz = sub_rn(fy, mul_rn(b, RCP(200.0)));
    const float X = mul_rn(lab_inv(fx), F32(0.950456)), Z = mul_rn(lab_inv(fz), F32(1.088754));
    const float r = sub_rn(sub_rn(mul_rn(F32(3.240479), X), mul_rn(F32(1.537150), Y)), mul_rn(F32(0.498535), Z));
    const float g = add_rn(add_rn(mul_rn(F32(-0.969256), X), mul_rn(F32(1.875991), Y)), mul_rn(F32(0.041556), Z));
    const float bl = add_rn(sub_rn(mul_rn(F32(0.055648), X), mul_rn(F32(0.204043), Y)), mul_rn(F32(1.057311), Z));
    const float c3[3] = {blue ? bl : r, g, blue ? r : bl};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float c = c3[i] < 0.f ? 0.f : (c3[i] > 1.f ? 1.f : c3[i]);
        if (!linear)
            c = c <= F32(0.0031308) ? mul_rn(c, F32(12.92)) : sub_rn(mul_rn(F32(1.055), powf(fmaxf(c, F32(1e-12)), F32(1.0 / 2.4))), F32(0.055));
        out[i] = to_u8(mul_rn(c, 255.0f));
    }
}

__device__ __forceinline__ void lab_step(int mode, const int in[3], int out[3]) {
    const bool linear = mode & NESR_LAB_LINEAR, blue = mode & NESR_LAB_FIRST_IS_BLUE;
    if (mode & NESR_LAB_FROM_LAB) lab2rgb(in, linear, blue, out);
    else rgb2lab(in, linear, blue, out);
}

// one pixel per thread; channel c of pixel i at src[c][i * src_step] (HWC: step 3, planar: step 1 and one pointer per plane)
__global__ __launch_bounds__(256) void lab_kernel(LabArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    int v[3], w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = a.src[c][i * a.src_step];
    lab_step(a.mode0, v, w);
    if (a.mode1 >= 0) {                 // a second conversion on the u8 result, which stays in registers
        lab_step(a.mode1, w, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) w[c] = v[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.dst[c][i * a.dst_step] = (uint8_t)w[c];
}

__device__ __forceinline__ int reflect101(int p, int n) {        // imgproc._reflect101_index (any distance outside)
    if ((unsigned)p < (unsigned)n) return p;                      // inside: no division
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    p %= period;
    p = p < 0 ? p + period : p;
    return p >= n ? period - p : p;
}

__device__ __forceinline__ int round_shift16(int v) {             // (v + 2^15) >> 16, saturated to u8
    v = (v + (1 << 15)) >> 16;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// imgproc.gaussian_blur_u8: a GT_X x GT_Y output tile per workgroup; the tile and its r-pixel halo (BORDER_REFLECT_101) in LDS, the
// horizontal pass into 16-bit sums (taps sum to 256: a sum is at most 255 * 256), the vertical pass in int32, one rounding.
constexpr int GT_X = 64, GT_Y = 32, GR_MAX = GAUSS_MAX_RADIUS;

template <int C>
__global__ __launch_bounds__(256) void gaussian_kernel(const uint8_t* __restrict__ src, int H, int W, GaussTaps taps, uint8_t* __restrict__ dst) {
    __shared__ uint8_t in[GT_Y + 2 * GR_MAX][(GT_X + 2 * GR_MAX) * C];
    __shared__ uint16_t hs[GT_Y + 2 * GR_MAX][GT_X * C];
    __shared__ int kt[2 * GR_MAX + 1];
    const int tid = threadIdx.x, r = taps.r, nt = 2 * r + 1;
    const int x0 = blockIdx.x * GT_X, y0 = blockIdx.y * GT_Y;
    const int rows = GT_Y + 2 * r, cols = GT_X + 2 * r;
    if (tid == 0) {
#pragma unroll
        for (int t = 0; t < 2 * GR_MAX + 1; ++t) kt[t] = taps.k[t];
    }
    for (int i = tid; i < rows * cols; i += 256) {
        const int ly = i / cols, lx = i - ly * cols;
        const uint8_t* p = src + ((size_t)reflect101(y0 - r + ly, H) * W + reflect101(x0 - r + lx, W)) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) in[ly][lx * C + c] = p[c];
    }
    __syncthreads();
    for (int i = tid; i < rows * GT_X * C; i += 256) {
        const int ly = i / (GT_X * C), j = i - ly * (GT_X * C);
        int s = 0;
        for (int t = 0; t < nt; ++t) s += kt[t] * in[ly][j + t * C];
        hs[ly][j] = (uint16_t)s;
    }
    __syncthreads();
    for (int i = tid; i < GT_Y * GT_X * C; i += 256) {
        const int oy = i / (GT_X * C), j = i - oy * (GT_X * C);
        const int y = y0 + oy, x = x0 + j / C;
        if (y >= H || x >= W) continue;
        int s = 0;
        for (int t = 0; t < nt; ++t) s += kt[t] * (int)hs[oy + t][j];
        dst[((size_t)y * W + x) * C + (j - (j / C) * C)] = (uint8_t)round_shift16(s);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// imgproc.postprocess_image in one pass: a PT_X x PT_Y tile of the RGB frame with a 9-pixel halo in LDS (reflect 101); gray (integer
// weights) over the 6-pixel halo; 13-tap (sigma 2) blur of gray and 19-tap (sigma 3) blur of RGB as separable passes through LDS;
// detail = saturate(gray - blur_2(gray)); where detail > 10 the pixel becomes round(1.5 x - 0.5 blur_3(x)) (exact in float), else
// it stays.  One read and one write of the frame.
constexpr int PT_X = 64, PT_Y = 32, R2 = 6, R3 = 9;

//
// MASKED = true is the image half of _segment_and_enhance (nesr/nesr.py:735-747; imgproc.segment_enhance): the same unsharp value,
// selected where the 3 x 3 dilate of a {0, 1} mask [H][W] is 1 instead of where the detail exceeds 10 -- the dilate is the max over
// the neighbours inside the image (cv2's default border for a dilate never wins a max); no gray plane, no sigma 2 blur.
template <bool MASKED>
__global__ __launch_bounds__(256) void postprocess_kernel(const uint8_t* __restrict__ src, int H, int W, SharpenTaps taps, const uint8_t* __restrict__ mask,
                                                          uint8_t* __restrict__ dst) {
    __shared__ uint8_t rgb[PT_Y + 2 * R3][(PT_X + 2 * R3) * 3];
    __shared__ uint8_t gray[MASKED ? 1 : PT_Y + 2 * R2][MASKED ? 1 : PT_X + 2 * R2];
    __shared__ uint16_t h3[PT_Y + 2 * R3][PT_X * 3];
    __shared__ uint16_t h2[MASKED ? 1 : PT_Y + 2 * R2][MASKED ? 1 : PT_X];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * PT_X, y0 = blockIdx.y * PT_Y;
    constexpr int rows = PT_Y + 2 * R3, cols = PT_X + 2 * R3;
    for (int i = tid; i < rows * cols; i += 256) {
        const int ly = i / cols, lx = i - ly * cols;
        const uint8_t* p = src + ((size_t)reflect101(y0 - R3 + ly, H) * W + reflect101(x0 - R3 + lx, W)) * 3;
        rgb[ly][lx * 3 + 0] = p[0];
        rgb[ly][lx * 3 + 1] = p[1];
        rgb[ly][lx * 3 + 2] = p[2];
    }
    __syncthreads();
    constexpr int grows = PT_Y + 2 * R2, gcols = PT_X + 2 * R2, d = R3 - R2;
    if constexpr (!MASKED) {
        for (int i = tid; i < grows * gcols; i += 256) {      // imgproc.rgb2gray_u8 (gray of a reflected pixel = reflected gray)
            const int ly = i / gcols, lx = i - ly * gcols;
            const uint8_t* p = &rgb[ly + d][(lx + d) * 3];
            gray[ly][lx] = (uint8_t)(((int)p[0] * 4899 + (int)p[1] * 9617 + (int)p[2] * 1868 + (1 << 13)) >> 14);
        }
    }
    for (int i = tid; i < rows * PT_X * 3; i += 256) {
        const int ly = i / (PT_X * 3), j = i - ly * (PT_X * 3);
        int s = 0;
#pragma unroll
        for (int t = 0; t < 2 * R3 + 1; ++t) s += taps.k3[t] * (int)rgb[ly][j + t * 3];
        h3[ly][j] = (uint16_t)s;
    }
    __syncthreads();
    if constexpr (!MASKED) {
        for (int i = tid; i < grows * PT_X; i += 256) {
            const int ly = i / PT_X, j = i - ly * PT_X;
            int s = 0;
#pragma unroll
            for (int t = 0; t < 2 * R2 + 1; ++t) s += taps.k2[t] * (int)gray[ly][j + t];
            h2[ly][j] = (uint16_t)s;
        }
        __syncthreads();
    }
    const int ox = tid & (PT_X - 1), x = x0 + ox;
    for (int oy = tid / PT_X; oy < PT_Y; oy += 256 / PT_X) {
        const int y = y0 + oy;
        if (y >= H || x >= W) continue;
        bool sharpen;
        if constexpr (MASKED) {
            int m = 0;
            for (int yy = max(y - 1, 0); yy <= min(y + 1, H - 1); ++yy)
                for (int xx = max(x - 1, 0); xx <= min(x + 1, W - 1); ++xx) m = max(m, (int)mask[(size_t)yy * W + xx]);
            sharpen = m == 1;
        } else {
            int s2 = 0;
#pragma unroll
            for (int t = 0; t < 2 * R2 + 1; ++t) s2 += taps.k2[t] * (int)h2[oy + t][ox];
            const int detail = (int)gray[oy + R2][ox + R2] - round_shift16(s2);     // saturate(gray - blur): only > 10 matters
            sharpen = detail > 10;
        }
        uint8_t* q = dst + ((size_t)y * W + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int v = rgb[oy + R3][(ox + R3) * 3 + c];
            if (sharpen) {
                int s3 = 0;
#pragma unroll
                for (int t = 0; t < 2 * R3 + 1; ++t) s3 += taps.k3[t] * (int)h3[oy + t][ox * 3 + c];
                q[c] = (uint8_t)to_u8((float)v * 1.5f - (float)round_shift16(s3) * 0.5f);      // exact: no rounding before rintf
            } else {
                q[c] = (uint8_t)v;
            }
        }
    }
}

// imgproc.ensemble_results on equal shapes: acc = fl32(acc + fl32(fl32(x) w)) over the images in order, truncated.  VEC: every
// pointer is 16-byte aligned -- a thread takes 16 bytes of each image with one load and stores 16; the < 16 tail bytes go to the
// threads after the last vector, one byte each.  Else one byte per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void ensemble_kernel(EnsembleArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nvec = VEC ? a.total / 16 : 0;
    if (VEC && i < nvec) {
        float acc[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] = 0.0f;
        for (int k = 0; k < a.n; ++k) {
            const uint4 v = reinterpret_cast<const uint4*>(a.img[k])[i];
            const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int b = 0; b < 16; ++b) acc[b] = add_rn(acc[b], mul_rn((float)((w4[b >> 2] >> (8 * (b & 3))) & 255u), a.w));
        }
        unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) o[b >> 2] |= ((unsigned)(int)acc[b] & 255u) << (8 * (b & 3));
        reinterpret_cast<uint4*>(a.out)[i] = make_uint4(o[0], o[1], o[2], o[3]);
        return;
    }
    const size_t j = nvec * 16 + (i - nvec);
    if (j >= a.total) return;
    float acc = 0.0f;
    for (int k = 0; k < a.n; ++k) acc = add_rn(acc, mul_rn((float)a.img[k][j], a.w));
    a.out[j] = (uint8_t)(int)acc;
}

}  // namespace

hipError_t launch_ensemble(const EnsembleArgs& a, hipStream_t s) {
    if (a.n < 1 || a.n > ENSEMBLE_MAX) return hipErrorInvalidValue;
    if (a.total == 0) return hipSuccess;
    uintptr_t bits = reinterpret_cast<uintptr_t>(a.out);
    for (int k = 0; k < a.n; ++k) bits |= reinterpret_cast<uintptr_t>(a.img[k]);
    const bool vec = (bits & 15) == 0;
    const size_t threads = vec ? a.total / 16 + a.total % 16 : a.total;
    const size_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL(ensemble_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(ensemble_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lab(const LabArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(lab_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gaussian(const uint8_t* src, int H, int W, int C, const GaussTaps& taps, uint8_t* dst, hipStream_t s) {
    if (taps.r < 0 || taps.r > GAUSS_MAX_RADIUS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((W + GT_X - 1) / GT_X), (unsigned)((H + GT_Y - 1) / GT_Y));
    if (C == 1) hipLaunchKernelGGL(gaussian_kernel<1>, grid, dim3(256), 0, s, src, H, W, taps, dst);
    else if (C == 3) hipLaunchKernelGGL(gaussian_kernel<3>, grid, dim3(256), 0, s, src, H, W, taps, dst);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_postprocess(const uint8_t* src, int H, int W, const SharpenTaps& taps, uint8_t* dst, hipStream_t s) {
    const dim3 grid((unsigned)((W + PT_X - 1) / PT_X), (unsigned)((H + PT_Y - 1) / PT_Y));
    hipLaunchKernelGGL(postprocess_kernel<false>, grid, dim3(256), 0, s, src, H, W, taps, static_cast<const uint8_t*>(nullptr), dst);
    return hipGetLastError();
}

hipError_t launch_segment_sharpen(const uint8_t* src, int H, int W, const SharpenTaps& taps, const uint8_t* mask, uint8_t* dst, hipStream_t s) {
    const dim3 grid((unsigned)((W + PT_X - 1) / PT_X), (unsigned)((H + PT_Y - 1) / PT_Y));
    hipLaunchKernelGGL(postprocess_kernel<true>, grid, dim3(256), 0, s, src, H, W, taps, mask, dst);
    return hipGetLastError();
}

}  // namespace nesr
