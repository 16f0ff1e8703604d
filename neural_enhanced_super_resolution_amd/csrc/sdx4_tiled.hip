// The x4 diffusion upscaler over windows, for gfx950: what stands between the networks when the denoising loop and the VAE decode
// run on overlapping windows of one shape (sdx4_api.cpp: nesr_sdx4_upscale_tiled_u8; vae_api.cpp: the tiled decode).  Five
// elementwise kernels; tests/sdx4_tiled_ref.py restates their indexing and their weights.
//
//   sdx4_gather_kernel       the window [n][channels][ty][tx] out of the full-frame buffer [channels][H][W], every sample the same:
//                            the UNet's input of a window (latents and noised image), or the window's latents for the VAE
//   sdx4_accumulate_kernel   m = neg + g (prompt - neg) (n = 2) of the window's model output; acc = fmaf(w, m, acc) at the window's
//                            place in the accumulator [lc][H][W].  Windows run one after the other on one stream: no atomics
//   sdx4_tiled_step_kernel   m = acc / (Sy Sx), sdx4_step_kernel's fmaf chain on the full-frame latents, acc <- 0
//   sdx4_blend_add_kernel    acc = fmaf(w, sample, acc): the VAE's f32 window [3][ty s][tx s] into the f32 frame [H s][W s][3]
//   sdx4_blend_finish_kernel acc / (Sy Sx), then the VAE epilogue's / 2 + 0.5, clamp, x 255, round half to even -> u8 [H s][W s][3]
//
// The weight of a window is separable, w = wy wx, and so is the normaliser S = Sy Sx (sdx4_api.h: Sdx4Axis): both are computed from
// the axis's four integers, no weight plane is stored.  With one window w = 1 and S = 1, and every kernel hands its value through
// unchanged: the tiled call then returns the untiled call's bits.
//
// A window's origin is only a multiple of the frame multiple, which may be 2, so a thread takes 2 adjacent pixels: 8-byte vector
// loads and stores, every one inside the extents the launcher checked.  The finish kernel works on whole rows of the frame (their
// length is a multiple of 4) and takes 4 pixels: three 16-byte loads, three 4-byte stores.
#include "sdx4_api.h"

namespace nesr {
namespace {

__device__ __forceinline__ float2 ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }
__device__ __forceinline__ void st2(float* p, float2 v) { *reinterpret_cast<float2*>(p) = v; }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// the weight of pixel i in the window at origin a; the sides on the frame's edge are not ramped
__device__ __forceinline__ float axis_weight(const Sdx4Axis& x, int a, int i) {
    float left = 1.0f, right = 1.0f;
    if (x.r > 0) {
        if (a > 0) left = (float)min(i - a + 1, x.r) / (float)x.r;
        if (a + x.t < x.n) right = (float)min(a + x.t - i, x.r) / (float)x.r;
    }
    return fminf(left, right);
}

// the sum of axis_weight over the windows that cover i, in ascending order of their origins: those on the stride, then the last
__device__ __forceinline__ float axis_sum(const Sdx4Axis& x, int i) {
    const int stride = x.t - x.r, last = x.n - x.t;
    const int strided = (last + stride - 1) / stride;      // origins 0, stride, ... below `last`
    const int first = i - x.t + 1 > 0 ? (i - x.t + stride) / stride : 0;
    const int end = min(i / stride, strided - 1);
    float s = 0.0f;
    for (int k = first; k <= end; ++k) s += axis_weight(x, k * stride, i);
    if (i >= last) s += axis_weight(x, last, i);
    return s;
}

// q -> (plane, row, first of 2 columns) of [planes][rows][2 half]
__device__ __forceinline__ void split(size_t q, int half, int rows, int& plane, int& row, int& col) {
    col = (int)(q % half) * 2;
    const size_t r = q / half;
    row = (int)(r % rows), plane = (int)(r / rows);
}

__global__ __launch_bounds__(256) void sdx4_gather_kernel(const Sdx4Gather a) {
    const int half = a.x.t / 2;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)a.channels * a.y.t * half) return;
    int c, y, x;
    split(q, half, a.y.t, c, y, x);
    const float2 v = ld2(a.src + ((size_t)c * a.y.n + a.y.a + y) * a.x.n + a.x.a + x);
    const size_t plane = (size_t)a.y.t * a.x.t;
    for (int s = 0; s < a.n; ++s) st2(a.dst + ((size_t)s * a.channels + c) * plane + (size_t)y * a.x.t + x, v);
}

__global__ __launch_bounds__(256) void sdx4_accumulate_kernel(const Sdx4Accumulate a) {
    const int half = a.x.t / 2;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)a.lc * a.y.t * half) return;
    int c, y, x;
    split(q, half, a.y.t, c, y, x);
    const size_t plane = (size_t)a.y.t * a.x.t, at = (size_t)c * plane + (size_t)y * a.x.t + x;
    float2 m = ld2(a.model + at);
    if (a.n == 2) {
        const float2 p = ld2(a.model + (size_t)a.lc * plane + at);
        m.x = fmaf(a.g, p.x - m.x, m.x), m.y = fmaf(a.g, p.y - m.y, m.y);
    }
    const float wy = axis_weight(a.y, a.y.a, a.y.a + y);
    const float w0 = wy * axis_weight(a.x, a.x.a, a.x.a + x), w1 = wy * axis_weight(a.x, a.x.a, a.x.a + x + 1);
    float* dst = a.acc + ((size_t)c * a.y.n + a.y.a + y) * a.x.n + a.x.a + x;
    float2 v = ld2(dst);
    v.x = fmaf(w0, m.x, v.x), v.y = fmaf(w1, m.y, v.y);
    st2(dst, v);
}

__device__ __forceinline__ float tiled_step_one(const Sdx4TiledStep& a, float x, float m) {
    const float x0 = fmaf(a.c0x, x, a.c0m * m), e = fmaf(a.cex, x, a.cem * m);
    return fmaf(a.sp, x0, a.sq * e);
}

__global__ __launch_bounds__(256) void sdx4_tiled_step_kernel(const Sdx4TiledStep a) {
    const int half = a.x.n / 2;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)a.lc * a.y.n * half) return;
    int c, y, x;
    split(q, half, a.y.n, c, y, x);
    const size_t at = ((size_t)c * a.y.n + y) * a.x.n + x;
    const float sy = axis_sum(a.y, y);
    const float s0 = sy * axis_sum(a.x, x), s1 = sy * axis_sum(a.x, x + 1);
    const float2 acc = ld2(a.acc + at), lat = ld2(a.frame + at);
    st2(a.frame + at, make_float2(tiled_step_one(a, lat.x, acc.x / s0), tiled_step_one(a, lat.y, acc.y / s1)));
    st2(a.acc + at, make_float2(0.0f, 0.0f));
}

__global__ __launch_bounds__(256) void sdx4_blend_add_kernel(const Sdx4BlendAdd a) {
    const int half = a.x.t / 2;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)a.y.t * half) return;
    const int x = (int)(q % half) * 2, y = (int)(q / half);
    const size_t plane = (size_t)a.y.t * a.x.t, at = (size_t)y * a.x.t + x;
    const float2 r = ld2(a.sample + at), g = ld2(a.sample + plane + at), b = ld2(a.sample + 2 * plane + at);
    const float wy = axis_weight(a.y, a.y.a, a.y.a + y);
    const float w0 = wy * axis_weight(a.x, a.x.a, a.x.a + x), w1 = wy * axis_weight(a.x, a.x.a, a.x.a + x + 1);
    float* dst = a.acc + ((size_t)(a.y.a + y) * a.x.n + a.x.a + x) * 3;      // r g | b r | g b of two pixels
    float2 v0 = ld2(dst), v1 = ld2(dst + 2), v2 = ld2(dst + 4);
    v0.x = fmaf(w0, r.x, v0.x), v0.y = fmaf(w0, g.x, v0.y), v1.x = fmaf(w0, b.x, v1.x);
    v1.y = fmaf(w1, r.y, v1.y), v2.x = fmaf(w1, g.y, v2.x), v2.y = fmaf(w1, b.y, v2.y);
    st2(dst, v0), st2(dst + 2, v1), st2(dst + 4, v2);
}

__device__ __forceinline__ uint32_t quantise(float v, float s) {
    v = fminf(fmaxf(v / s / 2.0f + 0.5f, 0.f), 1.f) * 255.0f;
    return (uint32_t)(uint8_t)rintf(v);
}

__global__ __launch_bounds__(256) void sdx4_blend_finish_kernel(const Sdx4BlendFinish a) {
    const int quarter = a.x.n / 4;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)a.y.n * quarter) return;
    const int x = (int)(q % quarter) * 4, y = (int)(q / quarter);
    const size_t at = ((size_t)y * a.x.n + x) * 3;
    const float4 f0 = ld4(a.acc + at), f1 = ld4(a.acc + at + 4), f2 = ld4(a.acc + at + 8);      // r g b r | g b r g | b r g b
    const float sy = axis_sum(a.y, y);
    const float s0 = sy * axis_sum(a.x, x), s1 = sy * axis_sum(a.x, x + 1), s2 = sy * axis_sum(a.x, x + 2), s3 = sy * axis_sum(a.x, x + 3);
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out + at);
    out[0] = quantise(f0.x, s0) | quantise(f0.y, s0) << 8 | quantise(f0.z, s0) << 16 | quantise(f0.w, s1) << 24;
    out[1] = quantise(f1.x, s1) | quantise(f1.y, s1) << 8 | quantise(f1.z, s2) << 16 | quantise(f1.w, s2) << 24;
    out[2] = quantise(f2.x, s2) | quantise(f2.y, s3) << 8 | quantise(f2.z, s3) << 16 | quantise(f2.w, s3) << 24;
}

bool aligned(const void* p, size_t to) { return p && (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
// an axis the kernels may index: even lengths, the window inside the frame, a ramp shorter than the window
bool axis_ok(const Sdx4Axis& x, bool window) {
    if (x.n < 2 || x.n > (1 << 24) || x.n % 2 || x.t < 2 || x.t > x.n || x.t % 2 || x.r < 0 || x.r >= x.t) return false;
    return !window || (x.a >= 0 && x.a % 2 == 0 && x.a <= x.n - x.t);
}
bool frame_ok(const Sdx4Axis& y, const Sdx4Axis& x, int planes) { return (long long)y.n * x.n * planes <= (1ll << 30); }
unsigned blocks(size_t threads) { return (unsigned)((threads + 255) / 256); }

}  // namespace

hipError_t launch_sdx4_gather(const Sdx4Gather& a, hipStream_t s) {
    if (a.n < 1 || a.n > 2 || a.channels < 1 || a.channels > SDX4_MAX_LATENT_CHANNELS + SDX4_IMAGE_CHANNELS || !axis_ok(a.y, true) || !axis_ok(a.x, true) ||
        !frame_ok(a.y, a.x, a.channels) || !aligned(a.src, 8) || !aligned(a.dst, 8))
        return hipErrorInvalidValue;
    sdx4_gather_kernel<<<dim3(blocks((size_t)a.channels * a.y.t * (a.x.t / 2))), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_sdx4_accumulate(const Sdx4Accumulate& a, hipStream_t s) {
    if (a.n < 1 || a.n > 2 || a.lc < 1 || a.lc > SDX4_MAX_LATENT_CHANNELS || !axis_ok(a.y, true) || !axis_ok(a.x, true) || !frame_ok(a.y, a.x, a.lc) || !aligned(a.model, 8) ||
        !aligned(a.acc, 8) || !(a.g == a.g))
        return hipErrorInvalidValue;
    sdx4_accumulate_kernel<<<dim3(blocks((size_t)a.lc * a.y.t * (a.x.t / 2))), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_sdx4_tiled_step(const Sdx4TiledStep& a, hipStream_t s) {
    if (a.lc < 1 || a.lc > SDX4_MAX_LATENT_CHANNELS || !axis_ok(a.y, false) || !axis_ok(a.x, false) || !frame_ok(a.y, a.x, a.lc + SDX4_IMAGE_CHANNELS) || !aligned(a.acc, 8) ||
        !aligned(a.frame, 8))
        return hipErrorInvalidValue;
    for (float v : {a.c0x, a.c0m, a.cex, a.cem, a.sp, a.sq})
        if (!(v == v)) return hipErrorInvalidValue;
    sdx4_tiled_step_kernel<<<dim3(blocks((size_t)a.lc * a.y.n * (a.x.n / 2))), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_sdx4_blend_add(const Sdx4BlendAdd& a, hipStream_t s) {
    if (!axis_ok(a.y, true) || !axis_ok(a.x, true) || !frame_ok(a.y, a.x, 3) || !aligned(a.sample, 8) || !aligned(a.acc, 8)) return hipErrorInvalidValue;
    sdx4_blend_add_kernel<<<dim3(blocks((size_t)a.y.t * (a.x.t / 2))), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_sdx4_blend_finish(const Sdx4BlendFinish& a, hipStream_t s) {
    if (!axis_ok(a.y, false) || !axis_ok(a.x, false) || a.x.n % 4 || !frame_ok(a.y, a.x, 3) || !aligned(a.acc, 16) || !aligned(a.out, 4)) return hipErrorInvalidValue;
    sdx4_blend_finish_kernel<<<dim3(blocks((size_t)a.y.n * (a.x.n / 4))), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace nesr
