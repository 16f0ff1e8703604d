// The arithmetic between the networks of the x4 diffusion upscaler (StableDiffusionUpscalePipeline's loop) for gfx950: the
// low-res scheduler's add_noise on the input frame, the initial latents, classifier-free guidance and the DDIM step.  Two kernels,
// each one read and one write of small tensors, both writing straight into the UNet's NCHW input [n][lc + 3][hw] so that
// cat(latents, image) is never stored.  tests/sdx4_kernel_ref.py restates their indexing.
//
//   sdx4_prepare_kernel   a thread takes 4 pixels of every plane: u8 RGB -> v / 127.5 - 1 -> sa x + sb noise into channels lc .. lc + 2
//                         of every sample; sigma latents into channels 0 .. lc - 1 of every sample and into the latents buffer.
//   sdx4_step_kernel      a thread takes 4 values of the latents: m = neg + g (prompt - neg) (n = 2), x0 = c0x x + c0m m,
//                         e = cex x + cem m, x' = sp x0 + sq e into the latents buffer and channels 0 .. lc - 1 of every sample.
//                         The six coefficients are the host's (v-prediction or epsilon), rounded once from double.
//
// 16 bytes a thread (hw is a multiple of 4: h and w are even), vector loads and stores only, every one guarded by the plane's extent.
// The products are written as explicit fmaf chains: the order of the roundings is this file's, not the compiler's.
#include "sdx4_api.h"

namespace nesr {
namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

__global__ __launch_bounds__(256) void sdx4_prepare_kernel(const Sdx4Prepare a) {
    const int q = blockIdx.x * 256 + threadIdx.x;      // pixels 4 q .. 4 q + 3
    if (q * 4 >= a.hw) return;
    const int p = q * 4, planes = a.lc + SDX4_IMAGE_CHANNELS;
    const uint32_t* f = reinterpret_cast<const uint32_t*>(a.frame + (size_t)p * 3);      // 12 bytes: r g b r | g b r g | b r g b
    const uint32_t w0 = f[0], w1 = f[1], w2 = f[2];
    const uint32_t px[4][3] = {{w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u}, {w0 >> 24, w1 & 255u, (w1 >> 8) & 255u},
                               {(w1 >> 16) & 255u, w1 >> 24, w2 & 255u}, {(w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24}};
#pragma unroll
    for (int c = 0; c < SDX4_IMAGE_CHANNELS; ++c) {
        const float4 nz = ld4(a.noise + (size_t)c * a.hw + p);
        float4 v;
        v.x = fmaf(a.sa, (float)px[0][c] / 127.5f - 1.0f, a.sb * nz.x), v.y = fmaf(a.sa, (float)px[1][c] / 127.5f - 1.0f, a.sb * nz.y);
        v.z = fmaf(a.sa, (float)px[2][c] / 127.5f - 1.0f, a.sb * nz.z), v.w = fmaf(a.sa, (float)px[3][c] / 127.5f - 1.0f, a.sb * nz.w);
        for (int s = 0; s < a.n; ++s) st4(a.sample + ((size_t)s * planes + a.lc + c) * a.hw + p, v);
    }
    for (int k = 0; k < a.lc; ++k) {
        const float4 l = ld4(a.latents + (size_t)k * a.hw + p);
        const float4 v = make_float4(a.sigma * l.x, a.sigma * l.y, a.sigma * l.z, a.sigma * l.w);
        st4(a.lat_out + (size_t)k * a.hw + p, v);
        for (int s = 0; s < a.n; ++s) st4(a.sample + ((size_t)s * planes + k) * a.hw + p, v);
    }
}

__device__ __forceinline__ float sdx4_step_one(const Sdx4Step& a, float x, float m0, float m1) {
    const float m = a.n == 2 ? fmaf(a.g, m1 - m0, m0) : m0;
    const float x0 = fmaf(a.c0x, x, a.c0m * m), e = fmaf(a.cex, x, a.cem * m);
    return fmaf(a.sp, x0, a.sq * e);
}

__global__ __launch_bounds__(256) void sdx4_step_kernel(const Sdx4Step a) {
    const size_t count = (size_t)a.lc * a.hw, i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;      // 4 values of [lc][hw]
    if (i >= count) return;
    const float4 x = ld4(a.latents + i), m0 = ld4(a.model + i), m1 = a.n == 2 ? ld4(a.model + count + i) : m0;
    const float4 v = make_float4(sdx4_step_one(a, x.x, m0.x, m1.x), sdx4_step_one(a, x.y, m0.y, m1.y), sdx4_step_one(a, x.z, m0.z, m1.z),
                                 sdx4_step_one(a, x.w, m0.w, m1.w));
    st4(a.lat_out + i, v);
    const size_t stride = (size_t)(a.lc + SDX4_IMAGE_CHANNELS) * a.hw;      // the latents are the first lc planes of a sample
    for (int s = 0; s < a.n; ++s) st4(a.sample + s * stride + i, v);
}

bool aligned(const void* p, size_t to) { return p && (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
bool extent_ok(int n, int hw, int lc) { return n >= 1 && n <= 2 && hw >= 4 && hw % 4 == 0 && hw <= (1 << 24) && lc >= 1 && lc <= SDX4_MAX_LATENT_CHANNELS; }

}  // namespace

hipError_t launch_sdx4_prepare(const Sdx4Prepare& a, hipStream_t s) {
    if (!extent_ok(a.n, a.hw, a.lc) || !aligned(a.frame, 4) || !aligned(a.noise, 16) || !aligned(a.latents, 16) || !aligned(a.sample, 16) || !aligned(a.lat_out, 16))
        return hipErrorInvalidValue;
    if (!(a.sa == a.sa) || !(a.sb == a.sb) || !(a.sigma == a.sigma)) return hipErrorInvalidValue;
    sdx4_prepare_kernel<<<dim3((a.hw / 4 + 255) / 256), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_sdx4_step(const Sdx4Step& a, hipStream_t s) {
    if (!extent_ok(a.n, a.hw, a.lc) || !aligned(a.model, 16) || !aligned(a.latents, 16) || !aligned(a.sample, 16) || !aligned(a.lat_out, 16)) return hipErrorInvalidValue;
    for (float v : {a.g, a.c0x, a.c0m, a.cex, a.cem, a.sp, a.sq})
        if (!(v == v)) return hipErrorInvalidValue;
    sdx4_step_kernel<<<dim3((unsigned)(((size_t)a.lc * a.hw / 4 + 255) / 256)), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace nesr
