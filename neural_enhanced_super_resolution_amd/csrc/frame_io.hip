// Whole frames at the edges of RealESRGANer.enhance, for every kind of frame it takes besides 8-bit BGR (HBM-bound, one pass each).
//
// pack_frame: enhance()'s host preparation (realesrgan utils.py, RealESRGANer.enhance): `img.astype(np.float32) / max_range`,
//   cv2.cvtColor GRAY2RGB (gray replicated) or BGR2RGB (colour flipped), HWC -> CHW; for BGRA the alpha samples as well, either
//   GRAY2RGB'd for a second pass through the network or as one plane for cv2.resize(alpha, INTER_LINEAR).
// unpack_frame: what enhance() does with the network's output: `.float().clamp_(0, 1)`, `[[2, 1, 0]]` and CHW -> HWC, cv2.cvtColor
//   BGR2GRAY for gray frames and for a network-upsampled alpha, `(x * max_range).round().astype(uint8 | uint16)`.
// Every product and sum is rounded by itself (mul_rn / add_rn), as numpy's separate operations are, so both are bit for bit
// frame_io.py's torch chains and the numpy lines they restate.
//
// A thread owns four neighbouring pixels of a row.  When every pointer and pitch allows it (`vec`) the samples move as 32-bit to
// 128-bit words and the planes as float4; otherwise one sample and one float at a time.
#include "nesr_kernels.h"

namespace nesr {
namespace {

template <int NW>
__device__ inline void load_words(const unsigned char* p, int al, uint32_t* w) {
    if constexpr (NW % 4 == 0) {
        if (al >= 16) {
#pragma unroll
            for (int i = 0; i < NW / 4; ++i) {
                const uint4 v = reinterpret_cast<const uint4*>(p)[i];
                w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
            }
            return;
        }
    }
    if constexpr (NW % 2 == 0) {
        if (al >= 8) {
#pragma unroll
            for (int i = 0; i < NW / 2; ++i) {
                const uint2 v = reinterpret_cast<const uint2*>(p)[i];
                w[2 * i] = v.x; w[2 * i + 1] = v.y;
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
}

template <int NW>
__device__ inline void store_words(unsigned char* p, int al, const uint32_t* w) {
    if constexpr (NW % 4 == 0) {
        if (al >= 16) {
#pragma unroll
            for (int i = 0; i < NW / 4; ++i) reinterpret_cast<uint4*>(p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
            return;
        }
    }
    if constexpr (NW % 2 == 0) {
        if (al >= 8) {
#pragma unroll
            for (int i = 0; i < NW / 2; ++i) reinterpret_cast<uint2*>(p)[i] = make_uint2(w[2 * i], w[2 * i + 1]);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) reinterpret_cast<uint32_t*>(p)[i] = w[i];
}

// sample k of a run of S-byte samples held as little-endian 32-bit words
template <int S>
__device__ inline unsigned word_sample(const uint32_t* w, int k) {
    return S == 1 ? (w[k / 4] >> (8 * (k % 4))) & 255u : (w[k / 2] >> (16 * (k % 2))) & 65535u;
}

// S = bytes per sample, C = samples per pixel; al = what the source rows are aligned to (vec only)
template <int S, int C>
__global__ __launch_bounds__(256) void pack_frame_kernel(FramePack p, int vec, int al) {
    const int groups = (p.W + 3) / 4;
    const size_t total = (size_t)p.H * groups, plane = (size_t)p.H * p.W;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (size_t)y * groups) * 4;
        const int n = p.W - x0 < 4 ? p.W - x0 : 4;
        const unsigned char* row = p.src + (size_t)y * p.src_pitch + (size_t)x0 * C * S;
        unsigned q[4 * C];
        if (vec) {
            uint32_t w[C * S];
            load_words<C * S>(row, al, w);
#pragma unroll
            for (int k = 0; k < 4 * C; ++k) q[k] = word_sample<S>(w, k);
        } else {
#pragma unroll
            for (int k = 0; k < 4 * C; ++k)
                q[k] = k < n * C ? (S == 1 ? (unsigned)row[k] : (unsigned)reinterpret_cast<const uint16_t*>(row)[k]) : 0u;
        }
        float v[4 * C], h[4 * C];      // v: img / max_range; h: the same through fp16 (`self.img.half()`) when asked
#pragma unroll
        for (int k = 0; k < 4 * C; ++k) {
            v[k] = (float)q[k] / p.max_range;
            h[k] = p.through_fp16 ? (float)(_Float16)v[k] : v[k];
        }
        const size_t at = (size_t)y * p.W + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cs = C == 1 ? 0 : 2 - c;     // gray: replicated; colour: BGR -> RGB
            float* d = p.image + c * plane + at;
            if (vec) *reinterpret_cast<float4*>(d) = make_float4(h[cs], h[C + cs], h[2 * C + cs], h[3 * C + cs]);
            else
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n) d[i] = h[i * C + cs];
        }
        if (C == 4 && p.alpha) {
            const bool one = p.alpha_form == FRAME_ALPHA_PLANE;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (one && c) break;
                float* d = p.alpha + c * plane + at;
                const float* a = one ? v : h;
                if (vec) *reinterpret_cast<float4*>(d) = make_float4(a[C - 1], a[2 * C - 1], a[3 * C - 1], a[4 * C - 1]);
                else
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < n) d[i] = a[i * C + C - 1];
            }
        }
    }
}

__device__ inline float unit(float v, int through_fp16) {
    if (through_fp16) v = (float)(_Float16)v;      // RealESRGANer(half=True): the network's output is an fp16 tensor upstream
    return fminf(fmaxf(v, 0.f), 1.f);
}
// cv2.COLOR_BGR2GRAY on float32 as enhance() restates it: b 0.114 + g 0.587 + r 0.299, left to right, nothing contracted
__device__ inline float gray(float r, float g, float b) {
    return add_rn(add_rn(mul_rn(b, 0.114f), mul_rn(g, 0.587f)), mul_rn(r, 0.299f));
}

__device__ inline void load4(const float* p, int n, bool vec, float* o) {
    if (vec) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = i < n ? p[i] : 0.f;
    }
}

// S = bytes per sample of the finished frame, C = its samples per pixel; al = what the destination rows are aligned to (vec only)
template <int S, int C>
__global__ __launch_bounds__(256) void unpack_frame_kernel(FrameUnpack u, int vec, int al) {
    const int groups = (u.W + 3) / 4;
    const size_t total = (size_t)u.H * groups;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (size_t)y * groups) * 4;
        const int n = u.W - x0 < 4 ? u.W - x0 : 4;
        float rgb[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            load4(u.image + c * u.image_plane + (size_t)y * u.image_row + x0, n, vec, rgb[c]);
#pragma unroll
            for (int i = 0; i < 4; ++i) rgb[c][i] = unit(rgb[c][i], u.through_fp16);
        }
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (C == 4) {
            if (u.alpha_form == FRAME_ALPHA_PLANE) {
                load4(u.alpha + (size_t)y * u.alpha_row + x0, n, vec, a);
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = unit(a[i], 0);
            } else {
                float t[3][4];
#pragma unroll
                for (int c = 0; c < 3; ++c) load4(u.alpha + c * u.alpha_plane + (size_t)y * u.alpha_row + x0, n, vec, t[c]);
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = gray(unit(t[0][i], u.through_fp16), unit(t[1][i], u.through_fp16), unit(t[2][i], u.through_fp16));
            }
        }
        unsigned q[4 * C];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (C == 1) {
                q[i] = (unsigned)rintf(mul_rn(gray(rgb[0][i], rgb[1][i], rgb[2][i]), u.max_range));
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) q[i * C + c] = (unsigned)rintf(mul_rn(rgb[2 - c][i], u.max_range));     // RGB -> BGR
                if (C == 4) q[i * C + 3] = (unsigned)rintf(mul_rn(a[i], u.max_range));
            }
        }
        unsigned char* row = u.dst + (size_t)y * u.dst_pitch + (size_t)x0 * C * S;
        if (vec) {
            uint32_t w[C * S];
#pragma unroll
            for (int k = 0; k < C * S; ++k)
                w[k] = S == 1 ? (q[4 * k] & 255u) | (q[4 * k + 1] & 255u) << 8 | (q[4 * k + 2] & 255u) << 16 | (q[4 * k + 3] & 255u) << 24
                              : (q[2 * k] & 65535u) | (q[2 * k + 1] & 65535u) << 16;
            store_words<C * S>(row, al, w);
        } else {
#pragma unroll
            for (int k = 0; k < 4 * C; ++k)
                if (k < n * C) {
                    if (S == 1) row[k] = (unsigned char)q[k];
                    else reinterpret_cast<uint16_t*>(row)[k] = (uint16_t)q[k];
                }
        }
    }
}

int blocks_for(int H, int W) {
    const size_t total = (size_t)H * ((W + 3) / 4);
    const size_t b = (total + 255) / 256;
    return (int)(b > 8192 ? 8192 : b);
}
int align_of(uintptr_t bits) { return (bits & 15) == 0 ? 16 : ((bits & 7) == 0 ? 8 : 4); }

}  // namespace

#define FRAME_LAUNCH(kernel, S_, C_) hipLaunchKernelGGL((kernel<S_, C_>), dim3(blocks_for(a.H, a.W)), dim3(256), 0, s, a, vec, al)
#define FRAME_DISPATCH(kernel)                                         \
    do {                                                               \
        if (a.bytes == 1 && a.C == 1) FRAME_LAUNCH(kernel, 1, 1);      \
        else if (a.bytes == 1 && a.C == 3) FRAME_LAUNCH(kernel, 1, 3); \
        else if (a.bytes == 1 && a.C == 4) FRAME_LAUNCH(kernel, 1, 4); \
        else if (a.bytes == 2 && a.C == 1) FRAME_LAUNCH(kernel, 2, 1); \
        else if (a.bytes == 2 && a.C == 3) FRAME_LAUNCH(kernel, 2, 3); \
        else if (a.bytes == 2 && a.C == 4) FRAME_LAUNCH(kernel, 2, 4); \
        else return hipErrorInvalidValue;                              \
    } while (0)

hipError_t launch_pack_frame(const FramePack& a, hipStream_t s) {
    if (a.H <= 0 || a.W <= 0) return hipSuccess;
    const uintptr_t src = reinterpret_cast<uintptr_t>(a.src) | (uintptr_t)a.src_pitch;
    const bool alpha = a.C == 4 && a.alpha;
    const int vec = a.W % 4 == 0 && (src & 3) == 0 && (reinterpret_cast<uintptr_t>(a.image) & 15) == 0 &&
                    (!alpha || (reinterpret_cast<uintptr_t>(a.alpha) & 15) == 0);
    const int al = align_of(src);
    FRAME_DISPATCH(pack_frame_kernel);
    return hipGetLastError();
}

hipError_t launch_unpack_frame(const FrameUnpack& a, hipStream_t s) {
    if (a.H <= 0 || a.W <= 0) return hipSuccess;
    const uintptr_t dst = reinterpret_cast<uintptr_t>(a.dst) | (uintptr_t)a.dst_pitch;
    uintptr_t in = reinterpret_cast<uintptr_t>(a.image) | (uintptr_t)a.image_plane * 4 | (uintptr_t)a.image_row * 4;
    if (a.C == 4) in |= reinterpret_cast<uintptr_t>(a.alpha) | (uintptr_t)a.alpha_row * 4 | (a.alpha_form == FRAME_ALPHA_RGB ? (uintptr_t)a.alpha_plane * 4 : 0);
    const int vec = a.W % 4 == 0 && (dst & 3) == 0 && (in & 15) == 0;
    const int al = align_of(dst);
    FRAME_DISPATCH(unpack_frame_kernel);
    return hipGetLastError();
}

}  // namespace nesr
