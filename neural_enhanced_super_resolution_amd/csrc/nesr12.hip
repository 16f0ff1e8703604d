// The input of the network SuperResolutionPipeline builds (RRDBNet(num_in_ch=12), nesr/nesr.py:216): one launch turns a window of
// an RGB u8 HWC frame into conv_first's 12 input channels, in the context's own activation layout and element type -- what
// nesr_adapter.build_12channel / build_3channel_x4 (a dozen torch launches and a [1,12,H,W] float tensor) followed by
// pack_input_kernel produce, bit for bit.
//
//   NESR_INPUT_12CH (nesr/nesr.py:851-882), bgr = the pixel flipped to BGR (cv2.COLOR_RGB2BGR), t = (float)bgr / 255.0f (IEEE):
//     channels 0-2 t | 3-5 min(max(t * 1.1f, 0), 1) | 6-8 min(max(t * 0.9f, 0), 1) | 9-11 GaussianBlur3x3(bgr) / 255.0f
//     cv2.GaussianBlur(u8, (3, 3), 0): taps [1 2 1] x [1 2 1], (S + 8) >> 4, BORDER_REFLECT_101 at the WINDOW's edges (the
//     reference blurs a tile after cropping it, nesr/nesr.py:385-395 -> :868)
//   NESR_INPUT_3CH_X4 (nesr/nesr.py:915-927): t four times.
//
// HBM-bound, one pass: 3 bytes read and 32 or 64 bytes written per pixel.  A workgroup stages its 64 x 16 pixels plus the
// one-pixel ring in LDS (every source byte is fetched once, the ring twice), a lane then owns a pixel's 16 stored channels
// (12 + the zero padding of the K-group), which are contiguous in all four layouts: whole 16-byte stores, coalesced over the lanes.
#include "../../include/nesr_hip.h"
#include "nesr_kernels.h"
#include "pack_elem.h"

namespace nesr {
namespace {

constexpr int TW = 64, TH = 16, ROWS_PER_LANE = TH / 4;      // 256 lanes = 64 columns x 4 row phases
constexpr int LW = (TW + 2) * 3;                             // staged bytes per row

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }   // n >= 2, -1 <= i <= n

__global__ __launch_bounds__(256) void pack_nesr12_kernel(Pack12Args a) {
    __shared__ uint8_t tile[(TH + 2) * LW];
    const int bx = blockIdx.x * TW, by = blockIdx.y * TH;
    // stage rows by - 1 .. by + TH, columns bx - 1 .. bx + TW of the window; beyond the window's edge the reflected pixel, beyond
    // the last tile's pixels (never read for a stored value) a clamped one
    for (int i = threadIdx.x; i < (TH + 2) * (TW + 2); i += 256) {
        const int ry = i / (TW + 2), rx = i - ry * (TW + 2);
        int y = by + ry - 1, x = bx + rx - 1;
        y = reflect101(y > a.h ? a.h : y, a.h);
        x = reflect101(x > a.w ? a.w : x, a.w);
        const uint8_t* p = a.src + (size_t)(a.y0 + y) * a.src_stride + (size_t)(a.x0 + x) * 3;
        uint8_t* q = tile + ry * LW + rx * 3;
        q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    }
    __syncthreads();
    const int lx = threadIdx.x & (TW - 1), ph = threadIdx.x / TW;
    const int x = bx + lx;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < ROWS_PER_LANE; ++r) {
        const int ly = ph + 4 * r, y = by + ly;
        if (x >= a.w || y >= a.h) continue;
        const uint8_t* c = tile + (ly + 1) * LW + (lx + 1) * 3;      // the pixel; its neighbours at +-3 and +-LW
        float v[16];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int k = 2 - ch;                                     // BGR channel ch is RGB byte 2 - ch
            const float t = (float)c[k] / 255.0f;
            v[ch] = t;
            if (a.mode == NESR_INPUT_12CH) {
                const int s = (c[k - LW - 3] + 2 * c[k - LW] + c[k - LW + 3]) + 2 * (c[k - 3] + 2 * c[k] + c[k + 3]) + (c[k + LW - 3] + 2 * c[k + LW] + c[k + LW + 3]);
                v[3 + ch] = fminf(fmaxf(t * 1.1f, 0.f), 1.f);
                v[6 + ch] = fminf(fmaxf(t * 0.9f, 0.f), 1.f);
                v[9 + ch] = (float)((s + 8) >> 4) / 255.0f;
            } else {
                v[3 + ch] = v[6 + ch] = v[9 + ch] = t;
            }
        }
        v[12] = v[13] = v[14] = v[15] = 0.f;
        const size_t pix = (size_t)y * a.w + x;
        if (a.bf16 == 0) {                   // f32 NHWC, K-groups of 8: channel co at (co / 8) * chunk + pix * map.pix + co % 8
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                float4* d = reinterpret_cast<float4*>(static_cast<float*>(a.dst) + (size_t)g * a.dst_map.chunk + pix * a.dst_map.pix);
                d[0] = make_float4(v[8 * g], v[8 * g + 1], v[8 * g + 2], v[8 * g + 3]);
                d[1] = make_float4(v[8 * g + 4], v[8 * g + 5], v[8 * g + 6], v[8 * g + 7]);
            }
        } else {                             // 16-bit blocked: channel co at pix * map.pix + co, the f16 pair's low halves 16 further on
            uint16_t e[16], lo[16];
#pragma unroll
            for (int co = 0; co < 16; ++co) {
                if (a.bf16 == 2) {
                    bad |= !f2hl(v[co], e[co], lo[co]);
                } else if (a.bf16 == 3) {
                    bad |= !(__builtin_fabsf(v[co]) <= 65504.f);
                    e[co] = __builtin_bit_cast(uint16_t, (_Float16)v[co]);
                } else {
                    e[co] = f2bf(v[co]);
                }
            }
            auto pack8 = [](const uint16_t* h) {
                return make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
            };
            uint4* d = reinterpret_cast<uint4*>(static_cast<uint16_t*>(a.dst) + pix * a.dst_map.pix);
            d[0] = pack8(e);
            d[1] = pack8(e + 8);
            if (a.bf16 == 2) {
                d[2] = pack8(lo);
                d[3] = pack8(lo + 8);
            }
        }
    }
    // the range word: a lane-divergent vector store by the lanes that met such a value (as pack_input_kernel)
    if (bad && a.status) __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

hipError_t launch_pack_nesr12(const Pack12Args& a, hipStream_t s) {
    // 16 stored channels (12 + the K-group's padding) in every layout; a one-pixel side has no reflected neighbour
    if (a.cp != 16 || a.h < 2 || a.w < 2 || (a.mode != NESR_INPUT_12CH && a.mode != NESR_INPUT_3CH_X4)) return hipErrorInvalidValue;
    if (a.dst_map.pix != (a.bf16 == 2 ? 32 : 16) || (a.bf16 == 0 && a.dst_map.chunk != 8)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_nesr12_kernel, dim3((a.w + TW - 1) / TW, (a.h + TH - 1) / TH), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace nesr
