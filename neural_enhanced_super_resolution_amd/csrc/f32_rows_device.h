// Device bodies that vae.hip and unet.hip share: the f32-row scheme's 3x3 conv (patch loader and tap loop), GroupNorm statistics
// (partial sums, moments, VaeNorm) and streamed attention (scores, online softmax, P V).  Each fixes an order of operations that the
// per-launch pins of both files hold bit for bit: the MFMA chain in ascending c, the double sums in a fixed order, the (hi, lo) split
// of the mean.  So there is one copy; a kernel keeps its own prologue (which tile, sample, source) and epilogue (what it stores).
// Device only; a workgroup is 256 threads.  MFMA operand maps: vae.hip's header.
#pragma once
#include "unet_api.h"

namespace nesr {
namespace {

static_assert(VAE_CONV_KC == UNET_KC, "one K chunk for both conv front ends");
static_assert(VAE_ATTN_BQ == UNET_ATTN_BQ && VAE_ATTN_BK == UNET_ATTN_BK && VAE_ATTN_BQ == 32 && VAE_ATTN_BK == 32, "one attention tile: 32 queries x 32 keys");

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4f mfma4(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float normed(float v, const VaeNorm& n) { return ((v - n.mean_hi) - n.mean_lo) * n.a + n.beta; }

// ---------------------------------------------------------------------------------------------------------------- conv 3x3
// The input patch of 4 x 16 output pixels at stride S, a K chunk of 64 / S channels at a time.
template <int S>
struct ConvGeom {
    static constexpr int KC = VAE_CONV_KC / S;
    static constexpr int PW = VAE_CONV_TW * S + 3 - S, PH = VAE_CONV_TH * S + 3 - S;
    static constexpr int LD = KC + 4;      // = 4 (mod 32): a wave's 64 reads meet 64 banks
    static constexpr int FLOATS = PH * PW * LD;
};

// Channels c0 .. c0 + kc of the patch of output tile (y0, x0) -> lds [PH PW][LD], by the workgroup.  `base` holds rows of stride cs
// on a grid sw wide: the DH x DW domain itself, or (up) its nearest-x2 source.  `norm`: GroupNorm + SiLU on every tap inside the
// domain; a tap outside is 0 (the conv pads after the activation).
template <int S>
__device__ __forceinline__ void conv_load_patch(float* lds, const float* base, const VaeNorm* norm, int cs, int c0, int kc, int y0, int x0, int DH, int DW,
                                                int sw, bool up) {
    typedef ConvGeom<S> G;
    const unsigned nq = (unsigned)kc >> 2;      // unsigned: the divisions below stay the short ones
    for (unsigned idx = threadIdx.x; idx < G::PH * G::PW * nq; idx += 256) {
        const unsigned q = idx % nq, pos = idx / nq, px = pos % G::PW, py = pos / G::PW;
        const int gy = y0 * S - 1 + (int)py, gx = x0 * S - 1 + (int)px;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < DH && gx >= 0 && gx < DW) {
            const int sy = up ? gy >> 1 : gy, sx = up ? gx >> 1 : gx;
            const int c = c0 + q * 4;      // c + 3 < the source's K <= cs
            v = *reinterpret_cast<const float4*>(base + ((size_t)sy * sw + sx) * cs + c);
            if (norm) {
                v.x = silu(normed(v.x, norm[c])), v.y = silu(normed(v.y, norm[c + 1]));
                v.z = silu(normed(v.z, norm[c + 2])), v.w = silu(normed(v.w, norm[c + 3]));
            }
        }
        *reinterpret_cast<float4*>(lds + pos * G::LD + q * 4) = v;
    }
}

// acc[j][i] += the nine taps of the chunk in lds (kc channels) x the weights of column tiles ni0 (j = 0) and ni1 (j = 1), for the
// wave's four pixel rows i.  w [9 tap_rows][coutp]; row0: the row of tap 0 at the chunk's first channel.
template <int S>
__device__ __forceinline__ void conv_taps(const float* lds, const float* w, int row0, int tap_rows, int coutp, int kc, int ni0, int ni1, v4f (&acc)[2][VAE_CONV_TH]) {
    typedef ConvGeom<S> G;
    const int lane = threadIdx.x & 63;
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const float* ap = lds + (ky * G::PW + (lane & 15) * S + kx) * G::LD + (lane >> 4);
        const float* bp = w + (size_t)(tap * tap_rows + row0 + (lane >> 4)) * coutp + (lane & 15);
        int c = 0;
        for (; c + 16 <= kc; c += 16) {      // four weight fragments a tile in flight; the MFMAs stay in ascending c
            float b0[4], b1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) b0[u] = bp[(size_t)(c + 4 * u) * coutp + ni0 * 16], b1[u] = bp[(size_t)(c + 4 * u) * coutp + ni1 * 16];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int i = 0; i < VAE_CONV_TH; ++i) {
                    const float av = ap[i * S * G::PW * G::LD + c + 4 * u];
                    acc[0][i] = mfma4(av, b0[u], acc[0][i]);
                    acc[1][i] = mfma4(av, b1[u], acc[1][i]);
                }
            }
        }
        for (; c < kc; c += 4) {
            const float b0 = bp[(size_t)c * coutp + ni0 * 16], b1 = bp[(size_t)c * coutp + ni1 * 16];
#pragma unroll
            for (int i = 0; i < VAE_CONV_TH; ++i) {
                const float av = ap[i * S * G::PW * G::LD + c];
                acc[0][i] = mfma4(av, b0, acc[0][i]);
                acc[1][i] = mfma4(av, b1, acc[1][i]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- GroupNorm statistics
// One block's partial sums: per channel of rows in [m][cs] the sum and the sum of squares of pixels 512 blockIdx.x .. in double ->
// out [cs][2].  256 / nq pixel lanes (nq = cs / 4 <= 256: at least one), folded through LDS in lane order.
__device__ __forceinline__ void gn_partial_block(const float* in, int cs, int m, double* out) {
    __shared__ double red[256 * 8];
    const int t = threadIdx.x, nq = cs >> 2, npl = 256 / nq;
    const int q4 = t % nq, pl = t / nq;
    const size_t p0 = (size_t)blockIdx.x * VAE_GN_PIXELS;
    const size_t p1 = p0 + VAE_GN_PIXELS < (size_t)m ? p0 + VAE_GN_PIXELS : (size_t)m;
    if (pl < npl) {
        double s[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
        for (size_t p = p0 + pl; p < p1; p += npl) {
            const float4 v = *reinterpret_cast<const float4*>(in + p * cs + q4 * 4);
            const double e[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += e[k], ss[k] += e[k] * e[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            red[((size_t)pl * cs + q4 * 4 + k) * 2] = s[k];
            red[((size_t)pl * cs + q4 * 4 + k) * 2 + 1] = ss[k];
        }
    }
    __syncthreads();
    for (int c = t; c < cs; c += 256) {
        double s = 0.0, ss = 0.0;
        for (int l = 0; l < npl; ++l) s += red[((size_t)l * cs + c) * 2], ss += red[((size_t)l * cs + c) * 2 + 1];
        out[(size_t)c * 2] = s;
        out[(size_t)c * 2 + 1] = ss;
    }
}

// Every thread's (s, ss) of a group of n values, added as a tree -> the group's mean and 1 / sqrt(biased variance + eps), in all threads.
__device__ __forceinline__ void gn_moments(double s, double ss, double n, float eps, double& mean, double& rstd) {
    __shared__ double rs[256], rq[256];
    const int t = threadIdx.x;
    rs[t] = s, rq[t] = ss;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) rs[t] += rs[t + h], rq[t] += rq[t + h];
        __syncthreads();
    }
    mean = rs[0] / n;
    double var = rq[0] / n - mean * mean;      // biased; the moments are double
    if (var < 0.0) var = 0.0;
    rstd = 1.0 / sqrt(var + (double)eps);
}

__device__ __forceinline__ VaeNorm make_norm(double mean, double rstd, float gamma, float beta) {
    VaeNorm o;
    o.mean_hi = (float)mean, o.mean_lo = (float)(mean - (double)o.mean_hi);
    o.a = (float)((double)gamma * rstd), o.beta = beta;
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- streamed attention
// A step of the stream over key chunks, 32 queries a workgroup: Q [32][ldc] and the chunk's keys KV [32][ldc] in LDS -> scores S
// [32][ATTN_LDS_S] -> weights exp(S - max) and alpha[32] = exp(old max - new max) -> the values through KV [32][ldv], O = O alpha + P V.
constexpr int ATTN_LDS_S = VAE_ATTN_BK + 4;

// S = Q K^T / root over K columns as four 16 x 16 tiles, one a wave; a key at or past n scores -inf
__device__ __forceinline__ void attn_scores(float* S, const float* Q, const float* KV, int ldc, int K, float root, int k0, int n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mi = wave >> 1, ni = wave & 1;
    const float* ap = Q + (mi * 16 + (lane & 15)) * ldc + (lane >> 4);
    const float* bp = KV + (ni * 16 + (lane & 15)) * ldc + (lane >> 4);
    v4f s0 = v4f{0.f, 0.f, 0.f, 0.f}, s1 = s0;      // even and odd k steps: two chains in flight, added once
    for (int k = 0; k < K; k += 8) {
        s0 = mfma4(ap[k], bp[k], s0);
        s1 = mfma4(ap[k + 4], bp[k + 4], s1);
    }
    const int j = ni * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) S[(mi * 16 + (lane >> 4) * 4 + r) * ATTN_LDS_S + j] = k0 + j < n ? (s0[r] + s1[r]) / root : -INFINITY;
}

// 8 threads a query row (row threadIdx.x >> 3, an eighth of a wave) turn its scores into weights and keep its running maximum and
// sum, the same in all 8
__device__ __forceinline__ void attn_softmax_step(float* S, float* alpha, float& m_run, float& l_run) {
    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;
    float sv[4], mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) sv[u] = S[row * ATTN_LDS_S + sub + 8 * u], mx = fmaxf(mx, sv[u]);
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    const float m_new = fmaxf(m_run, mx);      // finite: key k0 exists
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) sv[u] = expf(sv[u] - m_new), sum += sv[u];
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) sum += __shfl_xor(sum, d);
    const float al = expf(m_run - m_new);       // 0 in the first chunk
    l_run = l_run * al + sum;
    m_run = m_new;
#pragma unroll
    for (int u = 0; u < 4; ++u) S[row * ATTN_LDS_S + sub + 8 * u] = sv[u];
    if (sub == 0) alpha[row] = al;
}

// acc[j] = acc[j] alpha + P V for the wave's column tiles wave + 4 j < nt (at most NTW) of both 16-query halves
template <int NTW>
__device__ __forceinline__ void attn_pv(v4f (&acc)[NTW][2], const float* S, const float* alpha, const float* KV, int ldv, int nt) {
    constexpr int BK = VAE_ATTN_BK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float pa[2][BK / 4], al[2][4];      // this lane's A fragments of P and its rows' factors, the same for every column tile
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int u = 0; u < BK / 4; ++u) pa[i][u] = S[(i * 16 + (lane & 15)) * ATTN_LDS_S + 4 * u + (lane >> 4)];
#pragma unroll
        for (int r = 0; r < 4; ++r) al[i][r] = alpha[i * 16 + (lane >> 4) * 4 + r];
    }
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int ni = wave + 4 * j;
        if (ni >= nt) break;      // the same for a wave
        const float* bp = KV + (lane >> 4) * ldv + ni * 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][i][r] *= al[i][r];
#pragma unroll
        for (int u = 0; u < BK / 4; ++u) {
            const float b = bp[4 * u * ldv];
            acc[j][0] = mfma4(pa[0][u], b, acc[j][0]);
            acc[j][1] = mfma4(pa[1][u], b, acc[j][1]);
        }
    }
}

}  // namespace
}  // namespace nesr
