// The UNet of the x4 diffusion upscaler (diffusers' UNet2DConditionModel.forward) for gfx950: f32 storage, every product of a
// conv, a projection and the attention on the f32-input MFMA (v_mfma_f32_16x16x4_f32, an exact f32 fmaf chain).  tests/unet_ref.py
// is the restatement the kernels are held to.  The layout, the operand maps and the GroupNorm scheme are those of vae.hip.
//
// Shared with vae.hip, one copy in f32_rows_device.h: the conv's patch loader and tap loop, the GroupNorm partial sums, moments and
// VaeNorm, the attention's score tile, softmax step and P V.  They fix the order of every sum, so both files' pins hold the same bits.
// This file's own: every kernel's prologue and epilogue, because a launch takes two samples (a sample index in the grid), a conv and
// a GroupNorm take two sources (the loop over them, the seam in the finish's gather), the downsampler is the conv at stride 2, and
// the attention has heads of up to 128 columns padded to 16 (its chunk loader, its static LDS, its pad columns); and whole kernels
// with no counterpart: the K-tiled row GEMM with LayerNorm and GEGLU, the LayerNorm statistics, the embedding, the inputs.
//
// A workgroup is 256 threads (4 waves):
//
//   unet_in_kernel          NCHW sample or row-major text states -> zero padded rows.
//   unet_emb_kernel         one workgroup: the sinusoid in double, rounded once; linear_1, SiLU, linear_2, + the class row; leaves
//                           silu(emb), which is all any consumer reads.  Plain FMAs (M = 1: the samples share t and the label).
//   unet_temb_kernel        every ResnetBlock's time_emb_proj(silu(emb)) + conv1's bias in one launch: conv1's bias of this forward.
//   unet_conv_kernel<S>     3x3 / pad 1 conv as an implicit GEMM: 4 rows of 16 output pixels and 128 output channels a workgroup,
//                           the input through LDS in K chunks of 64 / S channels of the (3 + 4 S - S) x (3 + 16 S - S) patch.
//                           S = 1 reads rows or their nearest-x2 grid; S = 2 is the downsampler.  Two sources run one after the
//                           other through the same patch buffer: cat(hidden, skip) is never stored.  GroupNorm + SiLU in the
//                           loader on every tap inside the image.  Loader and tap loop: conv_load_patch<S>, conv_taps<S>.
//   unet_gn_partial_kernel  GroupNorm statistics as in vae.hip (double sums per 512 pixels and channel, then one workgroup a group
//   unet_gn_finish_kernel   and sample in a fixed order); the finish reads two sources' partial sums, so a group may straddle the seam.
//   unet_ln_stats_kernel    LayerNorm: one wave a row, two passes (mean, then the squared deviations), sums in double.
//   unet_rows_kernel        K-tiled row GEMM: 32 rows x 256 columns a workgroup, K through LDS in chunks of 64 (8.5 KB at any K).
//                           Prologue none | GroupNorm | LayerNorm; epilogue bias, + residual, or GEGLU: the workgroup computes the
//                           matching tiles of both halves and stores h gelu(g), so the 8 x dim intermediate never exists.
//   unet_attn_kernel        multi-head attention streamed over key chunks of 32 (vae_attn_kernel's scheme per head and sample): a
//                           running maximum and sum per query, the accumulator rescaled with every chunk.  No n x m matrix anywhere.
//
// Every global load and store is guarded by the row count, the image extent and the real width; reductions run in a fixed
// order without atomics, and no workgroup's arithmetic depends on the sample count: a sample alone gives the bits it gives as
// one of two.
#include "unet_api.h"

#include "f32_rows_device.h"
#include "nesr_kernels.h"

namespace nesr {
namespace {

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// ---------------------------------------------------------------------------------------------------------------- inputs
__global__ __launch_bounds__(256) void unet_in_kernel(const UnetIn a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;      // one element of the rows
    if (i >= (size_t)a.rows * a.cs) return;
    const int c = (int)(i % a.cs);
    const size_t row = i / a.cs;
    float v = 0.f;
    if (c < a.c) {
        if (a.nchw) {
            const size_t s = row / a.m, p = row - s * a.m;
            v = a.src[(s * a.c + c) * a.m + p];
        } else {
            v = a.src[row * a.c + c];
        }
    }
    a.out[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- embedding
__global__ __launch_bounds__(256) void unet_emb_kernel(const UnetEmb a) {
    __shared__ float sn[UNET_MAX_WIDTH];
    __shared__ float hid[UNET_MAX_TEMB];
    const int t = threadIdx.x, half = a.c0 >> 1;
    for (int i = t; i < a.c0; i += 256) {      // [cos | sin]: flip_sin_to_cos
        const int j = i < half ? i : i - half;
        const double ang = a.timestep * exp(-9.210340371976184 * (double)j / (double)half);      // ln 10000
        sn[i] = (float)(i < half ? cos(ang) : sin(ang));
    }
    __syncthreads();
    for (int j = t; j < a.td; j += 256) {
        float acc = a.b1[j];
        for (int k = 0; k < a.c0; ++k) acc = fmaf(sn[k], a.w1[(size_t)k * a.tdp + j], acc);
        hid[j] = silu(acc);
    }
    __syncthreads();
    for (int j = t; j < a.tdp; j += 256) {
        float v = 0.f;
        if (j < a.td) {
            float acc = a.b2[j];
            for (int k = 0; k < a.td; ++k) acc = fmaf(hid[k], a.w2[(size_t)k * a.tdp + j], acc);
            v = silu(acc + a.cls[j]);
        }
        a.out[j] = v;
    }
}

__global__ __launch_bounds__(256) void unet_temb_kernel(const UnetTemb a) {
    const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x, coutp = a.r[r].coutp;
    if (c >= coutp) return;
    const float* w = a.weights + a.r[r].w;
    float acc = 0.f;
    for (int k = 0; k < a.td; ++k) acc = fmaf(a.semb[k], w[(size_t)k * coutp + c], acc);
    a.out[(size_t)r * UNET_MAX_WIDTH + c] = a.weights[a.r[r].cb + c] + (a.weights[a.r[r].b + c] + acc);
}

// ---------------------------------------------------------------------------------------------------------------- conv 3x3
constexpr int CV_TW = VAE_CONV_TW, CV_TH = VAE_CONV_TH, CV_NB = VAE_CONV_NB;
template <int S>
__global__ __launch_bounds__(256) void unet_conv_kernel(const UnetConv a) {
    typedef ConvGeom<S> G;
    __shared__ float lds[G::FLOATS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * CV_TW, y0 = blockIdx.y * CV_TH;
    const int nblk = (a.coutp + CV_NB - 1) / CV_NB, sample = blockIdx.z / nblk, blk = blockIdx.z - sample * nblk;
    const int ntiles = a.coutp >> 4, ni0 = blk * (CV_NB / 16) + wave * 2;
    const bool work = ni0 < ntiles, two = ni0 + 1 < ntiles;      // the same for a wave
    const int ni1 = two ? ni0 + 1 : ni0;                           // a tile that is not there reads the first one's weights and is dropped
    const int DH = a.H * S, DW = a.W * S;                          // the conv's input domain
    const int sw = a.up ? a.W >> 1 : DW;                           // the source grid
    const size_t sm = a.up ? (size_t)(a.H >> 1) * (a.W >> 1) : (size_t)DH * DW;
    const int cinp0 = (a.in[0].c + 3) & ~3, cinp1 = a.in[1].p ? (a.in[1].c + 3) & ~3 : 0, cinp = cinp0 + cinp1;
    v4f acc[2][CV_TH];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < CV_TH; ++i) acc[j][i] = v4f{0.f, 0.f, 0.f, 0.f};

    bool first = true;
    for (int seg = 0; seg < 2; ++seg) {
        const UnetSrc src = a.in[seg];
        if (!src.p) break;
        const int cseg = seg == 0 ? cinp0 : cinp1, wrow = seg == 0 ? 0 : cinp0;
        const float* base = src.p + (size_t)sample * sm * src.cs;
        const VaeNorm* norm = src.norm ? src.norm + (size_t)sample * src.cs : nullptr;
        for (int c0 = 0; c0 < cseg; c0 += G::KC) {
            const int kc = cseg - c0 < G::KC ? cseg - c0 : G::KC;
            if (!first) __syncthreads();      // the chunk before is read
            first = false;
            conv_load_patch<S>(lds, base, norm, src.cs, c0, kc, y0, x0, DH, DW, sw, a.up != 0);
            __syncthreads();
            if (work) conv_taps<S>(lds, a.w, wrow + c0, cinp, a.coutp, kc, ni0, ni1, acc);
        }
    }
    if (!work) return;
    const size_t om = (size_t)a.H * a.W;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j == 1 && !two) break;
        const int c = (ni0 + j) * 16 + (lane & 15);      // < coutp
        const float bias = a.bias[c];
#pragma unroll
        for (int i = 0; i < CV_TH; ++i) {
            const int y = y0 + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = x0 + (lane >> 4) * 4 + r;
                if (y >= a.H || x >= a.W) continue;
                const size_t p = (size_t)y * a.W + x, row = (size_t)sample * om + p;
                float v = acc[j][i][r] + bias;
                if (a.res) v += a.res[row * a.coutp + c];
                if (!a.out_nchw) a.out[row * a.coutp + c] = v;      // the zero columns too
                else if (c < a.cout) a.out[((size_t)sample * a.cout + c) * om + p] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- GroupNorm statistics
__global__ __launch_bounds__(256) void unet_gn_partial_kernel(const UnetSrc src, int m, double* partial) {
    const int cs = src.cs, sample = blockIdx.y;
    gn_partial_block(src.p + (size_t)sample * m * cs, cs, m, partial + ((size_t)sample * gridDim.x + blockIdx.x) * cs * 2);
}

// block x = g < groups: group g of sample y; block `groups`: the padded channels, which normalise to zero
__global__ __launch_bounds__(256) void unet_gn_finish_kernel(const UnetGn a, int nblocks) {
    const int t = threadIdx.x, g = blockIdx.x, sample = blockIdx.y;
    const int c0 = a.in[0].c, c1 = a.in[1].p ? a.in[1].c : 0, cs0 = a.in[0].cs, cs1 = a.in[1].cs, cpg = (c0 + c1) / a.groups;
    VaeNorm* out0 = a.in[0].norm ? const_cast<VaeNorm*>(a.in[0].norm) + (size_t)sample * cs0 : nullptr;
    VaeNorm* out1 = c1 ? const_cast<VaeNorm*>(a.in[1].norm) + (size_t)sample * cs1 : nullptr;
    if (g == a.groups) {
        for (int c = c0 + t; c < cs0; c += 256) out0[c] = VaeNorm{0.f, 0.f, 0.f, 0.f};
        for (int c = c1 + t; c1 && c < cs1; c += 256) out1[c] = VaeNorm{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const double* p0 = a.partial[0] + (size_t)sample * nblocks * cs0 * 2;
    const double* p1 = c1 ? a.partial[1] + (size_t)sample * nblocks * cs1 * 2 : nullptr;
    double s = 0.0, ss = 0.0;
    const long long items = (long long)nblocks * cpg;
    for (long long it = t; it < items; it += 256) {
        const size_t blk = (size_t)(it / cpg);
        const int c = g * cpg + (int)(it % cpg);
        const double* at = c < c0 ? p0 + (blk * cs0 + c) * 2 : p1 + (blk * cs1 + (c - c0)) * 2;
        s += at[0], ss += at[1];
    }
    double mean, rstd;
    gn_moments(s, ss, (double)a.m * cpg, a.eps, mean, rstd);
    for (int k = t; k < cpg; k += 256) {
        const int c = g * cpg + k;
        const VaeNorm o = make_norm(mean, rstd, a.gamma[c], a.beta[c]);
        if (c < c0) out0[c] = o;
        else out1[c - c0] = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm statistics
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(256) void unet_ln_stats_kernel(const UnetLnStats a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.m) return;      // the same for a wave
    const int nq = a.cs >> 2;      // <= 256: at most four float4 a lane
    float x[16];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int q = lane + 64 * u;
        const float4 v = q < nq ? *reinterpret_cast<const float4*>(a.in + (size_t)row * a.cs + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        x[4 * u] = v.x, x[4 * u + 1] = v.y, x[4 * u + 2] = v.z, x[4 * u + 3] = v.w;
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if ((lane + 64 * u) * 4 + e < a.c) s += (double)x[4 * u + e];
    const double mean = wave_sum(s) / (double)a.c;
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if ((lane + 64 * u) * 4 + e < a.c) {
                const double dv = (double)x[4 * u + e] - mean;
                ss += dv * dv;
            }
    const double var = wave_sum(ss) / (double)a.c;
    if (lane == 0) {
        const float hi = (float)mean;
        a.out[row] = make_float4(hi, (float)(mean - (double)hi), (float)(1.0 / sqrt(var + (double)a.eps)), 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------- K-tiled rows
constexpr int RW_LD = UNET_KC + 4;

__global__ __launch_bounds__(256) void unet_rows_kernel(const UnetRows a) {
    __shared__ float lds[UNET_BM * RW_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, row0 = blockIdx.x * UNET_BM;
    const int out_tiles = a.np >> 4;
    int col[4];      // this wave's four B tiles: plain, four output tiles; GEGLU, two output tiles' value and gate halves
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int ot = a.geglu ? blockIdx.y * 8 + wave * 2 + (u & 1) : blockIdx.y * 16 + wave * 4 + u;
        ok[u] = ot < out_tiles;
        col[u] = (ok[u] ? ot * 16 : 0) + (a.geglu ? (u >> 1) * a.np : 0);      // a tile that is not there reads tile 0 and is dropped
    }
    v4f acc[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u][0] = acc[u][1] = v4f{0.f, 0.f, 0.f, 0.f};

    bool first = true;
    int krow = 0;
    for (int seg = 0; seg < 2; ++seg) {
        const UnetSrc src = a.in[seg];
        if (!src.p) break;
        for (int k0 = 0; k0 < src.cs; k0 += UNET_KC) {
            const int kc = src.cs - k0 < UNET_KC ? src.cs - k0 : UNET_KC, nq = kc >> 2;      // a multiple of 16
            if (!first) __syncthreads();      // the chunk before is read
            first = false;
            for (int idx = t; idx < UNET_BM * nq; idx += 256) {
                const int r = idx / nq, q = idx - r * nq, c = k0 + q * 4, row = row0 + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < a.m) {
                    v = *reinterpret_cast<const float4*>(src.p + (size_t)row * src.cs + c);
                    if (a.prologue == UNET_PRO_GROUPNORM) {
                        const VaeNorm* nm = src.norm + (size_t)(row / a.rows_per_sample) * src.cs + c;
                        v.x = normed(v.x, nm[0]), v.y = normed(v.y, nm[1]), v.z = normed(v.z, nm[2]), v.w = normed(v.w, nm[3]);
                    } else if (a.prologue == UNET_PRO_LAYERNORM) {
                        const float4 st = a.ln[row];
                        const float4 g = *reinterpret_cast<const float4*>(a.ln_g + c), b = *reinterpret_cast<const float4*>(a.ln_b + c);
                        v.x = ((v.x - st.x) - st.y) * st.z * g.x + b.x, v.y = ((v.y - st.x) - st.y) * st.z * g.y + b.y;
                        v.z = ((v.z - st.x) - st.y) * st.z * g.z + b.z, v.w = ((v.w - st.x) - st.y) * st.z * g.w + b.w;
                    }
                }
                *reinterpret_cast<float4*>(lds + r * RW_LD + q * 4) = v;
            }
            __syncthreads();
            if (!ok[0]) continue;      // the same for a wave; its first tile is its lowest
            const float* ap = lds + (lane & 15) * RW_LD + (lane >> 4);
            const float* bp = a.w + (size_t)(krow + k0 + (lane >> 4)) * a.ldw + (lane & 15);
            for (int k = 0; k < kc; k += 16) {      // sixteen weight fragments in flight; the MFMAs stay in ascending k
                float b[4][4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int u = 0; u < 4; ++u) b[kk][u] = bp[(size_t)(k + 4 * kk) * a.ldw + col[u]];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const float a0 = ap[k + 4 * kk], a1 = ap[16 * RW_LD + k + 4 * kk];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc[u][0] = mfma4(a0, b[kk][u], acc[u][0]);
                        acc[u][1] = mfma4(a1, b[kk][u], acc[u][1]);
                    }
                }
            }
        }
        krow += src.cs;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (!ok[u] || (a.geglu && u >= 2)) continue;
        const int c = col[u] + (lane & 15);      // the output column: u < 2 of GEGLU carries no half offset
        const float bias = a.b[c], gate_bias = a.geglu ? a.b[a.np + c] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + i * 16 + (lane >> 4) * 4 + r;
                if (row >= a.m) continue;
                float v = acc[u][i][r] + bias;
                if (a.geglu) v *= gelu_erf(acc[(u + 2) & 3][i][r] + gate_bias);      // tile u + 2 is this tile's gate
                if (a.res) v += a.res[(size_t)row * a.np + c];
                a.out[(size_t)row * a.np + c] = v;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------- streamed attention
// vae_attn_kernel's scheme per (query block, head, sample): Q [32][dp + 4] stays in LDS, dp = the head width rounded up to 16 and
// zero filled; a chunk is 32 keys [32][dp + 4], then their values [32][dp + 16] through the same buffer; wave w owns the output
// column tiles w and w + 4 of both 16-query halves.
constexpr int AT_DP = UNET_MAX_HEAD, AT_S = UNET_ATTN_BK + 4;
static_assert(AT_S == ATTN_LDS_S, "the score stride of the shared attention bodies");

// rows k0 .. k0 + 31 of `src` (row stride ld_src; d real columns, zeros to dp and past row n) -> dst [32][ld_dst]
__device__ __forceinline__ void attn_chunk(float* dst, int ld_dst, const float* src, size_t ld_src, int k0, int n, int d, int dp) {
    const int nq = dp >> 2, total = UNET_ATTN_BK * nq;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int r = idx / nq, c = (idx - r * nq) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + r < n && c < d) v = *reinterpret_cast<const float4*>(src + (size_t)(k0 + r) * ld_src + c);      // d is a multiple of 8
        *reinterpret_cast<float4*>(dst + r * ld_dst + c) = v;
    }
}

__global__ __launch_bounds__(256) void unet_attn_kernel(const UnetAttn a) {
    constexpr int BQ = UNET_ATTN_BQ, BK = UNET_ATTN_BK;
    __shared__ float Q[BQ * (AT_DP + 4)];
    __shared__ float KV[BK * (AT_DP + 16)];
    __shared__ float S[BQ * AT_S];
    __shared__ float alpha[BQ], lsum[BQ];
    const int dp = (a.d + 15) & ~15, ldc = dp + 4, ldv = dp + 16, nt = dp >> 4;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q0 = blockIdx.x * BQ, head = blockIdx.y, sample = blockIdx.z;
    const float* qp = a.q + (size_t)sample * a.nq * a.ldq + head * a.d;
    const float* kp = a.k + (size_t)sample * a.nk * a.ldkv + head * a.d;
    const float* vp = a.v + (size_t)sample * a.nk * a.ldkv + head * a.d;
    attn_chunk(Q, ldc, qp, a.ldq, q0, a.nq, a.d, dp);
    v4f acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j][0] = acc[j][1] = v4f{0.f, 0.f, 0.f, 0.f};
    const float root = sqrtf((float)a.d);
    const int row = t >> 3, sub = t & 7;       // the 8 threads of a query row: an eighth of a wave
    float m_run = -INFINITY, l_run = 0.f;      // the same in all 8

    for (int k0 = 0; k0 < a.nk; k0 += BK) {
        __syncthreads();      // Q is there; the chunk before is done with KV, S and alpha
        attn_chunk(KV, ldc, kp, a.ldkv, k0, a.nk, a.d, dp);
        __syncthreads();
        attn_scores(S, Q, KV, ldc, dp, root, k0, a.nk);
        __syncthreads();      // the scores are there, the keys are read
        attn_softmax_step(S, alpha, m_run, l_run);
        attn_chunk(KV, ldv, vp, a.ldkv, k0, a.nk, a.d, dp);
        __syncthreads();
        attn_pv<2>(acc, S, alpha, KV, ldv, nt);
    }
    if (sub == 0) lsum[row] = l_run;
    __syncthreads();
    float* op = a.out + (size_t)sample * a.nq * a.ldo;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ni = wave + 4 * j, c = ni * 16 + (lane & 15);
        if (ni >= nt) break;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = i * 16 + (lane >> 4) * 4 + r;
                if (q0 + qr < a.nq && c < a.d) op[(size_t)(q0 + qr) * a.ldo + head * a.d + c] = acc[j][i][r] / lsum[qr];
            }
    }
    const int pad = a.ldo - a.heads * a.d;      // the columns past the real width (under 16), by the last head's workgroups
    if (head == a.heads - 1 && pad > 0)
        for (int idx = t; idx < BQ * pad; idx += 256) {
            const int qr = idx / pad, c = a.heads * a.d + idx - qr * pad;
            if (q0 + qr < a.nq) op[(size_t)(q0 + qr) * a.ldo + c] = 0.f;
        }
}

bool src_ok(const UnetSrc& s, int max_cs) { return s.p && s.c >= 1 && s.cs >= 16 && s.cs % 16 == 0 && s.cs >= s.c && s.cs <= max_cs; }

}  // namespace

size_t unet_conv_lds_bytes(int stride) {
    return sizeof(float) * (stride == 2 ? ConvGeom<2>::FLOATS : ConvGeom<1>::FLOATS);
}
size_t unet_rows_lds_bytes() { return sizeof(float) * UNET_BM * RW_LD; }
size_t unet_attn_lds_bytes() { return sizeof(float) * (UNET_ATTN_BQ * (AT_DP + 4) + UNET_ATTN_BK * (AT_DP + 16) + UNET_ATTN_BQ * AT_S + 2 * UNET_ATTN_BQ); }
size_t unet_emb_lds_bytes() { return sizeof(float) * (UNET_MAX_WIDTH + UNET_MAX_TEMB); }

hipError_t launch_unet_in(const UnetIn& a, hipStream_t s) {
    if (!a.src || !a.out || a.c < 1 || a.cs < a.c || a.cs % 16 || a.rows < 1 || (a.nchw && (a.m < 1 || a.rows % a.m))) return hipErrorInvalidValue;
    const size_t blocks = ((size_t)a.rows * a.cs + 255) / 256;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    unet_in_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_unet_emb(const UnetEmb& a, hipStream_t s) {
    if (!a.w1 || !a.b1 || !a.w2 || !a.b2 || !a.cls || !a.out) return hipErrorInvalidValue;
    if (a.c0 < 2 || a.c0 % 2 || a.c0 > UNET_MAX_WIDTH || a.td < 1 || a.td > UNET_MAX_TEMB || a.tdp < a.td || a.tdp % 16) return hipErrorInvalidValue;
    unet_emb_kernel<<<dim3(1), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_unet_temb(const UnetTemb& a, hipStream_t s) {
    if (!a.semb || !a.weights || !a.out || a.count < 1 || a.count > UNET_MAX_RESNETS || a.td < 1) return hipErrorInvalidValue;
    for (int r = 0; r < a.count; ++r)
        if (a.r[r].coutp < 16 || a.r[r].coutp > UNET_MAX_WIDTH) return hipErrorInvalidValue;
    unet_temb_kernel<<<dim3(UNET_MAX_WIDTH / 256, a.count), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_unet_conv(const UnetConv& a, hipStream_t s) {
    if (!a.w || !a.bias || !a.out || a.n < 1 || a.n > 2 || a.H < 1 || a.W < 1 || (long long)a.n * a.H * a.W > UNET_MAX_PIXELS) return hipErrorInvalidValue;
    if (!src_ok(a.in[0], UNET_MAX_WIDTH) || (a.in[1].p && !src_ok(a.in[1], UNET_MAX_WIDTH))) return hipErrorInvalidValue;
    if (a.cout < 1 || a.coutp != (a.cout + 15) / 16 * 16 || a.coutp > UNET_MAX_WIDTH) return hipErrorInvalidValue;
    if ((a.stride != 1 && a.stride != 2) || (a.stride == 2 && a.up) || (a.up && (a.H % 2 || a.W % 2))) return hipErrorInvalidValue;
    if (a.out_nchw && a.res) return hipErrorInvalidValue;
    const unsigned nblk = (a.coutp + CV_NB - 1) / CV_NB;
    const dim3 grid((a.W + CV_TW - 1) / CV_TW, (a.H + CV_TH - 1) / CV_TH, a.n * nblk);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (a.stride == 2) unet_conv_kernel<2><<<grid, dim3(256), 0, s>>>(a);
    else unet_conv_kernel<1><<<grid, dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

static bool gn_ok(const UnetGn& a) {
    if (a.n < 1 || a.n > 2 || a.m < 1 || !a.gamma || !a.beta || a.groups < 1 || !(a.eps >= 0.f) || unet_gn_blocks(a.m) > 65535u) return false;
    if (!src_ok(a.in[0], UNET_MAX_WIDTH) || !a.in[0].norm || !a.partial[0]) return false;
    if (a.in[1].p && (!src_ok(a.in[1], UNET_MAX_WIDTH) || !a.in[1].norm || !a.partial[1])) return false;
    return (a.in[0].c + (a.in[1].p ? a.in[1].c : 0)) % a.groups == 0;
}

hipError_t launch_unet_gn_partial(const UnetGn& a, int source, hipStream_t s) {
    if (!gn_ok(a) || source < 0 || source > 1 || !a.in[source].p) return hipErrorInvalidValue;
    unet_gn_partial_kernel<<<dim3((unsigned)unet_gn_blocks(a.m), a.n), dim3(256), 0, s>>>(a.in[source], a.m, a.partial[source]);
    return hipGetLastError();
}

hipError_t launch_unet_gn_finish(const UnetGn& a, hipStream_t s) {
    if (!gn_ok(a)) return hipErrorInvalidValue;
    unet_gn_finish_kernel<<<dim3(a.groups + 1, a.n), dim3(256), 0, s>>>(a, (int)unet_gn_blocks(a.m));
    return hipGetLastError();
}

hipError_t launch_unet_ln_stats(const UnetLnStats& a, hipStream_t s) {
    if (!a.in || !a.out || a.m < 1 || a.c < 1 || a.cs < a.c || a.cs % 16 || a.cs > UNET_MAX_WIDTH || !(a.eps >= 0.f)) return hipErrorInvalidValue;
    unet_ln_stats_kernel<<<dim3((a.m + 3) / 4), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_unet_rows(const UnetRows& a, hipStream_t s) {
    if (!a.w || !a.b || !a.out || a.m < 1 || a.m > 0x7fffffff - UNET_BM || a.rows_per_sample < 1) return hipErrorInvalidValue;
    if (!src_ok(a.in[0], 4 * UNET_MAX_WIDTH) || (a.in[1].p && !src_ok(a.in[1], UNET_MAX_WIDTH))) return hipErrorInvalidValue;
    if (a.np < 16 || a.np % 16 || a.ldw != (a.geglu ? 2 * a.np : a.np)) return hipErrorInvalidValue;
    if (a.out == a.in[0].p || a.out == a.in[1].p) return hipErrorInvalidValue;
    if (a.prologue == UNET_PRO_GROUPNORM) {
        if (!a.in[0].norm || (a.in[1].p && !a.in[1].norm)) return hipErrorInvalidValue;
    } else if (a.prologue == UNET_PRO_LAYERNORM) {
        if (!a.ln || !a.ln_g || !a.ln_b || a.in[1].p) return hipErrorInvalidValue;
    } else if (a.prologue != UNET_PRO_NONE) {
        return hipErrorInvalidValue;
    }
    if (a.geglu && a.res) return hipErrorInvalidValue;
    const int bn = a.geglu ? UNET_BN / 2 : UNET_BN;
    const dim3 grid((a.m + UNET_BM - 1) / UNET_BM, (a.np + bn - 1) / bn);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    unet_rows_kernel<<<grid, dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_unet_attn(const UnetAttn& a, hipStream_t s) {
    if (!a.q || !a.k || !a.v || !a.out || a.samples < 1 || a.samples > 2 || a.nq < 1 || a.nk < 1 || a.heads < 1 || a.heads > 65535) return hipErrorInvalidValue;
    if (a.d < 8 || a.d > UNET_MAX_HEAD || a.d % 8) return hipErrorInvalidValue;
    const int dim = a.heads * a.d;
    if (a.ldq < dim || a.ldkv < dim || a.ldo < dim || a.ldq % 4 || a.ldkv % 4 || a.ldo - dim >= 16) return hipErrorInvalidValue;
    unet_attn_kernel<<<dim3((a.nq + UNET_ATTN_BQ - 1) / UNET_ATTN_BQ, a.heads, a.samples), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace nesr
