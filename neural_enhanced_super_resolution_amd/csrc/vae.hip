// The VAE decoder of the x4 diffusion upscaler (diffusers' AutoencoderKL.decode) for gfx950: f32 storage, every product on the
// f32-input MFMA (v_mfma_f32_16x16x4_f32, an exact f32 fmaf chain).  tests/vae_ref.py is the restatement the kernels are held to.
//
// Six kernels; a workgroup is 256 threads (4 waves):
//
//   vae_in_kernel             latents NCHW -> pixel-major rows [H W][16], divided by the scaling factor.
//   vae_conv_kernel           3x3 / pad 1 conv as an implicit GEMM over rows.  A workgroup owns 4 rows of 16 output pixels and
//                             128 output channels (two 16-wide tiles a wave, one accumulator per pixel row and tile); the input
//                             width goes through LDS in K chunks of 64 channels, the 6 x 18 patch of a chunk at a time (29 KB: a
//                             512-wide patch whole would be 221 KB).  The loader gathers rows or their nearest-x2 grid and applies
//                             GroupNorm + SiLU to every tap inside the image; a tap outside is 0 (the conv pads after the
//                             activation).  The epilogue adds the bias and a residual and stores rows, or the sample as NCHW f32,
//                             or the frame: / 2 + 0.5, clamp, x 255, round to nearest even, HWC u8.
//   vae_stats_partial_kernel  GroupNorm statistics, first half: per 512 pixels and channel the sum and the sum of squares in
//   vae_stats_finish_kernel   double, each into its own slot; second half: one workgroup a group adds the slots in a fixed order,
//                             and leaves (mean, gamma rstd, beta) per channel.  No atomics, no workgroup waits on another.
//   vae_rows_kernel           32 pixel rows a workgroup: (GroupNorm) -> x w + b -> + residual: the 1x1 convs (post_quant_conv, a
//                             ResnetBlock's shortcut) and the attention's q | k | v and output projections.
//   vae_attn_kernel           single-head attention streamed over the keys: 32 queries a workgroup, chunks of 32 keys, then their
//                             values, through one LDS buffer; a running maximum and sum per query, and the output accumulator (in
//                             registers) rescaled by exp(old max - new max) with every chunk.  No N x N matrix exists anywhere.
//
// MFMA operand maps (16x16x4 f32): lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result register r of lane
// l is D[row 4 (l >> 4) + r][col l & 15].  Every global load and store is guarded by the pixel count, the image extent and the real
// width; a forward repeated gives the same bits.
//
// The conv's patch loader and tap loop, the GroupNorm partial sums, moments and VaeNorm, and the attention's score tile, softmax step
// and P V are in f32_rows_device.h, one copy for this file and unet.hip; the kernels here keep their prologues and epilogues.
#include "vae_api.h"

#include "f32_rows_device.h"
#include "nesr_kernels.h"

namespace nesr {
namespace {

// acc[i] += A[m-tile i][K] x B[K][one n-tile], i < CNT, K a multiple of 16 (swin2sr.hip's chain: ascending k, four B fragments in flight)
template <int CNT>
__device__ __forceinline__ void mma_n(const float* ap, int a_tile, const float* bp, int sbk, int K, v4f (&acc)[2]) {
    for (int k = 0; k < K; k += 16) {
        float b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = bp[(size_t)(k + 4 * u) * sbk];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < CNT; ++i) acc[i] = mfma4(ap[i * a_tile + k + 4 * u], b[u], acc[i]);
        }
    }
}

// D[16 mt][16 nt] = A[16 mt][K] x B[K][16 nt] by the workgroup's four waves, mt <= 2; A in LDS (row stride lda), B(k, n) =
// B[k sbk + n sbn] in LDS or memory.  store(row, col, value) gets every element once.
template <class Store>
__device__ __forceinline__ void wg_gemm(const float* A, int lda, int mt, int K, const float* B, int sbk, int sbn, int nt, Store store) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int ni = wave; ni < nt; ni += 4) {
        v4f acc[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
        const float* ap = A + (lane & 15) * lda + (lane >> 4);
        const float* bp = B + (size_t)(lane >> 4) * sbk + (size_t)(ni * 16 + (lane & 15)) * sbn;
        if (mt == 1) mma_n<1>(ap, 16 * lda, bp, sbk, K, acc);
        else mma_n<2>(ap, 16 * lda, bp, sbk, K, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (i < mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) store(i * 16 + (lane >> 4) * 4 + r, ni * 16 + (lane & 15), acc[i][r]);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------- latents in
__global__ __launch_bounds__(256) void vae_in_kernel(const VaeIn a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;      // one element of the rows
    if (i >= (size_t)a.m * 16) return;
    const int c = (int)(i & 15);
    const size_t p = i >> 4;
    a.out[i] = c < a.c ? a.z[(size_t)c * a.m + p] / a.divisor : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- conv 3x3
__global__ __launch_bounds__(256) void vae_conv_kernel(const VaeConv a) {
    typedef ConvGeom<1> G;
    __shared__ float lds[G::FLOATS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * VAE_CONV_TW, y0 = blockIdx.y * VAE_CONV_TH;
    const int ntiles = a.coutp >> 4, ni0 = blockIdx.z * (VAE_CONV_NB / 16) + wave * 2;
    const bool work = ni0 < ntiles, two = ni0 + 1 < ntiles;      // the same for a wave
    const int ni1 = two ? ni0 + 1 : ni0;                           // a tile that is not there reads the first one's weights and is dropped
    const bool up = a.in_mode == VAE_IN_NEAREST2;
    v4f acc[2][VAE_CONV_TH];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < VAE_CONV_TH; ++i) acc[j][i] = v4f{0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < a.cinp; c0 += G::KC) {
        const int kc = a.cinp - c0 < G::KC ? a.cinp - c0 : G::KC;
        if (c0 > 0) __syncthreads();      // the chunk before is read
        conv_load_patch<1>(lds, a.in, a.norm, a.cs_in, c0, kc, y0, x0, a.H, a.W, up ? a.W >> 1 : a.W, up);
        __syncthreads();
        if (work) conv_taps<1>(lds, a.w, c0, a.cinp, a.coutp, kc, ni0, ni1, acc);
    }
    if (!work) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j == 1 && !two) break;
        const int c = (ni0 + j) * 16 + (lane & 15);      // < coutp
        const float bias = a.bias[c];
#pragma unroll
        for (int i = 0; i < VAE_CONV_TH; ++i) {
            const int y = y0 + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = x0 + (lane >> 4) * 4 + r;
                if (y >= a.H || x >= a.W) continue;
                const size_t p = (size_t)y * a.W + x;
                float v = acc[j][i][r] + bias;
                if (a.res) v += a.res[p * a.cs_res + c];      // c < coutp <= cs_res
                if (a.out_mode == VAE_OUT_ROWS) {
                    static_cast<float*>(a.out)[p * a.cs_out + c] = v;      // coutp == cs_out: the zero columns too
                    continue;
                }
                if (c >= a.cout) continue;
                if (a.out_mode == VAE_OUT_F32) {
                    static_cast<float*>(a.out)[(size_t)c * a.H * a.W + p] = v;
                } else {
                    v = fminf(fmaxf(v / 2.0f + 0.5f, 0.f), 1.f) * 255.0f;
                    static_cast<uint8_t*>(a.out)[p * a.cout + c] = (uint8_t)rintf(v);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- GroupNorm statistics
__global__ __launch_bounds__(256) void vae_stats_partial_kernel(const VaeStats a) {
    gn_partial_block(a.in, a.cs, a.m, a.partial + (size_t)blockIdx.x * a.cs * 2);
}

// block g < groups: group g; block `groups`: the padded channels, which normalise to zero
__global__ __launch_bounds__(256) void vae_stats_finish_kernel(const VaeStats a, int nblocks) {
    const int t = threadIdx.x, g = blockIdx.x, cpg = a.c / a.groups;
    if (g == a.groups) {
        for (int c = a.c + t; c < a.cs; c += 256) a.out[c] = VaeNorm{0.f, 0.f, 0.f, 0.f};
        return;
    }
    double s = 0.0, ss = 0.0;
    const long long items = (long long)nblocks * cpg;
    for (long long it = t; it < items; it += 256) {
        const size_t at = ((size_t)(it / cpg) * a.cs + g * cpg + (int)(it % cpg)) * 2;
        s += a.partial[at], ss += a.partial[at + 1];
    }
    double mean, rstd;
    gn_moments(s, ss, (double)a.m * cpg, a.eps, mean, rstd);
    for (int k = t; k < cpg; k += 256) {
        const int c = g * cpg + k;
        a.out[c] = make_norm(mean, rstd, a.gamma[c], a.beta[c]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- pixel rows
__global__ __launch_bounds__(256) void vae_rows_kernel(const VaeRows a) {
    extern __shared__ float lds[];
    const int lda = a.cs_in + 4, nq = a.cs_in >> 2;
    const int t = threadIdx.x, row0 = blockIdx.x * VAE_BM;
    for (int idx = t; idx < VAE_BM * nq; idx += 256) {
        const int r = idx / nq, q = idx - r * nq, c = q * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < a.m) {
            v = *reinterpret_cast<const float4*>(a.in + (size_t)(row0 + r) * a.cs_in + c);
            if (a.norm) {
                v.x = normed(v.x, a.norm[c]), v.y = normed(v.y, a.norm[c + 1]);
                v.z = normed(v.z, a.norm[c + 2]), v.w = normed(v.w, a.norm[c + 3]);
            }
        }
        *reinterpret_cast<float4*>(lds + r * lda + c) = v;
    }
    __syncthreads();
    const float* b = a.b;
    const float* res = a.res;
    float* out = a.out;
    const int m = a.m, np = a.np;
    wg_gemm(lds, lda, VAE_BM / 16, a.cs_in, a.w, np, 1, np >> 4, [=](int i, int j, float v) {
        const int row = row0 + i;
        if (row >= m) return;
        v += b[j];
        if (res) v += res[(size_t)row * np + j];
        out[(size_t)row * np + j] = v;
    });
}

// ---------------------------------------------------------------------------------------------------------------- streamed attention
// 32 queries a workgroup; Q [32][cs + 4] stays in LDS, the output accumulator in registers: wave w owns the 16-wide column tiles
// w, w + 4, ... (at most 8 at cs = 512) of both 16-query halves.  A chunk is 32 keys: K [32][cs + 4] through the one chunk buffer,
// S = Q K^T / sqrt(C) as four 16 x 16 tiles, one a wave; 8 threads a query row keep its running maximum and sum and turn S into
// exp(S - max); then V [32][cs + 16] through the same buffer (its stride spreads a B fragment over all 64 banks) and
// O = O exp(old max - new max) + P V.
constexpr int ATTN_NTW = 8;      // column tiles a wave can own: 4 waves x 8 x 16 = 512 columns

// rows k0 .. k0 + 31 of `src` (row stride ld_src, nq float4 a row; zeros past row n) -> dst [32][ld_dst], by the workgroup.  A thread's
// loads go out four at a time before the first store: the chunk is a few round trips to memory, not sixteen.
__device__ __forceinline__ void load_chunk(float* dst, int ld_dst, const float* src, size_t ld_src, int k0, int n, int nq) {
    const int total = VAE_ATTN_BK * nq;
    for (int idx0 = threadIdx.x; idx0 < total; idx0 += 4 * 256) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = idx0 + 256 * u, r = idx / nq, c = (idx - r * nq) * 4;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < total && k0 + r < n) v[u] = *reinterpret_cast<const float4*>(src + (size_t)(k0 + r) * ld_src + c);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = idx0 + 256 * u, r = idx / nq, c = (idx - r * nq) * 4;
            if (idx < total) *reinterpret_cast<float4*>(dst + r * ld_dst + c) = v[u];
        }
    }
}

__global__ __launch_bounds__(256) void vae_attn_kernel(const VaeAttn a) {
    extern __shared__ float lds[];
    constexpr int BQ = VAE_ATTN_BQ, BK = VAE_ATTN_BK, LDS_S = ATTN_LDS_S;
    const int ldc = a.cs + 4, ldv = a.cs + 16, nq = a.cs >> 2, nt = a.cs >> 4;
    float* Q = lds;                   // [BQ][ldc]
    float* KV = Q + BQ * ldc;         // [BK][ldv] a chunk's keys (stride ldc), then its values (stride ldv)
    float* S = KV + BK * ldv;         // [BQ][LDS_S] a chunk's scores, then its weights
    float* alpha = S + BQ * LDS_S;    // [BQ] exp(old max - new max) of the chunk
    float* lsum = alpha + BQ;         // [BQ] the final sums
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q0 = blockIdx.x * BQ;
    const size_t ld3 = (size_t)3 * a.cs;
    for (int idx = t; idx < BQ * nq; idx += 256) {
        const int r = idx / nq, c = (idx - r * nq) * 4;
        *reinterpret_cast<float4*>(Q + r * ldc + c) =
            q0 + r < a.n ? *reinterpret_cast<const float4*>(a.qkv + (size_t)(q0 + r) * ld3 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    v4f acc[ATTN_NTW][2];
#pragma unroll
    for (int j = 0; j < ATTN_NTW; ++j) acc[j][0] = acc[j][1] = v4f{0.f, 0.f, 0.f, 0.f};
    const float root = sqrtf((float)a.c);
    const int row = t >> 3, sub = t & 7;       // the 8 threads of a query row: an eighth of a wave
    float m_run = -INFINITY, l_run = 0.f;      // the same in all 8

    for (int k0 = 0; k0 < a.n; k0 += BK) {
        __syncthreads();      // Q is there; the chunk before is done with KV, S and alpha
        load_chunk(KV, ldc, a.qkv + a.cs, ld3, k0, a.n, nq);
        __syncthreads();
        attn_scores(S, Q, KV, ldc, a.cs, root, k0, a.n);
        __syncthreads();      // the scores are there, the keys are read
        attn_softmax_step(S, alpha, m_run, l_run);
        load_chunk(KV, ldv, a.qkv + 2 * a.cs, ld3, k0, a.n, nq);
        __syncthreads();
        attn_pv<ATTN_NTW>(acc, S, alpha, KV, ldv, nt);
    }
    if (sub == 0) lsum[row] = l_run;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ATTN_NTW; ++j) {
        const int ni = wave + 4 * j;
        if (ni >= nt) break;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = i * 16 + (lane >> 4) * 4 + r;
                if (q0 + qr < a.n) a.out[(size_t)(q0 + qr) * a.cs + ni * 16 + (lane & 15)] = acc[j][i][r] / lsum[qr];
            }
    }
}

template <class K, class A>
hipError_t launch_lds(K kernel, const A& a, dim3 grid, size_t bytes, unsigned long long& done, hipStream_t s) {
    if (bytes > VAE_LDS_LIMIT) return hipErrorInvalidValue;
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), VAE_LDS_LIMIT, done);
    if (e != hipSuccess) return e;
    kernel<<<grid, dim3(256), bytes, s>>>(a);
    return hipGetLastError();
}

bool width_ok(int c, int cs) { return c >= 1 && cs >= 16 && cs % 16 == 0 && cs >= c && cs <= 512; }

}  // namespace

size_t vae_conv_lds_bytes() { return sizeof(float) * ConvGeom<1>::FLOATS; }
size_t vae_rows_lds_bytes(int cs_in) { return sizeof(float) * VAE_BM * (cs_in + 4); }
size_t vae_attn_lds_bytes(int cs) {
    return sizeof(float) * ((size_t)VAE_ATTN_BQ * (cs + 4) + (size_t)VAE_ATTN_BK * (cs + 16) + VAE_ATTN_BQ * (VAE_ATTN_BK + 4) + 2 * VAE_ATTN_BQ);
}

hipError_t launch_vae_in(const VaeIn& a, hipStream_t s) {
    if (!a.z || !a.out || a.c < 1 || a.c > 16 || a.m < 1 || !(a.divisor != 0.f)) return hipErrorInvalidValue;
    const size_t blocks = ((size_t)a.m * 16 + 255) / 256;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    vae_in_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_vae_conv(const VaeConv& a, hipStream_t s) {
    if (!a.in || !a.w || !a.bias || !a.out || a.H < 1 || a.W < 1 || (long long)a.H * a.W > VAE_MAX_PIXELS) return hipErrorInvalidValue;
    if (a.cin < 1 || a.cinp != (a.cin + 3) / 4 * 4 || a.cs_in % 16 || a.cs_in < a.cinp || a.cs_in > 512) return hipErrorInvalidValue;
    if (a.cout < 1 || a.coutp != (a.cout + 15) / 16 * 16 || a.coutp > 512) return hipErrorInvalidValue;
    if (a.in_mode == VAE_IN_NEAREST2) {
        if (a.H % 2 || a.W % 2) return hipErrorInvalidValue;
    } else if (a.in_mode != VAE_IN_ROWS) {
        return hipErrorInvalidValue;
    }
    if (a.res && a.cs_res < a.coutp) return hipErrorInvalidValue;
    if (a.out_mode == VAE_OUT_ROWS) {
        if (a.cs_out != a.coutp) return hipErrorInvalidValue;
    } else if (a.out_mode == VAE_OUT_F32 || a.out_mode == VAE_OUT_U8) {
        if (a.cout > 4 || a.res) return hipErrorInvalidValue;
    } else {
        return hipErrorInvalidValue;
    }
    const dim3 grid((a.W + VAE_CONV_TW - 1) / VAE_CONV_TW, (a.H + VAE_CONV_TH - 1) / VAE_CONV_TH, (a.coutp + VAE_CONV_NB - 1) / VAE_CONV_NB);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    vae_conv_kernel<<<grid, dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_vae_rows(const VaeRows& a, hipStream_t s) {
    if (!a.in || !a.w || !a.b || !a.out || a.m < 1 || a.m > 0x7fffffff - VAE_BM) return hipErrorInvalidValue;
    if (a.cs_in < 16 || a.cs_in % 16 || a.cs_in > 512 || a.np < 16 || a.np % 16) return hipErrorInvalidValue;
    if (a.out == a.in && a.np != a.cs_in) return hipErrorInvalidValue;
    static unsigned long long done = 0;
    return launch_lds(&vae_rows_kernel, a, dim3((a.m + VAE_BM - 1) / VAE_BM), vae_rows_lds_bytes(a.cs_in), done, s);
}

static bool stats_ok(const VaeStats& a) {
    return a.in && a.partial && a.gamma && a.beta && a.out && a.m >= 1 && width_ok(a.c, a.cs) && a.groups >= 1 && a.c % a.groups == 0 && a.eps >= 0.f &&
           vae_stats_blocks(a.m) <= 0x7fffffffu;
}

hipError_t launch_vae_stats_partial(const VaeStats& a, hipStream_t s) {
    if (!stats_ok(a)) return hipErrorInvalidValue;
    vae_stats_partial_kernel<<<dim3((unsigned)vae_stats_blocks(a.m)), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_vae_stats_finish(const VaeStats& a, hipStream_t s) {
    if (!stats_ok(a)) return hipErrorInvalidValue;
    vae_stats_finish_kernel<<<dim3(a.groups + 1), dim3(256), 0, s>>>(a, (int)vae_stats_blocks(a.m));
    return hipGetLastError();
}

hipError_t launch_vae_attn(const VaeAttn& a, hipStream_t s) {
    if (!a.qkv || !a.out || a.n < 1 || a.n > VAE_MAX_TOKENS || !width_ok(a.c, a.cs)) return hipErrorInvalidValue;
    static unsigned long long done = 0;
    return launch_lds(&vae_attn_kernel, a, dim3((a.n + VAE_ATTN_BQ - 1) / VAE_ATTN_BQ), vae_attn_lds_bytes(a.cs), done, s);
}

}  // namespace nesr
