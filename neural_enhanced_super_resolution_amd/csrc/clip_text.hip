// The text encoder of the x4 diffusion upscaler (transformers' CLIPTextModel(input_ids)[0]) for gfx950: the kernels the UNet's
// launchers do not cover.  Every product and every LayerNorm inside a layer is launch_unet_rows / launch_unet_ln_stats of unet.hip
// as they are; tests/clip_text_ref.py is the restatement the whole is held to.
//
// A workgroup is 256 threads (4 waves):
//
//   clip_embed_kernel   token row + position row -> zero padded rows; the ids come in the argument block.
//   clip_attn_kernel    causal multi-head attention, unet_attn_kernel's scheme (f32_rows_device.h: score tile, softmax step, P V)
//                       per (query block of 32, head, sample), streamed over the key chunks of 32 up to the block's own: a
//                       query block never loads a chunk that lies wholly in its future.  Inside the diagonal chunk a future key's
//                       score becomes -inf before the softmax step, so its weight is exp(-inf) = 0 exactly.  Query block and key
//                       chunk are both 32 wide and aligned, so every query sees the first key of every chunk it meets: a chunk's
//                       maximum is finite and no -inf - -inf arises.  Query 0 has one key of weight exp(0) / exp(0) = 1: exact.
//   clip_act_kernel     fc1's activation in place: erf GELU or x sigmoid(1.702 x).
//   clip_final_kernel   final_layer_norm applied with the statistics of launch_unet_ln_stats; leaves the row layout ([m][c]).
//
// Every global load and store is guarded by the row count and the real width; no atomics, every sum in a fixed order, and no
// workgroup's arithmetic depends on the sample count.
#include "clip_text_api.h"

#include "f32_rows_device.h"

namespace nesr {
namespace {

// ---------------------------------------------------------------------------------------------------------------- embedding
__global__ __launch_bounds__(256) void clip_embed_kernel(const ClipEmbed a) {
    const int nq = a.cs >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;      // one float4 of the rows: rows cs / 4 <= 512 x 256
    if (i >= a.rows * nq) return;
    const int row = i / nq, c = (i - row * nq) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < a.c) {      // c is a multiple of 4: a float4 lies inside the width or past it
        const float4 t = *reinterpret_cast<const float4*>(a.tok + (size_t)a.ids[row] * a.c + c);
        const float4 p = *reinterpret_cast<const float4*>(a.pos + (size_t)(row % a.tokens) * a.c + c);
        v = make_float4(t.x + p.x, t.y + p.y, t.z + p.z, t.w + p.w);
    }
    *reinterpret_cast<float4*>(a.out + (size_t)row * a.cs + c) = v;
}

// ---------------------------------------------------------------------------------------------------------------- causal attention
constexpr int AT_DP = UNET_MAX_HEAD, AT_S = UNET_ATTN_BK + 4;
static_assert(AT_S == ATTN_LDS_S, "the score stride of the shared attention bodies");
static_assert(UNET_ATTN_BQ == UNET_ATTN_BK, "a query block meets whole chunks and its own diagonal one");

// rows k0 .. k0 + 31 of `src` (row stride ld_src; d real columns, zeros to dp and past row n) -> dst [32][ld_dst]
__device__ __forceinline__ void clip_chunk(float* dst, int ld_dst, const float* src, size_t ld_src, int k0, int n, int d, int dp) {
    const int nq = dp >> 2, total = UNET_ATTN_BK * nq;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int r = idx / nq, c = (idx - r * nq) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + r < n && c < d) v = *reinterpret_cast<const float4*>(src + (size_t)(k0 + r) * ld_src + c);      // d is a multiple of 8
        *reinterpret_cast<float4*>(dst + r * ld_dst + c) = v;
    }
}

__global__ __launch_bounds__(256) void clip_attn_kernel(const ClipAttn a) {
    constexpr int BQ = UNET_ATTN_BQ, BK = UNET_ATTN_BK;
    __shared__ float Q[BQ * (AT_DP + 4)];
    __shared__ float KV[BK * (AT_DP + 16)];
    __shared__ float S[BQ * AT_S];
    __shared__ float alpha[BQ], lsum[BQ];
    const int dp = (a.d + 15) & ~15, ldc = dp + 4, ldv = dp + 16, nt = dp >> 4;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q0 = blockIdx.x * BQ, head = blockIdx.y, sample = blockIdx.z;
    const float* qp = a.q + (size_t)sample * a.tokens * a.ldq + head * a.d;
    const float* kp = a.k + (size_t)sample * a.tokens * a.ldkv + head * a.d;
    const float* vp = a.v + (size_t)sample * a.tokens * a.ldkv + head * a.d;
    clip_chunk(Q, ldc, qp, a.ldq, q0, a.tokens, a.d, dp);
    v4f acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j][0] = acc[j][1] = v4f{0.f, 0.f, 0.f, 0.f};
    const float root = sqrtf((float)a.d);
    const int row = t >> 3, sub = t & 7;       // the 8 threads of a query row: an eighth of a wave
    float m_run = -INFINITY, l_run = 0.f;      // the same in all 8
    const int kend = q0 + BQ < a.tokens ? q0 + BQ : a.tokens;      // the keys any query of this block sees

    for (int k0 = 0; k0 < kend; k0 += BK) {      // k0 <= q0: the last chunk is the diagonal one
        __syncthreads();      // Q is there; the chunk before is done with KV, S and alpha
        clip_chunk(KV, ldc, kp, a.ldkv, k0, a.tokens, a.d, dp);
        __syncthreads();
        attn_scores(S, Q, KV, ldc, dp, root, k0, a.tokens);
        __syncthreads();      // the scores are there, the keys are read
#pragma unroll
        for (int u = 0; u < 4; ++u)      // the four scores this thread reads next: a key after the query does not count
            if (k0 + sub + 8 * u > q0 + row) S[row * AT_S + sub + 8 * u] = -INFINITY;
        attn_softmax_step(S, alpha, m_run, l_run);
        clip_chunk(KV, ldv, vp, a.ldkv, k0, a.tokens, a.d, dp);
        __syncthreads();
        attn_pv<2>(acc, S, alpha, KV, ldv, nt);
    }
    if (sub == 0) lsum[row] = l_run;
    __syncthreads();
    float* op = a.out + (size_t)sample * a.tokens * a.ldo;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ni = wave + 4 * j, c = ni * 16 + (lane & 15);
        if (ni >= nt) break;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = i * 16 + (lane >> 4) * 4 + r;
                if (q0 + qr < a.tokens && c < a.d) op[(size_t)(q0 + qr) * a.ldo + head * a.d + c] = acc[j][i][r] / lsum[qr];
            }
    }
    const int pad = a.ldo - a.heads * a.d;      // the columns past the real width (under 16), by the last head's workgroups
    if (head == a.heads - 1 && pad > 0)
        for (int idx = t; idx < BQ * pad; idx += 256) {
            const int qr = idx / pad, c = a.heads * a.d + idx - qr * pad;
            if (q0 + qr < a.tokens) op[(size_t)(q0 + qr) * a.ldo + c] = 0.f;
        }
}

// ---------------------------------------------------------------------------------------------------------------- activation
__device__ __forceinline__ float clip_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float clip_quick_gelu(float v) { return v / (1.0f + expf(-1.702f * v)); }

__global__ __launch_bounds__(256) void clip_act_kernel(const ClipAct a) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= a.count) return;
    float4 v = *reinterpret_cast<const float4*>(a.x + i);
    if (a.act == CLIP_ACT_QUICK_GELU) v = make_float4(clip_quick_gelu(v.x), clip_quick_gelu(v.y), clip_quick_gelu(v.z), clip_quick_gelu(v.w));
    else v = make_float4(clip_gelu(v.x), clip_gelu(v.y), clip_gelu(v.z), clip_gelu(v.w));
    *reinterpret_cast<float4*>(a.x + i) = v;
}

// ---------------------------------------------------------------------------------------------------------------- final LayerNorm
__global__ __launch_bounds__(256) void clip_final_kernel(const ClipFinal a) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // one element of the result: m c <= 512 x 1024
    if (i >= a.m * a.c) return;
    const int row = i / a.c, c = i - row * a.c;
    const float4 st = a.ln[row];
    a.out[i] = ((a.in[(size_t)row * a.cs + c] - st.x) - st.y) * st.z * a.g[c] + a.b[c];      // the row GEMM's LayerNorm prologue
}

}  // namespace

size_t clip_attn_lds_bytes() { return sizeof(float) * (UNET_ATTN_BQ * (AT_DP + 4) + UNET_ATTN_BK * (AT_DP + 16) + UNET_ATTN_BQ * AT_S + 2 * UNET_ATTN_BQ); }

hipError_t launch_clip_embed(const ClipEmbed& a, hipStream_t s) {
    if (!a.tok || !a.pos || !a.out || a.vocab < 1 || a.positions < 1) return hipErrorInvalidValue;
    if (a.tokens < 1 || a.tokens > a.positions || a.rows < 1 || a.rows > CLIP_MAX_IDS || a.rows % a.tokens) return hipErrorInvalidValue;
    if (a.c < 4 || a.c % 4 || a.c > CLIP_MAX_HIDDEN || a.cs < a.c || a.cs % 16 || a.cs - a.c >= 16) return hipErrorInvalidValue;
    for (int r = 0; r < a.rows; ++r)
        if (a.ids[r] < 0 || a.ids[r] >= a.vocab) return hipErrorInvalidValue;
    clip_embed_kernel<<<dim3((a.rows * (a.cs / 4) + 255) / 256), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_clip_attn(const ClipAttn& a, hipStream_t s) {
    if (!a.q || !a.k || !a.v || !a.out || a.samples < 1 || a.samples > 2 || a.tokens < 1 || a.tokens > NESR_UNET_MAX_TEXT_TOKENS) return hipErrorInvalidValue;
    if (a.heads < 1 || a.heads > 65535 || a.d < 8 || a.d > UNET_MAX_HEAD || a.d % 8) return hipErrorInvalidValue;
    const int dim = a.heads * a.d;
    if (a.ldq < dim || a.ldkv < dim || a.ldo < dim || a.ldq % 4 || a.ldkv % 4 || a.ldo - dim >= 16) return hipErrorInvalidValue;
    clip_attn_kernel<<<dim3((a.tokens + UNET_ATTN_BQ - 1) / UNET_ATTN_BQ, a.heads, a.samples), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_clip_act(const ClipAct& a, hipStream_t s) {
    if (!a.x || a.count < 4 || a.count % 4 || a.count > (long long)CLIP_MAX_IDS * CLIP_MAX_INTER) return hipErrorInvalidValue;
    if (a.act != CLIP_ACT_GELU && a.act != CLIP_ACT_QUICK_GELU) return hipErrorInvalidValue;
    clip_act_kernel<<<dim3((unsigned)((a.count / 4 + 255) / 256)), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_clip_final(const ClipFinal& a, hipStream_t s) {
    if (!a.in || !a.ln || !a.g || !a.b || !a.out || a.m < 1 || a.m > CLIP_MAX_IDS) return hipErrorInvalidValue;
    if (a.c < 1 || a.c > CLIP_MAX_HIDDEN || a.cs < a.c || a.cs % 16) return hipErrorInvalidValue;
    clip_final_kernel<<<dim3((a.m * a.c + 255) / 256), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace nesr
