// Swin2SR (SwinV2 window-attention super-resolution transformer) for gfx950: f32 storage, every product on the f32-input MFMA
// (v_mfma_f32_16x16x4_f32, an exact f32 fmaf chain).  Stands behind transformers' Swin2SRForImageSuperResolution.forward in eval
// mode; tests/swin2sr_ref.py is the restatement the kernels are held to.
//
// Three kernels; a workgroup is 256 threads (4 waves), the attention block's 512 (8 waves: it is alone on its CU, see the LDS budget):
//
//   s2_conv_kernel   3x3 / pad 1 conv as an implicit GEMM over token-major rows.  A workgroup owns 4 rows of 16 output pixels and
//                    keeps their 6 x 18 input patch in LDS; a wave takes 16 output channels at a time with one accumulator per
//                    pixel row, so a weight fragment read from memory feeds four MFMAs.  The loader makes the patch from rows, from
//                    a nearest-x2 gather, or from the u8 / f32 frame with both paddings and the normalisation; the epilogue adds the
//                    bias, LeakyReLU, a residual, and stores rows, a PixelShuffle, or the final image (/ range + mean, crop, f32 or
//                    clamp -> x 255 -> round to nearest even -> u8).
//   s2_attn_kernel   one window a workgroup.  Gathers the ws^2 tokens through the cyclic shift; per head: q, k, v = X Wqkv + b,
//                    q and k L2-normalised, S = q k^T x temperature + bias table + region mask (from the tokens' coordinates,
//                    added twice as transformers does), softmax, P V; then output.dense, LayerNorm, + shortcut, scattered back
//                    through the reverse shift.  X, the context, one head's q | k | v and one head's scores live in LDS.
//   s2_rows_kernel   32 token rows a workgroup: (x w1 + b1, erf-GELU) -> (x w2 + b2) -> LayerNorm -> + residual, every step
//                    optional: the MLP block, the 1x1 projections (patch embedding with LayerNorm, a stage's end with its
//                    residual) and the encoder's LayerNorm.
//
// Two small HBM-bound kernels serve the overlapped route (nesr_swin2sr_upscale_overlapped_u8): s2_overlap_add_kernel adds a batch's
// f32 window outputs into the accumulator of the padded frame, s2_overlap_finish_kernel divides by the cover count and quantises.
//
// MFMA operand maps (16x16x4 f32): lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result register r of lane
// l is D[row 4 (l >> 4) + r][col l & 15].  Widths are padded to the tile with zeros (swin2sr_api.h).  No atomics, no workgroup
// waits on another: a forward repeated gives the same bits.  Every global load and store is guarded by the token count, the
// image extent and the real width.
//
// A launch takes a batch of images of one padded size (the tiles of a large frame, nesr_swin2sr_upscale_tiled_u8): the conv and the
// attention kernel read the image from blockIdx.z and offset their bases by it; zero padding, the cyclic shift and the region mask
// stay inside the image.  The row kernel sees batch * H * W rows.  A batch of one runs the arithmetic of a whole frame unchanged.
//
// The fp16 compute form (nesr_swin2sr_set_dtype, template argument T = f16): storage in memory stays f32, every GEMM takes both
// operands rounded to f16 (a plain cast: nearest even) and runs on v_mfma_f32_16x16x32_f16, a K tail of 16 on
// v_mfma_f32_16x16x16_f16; products and sums are f32.  Lane l holds A[row l & 15][k = 8 (l >> 4) + j] and
// B[k = 8 (l >> 4) + j][col l & 15], j < 8 (j < 4 and 4 (l >> 4) in the tail); the result map is the f32 one.  An A operand is
// staged in LDS as f16 with k contiguous (one 16-byte load a fragment); the rounding and the range check (elem16.h: a value that is
// non-finite or beyond 65504 raises the context's range word) happen at that store.  A weight is a second, f16 copy packed
// [n][K], so a fragment is one 16-byte load as well.  Every K is a multiple of 16 (a conv's input width is padded to 16 with zeros
// in the patch and in the weights).  Biases, temperature, bias table, mask, softmax, GELU, LayerNorm, residuals and the
// epilogues are the f32 code (the L2 normalisation of q and k alone is evaluated in double: see s2_attn_f16_kernel); the frame-loading first conv and a row launch without a product run as T = float.
// The LDS regions keep their f32 sizes: the 16-bit tiles lie inside them (see each kernel).
#include <type_traits>

#include "swin2sr_api.h"

#include "elem16.h"
#include "nesr_kernels.h"

namespace nesr {
namespace {

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 __attribute__((may_alias)) f16_alias;      // halves written over the f32 values of the same LDS row

template <class T>
constexpr bool is_f16 = std::is_same<T, f16>::value;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma4(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma4(f16x4 a, f16x4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }

// f32 -> f16 (nearest even) with the range check: `am` keeps the largest |x| pattern this lane rounded
__device__ __forceinline__ f16 round16(float v, unsigned& am) {
    am = E16<3>::amax(am, v);
    return (f16)v;
}
// Rounds value j of an LDS row of f32 in place: half j lies over float j / 2.  The row's 8 threads (one wave, in lockstep) read
// floats 8 it .. 8 it + 7 and then write halves over floats 4 it .. 4 it + 3, which are read already; volatile keeps a thread's
// loads and stores in program order, and LDS serves a wave's accesses in order.
__device__ __forceinline__ float load_in_place(const float* row, int j) { return *reinterpret_cast<const volatile float*>(row + j); }
__device__ __forceinline__ void round_in_place(float* row, int j, float v, unsigned& am) {
    *(reinterpret_cast<volatile f16_alias*>(row) + j) = round16(v, am);
}
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

__device__ __forceinline__ float sum8(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}
__device__ __forceinline__ double sum8(double v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}
__device__ __forceinline__ float max8(float v) {
    v = fmaxf(v, __shfl_xor(v, 1));
    v = fmaxf(v, __shfl_xor(v, 2));
    v = fmaxf(v, __shfl_xor(v, 4));
    return v;
}

// acc[i] += A[m-tile i][K] x B[K][one n-tile], i < CNT, K a multiple of 16.  ap: this lane's A element of k = 0 in the first
// m-tile (a_tile floats to the next); bp: its B element of k = 0, sbk floats to the next k.  The B fragments of four steps are
// loaded before the first MFMA needs one; the MFMAs run in ascending k, so the sum is the plain chain's.  CNT is the same for every
// lane: a scalar branch picks it.
template <int CNT>
__device__ __forceinline__ void mma_n(const float* ap, int a_tile, const float* bp, int sbk, int K, f32x4 (&acc)[4]) {
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
// The f16 form: ap and bp are the lane's A row and B column (k contiguous in both, 16-byte aligned); steps of 32, then a tail of 16.
template <int CNT>
__device__ __forceinline__ void mma_n(const f16* ap, int a_tile, const f16* bp, int, int K, f32x4 (&acc)[4]) {
    const int g = (threadIdx.x & 63) >> 4;
    int k = 0;
    for (; k + 64 <= K; k += 64) {      // two weight fragments in flight
        const f16x8 b0 = *reinterpret_cast<const f16x8*>(bp + k + 8 * g), b1 = *reinterpret_cast<const f16x8*>(bp + k + 32 + 8 * g);
#pragma unroll
        for (int i = 0; i < CNT; ++i) acc[i] = mfma4(*reinterpret_cast<const f16x8*>(ap + i * a_tile + k + 8 * g), b0, acc[i]);
#pragma unroll
        for (int i = 0; i < CNT; ++i) acc[i] = mfma4(*reinterpret_cast<const f16x8*>(ap + i * a_tile + k + 32 + 8 * g), b1, acc[i]);
    }
    if (k + 32 <= K) {
        const f16x8 b = *reinterpret_cast<const f16x8*>(bp + k + 8 * g);
#pragma unroll
        for (int i = 0; i < CNT; ++i) acc[i] = mfma4(*reinterpret_cast<const f16x8*>(ap + i * a_tile + k + 8 * g), b, acc[i]);
        k += 32;
    }
    if (k < K) {
        const f16x4 b = *reinterpret_cast<const f16x4*>(bp + k + 4 * g);
#pragma unroll
        for (int i = 0; i < CNT; ++i) acc[i] = mfma4(*reinterpret_cast<const f16x4*>(ap + i * a_tile + k + 4 * g), b, acc[i]);
    }
}

// D[16 mt][16 nt] = A[16 mt][K] x B[K][16 nt] by the workgroup's waves; A in LDS (row stride lda), B(k, n) = B[k sbk + n sbn] in
// LDS or memory; K a multiple of 16.  store(row, col, value) gets every element once.  T = f16: sbk is 1, lda and sbn count halves.
template <class T, class Store>
__device__ __forceinline__ void wg_gemm(const T* A, int lda, int mt, int K, const T* B, int sbk, int sbn, int nt, Store store) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    int mch = 4;                                           // m-tiles that share a B fragment; fewer while waves would idle
    while (mch > 1 && nt * ((mt + mch - 1) / mch) < nw) mch >>= 1;
    const int mchunks = (mt + mch - 1) / mch;
    for (int item = wave; item < nt * mchunks; item += nw) {
        const int ni = item % nt, m0 = (item / nt) * mch;
        const int cnt = mt - m0 < mch ? mt - m0 : mch;
        f32x4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        const T* ap = A + (m0 * 16 + (lane & 15)) * lda + (is_f16<T> ? 0 : lane >> 4);
        const T* bp = B + (is_f16<T> ? (size_t)0 : (size_t)(lane >> 4) * sbk) + (size_t)(ni * 16 + (lane & 15)) * sbn;
        switch (cnt) {
            case 1: mma_n<1>(ap, 16 * lda, bp, sbk, K, acc); break;
            case 2: mma_n<2>(ap, 16 * lda, bp, sbk, K, acc); break;
            case 3: mma_n<3>(ap, 16 * lda, bp, sbk, K, acc); break;
            default: mma_n<4>(ap, 16 * lda, bp, sbk, K, acc); break;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < cnt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) store((m0 + i) * 16 + (lane >> 4) * 4 + r, ni * 16 + (lane & 15), acc[i][r]);
            }
    }
}

// LayerNorm over the c real columns of a row of LDS, by the row's 8 threads (thread s8 the columns s8 + 8 i); returns mean, rstd
__device__ __forceinline__ void row_stats(const float* rp, int c, int s8, float eps, float& mean, float& rstd) {
    float s = 0.f;
    for (int j = s8; j < c; j += 8) s += rp[j];
    mean = sum8(s) / (float)c;
    float q = 0.f;
    for (int j = s8; j < c; j += 8) {
        const float dv = rp[j] - mean;
        q += dv * dv;
    }
    rstd = 1.0f / sqrtf(sum8(q) / (float)c + eps);
}

// ---------------------------------------------------------------------------------------------------------------- conv 3x3
constexpr int CP_W = S2_CONV_TW + 2, CP_H = S2_CONV_TH + 2;

__host__ __device__ inline int conv_ldp(int cinp) { return ((cinp - 4 + 31) / 32) * 32 + 4; }      // = 4 (mod 32): 64 banks a wave's read

// numpy's "symmetric" extension (the edge sample repeats), any distance
__device__ __forceinline__ int sym_index(int i, int n) {
    int t = i % (2 * n);
    return t < n ? t : 2 * n - 1 - t;
}

// T = f16 (rows and nearest-x2 inputs only): the patch is [6 x 18][cin16 + 8] halves, cin16 = the input width rounded up to 16, and
// the weights are a.wh [9][coutp][cin16]
__host__ __device__ inline int conv_cin16(int cin) { return (cin + 15) & ~15; }

template <class T>
__global__ __launch_bounds__(256) void s2_conv_kernel(const S2Conv a) {
    extern __shared__ float lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int x0 = blockIdx.x * S2_CONV_TW, y0 = blockIdx.y * S2_CONV_TH;
    const int cin16 = conv_cin16(a.cin);
    const int ldp = is_f16<T> ? cin16 + 8 : conv_ldp(a.cinp), nq = is_f16<T> ? cin16 >> 2 : a.cinp >> 2;
    unsigned am = 0;
    const size_t b = blockIdx.z, px_img = (size_t)a.H * a.W;      // the image of this workgroup; zero padding at its own border
    // image b's window in the frame (wy, wx) and its core inside the window's output [cy0, cy1) x [cx0, cx1); a whole frame: all of it
    int wy = 0, wx = 0, cy0 = 0, cy1 = a.oh, cx0 = 0, cx1 = a.ow;
    if (a.tile > 0) {
        const int ti = a.tile0 + (int)b, ty = ti / a.tiles_x, tx = ti - ty * a.tiles_x;
        int c0, c1;
        s2_tile_axis(a.FH, a.tile, a.tile_pad, ty, wy, c0, c1);
        cy0 = (c0 - wy) * a.up, cy1 = (c1 - wy) * a.up;
        s2_tile_axis(a.FW, a.tile, a.tile_pad, tx, wx, c0, c1);
        cx0 = (c0 - wx) * a.up, cx1 = (c1 - wx) * a.up;
    }
    int ovy = 0, ovx = 0;      // WINDOW_U8: image b's origin in the padded frame
    if (a.in_mode == S2_IN_WINDOW_U8) {
        const int ti = a.tile0 + (int)b, ty = ti / a.tiles_x, tx = ti - ty * a.tiles_x;
        int cnt, first, last;
        s2_overlap_axis(a.PH, a.H, a.ov_step, ty, 0, cnt, ovy, first, last);
        s2_overlap_axis(a.PW, a.W, a.ov_step, tx, 0, cnt, ovx, first, last);
    }
    const float* in_rows = static_cast<const float*>(a.in);
    if (a.in_mode == S2_IN_ROWS) in_rows += b * px_img * a.cs_in;
    else if (a.in_mode == S2_IN_NEAREST2) in_rows += b * (size_t)(a.H >> 1) * (a.W >> 1) * a.cs_in;
    else if (a.in_mode == S2_IN_FRAME_F32) in_rows += b * (size_t)a.cin * a.fh * a.fw;

    for (int idx = t; idx < CP_H * CP_W * nq; idx += 256) {
        const int q = idx % nq, pos = idx / nq, px = pos % CP_W, py = pos / CP_W;
        const int gy = y0 - 1 + py, gx = x0 - 1 + px;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && (!is_f16<T> || q * 4 < a.cinp)) {      // f16: zeros from cinp up to cin16
            if (a.in_mode == S2_IN_ROWS) {
                v = *reinterpret_cast<const float4*>(in_rows + ((size_t)gy * a.W + gx) * a.cs_in + q * 4);
            } else if (a.in_mode == S2_IN_NEAREST2) {
                v = *reinterpret_cast<const float4*>(in_rows + ((size_t)(gy >> 1) * (a.W >> 1) + (gx >> 1)) * a.cs_in + q * 4);
            } else if (a.in_mode == S2_IN_WINDOW_U8) {
                if (q == 0) {      // the frame's own symmetric extension at the window's place: the index is taken against the frame
                    const size_t at = ((size_t)sym_index(ovy + gy, a.FH) * a.FW + sym_index(ovx + gx, a.FW)) * a.cin;
                    float e[4] = {0.f, 0.f, 0.f, 0.f};
                    for (int ch = 0; ch < a.cin; ++ch) e[ch] = ((float)static_cast<const uint8_t*>(a.in)[at + ch] / 255.0f - a.mean[ch]) * a.range;
                    v = make_float4(e[0], e[1], e[2], e[3]);
                }
            } else if (q == 0) {
                // reflect back into the model's input (mh x mw), then symmetric back into the image's own window (fh x fw) of the frame
                int my = gy < a.mh ? gy : 2 * a.mh - 2 - gy, mx = gx < a.mw ? gx : 2 * a.mw - 2 - gx;
                const int fy = sym_index(my, a.fh), fx = sym_index(mx, a.fw);
                float e[4] = {0.f, 0.f, 0.f, 0.f};
                for (int ch = 0; ch < a.cin; ++ch) {
                    float p;
                    if (a.in_mode == S2_IN_FRAME_U8)
                        p = (float)static_cast<const uint8_t*>(a.in)[((size_t)(wy + fy) * a.FW + (wx + fx)) * a.cin + ch] / 255.0f;
                    else
                        p = in_rows[((size_t)ch * a.fh + fy) * a.fw + fx];
                    e[ch] = (p - a.mean[ch]) * a.range;
                }
                v = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
        if constexpr (is_f16<T>) {
            const f16x4 h = {round16(v.x, am), round16(v.y, am), round16(v.z, am), round16(v.w, am)};
            *reinterpret_cast<f16x4*>(reinterpret_cast<f16*>(lds) + (py * CP_W + px) * ldp + q * 4) = h;
        } else {
            *reinterpret_cast<float4*>(lds + (py * CP_W + px) * ldp + q * 4) = v;
        }
    }
    if constexpr (is_f16<T>) raise_range(a.status, am);
    __syncthreads();

    const int r2 = a.shuffle * a.shuffle, ncc = a.cout / r2;
    const float* res = a.res ? a.res + b * px_img * a.cs_res : nullptr;
    float* out_rows = static_cast<float*>(a.out);
    if (a.out_mode == S2_OUT_ROWS) out_rows += b * px_img * r2 * a.cs_out;
    else if (a.out_mode == S2_OUT_F32) out_rows += b * (size_t)ncc * a.oh * a.ow;
    const int out_y = wy * a.up, out_x = wx * a.up, out_pitch = a.tile > 0 ? a.FW * a.up : a.ow;      // U8: the window's place in the frame
    for (int ni = wave; ni < (a.coutp >> 4); ni += 4) {
        f32x4 acc[S2_CONV_TH];
#pragma unroll
        for (int i = 0; i < S2_CONV_TH; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - ky * 3;
            if constexpr (is_f16<T>) {      // one accumulator per pixel row as below; K = cin16 a tap
                const f16* ap = reinterpret_cast<const f16*>(lds) + (ky * CP_W + (lane & 15) + kx) * ldp;
                const f16* bp = static_cast<const f16*>(a.wh) + ((size_t)tap * a.coutp + ni * 16 + (lane & 15)) * cin16;
                mma_n<S2_CONV_TH>(ap, CP_W * ldp, bp, 1, cin16, acc);
                continue;
            }
            const float* ap = lds + (ky * CP_W + (lane & 15) + kx) * ldp + (lane >> 4);
            const float* bp = a.w + (size_t)(tap * a.cinp + (lane >> 4)) * a.coutp + ni * 16 + (lane & 15);
            int c = 0;
            for (; c + 16 <= a.cinp; c += 16) {      // four weight fragments in flight; the MFMAs stay in ascending c
                float b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) b[u] = bp[(size_t)(c + 4 * u) * a.coutp];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int i = 0; i < S2_CONV_TH; ++i) acc[i] = mfma4(ap[i * CP_W * ldp + c + 4 * u], b[u], acc[i]);
                }
            }
            for (; c < a.cinp; c += 4) {
                const float b = bp[(size_t)c * a.coutp];
#pragma unroll
                for (int i = 0; i < S2_CONV_TH; ++i) acc[i] = mfma4(ap[i * CP_W * ldp + c], b, acc[i]);
            }
        }
        const int c = ni * 16 + (lane & 15);
        const float bias = a.bias[c];
#pragma unroll
        for (int i = 0; i < S2_CONV_TH; ++i) {
            const int y = y0 + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = x0 + (lane >> 4) * 4 + r;
                if (y >= a.H || x >= a.W) continue;
                float v = acc[i][r] + bias;
                if (a.lrelu) v = v >= 0.f ? v : v * a.slope;
                if (res) v += res[((size_t)y * a.W + x) * a.cs_res + c];      // c < coutp <= cs_res
                if (a.out_mode == S2_OUT_ROWS && a.shuffle == 1) {
                    out_rows[((size_t)y * a.W + x) * a.cs_out + c] = v;      // coutp == cs_out: the zero columns too
                    continue;
                }
                if (c >= a.cout) continue;
                const int cc = c / r2, rem = c - cc * r2, r1 = rem / a.shuffle;
                const int oy = y * a.shuffle + r1, ox = x * a.shuffle + (rem - r1 * a.shuffle);
                if (a.out_mode == S2_OUT_ROWS) {
                    out_rows[((size_t)oy * (a.W * a.shuffle) + ox) * a.cs_out + cc] = v;
                    continue;
                }
                if (oy >= a.oh || ox >= a.ow) continue;
                v = v / a.range + a.mean[cc];
                if (a.out_mode == S2_OUT_F32) {
                    out_rows[((size_t)cc * a.oh + oy) * a.ow + ox] = v;
                } else {
                    if (oy < cy0 || oy >= cy1 || ox < cx0 || ox >= cx1) continue;      // a tile stores its core alone
                    v = fminf(fmaxf(v, 0.f), 1.f) * 255.0f;
                    static_cast<uint8_t*>(a.out)[((size_t)(out_y + oy) * out_pitch + (out_x + ox)) * ncc + cc] = (uint8_t)rintf(v);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- token rows
// T = f16 (a launch with w1): the input tile is [32][cs + 8] halves at the head of A's region and, with w2, the GELU output
// [32][n1p + 8] halves at the head of Hb's; the last product's result is f32 in its f32 place (A's tile is dead by then).  The
// weights are a.w1h [n1p][cs] and a.w2h [cs][n1p].
template <class T>
__global__ __launch_bounds__(256) void s2_rows_kernel(const S2Rows a) {
    extern __shared__ float lds[];
    const int lda = a.cs + 4, ldh = a.n1p + 4;
    float* A = lds;                      // [32][lda]
    float* Hb = lds + S2_BM * lda;       // [32][ldh]
    const int t = threadIdx.x, r8 = t >> 3, s8 = t & 7;
    const int row0 = blockIdx.x * S2_BM, grow = row0 + r8;
    const bool live = grow < a.m;
    float* cur = A;
    int ldcur = lda;

    if constexpr (is_f16<T>) {
        f16* Ah = reinterpret_cast<f16*>(A);
        f16* Hh = reinterpret_cast<f16*>(Hb);
        const int ldah = a.cs + 8, ldhh = a.n1p + 8;
        unsigned am = 0;
        for (int c = s8 * 4; c < a.cs; c += 32) {
            const float4 v = live ? *reinterpret_cast<const float4*>(a.in + (size_t)grow * a.cs + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            const f16x4 h = {round16(v.x, am), round16(v.y, am), round16(v.z, am), round16(v.w, am)};
            *reinterpret_cast<f16x4*>(Ah + r8 * ldah + c) = h;
        }
        __syncthreads();
        const float* b1 = a.b1;
        const int gelu = a.gelu;
        const bool second = a.w2 != nullptr;
        wg_gemm(Ah, ldah, S2_BM / 16, a.cs, static_cast<const f16*>(a.w1h), 1, a.cs, a.n1p >> 4, [&](int i, int j, float v) {
            v += b1[j];
            if (gelu) v = gelu_erf(v);
            if (second) Hh[i * ldhh + j] = round16(v, am);
            else Hb[i * ldh + j] = v;
        });
        __syncthreads();
        cur = Hb, ldcur = ldh;
        if (second) {
            const float* b2 = a.b2;
            wg_gemm(Hh, ldhh, S2_BM / 16, a.n1p, static_cast<const f16*>(a.w2h), 1, a.n1p, a.cs >> 4, [=](int i, int j, float v) { A[i * lda + j] = v + b2[j]; });
            __syncthreads();
            cur = A, ldcur = lda;
        }
        raise_range(a.status, am);
    } else {
    for (int c = s8 * 4; c < a.cs; c += 32)
        *reinterpret_cast<float4*>(A + r8 * lda + c) = live ? *reinterpret_cast<const float4*>(a.in + (size_t)grow * a.cs + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    if (a.w1) {
        const float* b1 = a.b1;
        const int gelu = a.gelu;
        wg_gemm(A, lda, S2_BM / 16, a.cs, a.w1, a.n1p, 1, a.n1p >> 4, [=](int i, int j, float v) {
            v += b1[j];
            Hb[i * ldh + j] = gelu ? gelu_erf(v) : v;
        });
        __syncthreads();
        cur = Hb, ldcur = ldh;
        if (a.w2) {
            const float* b2 = a.b2;
            wg_gemm(Hb, ldh, S2_BM / 16, a.n1p, a.w2, a.cs, 1, a.cs >> 4, [=](int i, int j, float v) { A[i * lda + j] = v + b2[j]; });
            __syncthreads();
            cur = A, ldcur = lda;
        }
    }
    }
    float* rp = cur + r8 * ldcur;
    float mean = 0.f, rstd = 1.f;
    if (a.ln_g) row_stats(rp, a.c, s8, a.eps, mean, rstd);
    if (!live) return;
    for (int j = s8; j < a.cs; j += 8) {
        float v = rp[j];
        if (a.ln_g) v = (v - mean) * rstd * a.ln_g[j] + a.ln_b[j];      // gain and bias are zero past c
        if (a.res) v += a.res[(size_t)grow * a.cs + j];
        a.out[(size_t)grow * a.cs + j] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- window attention
__device__ __forceinline__ int region_of(int i, int n, int ws, int shift) { return (i >= n - ws ? 1 : 0) + (i >= n - shift ? 1 : 0); }

__global__ __launch_bounds__(S2_ATTN_THREADS) void s2_attn_kernel(const S2Attn a) {
    extern __shared__ float lds[];
    const int n = a.ws * a.ws, np = (n + 15) & ~15, mt = np >> 4;
    const int ldc = a.cs + 4, ldq = 3 * a.dp + 4, lds_s = np + 4;
    float* X = lds;                       // [np][ldc] the window's tokens; later output.dense's result
    float* CTX = X + np * ldc;            // [np][ldc]
    float* QKV = CTX + np * ldc;          // [np][ldq] one head's q | k | v
    float* S = QKV + np * ldq;            // [np][lds_s] one head's scores
    int* tok = reinterpret_cast<int*>(S + np * lds_s);      // [np] the token's row in memory, -1 past n
    int* reg = tok + np;                                    // [np] its region
    const int t = threadIdx.x, r8 = t >> 3, s8 = t & 7, rpp = S2_ATTN_THREADS / 8;      // row-wise work: 8 threads a row, rpp rows a pass
    const size_t img = (size_t)blockIdx.z * a.H * a.W * a.cs;      // the window's image; tokens, the shift and the regions are its own
    const float* in = a.in + img;
    float* out = a.out + img;

    for (int i = t; i < np; i += S2_ATTN_THREADS) {
        int tk = -1, rg = -1;
        if (i < n) {
            const int iy = i / a.ws, ry = blockIdx.y * a.ws + iy, rx = blockIdx.x * a.ws + (i - iy * a.ws);      // in the rolled grid
            tk = ((ry + a.shift) % a.H) * a.W + (rx + a.shift) % a.W;                                            // roll(-s, -s) reads from + s
            rg = a.shift > 0 ? region_of(ry, a.H, a.ws, a.shift) * 3 + region_of(rx, a.W, a.ws, a.shift) : 0;
        }
        tok[i] = tk, reg[i] = rg;
    }
    __syncthreads();
    for (int i = r8; i < np; i += rpp) {
        const int tk = tok[i];
        for (int c = s8 * 4; c < a.cs; c += 32) {
            *reinterpret_cast<float4*>(X + i * ldc + c) = tk >= 0 ? *reinterpret_cast<const float4*>(in + (size_t)tk * a.cs + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(CTX + i * ldc + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __syncthreads();

    for (int h = 0; h < a.heads; ++h) {
        {   // q | k | v of the head
            const float* bq = a.bqkv + h * 3 * a.dp;
            wg_gemm(X, ldc, mt, a.cs, a.wqkv + h * 3 * a.dp, a.heads * 3 * a.dp, 1, (3 * a.dp) >> 4, [=](int i, int j, float v) { QKV[i * ldq + j] = v + bq[j]; });
        }
        __syncthreads();
        for (int i = r8; i < np; i += rpp) {      // F.normalize(q), F.normalize(k): x / max(|x|, 1e-12); the padded columns are zero
            for (int part = 0; part < 2; ++part) {
                float* p = QKV + i * ldq + part * a.dp;
                float ss = 0.f;
                for (int j = s8; j < a.dp; j += 8) ss += p[j] * p[j];
                const float nrm = fmaxf(sqrtf(sum8(ss)), 1e-12f);
                for (int j = s8; j < a.dp; j += 8) p[j] = p[j] / nrm;
            }
        }
        __syncthreads();
        {   // S = q k^T x temperature + bias + mask; a key past n scores -inf
            const float sc = a.scale[h];
            const float* bias = a.bias + (size_t)h * n * n;
            const int shift = a.shift;
            wg_gemm(QKV, ldq, mt, a.dp, QKV + a.dp, 1, ldq, mt, [=](int i, int j, float v) {
                float s = -INFINITY;
                if (j < n) {
                    s = v * sc;
                    if (i < n) s += bias[i * n + j];
                    if (shift > 0 && i < n && reg[i] != reg[j]) s = (s + -100.0f) + -100.0f;      // transformers adds its mask twice
                }
                S[i * lds_s + j] = s;
            });
        }
        __syncthreads();
        for (int i = r8; i < np; i += rpp) {
            float* sp = S + i * lds_s;
            float m = -INFINITY;
            for (int j = s8; j < np; j += 8) m = fmaxf(m, sp[j]);
            m = max8(m);
            float sum = 0.f;
            for (int j = s8; j < np; j += 8) {
                const float p = expf(sp[j] - m);
                sp[j] = p;
                sum += p;
            }
            sum = sum8(sum);
            for (int j = s8; j < np; j += 8) sp[j] = sp[j] / sum;
        }
        __syncthreads();
        {   // context[:, head] = P V
            const int d = a.d, col0 = h * a.d;
            wg_gemm(S, lds_s, mt, np, QKV + 2 * a.dp, ldq, 1, a.dp >> 4, [=](int i, int j, float v) {
                if (j < d) CTX[i * ldc + col0 + j] = v;
            });
        }
        __syncthreads();
    }

    {   // output.dense -> X
        const float* bo = a.bo;
        wg_gemm(CTX, ldc, mt, a.cs, a.wo, a.cs, 1, a.cs >> 4, [=](int i, int j, float v) { X[i * ldc + j] = v + bo[j]; });
    }
    __syncthreads();
    for (int i = r8; i < np; i += rpp) {
        const int tk = tok[i];
        float mean, rstd;
        row_stats(X + i * ldc, a.c, s8, a.eps, mean, rstd);
        if (tk < 0) continue;
        for (int j = s8; j < a.cs; j += 8) {
            const float v = (X[i * ldc + j] - mean) * rstd * a.ln_g[j] + a.ln_b[j];      // zero past c
            out[(size_t)tk * a.cs + j] = in[(size_t)tk * a.cs + j] + v;
        }
    }
}

// The fp16 form of the block above, inside the same LDS regions: X's holds the tokens [np][cs + 8] halves and, at the end,
// output.dense's f32 result; CTX's the context [np][cs + 8] halves; QKV's one head's q | k as f32 [np][2 dp + 4], normalised
// and rounded in place (q^ at half 0 of the row, k^ at half 2 dp), then V^T [dp][np + 8] halves; S's the f32 scores, whose softmax
// is rounded in place (P at half 0 of the row).  The weights are a.wqkvh [heads 3 dp][cs] and a.woh [cs][cs].
__global__ __launch_bounds__(S2_ATTN_THREADS) void s2_attn_f16_kernel(const S2Attn a) {
    extern __shared__ float lds[];
    const int n = a.ws * a.ws, np = (n + 15) & ~15, mt = np >> 4;
    const int ldc = a.cs + 4, ldq = 3 * a.dp + 4, lds_s = np + 4;
    float* X = lds;
    float* CTX = X + np * ldc;
    float* QK = CTX + np * ldc;
    float* S = QK + np * ldq;
    int* tok = reinterpret_cast<int*>(S + np * lds_s);
    int* reg = tok + np;
    const int ldxh = a.cs + 8, ldqk = 2 * a.dp + 4, ldv = np + 8;
    f16* Xh = reinterpret_cast<f16*>(X);
    f16* CTXh = reinterpret_cast<f16*>(CTX);
    f16* Vt = reinterpret_cast<f16*>(QK + np * ldqk);      // np (2 dp + 4) floats + dp (np + 8) halves <= np (3 dp + 4) floats for np >= 8
    const f16* QKh = reinterpret_cast<const f16*>(QK);
    const f16* Ph = reinterpret_cast<const f16*>(S);
    const int t = threadIdx.x, r8 = t >> 3, s8 = t & 7, rpp = S2_ATTN_THREADS / 8;
    const size_t img = (size_t)blockIdx.z * a.H * a.W * a.cs;
    const float* in = a.in + img;
    float* out = a.out + img;
    unsigned am = 0;

    for (int i = t; i < np; i += S2_ATTN_THREADS) {
        int tk = -1, rg = -1;
        if (i < n) {
            const int iy = i / a.ws, ry = blockIdx.y * a.ws + iy, rx = blockIdx.x * a.ws + (i - iy * a.ws);
            tk = ((ry + a.shift) % a.H) * a.W + (rx + a.shift) % a.W;
            rg = a.shift > 0 ? region_of(ry, a.H, a.ws, a.shift) * 3 + region_of(rx, a.W, a.ws, a.shift) : 0;
        }
        tok[i] = tk, reg[i] = rg;
    }
    __syncthreads();
    for (int i = r8; i < np; i += rpp) {
        const int tk = tok[i];
        for (int c = s8 * 4; c < a.cs; c += 32) {
            const float4 v = tk >= 0 ? *reinterpret_cast<const float4*>(in + (size_t)tk * a.cs + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            const f16x4 h = {round16(v.x, am), round16(v.y, am), round16(v.z, am), round16(v.w, am)};
            *reinterpret_cast<f16x4*>(Xh + i * ldxh + c) = h;
            *reinterpret_cast<f16x4*>(CTXh + i * ldxh + c) = f16x4{(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
        }
    }
    __syncthreads();

    for (int h = 0; h < a.heads; ++h) {
        {   // q | k as f32, v rounded and transposed
            const float* bq = a.bqkv + h * 3 * a.dp;
            const int dp2 = 2 * a.dp;
            wg_gemm(Xh, ldxh, mt, a.cs, static_cast<const f16*>(a.wqkvh) + (size_t)h * 3 * a.dp * a.cs, 1, a.cs, (3 * a.dp) >> 4, [&](int i, int j, float v) {
                v += bq[j];
                if (j < dp2) QK[i * ldqk + j] = v;
                else Vt[(j - dp2) * ldv + i] = round16(v, am);
            });
        }
        __syncthreads();
        // x / max(|x|, 1e-12) of the f32 q and k, rounded over the row's own values.  The norm and the quotient are evaluated in
        // double, so q^ carries one rounding, not the four of the f32 chain (squares, sum, root, quotient): a q^ within those
        // 1.5 ulp of an f16 rounding boundary would round the other way, and the temperature multiplies that f16 ulp by up to 100.
        for (int i = r8; i < np; i += rpp) {
            for (int part = 0; part < 2; ++part) {
                float* p = QK + i * ldqk + part * a.dp;
                double ss = 0.0;
                for (int j = s8; j < a.dp; j += 8) {
                    const double v = p[j];
                    ss += v * v;
                }
                const double inv = 1.0 / fmax(sqrt(sum8(ss)), 1e-12);
                for (int j = s8; j < a.dp; j += 8) round_in_place(p, j, (float)(load_in_place(p, j) * inv), am);
            }
        }
        __syncthreads();
        {
            const float sc = a.scale[h];
            const float* bias = a.bias + (size_t)h * n * n;
            const int shift = a.shift;
            wg_gemm(QKh, 2 * ldqk, mt, a.dp, QKh + 2 * a.dp, 1, 2 * ldqk, mt, [=](int i, int j, float v) {
                float s = -INFINITY;
                if (j < n) {
                    s = v * sc;
                    if (i < n) s += bias[i * n + j];
                    if (shift > 0 && i < n && reg[i] != reg[j]) s = (s + -100.0f) + -100.0f;
                }
                S[i * lds_s + j] = s;
            });
        }
        __syncthreads();
        for (int i = r8; i < np; i += rpp) {
            float* sp = S + i * lds_s;
            float m = -INFINITY;
            for (int j = s8; j < np; j += 8) m = fmaxf(m, sp[j]);
            m = max8(m);
            float sum = 0.f;
            for (int j = s8; j < np; j += 8) {
                const float p = expf(sp[j] - m);
                sp[j] = p;
                sum += p;
            }
            sum = sum8(sum);
            for (int j = s8; j < np; j += 8) round_in_place(sp, j, load_in_place(sp, j) / sum, am);
        }
        __syncthreads();
        {   // context[:, head] = P V, rounded for output.dense
            const int d = a.d, col0 = h * a.d;
            wg_gemm(Ph, 2 * lds_s, mt, np, Vt, 1, ldv, a.dp >> 4, [&](int i, int j, float v) {
                if (j < d) CTXh[i * ldxh + col0 + j] = round16(v, am);
            });
        }
        __syncthreads();
    }

    {   // output.dense -> X (f32; the tokens' halves are dead)
        const float* bo = a.bo;
        wg_gemm(CTXh, ldxh, mt, a.cs, static_cast<const f16*>(a.woh), 1, a.cs, a.cs >> 4, [=](int i, int j, float v) { X[i * ldc + j] = v + bo[j]; });
    }
    raise_range(a.status, am);
    __syncthreads();
    for (int i = r8; i < np; i += rpp) {
        const int tk = tok[i];
        float mean, rstd;
        row_stats(X + i * ldc, a.c, s8, a.eps, mean, rstd);
        if (tk < 0) continue;
        for (int j = s8; j < a.cs; j += 8) {
            const float v = (X[i * ldc + j] - mean) * rstd * a.ln_g[j] + a.ln_b[j];
            out[(size_t)tk * a.cs + j] = in[(size_t)tk * a.cs + j] + v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ overlapped tiles, averaged
// Both kernels walk the padded output in flat pixel order, four consecutive pixels a thread (a group may run over a row's end):
// E is planar with planes of a multiple of four floats, so a group is one aligned 16-byte access a channel and a wave's accesses
// are contiguous.  A group belongs to one thread in every launch; nothing is shared, nothing atomic.  HBM-bound.

// E[pixel] += Y[window][pixel - the window's origin] for the batch's windows that cover the pixel, in ascending tile index
// (tile rows outer, tiles of a row inner: the row-major order of the plan).  Groups [g0, g1) are the rows the batch's tiles touch.
__global__ __launch_bounds__(256) void s2_overlap_add_kernel(const S2Overlap a, size_t g0, size_t g1) {
    const size_t g = g0 + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= g1) return;
    const int OW = a.PW * a.up, ts = a.t * a.up, t1 = a.tile0 + a.batch;
    const size_t npx = (size_t)a.PH * a.up * OW, plane = s2_overlap_plane(a.PH, a.PW, a.up);
    int oy[4], ox[4], fy[4], ly[4], fx[4], lx[4];
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const size_t p = 4 * g + j;
        fy[j] = 0, ly[j] = -1, fx[j] = 0, lx[j] = -1;      // past the last pixel: no tile
        if (p >= npx) continue;
        oy[j] = (int)(p / OW), ox[j] = (int)(p - (size_t)oy[j] * OW);
        int cnt, st;
        s2_overlap_axis(a.PH, a.t, a.step, 0, oy[j] / a.up, cnt, st, fy[j], ly[j]);
        s2_overlap_axis(a.PW, a.t, a.step, 0, ox[j] / a.up, cnt, st, fx[j], lx[j]);
        any = any || (fy[j] * a.tiles_x + fx[j] < t1 && ly[j] * a.tiles_x + lx[j] >= a.tile0);
    }
    if (!any) return;
    float4* E = reinterpret_cast<float4*>(a.E) + g;
    float e[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float4 v = E[ch * (plane / 4)];
        e[ch][0] = v.x, e[ch][1] = v.y, e[ch][2] = v.z, e[ch][3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        for (int ty = fy[j]; ty <= ly[j]; ++ty)
            for (int tx = fx[j]; tx <= lx[j]; ++tx) {
                const int ti = ty * a.tiles_x + tx;
                if (ti < a.tile0 || ti >= t1) continue;
                int cnt, wy, wx, f, l;
                s2_overlap_axis(a.PH, a.t, a.step, ty, 0, cnt, wy, f, l);
                s2_overlap_axis(a.PW, a.t, a.step, tx, 0, cnt, wx, f, l);
                const float* y = a.Y + ((size_t)(ti - a.tile0) * 3 * ts + (oy[j] - wy * a.up)) * ts + (ox[j] - wx * a.up);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) e[ch][j] += y[(size_t)ch * ts * ts];
            }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) E[ch * (plane / 4)] = make_float4(e[ch][0], e[ch][1], e[ch][2], e[ch][3]);
}

// out = quantise(E / the number of tiles that covered the pixel) on the crop oh x ow: the count is cnt_y cnt_x, each the length of
// s2_overlap_axis's covering run; a true f32 division.  Groups [0, groups) hold the crop's rows.
__global__ __launch_bounds__(256) void s2_overlap_finish_kernel(const S2Overlap a, size_t groups) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const int OW = a.PW * a.up;
    const size_t plane = s2_overlap_plane(a.PH, a.PW, a.up);
    const float4* E = reinterpret_cast<const float4*>(a.E) + g;
    float e[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float4 v = E[ch * (plane / 4)];
        e[ch][0] = v.x, e[ch][1] = v.y, e[ch][2] = v.z, e[ch][3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const size_t p = 4 * g + j;
        const int oy = (int)(p / OW), ox = (int)(p - (size_t)oy * OW);
        if (oy >= a.oh || ox >= a.ow) continue;
        int cnt, st, fy, ly, fx, lx;
        s2_overlap_axis(a.PH, a.t, a.step, 0, oy / a.up, cnt, st, fy, ly);
        s2_overlap_axis(a.PW, a.t, a.step, 0, ox / a.up, cnt, st, fx, lx);
        const float n = (float)((ly - fy + 1) * (lx - fx + 1));
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float v = fminf(fmaxf(e[ch][j] / n, 0.f), 1.f) * 255.0f;
            a.out[((size_t)oy * a.ow + ox) * 3 + ch] = (uint8_t)rintf(v);
        }
    }
}

template <class K, class A>
hipError_t launch_lds(K kernel, const A& a, dim3 grid, int threads, size_t bytes, unsigned long long& done, hipStream_t s) {
    if (bytes > S2_LDS_LIMIT) return hipErrorInvalidValue;
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), S2_LDS_LIMIT, done);
    if (e != hipSuccess) return e;
    kernel<<<grid, dim3(threads), bytes, s>>>(a);
    return hipGetLastError();
}

}  // namespace

// f16: [6 x 18][cin16 + 8] halves, which is no more than the f32 patch from 20 input channels on (a few KiB below that)
size_t s2_conv_lds_bytes(const S2Conv& a) {
    if (a.f16) return (size_t)CP_H * CP_W * (conv_cin16(a.cin) + 8) * sizeof(f16);
    return (size_t)CP_H * CP_W * conv_ldp(a.cinp) * sizeof(float);
}

size_t s2_rows_lds_bytes(const S2Rows& a) { return (size_t)S2_BM * ((a.cs + 4) + (a.w1 ? a.n1p + 4 : 0)) * sizeof(float); }

size_t s2_attn_lds_bytes(const S2Attn& a) {
    const size_t np = (size_t)((a.ws * a.ws + 15) & ~15);
    return np * (2 * (a.cs + 4) + (3 * a.dp + 4) + (np + 4)) * sizeof(float) + 2 * np * sizeof(int);
}

hipError_t launch_s2_conv(const S2Conv& a, hipStream_t s) {
    // the shapes the tiles, the float4 loads and the index maps rest on
    if (!a.in || !a.w || !a.bias || !a.out || a.H < 1 || a.W < 1 || a.cin < 1 || a.cinp % 4 || a.cinp < a.cin || a.cout < 1 || a.coutp % 16 || a.coutp < a.cout)
        return hipErrorInvalidValue;
    if ((a.in_mode == S2_IN_ROWS || a.in_mode == S2_IN_NEAREST2) && (a.cs_in % 4 || a.cs_in < a.cinp)) return hipErrorInvalidValue;
    if (a.in_mode == S2_IN_NEAREST2 && (a.H % 2 || a.W % 2)) return hipErrorInvalidValue;
    if (a.in_mode == S2_IN_FRAME_U8 || a.in_mode == S2_IN_FRAME_F32) {
        if (a.cin > 4 || a.cinp != 4 || a.fh < 1 || a.fw < 1 || a.mh < a.fh || a.mw < a.fw || a.H < a.mh || a.W < a.mw) return hipErrorInvalidValue;
        if (a.H - a.mh > a.mh - 1 || a.W - a.mw > a.mw - 1) return hipErrorInvalidValue;      // a reflection reaches at most n - 1
    } else if (a.in_mode == S2_IN_WINDOW_U8) {      // every window lies inside the padded frame; sym_index takes any distance
        if (a.cin > 4 || a.cinp != 4 || a.tile != 0 || a.H != a.W || a.ov_step < 1 || a.ov_step > a.H || a.FH < 1 || a.FW < 1 || a.PH < a.FH || a.PW < a.FW ||
            a.H > a.PH || a.W > a.PW || a.tile0 < 0)
            return hipErrorInvalidValue;
        int ny, nx, v, f, l;
        s2_overlap_axis(a.PH, a.H, a.ov_step, 0, 0, ny, v, f, l);
        s2_overlap_axis(a.PW, a.W, a.ov_step, 0, 0, nx, v, f, l);
        if (a.tiles_x != nx || (long long)a.tile0 + a.batch > (long long)ny * nx) return hipErrorInvalidValue;
    } else if (a.in_mode != S2_IN_ROWS && a.in_mode != S2_IN_NEAREST2) {
        return hipErrorInvalidValue;
    }
    if (a.res && a.cs_res < a.coutp) return hipErrorInvalidValue;
    if (a.shuffle < 1 || a.cout % (a.shuffle * a.shuffle)) return hipErrorInvalidValue;
    const int ncc = a.cout / (a.shuffle * a.shuffle);
    if (a.out_mode == S2_OUT_ROWS) {
        if (a.shuffle == 1 ? a.cs_out != a.coutp : a.cs_out != ncc) return hipErrorInvalidValue;
    } else if (a.out_mode == S2_OUT_F32 || a.out_mode == S2_OUT_U8) {
        if (ncc > 4 || a.oh < 1 || a.ow < 1 || a.oh > a.H * a.shuffle || a.ow > a.W * a.shuffle) return hipErrorInvalidValue;
    } else {
        return hipErrorInvalidValue;
    }
    if (a.batch < 1 || a.batch > 65535) return hipErrorInvalidValue;
    const bool u8_in = a.in_mode == S2_IN_FRAME_U8, u8_out = a.out_mode == S2_OUT_U8;
    if (a.tile > 0) {      // image b is a tile of the FH x FW frame: every window read and every core written lies inside it
        if (!(u8_in || u8_out) || a.tile_pad < 0 || a.tile > (1 << 24) || a.tile_pad > (1 << 24) || a.FH < 1 || a.FW < 1 || a.up < 1 || a.tile0 < 0)
            return hipErrorInvalidValue;
        const int sy = s2_window_side(a.FH, a.tile, a.tile_pad), sx = s2_window_side(a.FW, a.tile, a.tile_pad);
        const long long ty = (a.FH + a.tile - 1) / a.tile, tx = (a.FW + a.tile - 1) / a.tile;
        if (a.tiles_x != tx || (long long)a.tile0 + a.batch > ty * tx) return hipErrorInvalidValue;
        if (u8_in && (a.fh != sy || a.fw != sx)) return hipErrorInvalidValue;
        if (u8_out && (a.oh != sy * a.up || a.ow != sx * a.up)) return hipErrorInvalidValue;
    } else if ((u8_in || u8_out) && a.batch != 1) {
        return hipErrorInvalidValue;      // u8 frames come one at a time, or as the tiles of one
    }
    static unsigned long long done = 0, done16 = 0;
    const dim3 grid((a.W + S2_CONV_TW - 1) / S2_CONV_TW, (a.H + S2_CONV_TH - 1) / S2_CONV_TH, a.batch);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (a.f16) {      // token rows in, both operands rounded; a frame-loading conv is never asked for in this form
        if (!a.wh || !a.status || (a.in_mode != S2_IN_ROWS && a.in_mode != S2_IN_NEAREST2)) return hipErrorInvalidValue;
        return launch_lds(&s2_conv_kernel<f16>, a, grid, 256, s2_conv_lds_bytes(a), done16, s);
    }
    return launch_lds(&s2_conv_kernel<float>, a, grid, 256, s2_conv_lds_bytes(a), done, s);
}

hipError_t launch_s2_rows(const S2Rows& a, hipStream_t s) {
    if (!a.in || !a.out || a.m < 1 || a.c < 1 || a.cs % 16 || a.cs < a.c) return hipErrorInvalidValue;
    if (a.w1 && (!a.b1 || a.n1p < 16 || a.n1p % 16 || (!a.w2 && a.n1p != a.cs))) return hipErrorInvalidValue;
    if (a.w2 && (!a.w1 || !a.b2)) return hipErrorInvalidValue;
    if (a.ln_g && !a.ln_b) return hipErrorInvalidValue;
    if (a.m > S2_ROWS_MAX) return hipErrorInvalidValue;      // the row index (and m + 31) stays an int; row x cs is size_t in the kernel
    static unsigned long long done = 0, done16 = 0;
    if (a.f16 && a.w1) {      // a launch without a product has nothing to round
        if (!a.w1h || (a.w2 && !a.w2h) || !a.status) return hipErrorInvalidValue;
        return launch_lds(&s2_rows_kernel<f16>, a, dim3((a.m + S2_BM - 1) / S2_BM), 256, s2_rows_lds_bytes(a), done16, s);
    }
    return launch_lds(&s2_rows_kernel<float>, a, dim3((a.m + S2_BM - 1) / S2_BM), 256, s2_rows_lds_bytes(a), done, s);
}

hipError_t launch_s2_attn(const S2Attn& a, hipStream_t s) {
    if (!a.in || !a.out || !a.wqkv || !a.bqkv || !a.scale || !a.bias || !a.wo || !a.bo || !a.ln_g || !a.ln_b) return hipErrorInvalidValue;
    if (a.ws < 1 || a.H < a.ws || a.W < a.ws || a.H % a.ws || a.W % a.ws || a.shift < 0 || a.shift >= a.ws) return hipErrorInvalidValue;
    if (a.heads < 1 || a.d < 1 || a.c != a.heads * a.d || a.dp % 16 || a.dp < a.d || a.cs % 16 || a.cs < a.c) return hipErrorInvalidValue;
    if (a.batch < 1 || a.batch > 65535) return hipErrorInvalidValue;
    static unsigned long long done = 0, done16 = 0;
    const dim3 grid(a.W / a.ws, a.H / a.ws, a.batch);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (a.f16) {
        if (!a.wqkvh || !a.woh || !a.status) return hipErrorInvalidValue;
        return launch_lds(&s2_attn_f16_kernel, a, grid, S2_ATTN_THREADS, s2_attn_lds_bytes(a), done16, s);
    }
    return launch_lds(&s2_attn_kernel, a, grid, S2_ATTN_THREADS, s2_attn_lds_bytes(a), done, s);
}

// the plan the two overlap kernels index by: E and Y are sized from it by the caller
static bool overlap_shape_ok(const S2Overlap& a) {
    if (!a.E || a.PH < 1 || a.PW < 1 || a.t < 1 || a.t > a.PH || a.t > a.PW || a.step < 1 || a.step > a.t || a.up < 1 || a.up > 8) return false;
    if ((long long)a.PH * a.up * a.PW * a.up > (1ll << 36)) return false;
    int ny, nx, v, f, l;
    s2_overlap_axis(a.PH, a.t, a.step, 0, 0, ny, v, f, l);
    s2_overlap_axis(a.PW, a.t, a.step, 0, 0, nx, v, f, l);
    return a.tiles_y == ny && a.tiles_x == nx && (long long)ny * nx <= 0x7fffffff;
}

hipError_t launch_s2_overlap_add(const S2Overlap& a, hipStream_t s) {
    if (!overlap_shape_ok(a) || !a.Y || a.tile0 < 0 || a.batch < 1 || (long long)a.tile0 + a.batch > (long long)a.tiles_y * a.tiles_x) return hipErrorInvalidValue;
    int cnt, y0, y1, f, l;      // the output rows between the first tile row's top and the last one's bottom
    s2_overlap_axis(a.PH, a.t, a.step, a.tile0 / a.tiles_x, 0, cnt, y0, f, l);
    s2_overlap_axis(a.PH, a.t, a.step, (a.tile0 + a.batch - 1) / a.tiles_x, 0, cnt, y1, f, l);
    const size_t row = (size_t)a.PW * a.up, g0 = (size_t)y0 * a.up * row / 4, g1 = ((size_t)(y1 + a.t) * a.up * row + 3) / 4;
    const size_t blocks = (g1 - g0 + 255) / 256;
    if (blocks < 1 || blocks > 0x7fffffffu) return hipErrorInvalidValue;
    s2_overlap_add_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(a, g0, g1);
    return hipGetLastError();
}

hipError_t launch_s2_overlap_finish(const S2Overlap& a, hipStream_t s) {
    if (!overlap_shape_ok(a) || !a.out || a.oh < 1 || a.ow < 1 || a.oh > a.PH * a.up || a.ow > a.PW * a.up) return hipErrorInvalidValue;
    const size_t groups = ((size_t)a.oh * a.PW * a.up + 3) / 4, blocks = (groups + 255) / 256;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    s2_overlap_finish_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(a, groups);
    return hipGetLastError();
}

}  // namespace nesr
