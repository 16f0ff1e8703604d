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
// MFMA operand maps (16x16x4 f32): lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result register r of lane
// l is D[row 4 (l >> 4) + r][col l & 15].  Widths are padded to the tile with zeros (swin2sr_api.h).  No atomics, no workgroup
// waits on another: a forward repeated gives the same bits.  Every global load and store is guarded by the token count, the
// image extent and the real width.
//
// A launch takes a batch of images of one padded size (the tiles of a large frame, nesr_swin2sr_upscale_tiled_u8): the conv and the
// attention kernel read the image from blockIdx.z and offset their bases by it; zero padding, the cyclic shift and the region mask
// stay inside the image.  The row kernel sees batch * H * W rows.  A batch of one runs the arithmetic of a whole frame unchanged.
#include "swin2sr_api.h"

#include "nesr_kernels.h"

namespace nesr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

__device__ __forceinline__ float sum8(float v) {
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

// D[16 mt][16 nt] = A[16 mt][K] x B[K][16 nt] by the workgroup's waves; A in LDS (row stride lda), B(k, n) = B[k sbk + n sbn] in
// LDS or memory; K a multiple of 16.  store(row, col, value) gets every element once.
template <class Store>
__device__ __forceinline__ void wg_gemm(const float* A, int lda, int mt, int K, const float* B, int sbk, int sbn, int nt, Store store) {
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
        const float* ap = A + (m0 * 16 + (lane & 15)) * lda + (lane >> 4);
        const float* bp = B + (size_t)(lane >> 4) * sbk + (size_t)(ni * 16 + (lane & 15)) * sbn;
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

__global__ __launch_bounds__(256) void s2_conv_kernel(const S2Conv a) {
    extern __shared__ float lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int x0 = blockIdx.x * S2_CONV_TW, y0 = blockIdx.y * S2_CONV_TH;
    const int ldp = conv_ldp(a.cinp), nq = a.cinp >> 2;
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
    const float* in_rows = static_cast<const float*>(a.in);
    if (a.in_mode == S2_IN_ROWS) in_rows += b * px_img * a.cs_in;
    else if (a.in_mode == S2_IN_NEAREST2) in_rows += b * (size_t)(a.H >> 1) * (a.W >> 1) * a.cs_in;
    else if (a.in_mode == S2_IN_FRAME_F32) in_rows += b * (size_t)a.cin * a.fh * a.fw;

    for (int idx = t; idx < CP_H * CP_W * nq; idx += 256) {
        const int q = idx % nq, pos = idx / nq, px = pos % CP_W, py = pos / CP_W;
        const int gy = y0 - 1 + py, gx = x0 - 1 + px;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
            if (a.in_mode == S2_IN_ROWS) {
                v = *reinterpret_cast<const float4*>(in_rows + ((size_t)gy * a.W + gx) * a.cs_in + q * 4);
            } else if (a.in_mode == S2_IN_NEAREST2) {
                v = *reinterpret_cast<const float4*>(in_rows + ((size_t)(gy >> 1) * (a.W >> 1) + (gx >> 1)) * a.cs_in + q * 4);
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
        *reinterpret_cast<float4*>(lds + (py * CP_W + px) * ldp + q * 4) = v;
    }
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
__global__ __launch_bounds__(256) void s2_rows_kernel(const S2Rows a) {
    extern __shared__ float lds[];
    const int lda = a.cs + 4, ldh = a.n1p + 4;
    float* A = lds;                      // [32][lda]
    float* Hb = lds + S2_BM * lda;       // [32][ldh]
    const int t = threadIdx.x, r8 = t >> 3, s8 = t & 7;
    const int row0 = blockIdx.x * S2_BM, grow = row0 + r8;
    const bool live = grow < a.m;

    for (int c = s8 * 4; c < a.cs; c += 32)
        *reinterpret_cast<float4*>(A + r8 * lda + c) = live ? *reinterpret_cast<const float4*>(a.in + (size_t)grow * a.cs + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    float* cur = A;
    int ldcur = lda;
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

template <class K, class A>
hipError_t launch_lds(K kernel, const A& a, dim3 grid, int threads, size_t bytes, unsigned long long& done, hipStream_t s) {
    if (bytes > S2_LDS_LIMIT) return hipErrorInvalidValue;
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), S2_LDS_LIMIT, done);
    if (e != hipSuccess) return e;
    kernel<<<grid, dim3(threads), bytes, s>>>(a);
    return hipGetLastError();
}

}  // namespace

size_t s2_conv_lds_bytes(const S2Conv& a) { return (size_t)CP_H * CP_W * conv_ldp(a.cinp) * sizeof(float); }

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
    static unsigned long long done = 0;
    const dim3 grid((a.W + S2_CONV_TW - 1) / S2_CONV_TW, (a.H + S2_CONV_TH - 1) / S2_CONV_TH, a.batch);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    return launch_lds(&s2_conv_kernel, a, grid, 256, s2_conv_lds_bytes(a), done, s);
}

hipError_t launch_s2_rows(const S2Rows& a, hipStream_t s) {
    if (!a.in || !a.out || a.m < 1 || a.c < 1 || a.cs % 16 || a.cs < a.c) return hipErrorInvalidValue;
    if (a.w1 && (!a.b1 || a.n1p < 16 || a.n1p % 16 || (!a.w2 && a.n1p != a.cs))) return hipErrorInvalidValue;
    if (a.w2 && (!a.w1 || !a.b2)) return hipErrorInvalidValue;
    if (a.ln_g && !a.ln_b) return hipErrorInvalidValue;
    if (a.m > S2_ROWS_MAX) return hipErrorInvalidValue;      // the row index (and m + 31) stays an int; row x cs is size_t in the kernel
    static unsigned long long done = 0;
    return launch_lds(&s2_rows_kernel, a, dim3((a.m + S2_BM - 1) / S2_BM), 256, s2_rows_lds_bytes(a), done, s);
}

hipError_t launch_s2_attn(const S2Attn& a, hipStream_t s) {
    if (!a.in || !a.out || !a.wqkv || !a.bqkv || !a.scale || !a.bias || !a.wo || !a.bo || !a.ln_g || !a.ln_b) return hipErrorInvalidValue;
    if (a.ws < 1 || a.H < a.ws || a.W < a.ws || a.H % a.ws || a.W % a.ws || a.shift < 0 || a.shift >= a.ws) return hipErrorInvalidValue;
    if (a.heads < 1 || a.d < 1 || a.c != a.heads * a.d || a.dp % 16 || a.dp < a.d || a.cs % 16 || a.cs < a.c) return hipErrorInvalidValue;
    if (a.batch < 1 || a.batch > 65535) return hipErrorInvalidValue;
    static unsigned long long done = 0;
    const dim3 grid(a.W / a.ws, a.H / a.ws, a.batch);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    return launch_lds(&s2_attn_kernel, a, grid, S2_ATTN_THREADS, s2_attn_lds_bytes(a), done, s);
}

}  // namespace nesr
