// SegFormer (MiT encoder + all-MLP decode head) for gfx950, f32 storage, every product on the f32-input MFMA
// (v_mfma_f32_16x16x4_f32: an exact f32 fmaf chain, so an argmax over 150 logits sees f32 arithmetic and nothing less).
// Stands behind transformers' SegformerForSemanticSegmentation.forward in eval mode, the model the reference runs on every
// iteration (nesr/nesr.py:285-301, 713-716).
//
// Two kernels.  A workgroup of 256 threads (4 waves) owns SEG_BM = 32 token rows in both.
//
//   seg_fused_kernel<A>:  R[32][n1] = A[32][k1] x w1 (+ bias1)      A made on the fly, 32 columns of K at a time: a conv patch
//                         R = LayerNorm(R) | relu(R * s + t) | R += res     (patch embed, sequence reduction), gelu(dwconv3x3)
//                         out1 = R                                   (Mix-FFN), the decode head's upsampled concatenation; or
//                         out2 = R x w2 + bias2  |  argmax           the rows themselves (LayerNorm + projection)
//   seg_attn_kernel:      per head, softmax(q k^T / sqrt(32)) v with K and V of the head in LDS, SEG_KCH keys at a time and an
//                         online softmax across chunks; then o_proj and the residual on the 32 rows.
//
// MFMA operand maps (16x16x4 f32): lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; the result register r
// of lane l is D[row 4 (l >> 4) + r][col l & 15].  Wave w takes m-tile w & 1 and the n-tiles (w >> 1) + 2 i; every product has an even
// number of n-tiles (widths are multiples of 32, key chunks are padded to 32).
// LDS strides: a tile whose row index sits in the lane's low four bits (every A operand, and K as the B operand of q k^T) has a row
// stride = 4 (mod 32) words; a tile whose k index walks its rows (the weight chunks, stride 272, and V, stride 48) has a row stride
// = 16 (mod 32) words.  Either way a wave's operand read touches 64 different banks.  No atomics anywhere: a forward repeated gives the same bits.
#include "segformer_api.h"

#include "nesr_kernels.h"

namespace nesr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LDA = 36;                 // As[32][36]
constexpr int LDB = 272;                // Bs[32][272]
constexpr int LDO = SEG_MAX_C + 4;      // output tile [32][260]
constexpr int AS_FLOATS = SEG_BM * LDA;
constexpr int BS_FLOATS = 32 * LDB;
static_assert(AS_FLOATS + BS_FLOATS >= SEG_BM * LDO, "the output tile lies over As | Bs");

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// 32 columns of K: acc[i] += A[16 rows of m-tile][32] x Bs[32][n-tile (w >> 1) + 2 i], i < CNT.  The tile count of a product is even
// and comes from the kernel's arguments, so CNT = ntiles / 2 is the same for every wave and the dispatch below is a scalar
// branch: a per-lane condition around an MFMA makes the compiler copy the accumulators through selects.
template <int CNT>
__device__ __forceinline__ void mma_chunk_n(const float* ap, const float* bp, int ldb_rows, int ldb_tiles, f32x4 (&acc)[8]) {
#pragma unroll
    for (int k4 = 0; k4 < 8; ++k4) {
        const float av = ap[k4 * 4];
#pragma unroll
        for (int i = 0; i < CNT; ++i) acc[i] = mfma4(av, bp[k4 * 4 * ldb_rows + i * ldb_tiles], acc[i]);
    }
}

// ap: this lane's A element of k = 0; bp: its B element of k = 0 in its first n-tile; B(k, tile i) = bp[k * ldb_rows + i * ldb_tiles]
__device__ __forceinline__ void mma_dispatch(const float* ap, const float* bp, int ldb_rows, int ldb_tiles, int cnt, f32x4 (&acc)[8]) {
    switch (cnt) {
        case 1: mma_chunk_n<1>(ap, bp, ldb_rows, ldb_tiles, acc); break;
        case 2: mma_chunk_n<2>(ap, bp, ldb_rows, ldb_tiles, acc); break;
        case 3: mma_chunk_n<3>(ap, bp, ldb_rows, ldb_tiles, acc); break;
        case 4: mma_chunk_n<4>(ap, bp, ldb_rows, ldb_tiles, acc); break;
        case 5: mma_chunk_n<5>(ap, bp, ldb_rows, ldb_tiles, acc); break;
        case 6: mma_chunk_n<6>(ap, bp, ldb_rows, ldb_tiles, acc); break;
        case 7: mma_chunk_n<7>(ap, bp, ldb_rows, ldb_tiles, acc); break;
        default: mma_chunk_n<8>(ap, bp, ldb_rows, ldb_tiles, acc); break;
    }
}

__device__ __forceinline__ void mma_chunk(const float* A, int lda, const float* Bs, int ntiles, f32x4 (&acc)[8]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* ap = A + ((wave & 1) * 16 + (lane & 15)) * lda + (lane >> 4);
    const float* bp = Bs + (lane >> 4) * LDB + (wave >> 1) * 16 + (lane & 15);
    mma_dispatch(ap, bp, LDB, 32, ntiles >> 1, acc);
}

// Bs[kk][n] = w[k0 + kk][n0 + n], kk < 32, n < nc (nc a multiple of 16, every row start 16-byte aligned)
__device__ __forceinline__ void load_b(const float* __restrict__ w, int ldw, int k0, int n0, int nc, float* Bs) {
    const int nq = nc >> 2;
    for (int i = threadIdx.x; i < 32 * nq; i += 256) {
        const int kk = i / nq, q = i - kk * nq;
        *reinterpret_cast<float4*>(Bs + kk * LDB + q * 4) = *reinterpret_cast<const float4*>(w + (size_t)(k0 + kk) * ldw + n0 + q * 4);
    }
}

__device__ __forceinline__ void store_acc(float* T, int ldt, int ntiles, const f32x4 (&acc)[8]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* tp = T + ((wave & 1) * 16 + (lane >> 4) * 4) * ldt + (wave >> 1) * 16 + (lane & 15);
    const int cnt = ntiles >> 1;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < cnt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) tp[r * ldt + i * 32] = acc[i][r];
        }
}

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

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// ---- the A operand: columns k .. k + 3 (k a multiple of 4) of row `grow`
__device__ __forceinline__ float4 load_conv(const SegFused& a, int grow, bool live, int k) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!live || k >= a.k1_real) return v;
    const int oy = grow / a.out_w, ox = grow - oy * a.out_w;
    const int y0 = oy * a.stride - a.pad, x0 = ox * a.stride - a.pad;
    if (a.nchw) {      // k = (c * ksz + ky) * ksz + kx, torch's own weight order
        float e[4];
        const int kk2 = a.ksz * a.ksz;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k + j;
            e[j] = 0.f;
            if (kk < a.k1_real) {
                const int c = kk / kk2, rem = kk - c * kk2, ky = rem / a.ksz, kx = rem - ky * a.ksz;
                const int iy = y0 + ky, ix = x0 + kx;
                if (iy >= 0 && iy < a.in_h && ix >= 0 && ix < a.in_w) e[j] = a.in[((size_t)c * a.in_h + iy) * a.in_w + ix];
            }
        }
        v = make_float4(e[0], e[1], e[2], e[3]);
    } else {           // k = (ky * ksz + kx) * in_c + c, in_c a multiple of 4: the four share a tap
        const int tap = k / a.in_c, c = k - tap * a.in_c, ky = tap / a.ksz, kx = tap - ky * a.ksz;
        const int iy = y0 + ky, ix = x0 + kx;
        if (iy >= 0 && iy < a.in_h && ix >= 0 && ix < a.in_w)
            v = *reinterpret_cast<const float4*>(a.in + ((size_t)iy * a.in_w + ix) * a.in_c + c);
    }
    return v;
}

__device__ __forceinline__ float4 load_dwgelu(const SegFused& a, int grow, bool live, int k) {
    if (!live) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int y = grow / a.gw, x = grow - y * a.gw;
    float4 s = *reinterpret_cast<const float4*>(a.dw_b + k);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = y + dy - 1;
        if (yy < 0 || yy >= a.gh) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int xx = x + dx - 1;
            if (xx < 0 || xx >= a.gw) continue;
            const float4 w = *reinterpret_cast<const float4*>(a.dw_w + (dy * 3 + dx) * a.k1 + k);
            const float4 p = *reinterpret_cast<const float4*>(a.in + ((size_t)yy * a.gw + xx) * a.k1 + k);
            s.x = fmaf(w.x, p.x, s.x);
            s.y = fmaf(w.y, p.y, s.y);
            s.z = fmaf(w.z, p.z, s.z);
            s.w = fmaf(w.w, p.w, s.w);
        }
    }
    return make_float4(gelu_erf(s.x), gelu_erf(s.y), gelu_erf(s.z), gelu_erf(s.w));
}

// torch's upsample_bilinear2d, align_corners=False: src = in / out * (dst + 0.5) - 0.5, clamped at 0
__device__ __forceinline__ void bilinear_tap(int dst, int in, int out, int& i0, int& i1, float& l1) {
    float src = ((float)in / (float)out) * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
}

__device__ __forceinline__ float4 load_decode(const SegFused& a, int grow, bool live, int k) {
    if (!live) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int seg = k / a.dec, c = k - seg * a.dec, st = a.nstage - 1 - seg;
    const float* p = st == 0 ? a.proj[0] : (st == 1 ? a.proj[1] : (st == 2 ? a.proj[2] : a.proj[3]));
    const int hi = st == 0 ? a.sh[0] : (st == 1 ? a.sh[1] : (st == 2 ? a.sh[2] : a.sh[3]));
    const int wi = st == 0 ? a.sw[0] : (st == 1 ? a.sw[1] : (st == 2 ? a.sw[2] : a.sw[3]));
    const int y = grow / a.sw[0], x = grow - y * a.sw[0];
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_tap(y, hi, a.sh[0], y0, y1, ly);
    bilinear_tap(x, wi, a.sw[0], x0, x1, lx);
    const float4 p00 = *reinterpret_cast<const float4*>(p + ((size_t)y0 * wi + x0) * a.dec + c);
    const float4 p01 = *reinterpret_cast<const float4*>(p + ((size_t)y0 * wi + x1) * a.dec + c);
    const float4 p10 = *reinterpret_cast<const float4*>(p + ((size_t)y1 * wi + x0) * a.dec + c);
    const float4 p11 = *reinterpret_cast<const float4*>(p + ((size_t)y1 * wi + x1) * a.dec + c);
    const float my = 1.f - ly, mx = 1.f - lx;
    return make_float4(my * (mx * p00.x + lx * p01.x) + ly * (mx * p10.x + lx * p11.x), my * (mx * p00.y + lx * p01.y) + ly * (mx * p10.y + lx * p11.y),
                       my * (mx * p00.z + lx * p01.z) + ly * (mx * p10.z + lx * p11.z), my * (mx * p00.w + lx * p01.w) + ly * (mx * p10.w + lx * p11.w));
}

template <int MODE>
__global__ __launch_bounds__(256) void seg_fused_kernel(const SegFused a) {
    extern __shared__ float lds[];
    float* As = lds;
    float* Bs = lds + AS_FLOATS;
    float* R = Bs + BS_FLOATS;      // [32][n1 + 4]
    float* O = lds;                 // [32][LDO], over As | Bs
    const int t = threadIdx.x;
    const int row0 = blockIdx.x * SEG_BM;
    const int ldr = a.n1 + 4;
    const int r8 = t >> 3, s8 = t & 7;      // row-wise work: 8 threads a row, thread s8 the float4s at columns 4 s8 + 32 i
    const int grow = row0 + r8;
    const bool live = grow < a.m;

    if (MODE == SEG_A_ROWS) {
        for (int c = s8 * 4; c < a.n1; c += 32)
            *reinterpret_cast<float4*>(R + r8 * ldr + c) =
                live ? *reinterpret_cast<const float4*>(a.in + (size_t)grow * a.n1 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        f32x4 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < a.k1; k0 += 32) {
            const int k = k0 + s8 * 4;
            const float4 av = MODE == SEG_A_CONV ? load_conv(a, grow, live, k) : (MODE == SEG_A_DWGELU ? load_dwgelu(a, grow, live, k) : load_decode(a, grow, live, k));
            *reinterpret_cast<float4*>(As + r8 * LDA + s8 * 4) = av;
            load_b(a.w1, a.n1, k0, 0, a.n1, Bs);
            __syncthreads();
            mma_chunk(As, LDA, Bs, a.n1 >> 4, acc);
            __syncthreads();
        }
        store_acc(R, ldr, a.n1 >> 4, acc);
    }
    __syncthreads();

    // ---- the row-wise stage on R
    {
        float* rp = R + r8 * ldr;
        if (a.bias1)
            for (int c = s8 * 4; c < a.n1; c += 32) {
                float4 v = *reinterpret_cast<float4*>(rp + c);
                const float4 b = *reinterpret_cast<const float4*>(a.bias1 + c);
                v.x += b.x, v.y += b.y, v.z += b.z, v.w += b.w;
                *reinterpret_cast<float4*>(rp + c) = v;
            }
        float mean = 0.f, rstd = 1.f;
        if (a.ln_g) {
            float s = 0.f;
            for (int c = s8 * 4; c < a.n1; c += 32) {
                const float4 v = *reinterpret_cast<float4*>(rp + c);
                s += (v.x + v.y) + (v.z + v.w);
            }
            mean = sum8(s) / (float)a.n1;
            float q = 0.f;
            for (int c = s8 * 4; c < a.n1; c += 32) {
                const float4 v = *reinterpret_cast<float4*>(rp + c);
                const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
                q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
            }
            rstd = 1.0f / sqrtf(sum8(q) / (float)a.n1 + 1e-5f);
        }
        for (int c = s8 * 4; c < a.n1; c += 32) {
            float4 v = *reinterpret_cast<float4*>(rp + c);
            if (a.ln_g) {
                const float4 g = *reinterpret_cast<const float4*>(a.ln_g + c), b = *reinterpret_cast<const float4*>(a.ln_b + c);
                v.x = (v.x - mean) * rstd * g.x + b.x;
                v.y = (v.y - mean) * rstd * g.y + b.y;
                v.z = (v.z - mean) * rstd * g.z + b.z;
                v.w = (v.w - mean) * rstd * g.w + b.w;
            }
            if (a.bn_scale) {
                const float4 g = *reinterpret_cast<const float4*>(a.bn_scale + c), b = *reinterpret_cast<const float4*>(a.bn_shift + c);
                v.x = fmaxf(fmaf(v.x, g.x, b.x), 0.f);
                v.y = fmaxf(fmaf(v.y, g.y, b.y), 0.f);
                v.z = fmaxf(fmaf(v.z, g.z, b.z), 0.f);
                v.w = fmaxf(fmaf(v.w, g.w, b.w), 0.f);
            }
            if (a.res && live) {
                const float4 x = *reinterpret_cast<const float4*>(a.res + (size_t)grow * a.n1 + c);
                v.x += x.x, v.y += x.y, v.z += x.z, v.w += x.w;
            }
            *reinterpret_cast<float4*>(rp + c) = v;
            if (a.out1 && live) *reinterpret_cast<float4*>(a.out1 + (size_t)grow * a.n1 + c) = v;
        }
    }
    if (!a.w2) return;

    // ---- the second product, 256 columns at a time
    const int n2p = (a.n2 + 31) & ~31;      // an even number of n-tiles
    for (int n0 = 0; n0 < n2p; n0 += 256) {
        const int nc = n2p - n0 < 256 ? n2p - n0 : 256;
        f32x4 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < a.n1; k0 += 32) {
            __syncthreads();      // R is written; Bs and the tile over it are read
            load_b(a.w2, a.ldw2, k0, n0, nc, Bs);
            __syncthreads();
            mma_chunk(R + k0, ldr, Bs, nc >> 4, acc);
        }
        __syncthreads();
        store_acc(O, LDO, nc >> 4, acc);
        __syncthreads();
        if (a.out_mode == SEG_OUT_ROWS) {
            if (live)
                for (int c = s8 * 4; c < nc && n0 + c < a.n2; c += 32) {
                    float4 v = *reinterpret_cast<float4*>(O + r8 * LDO + c);
                    const float4 b = *reinterpret_cast<const float4*>(a.bias2 + n0 + c);
                    v.x += b.x, v.y += b.y, v.z += b.z, v.w += b.w;
                    *reinterpret_cast<float4*>(a.out2 + (size_t)grow * a.ld_out2 + n0 + c) = v;
                }
        } else if (a.out_mode == SEG_OUT_NCHW) {
            const int r = t & 31;
            if (row0 + r < a.m)
                for (int c = t >> 5; c < nc && n0 + c < a.n2; c += 8)
                    a.out2[(size_t)(n0 + c) * a.ld_out2 + row0 + r] = O[r * LDO + c] + a.bias2[n0 + c];
        } else {                  // argmax over the n2 (<= 256) columns, the lowest index among equals
            float best = -INFINITY;
            int bi = a.n2;
            for (int c = s8; c < a.n2; c += 8) {
                const float v = O[r8 * LDO + c] + a.bias2[c];
                if (v > best || bi == a.n2) best = v, bi = c;
            }
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) {
                const float ov = __shfl_xor(best, m);
                const int oi = __shfl_xor(bi, m);
                if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;
            }
            if (live && s8 == 0) a.out2_u8[grow] = (uint8_t)bi;
        }
    }
}

// ---- attention + o_proj + residual
constexpr int LDK = 36;                       // Ks[SEG_KCH][36], Qs[32][36]
constexpr int LDV = 48;                       // Vs[SEG_KCH][48]
constexpr int LDS_S = SEG_KCH + 4;            // S[32][260]
constexpr int KS_FLOATS = SEG_KCH * LDK, VS_FLOATS = SEG_KCH * LDV, S_FLOATS = SEG_BM * LDS_S, QS_FLOATS = SEG_BM * LDK;
static_assert(KS_FLOATS + VS_FLOATS >= BS_FLOATS, "o_proj's weight chunk lies over Ks | Vs");
static_assert(S_FLOATS >= SEG_BM * LDO, "o_proj's output tile lies over S");

__global__ __launch_bounds__(256) void seg_attn_kernel(const SegAttn a) {
    extern __shared__ float lds[];
    float* Ks = lds;
    float* Vs = Ks + KS_FLOATS;
    float* S = Vs + VS_FLOATS;
    float* Qs = S + S_FLOATS;
    float* stat = Qs + QS_FLOATS;             // running max [32], running sum [32], rescale of this chunk [32]
    float* ctx = stat + 3 * SEG_BM;           // [32][c + 4]
    const int ldc = a.c + 4;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row0 = blockIdx.x * SEG_BM;
    const int r8 = t >> 3, s8 = t & 7;
    const int grow = row0 + r8;
    const bool live = grow < a.m;
    const int mt = wave & 1, nt0 = wave >> 1;
    const float scale = 0.17677669529663688110f;      // 32^-1/2

    for (int h = 0; h < a.heads; ++h) {
        *reinterpret_cast<float4*>(Qs + r8 * LDK + s8 * 4) =
            live ? *reinterpret_cast<const float4*>(a.q + (size_t)grow * a.q_ld + h * 32 + s8 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < SEG_BM) stat[t] = -INFINITY, stat[SEG_BM + t] = 0.f;
        f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < a.keys; c0 += SEG_KCH) {
            const int lc = a.keys - c0 < SEG_KCH ? a.keys - c0 : SEG_KCH;
            const int lcp = (lc + 31) & ~31;      // an even number of 16-key tiles
            for (int i = t; i < lcp * 8; i += 256) {
                const int j = i >> 3, d = (i & 7) * 4;
                float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
                if (j < lc) {
                    kv = *reinterpret_cast<const float4*>(a.k + (size_t)(c0 + j) * a.kv_ld + h * 32 + d);
                    vv = *reinterpret_cast<const float4*>(a.v + (size_t)(c0 + j) * a.kv_ld + h * 32 + d);
                }
                *reinterpret_cast<float4*>(Ks + j * LDK + d) = kv;
                *reinterpret_cast<float4*>(Vs + j * LDV + d) = vv;
            }
            __syncthreads();
            {   // S = q k^T / sqrt(32); a key past the end scores -inf
                f32x4 acc[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                const int cnt = lcp >> 5;
                const float* ap = Qs + (mt * 16 + (lane & 15)) * LDK + (lane >> 4);
                const float* bp = Ks + (nt0 * 16 + (lane & 15)) * LDK + (lane >> 4);
                mma_dispatch(ap, bp, 1, 32 * LDK, cnt, acc);
                float* sp = S + (mt * 16 + (lane >> 4) * 4) * LDS_S + nt0 * 16 + (lane & 15);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (i < cnt) {
                        const bool key_ok = (nt0 + 2 * i) * 16 + (lane & 15) < lc;
#pragma unroll
                        for (int r = 0; r < 4; ++r) sp[r * LDS_S + i * 32] = key_ok ? acc[i][r] * scale : -INFINITY;
                    }
            }
            __syncthreads();
            {   // online softmax of the 32 rows: S becomes exp(S - max so far)
                float* sp = S + r8 * LDS_S;
                float cm = -INFINITY;
                for (int c = s8; c < lcp; c += 8) cm = fmaxf(cm, sp[c]);
                const float m_old = stat[r8];
                const float m_new = fmaxf(m_old, max8(cm));
                float sum = 0.f;
                for (int c = s8; c < lcp; c += 8) {
                    const float p = expf(sp[c] - m_new);
                    sp[c] = p;
                    sum += p;
                }
                sum = sum8(sum);
                const float alpha = expf(m_old - m_new);
                if (s8 == 0) {
                    stat[r8] = m_new;
                    stat[SEG_BM + r8] = stat[SEG_BM + r8] * alpha + sum;
                    stat[2 * SEG_BM + r8] = alpha;
                }
            }
            __syncthreads();
            {   // o = o * alpha + P V: this wave's 16 rows x 16 dims, two chains over the keys
                const float* al = stat + 2 * SEG_BM + mt * 16 + (lane >> 4) * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) o0[r] *= al[r], o1[r] *= al[r];
                const float* ap = S + (mt * 16 + (lane & 15)) * LDS_S + (lane >> 4);
                const float* bp = Vs + (lane >> 4) * LDV + nt0 * 16 + (lane & 15);
                for (int k4 = 0; k4 < (lcp >> 2); k4 += 2) {
                    o0 = mfma4(ap[k4 * 4], bp[k4 * 4 * LDV], o0);
                    o1 = mfma4(ap[k4 * 4 + 4], bp[(k4 * 4 + 4) * LDV], o1);
                }
            }
            __syncthreads();
        }
        {
            const float* lp = stat + SEG_BM + mt * 16 + (lane >> 4) * 4;
            float* cp = ctx + (mt * 16 + (lane >> 4) * 4) * ldc + h * 32 + nt0 * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) cp[r * ldc] = (o0[r] + o1[r]) / lp[r];
        }
        __syncthreads();
    }

    // ---- x += ctx x wo + bo
    float* Bs = lds;
    float* O = S;
    f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.c; k0 += 32) {
        __syncthreads();
        load_b(a.wo, a.c, k0, 0, a.c, Bs);
        __syncthreads();
        mma_chunk(ctx + k0, ldc, Bs, a.c >> 4, acc);
    }
    store_acc(O, LDO, a.c >> 4, acc);
    __syncthreads();
    if (live)
        for (int c = s8 * 4; c < a.c; c += 32) {
            float4 v = *reinterpret_cast<float4*>(O + r8 * LDO + c);
            const float4 b = *reinterpret_cast<const float4*>(a.bo + c);
            float4 x = *reinterpret_cast<float4*>(a.x + (size_t)grow * a.c + c);
            x.x += v.x + b.x, x.y += v.y + b.y, x.z += v.z + b.z, x.w += v.w + b.w;
            *reinterpret_cast<float4*>(a.x + (size_t)grow * a.c + c) = x;
        }
}

template <int MODE>
hipError_t launch_fused_mode(const SegFused& a, hipStream_t s) {
    static unsigned long long done = 0;
    constexpr size_t max_bytes = (size_t)(AS_FLOATS + BS_FLOATS + SEG_BM * (SEG_MAX_C + 4)) * sizeof(float);
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&seg_fused_kernel<MODE>), max_bytes, done);
    if (e != hipSuccess) return e;
    seg_fused_kernel<MODE><<<dim3((a.m + SEG_BM - 1) / SEG_BM), dim3(256), seg_fused_lds_bytes(a), s>>>(a);
    return hipGetLastError();
}

}  // namespace

size_t seg_fused_lds_bytes(const SegFused& a) { return (size_t)(AS_FLOATS + BS_FLOATS + SEG_BM * (a.n1 + 4)) * sizeof(float); }

size_t seg_attn_lds_bytes(const SegAttn& a) {
    return (size_t)(KS_FLOATS + VS_FLOATS + S_FLOATS + QS_FLOATS + 3 * SEG_BM + SEG_BM * (a.c + 4)) * sizeof(float);
}

hipError_t launch_seg_fused(const SegFused& a, hipStream_t s) {
    // the shapes the kernel's tiles and float4 accesses rest on
    if (a.m < 1 || a.n1 < 32 || a.n1 > SEG_MAX_C || a.n1 % 32 || (a.a_mode != SEG_A_ROWS && (a.k1 < 32 || a.k1 % 32))) return hipErrorInvalidValue;
    if (a.w2 && (a.n2 < 1 || a.ldw2 % 32 || a.ldw2 < ((a.n2 + 31) & ~31))) return hipErrorInvalidValue;
    if (a.w2 && a.out_mode == SEG_OUT_ARGMAX && a.n2 > SEG_MAX_C) return hipErrorInvalidValue;
    if (a.w2 && a.out_mode == SEG_OUT_ROWS && a.n2 % 4) return hipErrorInvalidValue;
    switch (a.a_mode) {
        case SEG_A_ROWS: return launch_fused_mode<SEG_A_ROWS>(a, s);
        case SEG_A_CONV:
            if (!a.nchw && (a.in_c % 4 || a.k1_real != a.k1)) return hipErrorInvalidValue;
            return launch_fused_mode<SEG_A_CONV>(a, s);
        case SEG_A_DWGELU: return launch_fused_mode<SEG_A_DWGELU>(a, s);
        case SEG_A_DECODE:
            if (a.nstage < 1 || a.nstage > SEG_MAX_STAGES || a.dec % 32 || a.k1 != a.nstage * a.dec) return hipErrorInvalidValue;
            return launch_fused_mode<SEG_A_DECODE>(a, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_seg_attn(const SegAttn& a, hipStream_t s) {
    if (a.m < 1 || a.keys < 1 || a.heads < 1 || a.c != a.heads * 32 || a.c > SEG_MAX_C || a.q_ld % 4 || a.kv_ld % 4) return hipErrorInvalidValue;
    static unsigned long long done = 0;
    constexpr size_t max_bytes = (size_t)(KS_FLOATS + VS_FLOATS + S_FLOATS + QS_FLOATS + 3 * SEG_BM + SEG_BM * (SEG_MAX_C + 4)) * sizeof(float);
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&seg_attn_kernel), max_bytes, done);
    if (e != hipSuccess) return e;
    seg_attn_kernel<<<dim3((a.m + SEG_BM - 1) / SEG_BM), dim3(256), seg_attn_lds_bytes(a), s>>>(a);
    return hipGetLastError();
}

}  // namespace nesr
