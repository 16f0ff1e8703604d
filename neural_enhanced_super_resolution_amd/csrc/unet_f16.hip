// The fp16 compute form of the UNet's products for gfx950 (nesr_unet_set_dtype): the 3x3 conv and the K-tiled row GEMM of unet.hip
// with both operands rounded to f16 and f32 products and sums on the f16 matrix cores.  tests/unet_f16_emu.py is the specification.
// Storage stays f32 rows [n H W][cs]; the prologues (GroupNorm + SiLU, GroupNorm, LayerNorm), the bias, the residual and GEGLU's
// (h + b_h) gelu(g + b_g) are the f32 form's code, evaluated in f32.  Nothing else of a forward changes: statistics, attention,
// embedding and the inputs are unet.hip's kernels in either form.
//
// Operand maps (v_mfma_f32_16x16x32_f16): lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][column l & 15],
// j < 8, and D[row 4 (l >> 4) + r][column l & 15], r < 4.  The K tail of 16 runs on v_mfma_f32_16x16x16_f16: k = 4 (l >> 4) + j, j < 4.
//
//   A   the activation, staged in LDS as f16 with k contiguous in rows of KC + 8 halves: a fragment is one ds_read_b128, and the
//       16 rows of a quarter wave start 4 (mod 32) banks apart.  The prologue runs in f32 on the value loaded from memory; the
//       rounding and the range check (elem16.h) happen at the store into LDS.  A padding tap and a row past m are 0.
//   B   the f16 copy of the weights, k contiguous per output column (unet_api.h): a fragment of 8 k is one 16-byte global load.
//       The fragments of a K chunk (rows) or of the next tap (conv) are requested before the MFMAs that precede their use.
//
// A workgroup is 256 threads (4 waves) and owns 32 rows (rows) or 4 x 16 output pixels (conv) by 128, 64 or 32 output columns:
//
//   128   the waves side by side, two column tiles each            (template WR = 1, NT = 2)
//    64   the waves side by side, one column tile each             (WR = 1, NT = 1)
//    32   two waves side by side, each half of the rows            (WR = 2, NT = 1)
//
// The f32 kernels take 256 (rows) and 128 (conv) columns at any shape, which leaves a 1024-wide product of 32 rows on 4 workgroups;
// here the launcher picks the widest block whose grid still has a workgroup a CU.  The K chain of an output element stays in one
// wave, in ascending k per source (steps of 32, then the tail of 16), so which block computes an element does not change its
// bits, nor does m or the sample count.  No atomics; no workgroup waits on another.  GEGLU: a wave computes the value and the
// gate tile of its columns, so the 8 x dim intermediate never exists.
#include "unet_api.h"

#include "elem16.h"
#include "f32_rows_device.h"

namespace nesr {
namespace {

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4f mfma32(f16x8 a, f16x8 b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v4f mfma16(f16x4 a, f16x4 b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// f32 x 4 -> f16 x 4 (nearest even); `am` keeps the largest |x| pattern this lane rounded
__device__ __forceinline__ f16x4 round4(float4 v, unsigned& am) {
    am = E16<3>::amax(E16<3>::amax(E16<3>::amax(E16<3>::amax(am, v.x), v.y), v.z), v.w);
    return f16x4{(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
}

// ---------------------------------------------------------------------------------------------------------------- K-tiled rows
constexpr int R16_KC = 128, R16_LD = R16_KC + 8, R16_STEPS = R16_KC / 32;

template <int WR, int NT, bool GEGLU>
__global__ __launch_bounds__(256) void unet_rows_f16_kernel(const UnetRows16 a) {
    constexpr int CW = 4 / WR, RT = 2 / WR, BN = CW * NT * 16, NB = GEGLU ? 2 * NT : NT;      // NB: the B tiles of a wave
    __shared__ __attribute__((aligned(16))) f16 lds[UNET_BM * R16_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, wc = wave % CW, wr = wave / CW;
    const int row0 = blockIdx.x * UNET_BM, out_tiles = a.np >> 4;
    const int K = a.in[0].cs + (a.in[1].p ? a.in[1].cs : 0);
    bool ok[NT];
    int col[NT];
    const f16* bp[NB];      // this lane's weight row of each B tile: plain, NT output tiles; GEGLU, their value and gate halves
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int ot = blockIdx.y * (BN / 16) + wc * NT + u;
        ok[u] = ot < out_tiles;
        col[u] = ok[u] ? ot * 16 : 0;      // a tile that is not there reads tile 0 and is dropped
        bp[u] = a.w16 + (size_t)(col[u] + (lane & 15)) * K;
        if (GEGLU) bp[NT + u] = bp[u] + (size_t)a.np * K;
    }
    v4f acc[NB][RT];
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
        for (int i = 0; i < RT; ++i) acc[u][i] = v4f{0.f, 0.f, 0.f, 0.f};

    unsigned am = 0;
    bool first = true;
    int krow = 0;
    for (int seg = 0; seg < 2; ++seg) {
        const UnetSrc src = a.in[seg];
        if (!src.p) break;
        for (int k0 = 0; k0 < src.cs; k0 += R16_KC) {
            const int kc = src.cs - k0 < R16_KC ? src.cs - k0 : R16_KC, nq = kc >> 2;      // a multiple of 16
            f16x8 b[R16_STEPS][NB];      // the chunk's weight fragments, asked for before the activations are staged
            f16x4 bt[NB];
            if (ok[0]) {                 // the same for a wave; its first tile is its lowest
#pragma unroll
                for (int st = 0; st < R16_STEPS; ++st)
                    if (32 * st + 32 <= kc) {
#pragma unroll
                        for (int u = 0; u < NB; ++u) b[st][u] = *reinterpret_cast<const f16x8*>(bp[u] + krow + k0 + 32 * st + 8 * g);
                    }
                if (kc & 16) {
#pragma unroll
                    for (int u = 0; u < NB; ++u) bt[u] = *reinterpret_cast<const f16x4*>(bp[u] + krow + k0 + (kc & ~31) + 4 * g);
                }
            }
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
                        const float4 gm = *reinterpret_cast<const float4*>(a.ln_g + c), bb = *reinterpret_cast<const float4*>(a.ln_b + c);
                        v.x = ((v.x - st.x) - st.y) * st.z * gm.x + bb.x, v.y = ((v.y - st.x) - st.y) * st.z * gm.y + bb.y;
                        v.z = ((v.z - st.x) - st.y) * st.z * gm.z + bb.z, v.w = ((v.w - st.x) - st.y) * st.z * gm.w + bb.w;
                    }
                }
                *reinterpret_cast<f16x4*>(lds + r * R16_LD + q * 4) = round4(v, am);
            }
            __syncthreads();
            if (!ok[0]) continue;
            const f16* ap = lds + (wr * RT * 16 + (lane & 15)) * R16_LD;
#pragma unroll
            for (int st = 0; st < R16_STEPS; ++st)
                if (32 * st + 32 <= kc) {
#pragma unroll
                    for (int i = 0; i < RT; ++i) {
                        const f16x8 av = *reinterpret_cast<const f16x8*>(ap + i * 16 * R16_LD + 32 * st + 8 * g);
#pragma unroll
                        for (int u = 0; u < NB; ++u) acc[u][i] = mfma32(av, b[st][u], acc[u][i]);
                    }
                }
            if (kc & 16) {
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    const f16x4 av = *reinterpret_cast<const f16x4*>(ap + i * 16 * R16_LD + (kc & ~31) + 4 * g);
#pragma unroll
                    for (int u = 0; u < NB; ++u) acc[u][i] = mfma16(av, bt[u], acc[u][i]);
                }
            }
        }
        krow += src.cs;
    }
    raise_range(a.status, am);
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        if (!ok[u]) continue;
        const int c = col[u] + (lane & 15);
        const float bias = a.b[c], gate_bias = GEGLU ? a.b[a.np + c] : 0.f;
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + (wr * RT + i) * 16 + g * 4 + r;
                if (row >= a.m) continue;
                float v = acc[u][i][r] + bias;
                if (GEGLU) v *= gelu_erf(acc[GEGLU ? NT + u : u][i][r] + gate_bias);
                if (a.res) v += a.res[(size_t)row * a.np + c];
                a.out[(size_t)row * a.np + c] = v;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------- conv 3x3
constexpr int CV_TW = VAE_CONV_TW, CV_TH = VAE_CONV_TH;
static_assert(CV_TW == 16 && CV_TH == 4, "a workgroup's output tile: 4 rows of 16 pixels, one MFMA row tile a pixel row");

// The input patch of 4 x 16 output pixels at stride S as f16, a K chunk of 64 / S channels at a time, k contiguous.
template <int S>
struct Conv16Geom {
    static constexpr int KC = 64 / S, STEPS = KC / 32;
    static constexpr int PW = CV_TW * S + 3 - S, PH = CV_TH * S + 3 - S;
    static constexpr int LD = KC + 8;
    static constexpr int HALVES = PH * PW * LD;
};

// conv_load_patch of f32_rows_device.h with the store rounded to f16: channels c0 .. c0 + kc of the patch -> lds [PH PW][LD]
template <int S>
__device__ __forceinline__ void conv16_load_patch(f16* lds, const float* base, const VaeNorm* norm, int cs, int c0, int kc, int y0, int x0, int DH, int DW, int sw,
                                                  bool up, unsigned& am) {
    typedef Conv16Geom<S> G;
    const unsigned nq = (unsigned)kc >> 2;
    for (unsigned idx = threadIdx.x; idx < G::PH * G::PW * nq; idx += 256) {
        const unsigned q = idx % nq, pos = idx / nq, px = pos % G::PW, py = pos / G::PW;
        const int gy = y0 * S - 1 + (int)py, gx = x0 * S - 1 + (int)px;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < DH && gx >= 0 && gx < DW) {
            const int sy = up ? gy >> 1 : gy, sx = up ? gx >> 1 : gx;
            const int c = c0 + q * 4;      // c + 3 < cs
            v = *reinterpret_cast<const float4*>(base + ((size_t)sy * sw + sx) * cs + c);
            if (norm) {
                v.x = silu(normed(v.x, norm[c])), v.y = silu(normed(v.y, norm[c + 1]));
                v.z = silu(normed(v.z, norm[c + 2])), v.w = silu(normed(v.w, norm[c + 3]));
            }
        }
        *reinterpret_cast<f16x4*>(lds + pos * G::LD + q * 4) = round4(v, am);
    }
}

// the weight fragments of one tap of a chunk: STEPS steps of 32 and the tail of 16, for NT column tiles
template <int STEPS, int NT>
struct TapB {
    f16x8 b[STEPS][NT];
    f16x4 t[NT];
};

template <int STEPS, int NT>
__device__ __forceinline__ void load_tap(TapB<STEPS, NT>& o, const f16* const (&bp)[NT], int at, int kc, int g) {
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
        if (32 * st + 32 <= kc) {
#pragma unroll
            for (int u = 0; u < NT; ++u) o.b[st][u] = *reinterpret_cast<const f16x8*>(bp[u] + at + 32 * st + 8 * g);
        }
    if (kc & 16) {
#pragma unroll
        for (int u = 0; u < NT; ++u) o.t[u] = *reinterpret_cast<const f16x4*>(bp[u] + at + (kc & ~31) + 4 * g);
    }
}

template <int S, int WR, int NT>
__global__ __launch_bounds__(256) void unet_conv_f16_kernel(const UnetConv16 a) {
    typedef Conv16Geom<S> G;
    constexpr int CW = 4 / WR, RT = CV_TH / WR, NB = CW * NT * 16;      // RT: the pixel rows of a wave
    __shared__ __attribute__((aligned(16))) f16 lds[G::HALVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, wc = wave % CW, wr = wave / CW;
    const int x0 = blockIdx.x * CV_TW, y0 = blockIdx.y * CV_TH;
    const int nblk = (a.coutp + NB - 1) / NB, sample = blockIdx.z / nblk, blk = blockIdx.z - sample * nblk;
    const int ntiles = a.coutp >> 4, ni0 = blk * (NB / 16) + wc * NT;
    const bool work = ni0 < ntiles;                                  // the same for a wave
    const int DH = a.H * S, DW = a.W * S;                            // the conv's input domain
    const int sw = a.up ? a.W >> 1 : DW;                             // the source grid
    const size_t sm = a.up ? (size_t)(a.H >> 1) * (a.W >> 1) : (size_t)DH * DW;
    const int cs0 = a.in[0].cs, ktap = cs0 + (a.in[1].p ? a.in[1].cs : 0);
    bool ok[NT];
    const f16* bp[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        ok[u] = ni0 + u < ntiles;
        bp[u] = a.w16 + (size_t)((ok[u] ? ni0 + u : 0) * 16 + (lane & 15)) * 9 * ktap;      // a tile that is not there reads tile 0 and is dropped
    }
    v4f acc[NT][RT];
#pragma unroll
    for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int i = 0; i < RT; ++i) acc[u][i] = v4f{0.f, 0.f, 0.f, 0.f};

    unsigned am = 0;
    bool first = true;
    for (int seg = 0; seg < 2; ++seg) {
        const UnetSrc src = a.in[seg];
        if (!src.p) break;
        const int wrow = seg == 0 ? 0 : cs0;
        const float* base = src.p + (size_t)sample * sm * src.cs;
        const VaeNorm* norm = src.norm ? src.norm + (size_t)sample * src.cs : nullptr;
        for (int c0 = 0; c0 < src.cs; c0 += G::KC) {
            const int kc = src.cs - c0 < G::KC ? src.cs - c0 : G::KC;
            TapB<G::STEPS, NT> wb[2];      // the tap at work and the next one
            if (work) load_tap(wb[0], bp, wrow + c0, kc, g);
            if (!first) __syncthreads();      // the chunk before is read
            first = false;
            conv16_load_patch<S>(lds, base, norm, src.cs, c0, kc, y0, x0, DH, DW, sw, a.up != 0, am);
            __syncthreads();
            if (!work) continue;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap - ky * 3;
                if (tap + 1 < 9) load_tap(wb[(tap + 1) & 1], bp, (tap + 1) * ktap + wrow + c0, kc, g);
                const TapB<G::STEPS, NT>& w = wb[tap & 1];
                const f16* ap = lds + ((ky + wr * RT * S) * G::PW + (lane & 15) * S + kx) * G::LD;
#pragma unroll
                for (int st = 0; st < G::STEPS; ++st)
                    if (32 * st + 32 <= kc) {
#pragma unroll
                        for (int i = 0; i < RT; ++i) {
                            const f16x8 av = *reinterpret_cast<const f16x8*>(ap + i * S * G::PW * G::LD + 32 * st + 8 * g);
#pragma unroll
                            for (int u = 0; u < NT; ++u) acc[u][i] = mfma32(av, w.b[st][u], acc[u][i]);
                        }
                    }
                if (kc & 16) {
#pragma unroll
                    for (int i = 0; i < RT; ++i) {
                        const f16x4 av = *reinterpret_cast<const f16x4*>(ap + i * S * G::PW * G::LD + (kc & ~31) + 4 * g);
#pragma unroll
                        for (int u = 0; u < NT; ++u) acc[u][i] = mfma16(av, w.t[u], acc[u][i]);
                    }
                }
            }
        }
    }
    raise_range(a.status, am);
    if (!work) return;
    const size_t om = (size_t)a.H * a.W;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        if (!ok[u]) continue;
        const int c = (ni0 + u) * 16 + (lane & 15);      // < coutp
        const float bias = a.bias[c];
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const int y = y0 + wr * RT + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = x0 + g * 4 + r;
                if (y >= a.H || x >= a.W) continue;
                const size_t p = (size_t)y * a.W + x, row = (size_t)sample * om + p;
                float v = acc[u][i][r] + bias;
                if (a.res) v += a.res[row * a.coutp + c];
                if (!a.out_nchw) a.out[row * a.coutp + c] = v;      // the zero columns too
                else if (c < a.cout) a.out[((size_t)sample * a.cout + c) * om + p] = v;
            }
        }
    }
}

bool src16_ok(const UnetSrc& s, int max_cs) { return s.p && s.c >= 1 && s.cs >= 16 && s.cs % 16 == 0 && s.cs >= s.c && s.cs <= max_cs; }

// the widest block of 128, 64, 32 columns whose grid of `tiles` row or pixel tiles still has a workgroup a CU; else 32
int pick_block(long long tiles, int np) {
    for (int bn = 128; bn > 32; bn >>= 1)
        if (tiles * ((np + bn - 1) / bn) >= UNET_F16_FILL) return bn;
    return 32;
}

template <bool GEGLU>
void rows_launch(int bn, dim3 grid, const UnetRows16& a, hipStream_t s) {
    if (bn == 128) unet_rows_f16_kernel<1, 2, GEGLU><<<grid, dim3(256), 0, s>>>(a);
    else if (bn == 64) unet_rows_f16_kernel<1, 1, GEGLU><<<grid, dim3(256), 0, s>>>(a);
    else unet_rows_f16_kernel<2, 1, GEGLU><<<grid, dim3(256), 0, s>>>(a);
}

template <int S>
void conv_launch(int nb, dim3 grid, const UnetConv16& a, hipStream_t s) {
    if (nb == 128) unet_conv_f16_kernel<S, 1, 2><<<grid, dim3(256), 0, s>>>(a);
    else if (nb == 64) unet_conv_f16_kernel<S, 1, 1><<<grid, dim3(256), 0, s>>>(a);
    else unet_conv_f16_kernel<S, 2, 1><<<grid, dim3(256), 0, s>>>(a);
}

}  // namespace

size_t unet_rows_f16_lds_bytes() { return sizeof(f16) * UNET_BM * R16_LD; }
size_t unet_conv_f16_lds_bytes(int stride) { return sizeof(f16) * (stride == 2 ? Conv16Geom<2>::HALVES : Conv16Geom<1>::HALVES); }

int unet_rows_f16_block(int m, int np) { return pick_block(((long long)m + UNET_BM - 1) / UNET_BM, np); }
int unet_conv_f16_block(int n, int H, int W, int coutp) {
    return pick_block((long long)n * ((W + CV_TW - 1) / CV_TW) * ((H + CV_TH - 1) / CV_TH), coutp);
}

// the refusals of launch_unet_rows, on the f16 weight
hipError_t launch_unet_rows_f16(const UnetRows16& a, hipStream_t s) {
    if (!a.w16 || !a.b || !a.out || a.m < 1 || a.m > 0x7fffffff - UNET_BM || a.rows_per_sample < 1) return hipErrorInvalidValue;
    if (!src16_ok(a.in[0], 4 * UNET_MAX_WIDTH) || (a.in[1].p && !src16_ok(a.in[1], UNET_MAX_WIDTH))) return hipErrorInvalidValue;
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
    if (reinterpret_cast<uintptr_t>(a.w16) & 15) return hipErrorInvalidValue;      // a fragment is one 16-byte load
    const int bn = unet_rows_f16_block(a.m, a.np);
    const dim3 grid((a.m + UNET_BM - 1) / UNET_BM, (a.np + bn - 1) / bn);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (a.geglu) rows_launch<true>(bn, grid, a, s);
    else rows_launch<false>(bn, grid, a, s);
    return hipGetLastError();
}

// the refusals of launch_unet_conv, on the f16 weight
hipError_t launch_unet_conv_f16(const UnetConv16& a, hipStream_t s) {
    if (!a.w16 || !a.bias || !a.out || a.n < 1 || a.n > 2 || a.H < 1 || a.W < 1 || (long long)a.n * a.H * a.W > UNET_MAX_PIXELS) return hipErrorInvalidValue;
    if (!src16_ok(a.in[0], UNET_MAX_WIDTH) || (a.in[1].p && !src16_ok(a.in[1], UNET_MAX_WIDTH))) return hipErrorInvalidValue;
    if (a.cout < 1 || a.coutp != (a.cout + 15) / 16 * 16 || a.coutp > UNET_MAX_WIDTH) return hipErrorInvalidValue;
    if ((a.stride != 1 && a.stride != 2) || (a.stride == 2 && a.up) || (a.up && (a.H % 2 || a.W % 2))) return hipErrorInvalidValue;
    if (a.out_nchw && a.res) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(a.w16) & 15) return hipErrorInvalidValue;
    const int nb = unet_conv_f16_block(a.n, a.H, a.W, a.coutp);
    const unsigned nblk = (a.coutp + nb - 1) / nb;
    const dim3 grid((a.W + CV_TW - 1) / CV_TW, (a.H + CV_TH - 1) / CV_TH, a.n * nblk);
    if (grid.y > 65535u) return hipErrorInvalidValue;      // z: at most 2 samples x 32 blocks
    if (a.stride == 2) conv_launch<2>(nb, grid, a, s);
    else conv_launch<1>(nb, grid, a, s);
    return hipGetLastError();
}

}  // namespace nesr
