// Internal interface of the SegFormer path: the nesr_segformer_* entries of the C ABI (segformer_api.cpp) drive the kernels of
// segformer.hip (the network) and segformer_pre.hip (PIL's 8-bit resize and the normalisation).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nesr {

constexpr int SEG_BM = 32;        // token rows of one workgroup, every kernel of segformer.hip
constexpr int SEG_KCH = 256;      // keys of one attention chunk: K and V of a head stay in LDS up to this many
constexpr int SEG_MAX_C = 256;    // widest row a workgroup keeps in LDS (hidden sizes, decoder width, labels)
constexpr int SEG_MAX_STAGES = 4;

// Every weight matrix is stored transposed and zero padded, Wt[Kp][ldw]: Kp a multiple of 32, ldw a multiple of 32.

// How the A operand [SEG_BM rows][K] of the first product is made
enum {
    SEG_A_ROWS = 0,     // the rows themselves, in[row][c] (K = n1: no first product, the rows are its "result")
    SEG_A_CONV = 1,     // a k x k / stride s / pad p convolution's patch of an NCHW image or an NHWC token grid
    SEG_A_DWGELU = 2,   // gelu(depthwise 3x3 conv + bias) of a token grid [gh * gw][K]
    SEG_A_DECODE = 3,   // the decode head's concatenation: bilinear upsamples of the projected stage outputs, last stage first
};
// What becomes of the second product's [SEG_BM][n2] tile
enum {
    SEG_OUT_ROWS = 0,   // out2[row][c] = v + bias2[c]
    SEG_OUT_NCHW = 1,   // out2[c][row]  = v + bias2[c]              (the logits)
    SEG_OUT_ARGMAX = 2, // out2_u8[row]  = argmax_c (v + bias2[c]), the lowest c among equals
};

struct SegFused {
    int a_mode;
    int m;                   // rows (tokens of the output grid)
    // ---- first stage: R[32][n1] = A[32][k1] x w1[k1][n1] + bias1, or the rows (SEG_A_ROWS)
    const float* in;         // ROWS: [m][n1]; CONV: the image; DWGELU: [m][k1]
    int k1, n1;              // k1 padded to a multiple of 32 in w1; n1 a multiple of 32, <= SEG_MAX_C
    const float* w1;         // [k1p][n1]
    const float* bias1;      // [n1] or null
    // CONV
    int nchw, in_h, in_w, in_c, ksz, stride, pad, out_w, k1_real;
    // DWGELU: grid of the tokens, depthwise weights [9][k1] and bias [k1]
    int gh, gw;
    const float* dw_w;
    const float* dw_b;
    // DECODE: stage s (0 .. nstage-1) is proj[s] [sh[s] * sw[s]][dec], the concatenation holds stage nstage-1 first
    int nstage, dec;
    const float* proj[SEG_MAX_STAGES];
    int sh[SEG_MAX_STAGES], sw[SEG_MAX_STAGES];
    // ---- on R, in this order
    const float* ln_g;       // LayerNorm over the n1 columns (eps 1e-5), or null
    const float* ln_b;
    const float* bn_scale;   // max(R * scale + shift, 0) (the folded BatchNorm + ReLU), or null
    const float* bn_shift;
    const float* res;        // += res[row][c] (may be out1: the residual stream in place), or null
    float* out1;             // [m][n1] R as it is now, or null
    // ---- second product: [32][n2] = R x w2[n1][ldw2] in chunks of 256 columns, or w2 == null
    const float* w2;
    const float* bias2;      // [n2p]
    int n2, ldw2;            // real columns, padded row length of w2 (a multiple of 32)
    int out_mode;
    float* out2;
    int ld_out2;             // ROWS: row length; NCHW: plane size (m)
    uint8_t* out2_u8;
};

struct SegAttn {
    int m, keys, heads, c;        // queries, keys, heads of 32, c = heads * 32
    const float* q;               // q[row * q_ld + head * 32 + d]
    int q_ld;
    const float* k;               // k[key * kv_ld + head * 32 + d], v likewise
    const float* v;
    int kv_ld;
    const float* wo;              // [c][c] transposed
    const float* bo;              // [c]
    float* x;                     // [m][c]: x += o_proj(attention) in place
};

size_t seg_fused_lds_bytes(const SegFused& a);
size_t seg_attn_lds_bytes(const SegAttn& a);
hipError_t launch_seg_fused(const SegFused& a, hipStream_t s);
hipError_t launch_seg_attn(const SegAttn& a, hipStream_t s);

// ---- segformer_pre.hip: one pass of PIL's 8-bit resample.  Output index i of the pass reads inputs bounds[2i] ..
// bounds[2i] + bounds[2i + 1] - 1 with the integer coefficients coef[i * ksize + j] (22 fractional bits).
struct SegResample {
    const uint8_t* src;      // [h][w][c]
    int h, w, c;
    int vertical;            // 0: along x (output [h][out][c]); 1: along y (output [out][w][c])
    int out;
    const int* bounds;
    const int* coef;
    int ksize;
    uint8_t* dst;            // u8 output, or null
    float* dst_f32;          // vertical pass only: normalised NCHW planes [c][out][w] ((v / 255 - mean) / std), or null
    float mean[4], stdv[4];
};
hipError_t launch_seg_resample(const SegResample& a, hipStream_t s);

}  // namespace nesr
