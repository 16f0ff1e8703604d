// Internal interface of the Swin2SR path: the nesr_swin2sr_* entries of the C ABI (swin2sr_api.cpp) drive the three kernels of
// swin2sr.hip.  Not part of the public ABI.
//
// Activations are token-major f32 rows [H * W][cs], cs = the width rounded up to 16 (the MFMA tile); the columns past the real
// width are zero in every buffer.  Every weight matrix is stored transposed and zero padded, Wt[K][N]: K and N multiples of 16
// (a conv: K = 9 taps x the input width rounded up to 4), so a padded column meets a zero weight row and a padded output column
// comes out zero.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nesr {

constexpr size_t S2_LDS_LIMIT = 160 * 1024;      // LDS of one CU (gfx950); one workgroup may take all of it
constexpr int S2_BM = 32;                        // token rows of one workgroup of the row kernel
constexpr int S2_ATTN_THREADS = 512;              // the attention kernel's workgroup: 8 waves, two a SIMD
constexpr int S2_CONV_TW = 16, S2_CONV_TH = 4;   // output pixels of one workgroup of the conv kernel: 4 rows of 16

// where the conv's input patch comes from
enum {
    S2_IN_ROWS = 0,        // in[(y * W + x) * cs_in + c]
    S2_IN_NEAREST2 = 1,    // the nearest x2 upsample of an (H / 2) x (W / 2) grid of rows
    S2_IN_FRAME_U8 = 2,    // an HWC u8 frame [fh][fw][cin]: / 255, symmetric pad to mh x mw, reflect pad to H x W, (v - mean) * range
    S2_IN_FRAME_F32 = 3,   // an NCHW f32 image [cin][fh][fw]: the same without the / 255
};
// where the conv's result goes (after bias, LeakyReLU, residual and the PixelShuffle index map)
enum {
    S2_OUT_ROWS = 0,       // out[(oy * W r + ox) * cs_out + cc]
    S2_OUT_F32 = 1,        // v / range + mean, cropped to oh x ow, NCHW f32
    S2_OUT_U8 = 2,         // the same, then clamp to [0, 1], x 255, round to nearest even, HWC u8
};

struct S2Conv {
    int in_mode;
    const void* in;
    int H, W;                 // the conv's domain (its output grid before any shuffle)
    int cin, cinp, cs_in;     // real input channels, rounded up to 4 (K per tap), row stride of `in` (ROWS, NEAREST2)
    int fh, fw, mh, mw;       // FRAME: the frame, and the model's input size after the processor's symmetric padding
    float mean[4], range;
    const float* w;           // [9 * cinp][coutp]
    const float* bias;        // [coutp]
    int cout, coutp;          // real output channels, rounded up to 16
    int lrelu;
    float slope;
    const float* res;         // += res[(y * W + x) * cs_res + c], or null
    int cs_res;
    int shuffle;              // PixelShuffle factor r >= 1: channel c = (cc r + r1) r + r2 goes to pixel (y r + r1, x r + r2), channel cc
    int out_mode;
    void* out;
    int cs_out;               // ROWS: row stride
    int oh, ow;               // F32, U8: the crop
};

// rows [m][cs] -> (x w1 + b1, gelu) -> (x w2 + b2) -> LayerNorm -> + res -> out; every step optional
struct S2Rows {
    int m, c, cs;
    const float* in;
    const float* w1;          // [cs][n1p] or null
    const float* b1;
    int n1p, gelu;            // n1p == cs when there is no w2
    const float* w2;          // [n1p][cs] or null
    const float* b2;
    const float* ln_g;        // [cs] (zero past c) or null
    const float* ln_b;
    float eps;
    const float* res;         // [m][cs] or null (may be `out`)
    float* out;               // [m][cs] (may be `in`)
};

// one shifted-window attention block: out[token] = in[token] + LayerNorm(dense(attention(window of the token)))
struct S2Attn {
    int H, W, ws, shift, heads, d, dp, c, cs;     // d = c / heads, dp = d rounded up to 16
    const float* in;
    float* out;               // may be `in`: a token is read and written by its window's workgroup alone
    const float* wqkv;        // [cs][heads * 3 * dp]: per head the q, k and v columns, each padded to dp
    const float* bqkv;        // [heads * 3 * dp] (zero for k)
    const float* scale;       // [heads] exp(min(logit_scale, ln 100))
    const float* bias;        // [heads][ws^2][ws^2] 16 sigmoid(MLP(table))[index]
    const float* wo;          // [cs][cs]
    const float* bo;          // [cs]
    const float* ln_g;
    const float* ln_b;
    float eps;
};

size_t s2_conv_lds_bytes(const S2Conv& a);
size_t s2_rows_lds_bytes(const S2Rows& a);
size_t s2_attn_lds_bytes(const S2Attn& a);
hipError_t launch_s2_conv(const S2Conv& a, hipStream_t s);
hipError_t launch_s2_rows(const S2Rows& a, hipStream_t s);
hipError_t launch_s2_attn(const S2Attn& a, hipStream_t s);

}  // namespace nesr
