// Internal interface of the Swin2SR path: the nesr_swin2sr_* entries of the C ABI (swin2sr_api.cpp) drive the three kernels of
// swin2sr.hip.  Not part of the public ABI.
//
// Activations are token-major f32 rows [B][H * W][cs] (B images of one size, one after the other), cs = the width rounded up to
// 16 (the MFMA tile); the columns past the real width are zero in every buffer.  Every weight matrix is stored transposed and
// zero padded, Wt[K][N]: K and N multiples of 16 (a conv: K = 9 taps x the input width rounded up to 4), so a padded column
// meets a zero weight row and a padded output column comes out zero.
//
// A launch takes `batch` images of one padded size H x W: the conv and the attention kernel read the image index from
// blockIdx.z and offset every base by it in size_t; the row kernel sees batch * H * W rows.  batch = 1 is a whole frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nesr {

constexpr size_t S2_LDS_LIMIT = 160 * 1024;      // LDS of one CU (gfx950); one workgroup may take all of it
constexpr int S2_BM = 32;                        // token rows of one workgroup of the row kernel
constexpr int S2_ROWS_MAX = 0x7fffffff - S2_BM;  // token rows of one launch (batch * H * W): the row index is an int
constexpr int S2_ATTN_THREADS = 512;             // the attention kernel's workgroup: 8 waves, two a SIMD
constexpr int S2_CONV_TW = 16, S2_CONV_TH = 4;   // output pixels of one workgroup of the conv kernel: 4 rows of 16

// One axis of the tile plan of a frame of n pixels with cores of T and a context of P a side (nesr_swin2sr_tile_plan, and the
// conv kernel's frame loader and u8 epilogue, which derive image b's window from its tile index: no table on the device).
// Every window of the axis is S = min(T + 2 P, n) long; core i is [c0, c1) and its window starts at w0 = clamp(c0 - P, 0, n - S):
// a window at the edge slides inward instead of shrinking.
__host__ __device__ inline int s2_window_side(int n, int T, int P) { return T + 2 * P < n ? T + 2 * P : n; }
__host__ __device__ inline void s2_tile_axis(int n, int T, int P, int i, int& w0, int& c0, int& c1) {
    const int S = s2_window_side(n, T, P);
    c0 = i * T;
    c1 = c0 + T < n ? c0 + T : n;
    w0 = c0 - P;
    if (w0 > n - S) w0 = n - S;
    if (w0 < 0) w0 = 0;
}

// One axis of the overlapped plan (nesr_swin2sr_overlap_plan, the window loader and the two overlap kernels): a padded axis of n
// pixels, tiles of t <= n whose starts step by st = t - tile_overlap >= 1: 0, st, 2 st, ... below n - t, then n - t, so the last
// tile ends at n and is in general not on the stride.  Gives the number of starts, the start of tile i (0 <= i < count) and the
// first and last tile that cover pixel p (0 <= p < n): the covering tiles are contiguous, first <= last.
__host__ __device__ inline void s2_overlap_axis(int n, int t, int st, int i, int p, int& count, int& start, int& first, int& last) {
    count = (n - t + st - 1) / st + 1;
    start = i < count - 1 ? i * st : n - t;
    first = p < t ? 0 : (p - t) / st + 1;      // the first regular start above p - t; past the regular ones: the last tile
    if (first > count - 1) first = count - 1;
    last = p >= n - t ? count - 1 : p / st;
}

// where the conv's input patch comes from
enum {
    S2_IN_ROWS = 0,        // in[(y * W + x) * cs_in + c]
    S2_IN_NEAREST2 = 1,    // the nearest x2 upsample of an (H / 2) x (W / 2) grid of rows
    S2_IN_FRAME_U8 = 2,    // an HWC u8 frame [fh][fw][cin]: / 255, symmetric pad to mh x mw, reflect pad to H x W, (v - mean) * range
    S2_IN_FRAME_F32 = 3,   // an NCHW f32 image [cin][fh][fw]: the same without the / 255
    S2_IN_WINDOW_U8 = 4,   // an H x W window of the symmetric extension of an HWC u8 frame [FH][FW][cin] (see ov_step): / 255, (v - mean) * range
};
// where the conv's result goes (after bias, LeakyReLU, residual and the PixelShuffle index map)
enum {
    S2_OUT_ROWS = 0,       // out[(oy * W r + ox) * cs_out + cc]
    S2_OUT_F32 = 1,        // v / range + mean, cropped to oh x ow, NCHW f32
    S2_OUT_U8 = 2,         // the same, then clamp to [0, 1], x 255, round to nearest even, HWC u8
};

struct S2Conv {
    int batch;                // images in the launch; `in`, `res` and `out` hold them one after the other (but see `tile`)
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
    // tile > 0 (FRAME_U8 and OUT_U8 only): image b is tile tile0 + b, in row-major order, of the plan s2_tile_axis makes of an
    // FH x FW frame.  FRAME_U8 reads its fh x fw window at the window's origin of `in`, the whole frame (row pitch FW); OUT_U8
    // writes the tile's core alone, at its place in `out`, the whole FH up x FW up frame.  tile = 0: a u8 frame comes alone
    // (FH = fh, FW = fw, batch = 1).
    int tile, tile_pad, tiles_x, tile0, FH, FW, up;
    // WINDOW_U8 (tile = 0, H = W = t): image b is tile tile0 + b, in row-major order with tiles_x a row, of the overlapped plan
    // (s2_overlap_axis) of the FH x FW frame padded to PH x PW, stride ov_step; its pixel (y, x) is the frame's symmetric extension
    // at (win_y + y, win_x + x).  No padding of the window itself: H and W are multiples of the attention window already.
    int ov_step, PH, PW;
    // the fp16 form (ROWS and NEAREST2 inputs): wh [9][coutp][cin rounded up to 16] f16; status: the context's range word
    int f16;
    const void* wh;
    unsigned* status;
};

// rows [m][cs] (m = batch * H * W) -> (x w1 + b1, gelu) -> (x w2 + b2) -> LayerNorm -> + res -> out; every step optional
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
    // the fp16 form (launches with w1): w1h [n1p][cs], w2h [cs][n1p] f16; status: the context's range word
    int f16;
    const void* w1h;
    const void* w2h;
    unsigned* status;
};

// one shifted-window attention block: out[token] = in[token] + LayerNorm(dense(attention(window of the token)))
struct S2Attn {
    int batch;                // images [H * W][cs] one after the other in `in` and `out`; the shift wraps inside each
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
    // the fp16 form: wqkvh [heads * 3 * dp][cs], woh [cs][cs] f16; status: the context's range word
    int f16;
    const void* wqkvh;
    const void* woh;
    unsigned* status;
};

size_t s2_conv_lds_bytes(const S2Conv& a);
size_t s2_rows_lds_bytes(const S2Rows& a);
size_t s2_attn_lds_bytes(const S2Attn& a);
hipError_t launch_s2_conv(const S2Conv& a, hipStream_t s);
hipError_t launch_s2_rows(const S2Rows& a, hipStream_t s);
hipError_t launch_s2_attn(const S2Attn& a, hipStream_t s);

// The overlapped route's accumulator and its two kernels.  E is f32, planar [3][plane], plane = PH up x PW up rounded up to 4
// (a thread's four pixels are one 16-byte access a channel); Y holds a batch's window outputs [batch][3][t up][t up] f32.
struct S2Overlap {
    int PH, PW, t, step, up;      // the padded frame, the tile, its stride (input pixels) and the scale
    int tiles_y, tiles_x;         // s2_overlap_axis's counts of PH and PW
    int tile0, batch;             // add: Y holds tiles tile0 .. tile0 + batch - 1
    const float* Y;               // add
    float* E;
    uint8_t* out;                 // finish: HWC u8 [oh][ow][3], the crop of the padded output
    int oh, ow;
};
__host__ __device__ inline size_t s2_overlap_plane(int PH, int PW, int up) { return ((size_t)PH * up * PW * up + 3) / 4 * 4; }
hipError_t launch_s2_overlap_add(const S2Overlap& a, hipStream_t s);
hipError_t launch_s2_overlap_finish(const S2Overlap& a, hipStream_t s);

}  // namespace nesr
