// Internal interface of the VAE decoder path: the nesr_vae_* entries of the C ABI (vae_api.cpp) drive the kernels of vae.hip.
// Not part of the public ABI.
//
// Activations are pixel-major f32 rows [H * W][cs], cs = the width rounded up to 16 (the MFMA tile); the columns past the real
// width are zero in every buffer.  Every weight matrix is stored transposed and zero padded, Wt[K][N]: N a multiple of 16, K a
// multiple of 16 for a 1x1 product and 9 taps x the input width rounded up to 4 for a 3x3 conv (the padding of swin2sr_api.h).
//
// A GroupNorm is two launches over its input (fixed-order partial sums in double, then one workgroup a group) that leave four
// floats a channel, VaeNorm; the consumer's loader applies them: (x - mean) * a + beta, then SiLU in front of a conv.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nesr {

constexpr size_t VAE_LDS_LIMIT = 160 * 1024;     // LDS of one CU (gfx950)
constexpr int VAE_BM = 32;                       // pixel rows of one workgroup of the row kernel
constexpr int VAE_CONV_TW = 16, VAE_CONV_TH = 4; // output pixels of one workgroup of the conv kernel: 4 rows of 16
constexpr int VAE_CONV_KC = 64;                  // input channels of one K chunk of the conv kernel's patch
constexpr int VAE_CONV_NB = 128;                 // output channels of one workgroup of the conv kernel (two tiles a wave)
constexpr int VAE_ATTN_BQ = 32, VAE_ATTN_BK = 32;   // queries of a workgroup of the attention kernel, keys of one chunk
constexpr int VAE_GN_PIXELS = 512;               // pixels of one partial sum of the GroupNorm statistics
constexpr int VAE_MAX_TOKENS = 1 << 16;          // tokens (latent pixels) the attention takes: 256 x 256 latents
constexpr long long VAE_MAX_PIXELS = 1ll << 24;  // output pixels of one decode

// per channel, what a loader needs of a GroupNorm: x -> ((x - mean_hi) - mean_lo) * a + beta, a = gamma * rstd; zero past the width
struct VaeNorm {
    float mean_hi, mean_lo, a, beta;
};

enum { VAE_IN_ROWS = 0, VAE_IN_NEAREST2 = 1 };
enum {
    VAE_OUT_ROWS = 0,      // out[(y * W + x) * cs_out + c]
    VAE_OUT_F32 = 1,       // NCHW f32 [cout][H][W]
    VAE_OUT_U8 = 2,        // v / 2 + 0.5, clamp to [0, 1], x 255, round to nearest even, HWC u8 [H][W][cout]
};

struct VaeConv {
    int in_mode;
    const float* in;          // rows; NEAREST2: an (H / 2) x (W / 2) grid of them
    int H, W;                 // the conv's domain
    int cin, cinp, cs_in;     // real input channels, rounded up to 4 (K per tap), row stride of `in`
    const VaeNorm* norm;      // GroupNorm + SiLU on every tap inside the image (a tap outside is 0), or null
    const float* w;           // [9 * cinp][coutp]
    const float* bias;        // [coutp]
    int cout, coutp;
    const float* res;         // += res[(y * W + x) * cs_res + c], or null (may be `out`)
    int cs_res;
    int out_mode;
    void* out;
    int cs_out;               // ROWS: row stride (= coutp)
};

// rows [m][cs_in] -> (GroupNorm, no activation) -> x w + b -> + res -> out [m][np]
struct VaeRows {
    int m, cs_in, np;
    const float* in;
    const VaeNorm* norm;      // or null
    const float* w;           // [cs_in][np]
    const float* b;           // [np]
    const float* res;         // [m][np] or null (may be `out`)
    float* out;               // may be `in` when np == cs_in
};

// z NCHW f32 [c][H * W] -> rows [H * W][16], each value divided by `divisor` (1 for none); columns past c are zero
struct VaeIn {
    const float* z;
    int c, m;
    float divisor;
    float* out;
};

// GroupNorm statistics of rows [m][cs]: c real channels in `groups` groups
struct VaeStats {
    const float* in;
    int m, c, cs, groups;
    double* partial;          // [ceil(m / VAE_GN_PIXELS)][cs][2]: sum and sum of squares, one slot a block
    const float* gamma;       // [cs]
    const float* beta;        // [cs]
    float eps;
    VaeNorm* out;             // [cs]
};

// one head of width c over n tokens: qkv [n][3 cs] (q | k | v) -> out [n][cs] = softmax(q k^T / sqrt(c)) v, streamed over key chunks
struct VaeAttn {
    int n, c, cs;
    const float* qkv;
    float* out;
};

size_t vae_conv_lds_bytes();
size_t vae_rows_lds_bytes(int cs_in);
size_t vae_attn_lds_bytes(int cs);
inline size_t vae_stats_blocks(size_t m) { return (m + VAE_GN_PIXELS - 1) / VAE_GN_PIXELS; }
hipError_t launch_vae_in(const VaeIn& a, hipStream_t s);
hipError_t launch_vae_conv(const VaeConv& a, hipStream_t s);
hipError_t launch_vae_rows(const VaeRows& a, hipStream_t s);
hipError_t launch_vae_stats_partial(const VaeStats& a, hipStream_t s);
hipError_t launch_vae_stats_finish(const VaeStats& a, hipStream_t s);
hipError_t launch_vae_attn(const VaeAttn& a, hipStream_t s);

}  // namespace nesr
