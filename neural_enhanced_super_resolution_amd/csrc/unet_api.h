// Internal interface of the UNet path: the nesr_unet_* entries of the C ABI (unet_api.cpp) drive the kernels of unet.hip.
// Not part of the public ABI.
//
// Activations are pixel-major f32 rows [n H W][cs], sample after sample, cs = the width rounded up to 16 (the MFMA tile); the
// columns past the real width are zero in every buffer, as in vae_api.h.  A weight matrix is stored transposed and zero padded,
// Wt[K][N]; the K of a product over a concatenation is the two sources' padded widths one after the other.
//
// The launchers of vae_api.h take one sample and widths up to 512; this network has two samples a call, widths up to 1024 and
// inputs of two sources (up to 2048 channels), so unet.hip has launchers, argument structs and kernel entries of its own.  What is
// shared: VaeNorm, what a GroupNorm leaves per channel for its consumer's loader; the tile constants of the conv, the GroupNorm and
// the attention; and, in f32_rows_device.h, the device bodies of the conv (patch loader, tap loop), of the GroupNorm statistics and
// of the streamed attention, which both files' kernels call with their own tile, sample and source.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vae_api.h"

namespace nesr {

constexpr int UNET_MAX_WIDTH = 1024;               // a block's width, and cross_attention_dim
constexpr int UNET_MAX_TEMB = 4 * UNET_MAX_WIDTH;  // the embedding's width, 4 x block_out_channels[0]
constexpr int UNET_MAX_RESNETS = 30;               // 4 levels of 3 layers: 12 down, 2 mid, 16 up
constexpr int UNET_BM = 32;                        // rows of one workgroup of the row GEMM
constexpr int UNET_KC = 64;                        // K of one chunk of the row GEMM and of the stride-1 conv (stride 2: 32)
constexpr int UNET_BN = 256;                       // output columns of one workgroup of the row GEMM (GEGLU: 128, both halves)
constexpr int UNET_ATTN_BQ = 32, UNET_ATTN_BK = 32;   // queries of a workgroup of the attention, keys of one chunk
constexpr int UNET_MAX_HEAD = 128;                 // head width
constexpr int UNET_MAX_SELF_TOKENS = 1 << 16;      // tokens of a self-attention (256 x 256 at the level that has it)
constexpr long long UNET_MAX_PIXELS = 1ll << 22;   // n h w of one forward

// rows [rows][cs] <- src: NCHW (element (s, c, p) at (s C + c) m + p, row s m + p) or row-major [rows][C]; zero past C
struct UnetIn {
    const float* src;
    int nchw, c, cs, m;       // m: pixels of a sample (NCHW)
    long long rows;
    float* out;
};

// One source of a conv or of a row product: rows [n m][cs], c real channels; norm [n][cs] of its GroupNorm, or null.
struct UnetSrc {
    const float* p;
    int c, cs;
    const VaeNorm* norm;
};

// 3x3 conv, zero padding 1 on all sides: stride 1 over rows or over their nearest-x2 grid (up), or stride 2.  One or two
// sources (the concatenation hidden | skip); K per tap is each source's width rounded up to 4, one after the other.
struct UnetConv {
    int n, H, W;              // samples, the OUTPUT grid of one sample
    int stride, up;           // stride 2: the input grid is 2H x 2W; up: the input grid is (H / 2) x (W / 2)
    UnetSrc in[2];            // in[1].p null: one source.  A norm means GroupNorm + SiLU on every tap inside the image
    const float* w;           // [9 (cinp0 + cinp1)][coutp]
    const float* bias;        // [coutp]
    int cout, coutp;
    const float* res;         // += res[row coutp + c], or null (may be `out`)
    int out_nchw;             // 0: rows [n H W][coutp]; 1: [n][cout][H][W]
    float* out;
};

enum { UNET_PRO_NONE = 0, UNET_PRO_GROUPNORM = 1, UNET_PRO_LAYERNORM = 2 };

// rows -> prologue -> x w + b -> (+ res | GEGLU) -> out [m][np]
struct UnetRows {
    int m, rows_per_sample;
    UnetSrc in[2];            // K = cs0 + cs1; norm used by UNET_PRO_GROUPNORM (no activation)
    int prologue;
    const float4* ln;         // [m] (mean hi, mean lo, rstd, 0) of UNET_PRO_LAYERNORM, with gamma / beta [cs0]
    const float* ln_g;
    const float* ln_b;
    const float* w;           // [K][ldw]
    const float* b;           // [ldw]
    int ldw, np;              // np output columns; GEGLU: ldw = 2 np, out = (x w + b)[:, :np] * gelu((x w + b)[:, np:])
    int geglu;
    const float* res;         // [m][np] or null (may be `out`)
    float* out;               // never `in`
};

// per row of [m][cs] the mean and 1 / sqrt(var + eps) over the c real columns, two passes, sums in double
struct UnetLnStats {
    const float* in;
    int m, c, cs;
    float eps;
    float4* out;              // (mean hi, mean lo, rstd, 0)
};

// GroupNorm statistics of one or two sources side by side: c0 + c1 channels in `groups` groups (a group may straddle the seam)
struct UnetGn {
    int n, m;                 // samples, pixels of a sample
    UnetSrc in[2];            // .norm is the OUTPUT here: [n][cs] each
    double* partial[2];       // [n][blocks][cs][2]
    int groups;
    const float* gamma;       // [c0 + c1], the concatenation's order
    const float* beta;
    float eps;
};

// softmax(q k^T / sqrt(d)) v per sample and head, streamed over key chunks: q [samples nq][ldq], k and v [samples nk][ldkv], head
// h in columns [h d, (h + 1) d); out [samples nq][ldo], its columns past heads d zeroed
struct UnetAttn {
    int samples, nq, nk, heads, d;
    const float* q;
    const float* k;
    const float* v;
    int ldq, ldkv, ldo;
    float* out;
};

// silu(time_embedding(sinusoid(t)) + class row) -> out [tdp]
struct UnetEmb {
    double timestep;
    int c0, td, tdp;          // sinusoid width, embedding width and its padding
    const float* w1;          // [c0][tdp]
    const float* b1;
    const float* w2;          // [td][tdp]
    const float* b2;
    const float* cls;         // the label's row [tdp]
    float* out;
};

// per resnet r: out[r][c] = conv1.bias[c] + time_emb_proj.bias[c] + sum_k semb[k] Wt[k][c]: conv1's bias of this forward
struct UnetTemb {
    int count, td;
    const float* semb;
    const float* weights;     // the packed weights; the offsets below are in floats
    float* out;               // [count][UNET_MAX_WIDTH]
    struct {
        unsigned long long w, b, cb;
        int coutp;
    } r[UNET_MAX_RESNETS];
};

size_t unet_conv_lds_bytes(int stride);
size_t unet_rows_lds_bytes();
size_t unet_attn_lds_bytes();
size_t unet_emb_lds_bytes();
inline size_t unet_gn_blocks(size_t m) { return (m + VAE_GN_PIXELS - 1) / VAE_GN_PIXELS; }
hipError_t launch_unet_in(const UnetIn& a, hipStream_t s);
hipError_t launch_unet_conv(const UnetConv& a, hipStream_t s);
hipError_t launch_unet_rows(const UnetRows& a, hipStream_t s);
hipError_t launch_unet_ln_stats(const UnetLnStats& a, hipStream_t s);
hipError_t launch_unet_gn_partial(const UnetGn& a, int source, hipStream_t s);
hipError_t launch_unet_gn_finish(const UnetGn& a, hipStream_t s);
hipError_t launch_unet_attn(const UnetAttn& a, hipStream_t s);
hipError_t launch_unet_emb(const UnetEmb& a, hipStream_t s);
hipError_t launch_unet_temb(const UnetTemb& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------- the fp16 compute form
// unet_f16.hip: the products of launch_unet_conv and launch_unet_rows with both operands rounded to f16 (a plain cast: nearest even),
// f32 products and sums on v_mfma_f32_16x16x32_f16 (a K tail of 16 on v_mfma_f32_16x16x16_f16).  Storage, prologues, biases, residuals
// and GEGLU are the f32 form's.  The launchers take the f32 structs, whose `w` is ignored, with the weight as a second, f16 copy:
//
//   rows   W16[ldw][K],            K = cs0 + cs1, k contiguous: element (k, n) of Wt[K][ldw] lies at n K + k
//   conv   W16[coutp][9][cs0 + cs1]: per output channel and tap source 0's cs0 channels, then source 1's cs1; each source's K is its
//          row width cs (the width rounded up to 16, zeros past the real width), not the f32 form's width rounded up to 4
//
// so a B fragment of 8 k is one 16-byte load.  The activation is rounded after the prologue, at the store into LDS; a value that is
// non-finite or beyond +-65504 there raises `status` (elem16.h; null: unchecked).  An f16 subnormal operand is kept, not flushed.
//
// An output element's K chain runs in one workgroup in ascending k (per source: steps of 32, then the tail of 16), whatever the
// column block, so its bits do not depend on the block the launcher picks, on m or on n.  The launcher picks the widest of 128, 64
// and 32 output columns (conv: channels) a workgroup whose grid still has UNET_F16_FILL workgroups, else 32.
struct UnetRows16 : UnetRows {
    const _Float16* w16;
    unsigned* status;
};
struct UnetConv16 : UnetConv {
    const _Float16* w16;
    unsigned* status;
};
constexpr int UNET_F16_FILL = 256;      // one workgroup a CU of the MI355X
int unet_rows_f16_block(int m, int np);                              // the output columns of a workgroup: 128, 64 or 32
int unet_conv_f16_block(int n, int H, int W, int coutp);             // the output channels of a workgroup: 128, 64 or 32
size_t unet_rows_f16_lds_bytes();
size_t unet_conv_f16_lds_bytes(int stride);
hipError_t launch_unet_rows_f16(const UnetRows16& a, hipStream_t s);
hipError_t launch_unet_conv_f16(const UnetConv16& a, hipStream_t s);

}  // namespace nesr

// The forward of a finalized context on the caller's stream, as nesr_unet_forward_f32 makes it after its checks, without the fp16
// form's bracket: the range word is neither cleared in front nor read behind, and nothing waits.  The x4 pipeline (sdx4_api.cpp)
// calls it once a step between one unet_range_begin and one unet_range_end, so its call has no synchronisation inside.
// unet_range_begin clears the word (fp16 form; f32: nothing); unet_range_end waits for the stream and returns NESR_ERR_RANGE if it
// was raised (fp16 form; f32: nothing, no wait).
struct nesr_unet;
int unet_forward_unchecked(nesr_unet* c, const float* sample, int n, int ch, int h, int w, double timestep, int class_label, const float* text_states, int tokens,
                           float* out, size_t out_elems, hipStream_t s);
int unet_range_begin(nesr_unet* c, hipStream_t s);
int unet_range_end(nesr_unet* c, hipStream_t s, const char* entry);
