// Internal interface of the CLIP text encoder: the nesr_clip_text_* entries of the C ABI (clip_text_api.cpp) drive the kernels of
// clip_text.hip and, for every product and every LayerNorm inside a layer, the launchers of unet_api.h as they are.
// Not part of the public ABI.
//
// Activations are the UNet's rows: f32 [n tokens][cs], sample after sample, cs = the width rounded up to 16, zero past the width.
// q | k | v of a layer lie side by side in one buffer [n tokens][3 cs].  The token and position tables are [rows][c], unpadded
// (c is a multiple of 8: heads of 8 .. 128 columns in steps of 8).  The result leaves the row layout: [n tokens][c].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nesr_hip.h"
#include "unet_api.h"

namespace nesr {

constexpr int CLIP_MAX_HIDDEN = UNET_MAX_WIDTH;           // hidden_size
constexpr int CLIP_MAX_INTER = 4 * UNET_MAX_WIDTH;        // intermediate_size: the K the row GEMM's first source takes
constexpr int CLIP_MAX_IDS = 2 * NESR_UNET_MAX_TEXT_TOKENS;   // n tokens of one call; the ids travel in the launch's arguments

enum { CLIP_ACT_GELU = 0, CLIP_ACT_QUICK_GELU = 1 };

// out[row][0 .. cs) = tok[ids[row]] + pos[row % tokens], zero past c.  The ids are part of the argument block (2 KB at most): no
// copy, no buffer, nothing the host could change under a launch in flight.
struct ClipEmbed {
    const float* tok;         // [vocab][c]
    const float* pos;         // [positions][c]
    int vocab, positions;     // the launcher checks every id and `tokens` against them
    int rows, tokens, c, cs;  // rows = n tokens <= CLIP_MAX_IDS
    float* out;               // [rows][cs]
    int ids[CLIP_MAX_IDS];
};

// softmax(q k^T / sqrt(d) over keys 0 .. i) v for query i, per sample and head, streamed over key chunks: q, k, v [samples tokens]
// [ld], head h in columns [h d, (h + 1) d); out [samples tokens][ldo], its columns past heads d zeroed
struct ClipAttn {
    int samples, tokens, heads, d;
    const float* q;
    const float* k;
    const float* v;
    int ldq, ldkv, ldo;
    float* out;
};

// x = act(x) in place over `count` floats (a multiple of 4, x 16-byte aligned)
struct ClipAct {
    float* x;
    long long count;
    int act;
};

// out[row][0 .. c) = ((in[row][.] - mean hi) - mean lo) rstd g + b with the statistics launch_unet_ln_stats left
struct ClipFinal {
    const float* in;          // [m][cs]
    const float4* ln;         // [m]
    const float* g;
    const float* b;
    int m, c, cs;
    float* out;               // [m][c]
};

size_t clip_attn_lds_bytes();
hipError_t launch_clip_embed(const ClipEmbed& a, hipStream_t s);
hipError_t launch_clip_attn(const ClipAttn& a, hipStream_t s);
hipError_t launch_clip_act(const ClipAct& a, hipStream_t s);
hipError_t launch_clip_final(const ClipFinal& a, hipStream_t s);

}  // namespace nesr
