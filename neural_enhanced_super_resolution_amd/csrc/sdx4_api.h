// Internal interface of the x4 diffusion pipeline: the nesr_sdx4_* entries of the C ABI (sdx4_api.cpp) chain the three networks'
// entries with the two kernels of sdx4_step.hip, which stand for the arithmetic between them: the schedulers and the guidance.
// Not part of the public ABI.
//
// The UNet's input is NCHW [n][lc + 3][hw]: channels 0 .. lc - 1 are the latents, channels lc .. lc + 2 the noised low-res image.
// Both kernels write straight into it, so no concatenation is ever stored; the latents themselves are [lc][hw].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nesr_hip.h"

namespace nesr {

constexpr int SDX4_IMAGE_CHANNELS = 3;
constexpr int SDX4_MAX_LATENT_CHANNELS = 8;      // the VAE's limit
constexpr long long SDX4_MAX_FRAME_PIXELS = 1ll << 22;      // low-res pixels of a frame that runs over windows

// image: sample[s][lc + c][p] = sa (frame[p][c] / 127.5 - 1) + sb noise[c][p]; latents: sample[s][k][p] = lat_out[k][p] = sigma
// latents[k][p]; for every sample s < n.  hw is a multiple of 4 and the float pointers are 16-byte aligned, the frame 4-byte.
struct Sdx4Prepare {
    const uint8_t* frame;     // [hw][3]
    const float* noise;       // [3][hw]
    const float* latents;     // [lc][hw]
    int n, hw, lc;
    float sa, sb, sigma;      // sqrt(abar_L), sqrt(1 - abar_L) of the low-res scheduler; init_noise_sigma
    float* sample;            // [n][lc + 3][hw]
    float* lat_out;           // [lc][hw]
};

// m = n == 2 ? model[0] + g (model[1] - model[0]) : model[0]   (batch order [negative, prompt])
// x0 = c0x x + c0m m, e = cex x + cem m, x' = sp x0 + sq e -> lat_out[k][p] and sample[s][k][p] for every s; channels lc .. stay.
struct Sdx4Step {
    const float* model;       // [n][lc][hw]
    const float* latents;     // [lc][hw]
    int n, hw, lc;
    float g, c0x, c0m, cex, cem, sp, sq;
    float* lat_out;           // [lc][hw]; may be `latents`
    float* sample;            // [n][lc + 3][hw]
};

hipError_t launch_sdx4_prepare(const Sdx4Prepare& a, hipStream_t s);
hipError_t launch_sdx4_step(const Sdx4Step& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------- windows (sdx4_tiled.hip)
// One axis of the window plan (nesr_sdx4_tile_plan): windows of t at 0, t - r, ... below n - t, then n - t; r is the overlap and
// the ramp.  a: the origin of the window a launch works on (the kernels that normalise do not read it).  Output resolution: every
// field times the VAE's scale.  A window weighs i by min(left, right), left = a > 0 && r ? min(i - a + 1, r) / r : 1, right =
// a + t < n && r ? min(a + t - i, r) / r : 1; a pixel's normaliser is the sum over the axis's windows that cover it, ascending.
struct Sdx4Axis {
    int n, t, r, a;
};

// dst[s][c][y][x] = src[c][ay + y][ax + x] for every sample s < n, c < channels: the window's UNet input from the full-frame buffer
// (channels = lc + 3), or its latents (channels = lc, n = 1).  x.n, x.t and x.a are even; the pointers 8-byte aligned.
struct Sdx4Gather {
    const float* src;         // [channels][y.n][x.n]
    int n, channels;
    Sdx4Axis y, x;
    float* dst;               // [n][channels][y.t][x.t]
};

// acc[c][ay + y][ax + x] = fmaf(w(y, x), m, acc), m = n == 2 ? model[0] + g (model[1] - model[0]) : model[0], w = wy wx
struct Sdx4Accumulate {
    const float* model;       // [n][lc][y.t][x.t]
    int n, lc;
    Sdx4Axis y, x;
    float g;
    float* acc;               // [lc][y.n][x.n]
};

// m = acc / (Sy Sx), then sdx4_step_kernel's chain on x = frame[k]: x' -> frame[k] (channels lc .. stay), acc <- 0
struct Sdx4TiledStep {
    float* acc;               // [lc][y.n][x.n]
    float* frame;             // [lc + 3][y.n][x.n]
    int lc;
    Sdx4Axis y, x;            // .a unused
    float c0x, c0m, cex, cem, sp, sq;
};

// acc[Y][X][c] = fmaf(w(Y, X), sample[c][Y - ay][X - ax], acc) over the window's output pixels; the axes are at output resolution
struct Sdx4BlendAdd {
    const float* sample;      // [3][y.t][x.t], the VAE's f32 output of the window
    Sdx4Axis y, x;
    float* acc;               // [y.n][x.n][3]
};

// out = u8(rint(clamp(acc / (Sy Sx) / 2 + 0.5, 0, 1) 255)), the VAE epilogue's order; x.n is a multiple of 4
struct Sdx4BlendFinish {
    const float* acc;         // [y.n][x.n][3]
    Sdx4Axis y, x;            // .a unused
    uint8_t* out;             // [y.n][x.n][3]
};

hipError_t launch_sdx4_gather(const Sdx4Gather& a, hipStream_t s);
hipError_t launch_sdx4_accumulate(const Sdx4Accumulate& a, hipStream_t s);
hipError_t launch_sdx4_tiled_step(const Sdx4TiledStep& a, hipStream_t s);
hipError_t launch_sdx4_blend_add(const Sdx4BlendAdd& a, hipStream_t s);
hipError_t launch_sdx4_blend_finish(const Sdx4BlendFinish& a, hipStream_t s);

// the plan of one axis on the host: the number of windows and the origin of window k (the last ends at n)
inline int sdx4_axis_windows(int n, int t, int r) { return (n - t + (t - r) - 1) / (t - r) + 1; }
inline int sdx4_axis_origin(int n, int t, int r, int k) { return k == sdx4_axis_windows(n, t, r) - 1 ? n - t : k * (t - r); }
inline Sdx4Axis sdx4_axis(int n, int t, int r, int a, int scale = 1) { return Sdx4Axis{n * scale, t * scale, r * scale, a * scale}; }

// The VAE decode over windows (vae_api.cpp), for nesr_vae_decode_latents_tiled_u8 and for the pipeline: per window a gather of its
// latents, the f32 decode behind nesr_vae_decode_f32 with the scaling factor as nesr_vae_decode_latents_u8 divides by it, a
// blend-add; then one finish.  h x w latents, windows of ty x tx with ramp r; `buf` holds sdx4_vae_tiled_plan(...).total bytes.  The
// caller has checked the plan (sdx4_check_windows) and the context.  With a timer the three window kernels are counted and timed
// by it in `groups` (the pipeline's); with none they are launched as they are.
struct GroupTimer;
struct Sdx4TileGroups {
    int gather, add, finish;
};
// the regions of `buf`: one window's latents [lc][ty][tx], its f32 sample [3][ty s][tx s], the f32 frame [h s][w s][3].  Needs no
// context, so the pipeline's device-free size query uses it too.
struct Sdx4VaeTiledPlan {
    size_t window, sample, acc, total;
};
Sdx4VaeTiledPlan sdx4_vae_tiled_plan(int lc, int scale, int h, int w, int ty, int tx);
int sdx4_check_windows(const char* entry, const char* what, int h, int w, int multiple, int tile, int overlap, int* ty, int* tx);
int sdx4_vae_decode_tiled(nesr_vae* c, const float* latents, int h, int w, int ty, int tx, int r, char* buf, uint8_t* out, GroupTimer* timer, const char* model,
                          Sdx4TileGroups groups, hipStream_t s);

// What the pipeline asks of the three contexts it does not own (their structs are private to their files; defined at the end of
// clip_text_api.cpp, unet_api.cpp and vae_api.cpp).  `launches`: the context's launch counter as it stands.
struct Sdx4TextInfo {
    int device, hidden, positions, vocab;
    bool finalized;
    int64_t launches;
};
struct Sdx4UnetInfo {
    int device, cin, cout, levels, cross, classes;
    bool finalized;
    int64_t launches;
};
struct Sdx4VaeInfo {
    int device, latent, cout, blocks;
    bool finalized;
    int64_t launches;
};
Sdx4TextInfo sdx4_text_info(const nesr_clip_text* c);
Sdx4UnetInfo sdx4_unet_info(const nesr_unet* c);
Sdx4VaeInfo sdx4_vae_info(const nesr_vae* c);

}  // namespace nesr
