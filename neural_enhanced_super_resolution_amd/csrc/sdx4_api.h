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
