// The x4 diffusion upscaler as one call (nesr_sdx4_*): StableDiffusionUpscalePipeline's loop over the three networks' own entries
// (nesr_clip_text_encode_f32, nesr_unet_forward_f32, nesr_vae_decode_latents_u8) with the two kernels of sdx4_step.hip between
// them; nesr_sdx4_upscale_tiled_u8 runs the same loop and the decode over overlapping windows with the five kernels of
// sdx4_tiled.hip.  The schedulers' tables are computed here, on the host, in double, and reach the device as a handful of f32 coefficients
// in a launch's arguments: once the workspaces have their size, nothing is copied, allocated or synchronised between the first
// launch of a call and the last.  At the end: the single-launch test hooks nesr_sdx4_k_*.
//
// Recalled from diffusers, not checked against the library or a file: DDIMScheduler's "scaled_linear" betas,
// "leading" timesteps with steps_offset, the previous step t - T / N, final alpha-bar = alpha-bar[0] unless set_alpha_to_one, the
// v-prediction and epsilon forms of the eta = 0 step; DDPMScheduler's "squaredcos_cap_v2" betas and add_noise; the guidance's
// batch order [negative, prompt]; the noise level as the UNet's class label.
#include <cmath>
#include <cstring>

#include "api_common.h"
#include "sdx4_api.h"
#include "unet_api.h"

using namespace nesr;

namespace {

const char* const kName = "StableDiffusionX4Upscaler";

struct Ddim {
    int T = 1000, offset = 1;
    bool v_prediction = true;
    std::vector<double> abar;
    double final_abar = 1.0;
};

int unsupported(const char* entry, const std::string& field, const std::string& why) {
    return set_error(NESR_ERR_UNSUPPORTED, std::string(entry) + ": " + field + ": " + why);
}

// DDIMScheduler's tables
int make_ddim(const char* entry, Ddim& d, int T, double b0, double b1, const char* schedule, const char* prediction, int alpha_to_one, int offset, const char* spacing) {
    if (!schedule || !prediction || !spacing) return set_error(NESR_ERR_ARG, std::string(entry) + ": null scheduler field");
    if (T < 1 || T > 100000) return unsupported(entry, "num_train_timesteps", "1 .. 100000, got " + std::to_string(T));
    if (!(b0 > 0) || !(b1 >= b0) || !(b1 < 1)) return unsupported(entry, "beta_start / beta_end", "0 < beta_start <= beta_end < 1");
    const std::string sch = schedule, pred = prediction;
    if (sch != "scaled_linear" && sch != "linear") return unsupported(entry, "beta_schedule", "'" + sch + "' is not supported (scaled_linear, linear)");
    if (pred != "v_prediction" && pred != "epsilon") return unsupported(entry, "prediction_type", "'" + pred + "' is not supported (v_prediction, epsilon)");
    if (std::string(spacing) != "leading") return unsupported(entry, "timestep_spacing", "'" + std::string(spacing) + "' is not supported (leading)");
    if (offset < 0 || offset > 1) return unsupported(entry, "steps_offset", "0 or 1, got " + std::to_string(offset));
    d.T = T, d.offset = offset, d.v_prediction = pred == "v_prediction";
    d.abar.resize(T);
    const bool scaled = sch == "scaled_linear";
    const double lo = scaled ? std::sqrt(b0) : b0, hi = scaled ? std::sqrt(b1) : b1;
    double prod = 1.0;
    for (int i = 0; i < T; ++i) {
        const double v = T > 1 ? lo + (hi - lo) * (double)i / (double)(T - 1) : lo;
        prod *= 1.0 - (scaled ? v * v : v);
        d.abar[i] = prod;
    }
    d.final_abar = alpha_to_one ? 1.0 : d.abar[0];
    return NESR_OK;
}

int check_steps(const char* entry, const Ddim& d, int steps) {
    if (steps < 1 || steps > d.T) return set_error(NESR_ERR_ARG, std::string(entry) + ": steps must be 1 .. " + std::to_string(d.T) + " (num_train_timesteps), got " + std::to_string(steps));
    const int ratio = d.T / steps, top = (steps - 1) * ratio + d.offset;
    if (top >= d.T)
        return set_error(NESR_ERR_ARG, std::string(entry) + ": " + std::to_string(steps) + " steps put the first timestep at " + std::to_string(top) + ", past the table of " + std::to_string(d.T));
    return NESR_OK;
}

// step i of `steps`: its timestep, alpha-bar there and at the previous step, and the six coefficients of Sdx4Step
void ddim_step(const Ddim& d, int steps, int i, int& t, double& a, double& p, float coef[6]) {
    const int ratio = d.T / steps;
    t = (steps - 1 - i) * ratio + d.offset;
    const int prev = t - ratio;
    a = d.abar[t], p = prev >= 0 ? d.abar[prev] : d.final_abar;
    const double ra = std::sqrt(a), rb = std::sqrt(1.0 - a);
    if (d.v_prediction) coef[0] = (float)ra, coef[1] = (float)-rb, coef[2] = (float)rb, coef[3] = (float)ra;
    else coef[0] = (float)(1.0 / ra), coef[1] = (float)(-rb / ra), coef[2] = 0.f, coef[3] = 1.f;
    coef[4] = (float)std::sqrt(p), coef[5] = (float)std::sqrt(1.0 - p);
}

// DDPMScheduler's "squaredcos_cap_v2" alpha-bar
int make_low_res(const char* entry, std::vector<double>& abar, int T, const char* schedule) {
    if (!schedule) return set_error(NESR_ERR_ARG, std::string(entry) + ": null scheduler field");
    if (T < 1 || T > 100000) return unsupported(entry, "low_res num_train_timesteps", "1 .. 100000, got " + std::to_string(T));
    if (std::string(schedule) != "squaredcos_cap_v2") return unsupported(entry, "low_res beta_schedule", "'" + std::string(schedule) + "' is not supported (squaredcos_cap_v2)");
    const double half_pi = 1.5707963267948966;
    auto f = [&](double s) {
        const double c = std::cos((s + 0.008) / 1.008 * half_pi);
        return c * c;
    };
    abar.resize(T);
    double prod = 1.0;
    for (int i = 0; i < T; ++i) {
        prod *= 1.0 - std::min(1.0 - f((double)(i + 1) / T) / f((double)i / T), 0.999);
        abar[i] = prod;
    }
    return NESR_OK;
}

}  // namespace

// The window plan's rules for one pair (tile, overlap) on an h x w frame whose sides are multiples of `multiple`: ty = min(tile, h),
// tx = min(tile, w); the message names the value.  `what` is "tile" or "vae_tile".
int nesr::sdx4_check_windows(const char* entry, const char* what, int h, int w, int multiple, int tile, int overlap, int* ty, int* tx) {
    const std::string e = std::string(entry) + ": " + what;
    if (tile < 1 || tile % multiple) return set_error(NESR_ERR_ARG, e + " must be a positive multiple of " + std::to_string(multiple) + ", got " + std::to_string(tile));
    *ty = std::min(tile, h), *tx = std::min(tile, w);
    const int t = std::min(*ty, *tx);
    if (overlap < 0 || overlap >= t || overlap % multiple)
        return set_error(NESR_ERR_ARG, e + "_overlap must be a multiple of " + std::to_string(multiple) + " in 0 .. " + std::to_string(t - 1) + " (below the window of " +
                                           std::to_string(*ty) + " x " + std::to_string(*tx) + "), got " + std::to_string(overlap));
    if ((long long)*ty * *tx > NESR_VAE_MAX_TOKENS)
        return set_error(NESR_ERR_ARG, e + ": a window of " + std::to_string(*ty) + " x " + std::to_string(*tx) + " exceeds NESR_VAE_MAX_TOKENS = " + std::to_string(NESR_VAE_MAX_TOKENS) +
                                           " pixels");
    return NESR_OK;
}

struct nesr_sdx4 {
    nesr_clip_text* text = nullptr;
    nesr_unet* unet = nullptr;
    nesr_vae* vae = nullptr;
    int device = 0, lc = 4, levels = 4, scale = 4, max_noise_level = 350;
    Ddim ddim;
    std::vector<double> low_abar;
    char* ws_buf = nullptr;
    size_t ws_bytes = 0;
    int64_t last_launches = 0;
    GroupTimer timer;      // the pipeline's own kernels
};

namespace {

struct Plan {
    size_t text, sample, model, latents, total;
};

Plan plan(const nesr_sdx4* p, int n, int h, int w, int tokens) {
    Plan pl;
    ScratchCarver ws;
    const size_t hw = (size_t)h * w;
    pl.text = ws.take((size_t)n * tokens * sdx4_text_info(p->text).hidden * 4);
    pl.sample = ws.take((size_t)n * (p->lc + SDX4_IMAGE_CHANNELS) * hw * 4);
    pl.model = ws.take((size_t)n * p->lc * hw * 4);
    pl.latents = ws.take((size_t)p->lc * hw * 4);
    pl.total = ws.total();
    return pl;
}

// everything a call can be refused for, by the pipeline's own rules and by the three contexts' (their size queries check the frame)
int check_call(nesr_sdx4* p, const char* entry, int n, int h, int w, int tokens) {
    const std::string e = entry;
    const int div = 1 << (p->levels - 1);
    if (h < 1 || w < 1 || h % div || w % div)
        return set_error(NESR_ERR_ARG, e + ": h and w must be positive multiples of " + std::to_string(div) + " (2^(UNet levels - 1)), got " + std::to_string(h) + " x " + std::to_string(w));
    if ((long long)h * w > NESR_VAE_MAX_TOKENS)
        return set_error(NESR_ERR_ARG, e + ": a frame of " + std::to_string(h) + " x " + std::to_string(w) + " exceeds NESR_VAE_MAX_TOKENS = " + std::to_string(NESR_VAE_MAX_TOKENS) +
                                           " low-res pixels (the VAE attention's limit; tiling is out of scope)");
    size_t bytes = 0;
    int rc = nesr_clip_text_workspace_bytes(p->text, n, tokens, &bytes);
    if (!rc) rc = nesr_unet_workspace_bytes(p->unet, n, h, w, tokens, &bytes);
    if (!rc) rc = nesr_vae_workspace_bytes(p->vae, h, w, &bytes);
    return rc;
}

// the windows of a tiled call, both plans resolved
struct Windows {
    int ty, tx, r;          // the denoising loop's
    int vty, vtx, vr;       // the VAE decode's
};

struct TiledPlan {
    size_t text, frame, acc, window, model, vae, total;
};

// the pipeline's own bytes of a tiled call: the text states, the full-frame buffer [lc + 3][hw], the accumulator [lc][hw], a
// window's UNet input and output, and the tiled decode's buffers (a window's latents and sample, the f32 frame)
TiledPlan tiled_plan(int n, int lc, int hidden, int scale, int h, int w, int tokens, const Windows& wd) {
    TiledPlan pl;
    ScratchCarver ws;
    const size_t hw = (size_t)h * w, win = (size_t)wd.ty * wd.tx;
    pl.text = ws.take((size_t)n * tokens * hidden * 4);
    pl.frame = ws.take((lc + SDX4_IMAGE_CHANNELS) * hw * 4);
    pl.acc = ws.take(lc * hw * 4);
    pl.window = ws.take((size_t)n * (lc + SDX4_IMAGE_CHANNELS) * win * 4);
    pl.model = ws.take((size_t)n * lc * win * 4);
    pl.vae = ws.take(sdx4_vae_tiled_plan(lc, scale, h, w, wd.vty, wd.vtx).total);
    pl.total = ws.total();
    return pl;
}

// the frame and both window plans; vae_tile 0 and vae_overlap < 0 stand for tile and tile_overlap
int check_windows(const char* entry, int h, int w, int multiple, int tile, int tile_overlap, int vae_tile, int vae_overlap, Windows& wd) {
    const std::string e = entry;
    if (multiple < 2 || multiple % 2) return set_error(NESR_ERR_ARG, e + ": the frame multiple must be even (a UNet of at least two levels), got " + std::to_string(multiple));
    if (h < 1 || w < 1 || h % multiple || w % multiple)
        return set_error(NESR_ERR_ARG, e + ": h and w must be positive multiples of " + std::to_string(multiple) + " (2^(UNet levels - 1)), got " + std::to_string(h) + " x " + std::to_string(w));
    if ((long long)h * w > SDX4_MAX_FRAME_PIXELS)
        return set_error(NESR_ERR_ARG, e + ": a frame of " + std::to_string(h) + " x " + std::to_string(w) + " exceeds 2^22 low-res pixels");
    int rc = sdx4_check_windows(entry, "tile", h, w, multiple, tile, tile_overlap, &wd.ty, &wd.tx);
    if (rc) return rc;
    wd.r = tile_overlap;
    wd.vr = vae_overlap < 0 ? tile_overlap : vae_overlap;
    return sdx4_check_windows(entry, "vae_tile", h, w, multiple, vae_tile == 0 ? tile : vae_tile, wd.vr, &wd.vty, &wd.vtx);
}

}  // namespace

extern "C" {

int nesr_sdx4_tile_plan(int h, int w, int multiple, int tile, int tile_overlap, int* tiles_y, int* tiles_x, int* ty, int* tx, int32_t* plan, size_t capacity) {
    const char* e = "nesr_sdx4_tile_plan";
    if (!tiles_y || !tiles_x || !ty || !tx) return set_error(NESR_ERR_ARG, "nesr_sdx4_tile_plan: null pointer");
    Windows wd;
    const int rc = check_windows(e, h, w, multiple, tile, tile_overlap, 0, -1, wd);
    if (rc) return rc;
    const int ky = sdx4_axis_windows(h, wd.ty, wd.r), kx = sdx4_axis_windows(w, wd.tx, wd.r);
    *tiles_y = ky, *tiles_x = kx, *ty = wd.ty, *tx = wd.tx;
    if (!plan) return NESR_OK;
    const size_t need = (size_t)2 * ky * kx;
    if (capacity < need) return set_error(NESR_ERR_ARG, "nesr_sdx4_tile_plan: the plan needs " + std::to_string(need) + " integers, capacity is " + std::to_string(capacity));
    for (int iy = 0; iy < ky; ++iy)
        for (int ix = 0; ix < kx; ++ix) {
            plan[2 * (iy * kx + ix)] = sdx4_axis_origin(h, wd.ty, wd.r, iy);
            plan[2 * (iy * kx + ix) + 1] = sdx4_axis_origin(w, wd.tx, wd.r, ix);
        }
    return NESR_OK;
}

int nesr_sdx4_tiled_workspace_bytes(int n, int latent_channels, int text_hidden, int vae_scale, int h, int w, int tokens, int multiple, int tile, int tile_overlap, int vae_tile,
                                    int vae_overlap, size_t* bytes) {
    const char* e = "nesr_sdx4_tiled_workspace_bytes";
    if (!bytes) return set_error(NESR_ERR_ARG, "nesr_sdx4_tiled_workspace_bytes: null pointer");
    if (n < 1 || n > 2 || latent_channels < 1 || latent_channels > SDX4_MAX_LATENT_CHANNELS || text_hidden < 1 || tokens < 1 || vae_scale < 2 || vae_scale > 8 || vae_scale % 2)
        return set_error(NESR_ERR_ARG, "nesr_sdx4_tiled_workspace_bytes: n 1 or 2, latent_channels 1 .. 8, text_hidden and tokens positive, vae_scale 2, 4 or 8");
    Windows wd;
    const int rc = check_windows(e, h, w, multiple, tile, tile_overlap, vae_tile, vae_overlap, wd);
    if (rc) return rc;
    *bytes = tiled_plan(n, latent_channels, text_hidden, vae_scale, h, w, tokens, wd).total;
    return NESR_OK;
}

int nesr_sdx4_schedule(int num_train_timesteps, double beta_start, double beta_end, const char* beta_schedule, const char* prediction_type, int set_alpha_to_one,
                       int steps_offset, const char* timestep_spacing, int steps, int* timesteps, double* alpha_bars, float* coefficients) {
    const char* e = "nesr_sdx4_schedule";
    Ddim d;
    int rc = make_ddim(e, d, num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, set_alpha_to_one, steps_offset, timestep_spacing);
    if (!rc) rc = check_steps(e, d, steps);
    if (rc) return rc;
    for (int i = 0; i < steps; ++i) {
        int t;
        double a, pv;
        float coef[6];
        ddim_step(d, steps, i, t, a, pv, coef);
        if (timesteps) timesteps[i] = t;
        if (alpha_bars) alpha_bars[2 * i] = a, alpha_bars[2 * i + 1] = pv;
        if (coefficients) std::copy(coef, coef + 6, coefficients + 6 * i);
    }
    return NESR_OK;
}

int nesr_sdx4_noise_coefficients(int num_train_timesteps, const char* beta_schedule, int noise_level, double* alpha_bar, float* coefficients) {
    const char* e = "nesr_sdx4_noise_coefficients";
    std::vector<double> abar;
    const int rc = make_low_res(e, abar, num_train_timesteps, beta_schedule);
    if (rc) return rc;
    if (noise_level < 0 || noise_level >= num_train_timesteps)
        return set_error(NESR_ERR_ARG, std::string(e) + ": noise_level must be 0 .. " + std::to_string(num_train_timesteps - 1) + ", got " + std::to_string(noise_level));
    if (alpha_bar) *alpha_bar = abar[noise_level];
    if (coefficients) coefficients[0] = (float)std::sqrt(abar[noise_level]), coefficients[1] = (float)std::sqrt(1.0 - abar[noise_level]);
    return NESR_OK;
}

int nesr_sdx4_create(nesr_sdx4** out, nesr_clip_text* text, nesr_unet* unet, nesr_vae* vae, int num_train_timesteps, double beta_start, double beta_end,
                     const char* beta_schedule, const char* prediction_type, int clip_sample, int set_alpha_to_one, int steps_offset, const char* timestep_spacing,
                     double eta, int low_res_num_train_timesteps, const char* low_res_beta_schedule, int max_noise_level) {
    const char* e = "nesr_sdx4_create";
    if (!out) return set_error(NESR_ERR_ARG, "nesr_sdx4_create: null out");
    *out = nullptr;
    if (!text || !unet || !vae) return set_error(NESR_ERR_ARG, "nesr_sdx4_create: null context");
    if (clip_sample) return unsupported(e, "clip_sample", "true is not supported");
    if (eta != 0.0) return unsupported(e, "eta", "0 only (the deterministic DDIM step), got " + std::to_string(eta));
    Ddim d;
    std::vector<double> low;
    int rc = make_ddim(e, d, num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, set_alpha_to_one, steps_offset, timestep_spacing);
    if (!rc) rc = make_low_res(e, low, low_res_num_train_timesteps, low_res_beta_schedule);
    if (rc) return rc;
    if (max_noise_level < 0 || max_noise_level >= low_res_num_train_timesteps)
        return unsupported(e, "max_noise_level", "0 .. " + std::to_string(low_res_num_train_timesteps - 1) + " (the low-res scheduler's table), got " + std::to_string(max_noise_level));
    const Sdx4TextInfo ti = sdx4_text_info(text);
    const Sdx4UnetInfo ui = sdx4_unet_info(unet);
    const Sdx4VaeInfo vi = sdx4_vae_info(vae);
    if (ui.cin != vi.latent + SDX4_IMAGE_CHANNELS)
        return set_error(NESR_ERR_ARG, "nesr_sdx4_create: the UNet's in_channels " + std::to_string(ui.cin) + " is not the VAE's latent_channels " + std::to_string(vi.latent) + " + 3");
    if (ui.cout != vi.latent)
        return set_error(NESR_ERR_ARG, "nesr_sdx4_create: the UNet's out_channels " + std::to_string(ui.cout) + " is not the VAE's latent_channels " + std::to_string(vi.latent));
    if (ui.cross != ti.hidden)
        return set_error(NESR_ERR_ARG, "nesr_sdx4_create: the UNet's cross_attention_dim " + std::to_string(ui.cross) + " is not the text encoder's hidden_size " + std::to_string(ti.hidden));
    if (ui.classes <= max_noise_level)
        return set_error(NESR_ERR_ARG, "nesr_sdx4_create: the UNet's class table of " + std::to_string(ui.classes) + " (num_class_embeds) does not reach max_noise_level " +
                                           std::to_string(max_noise_level));
    if (vi.cout != 3) return set_error(NESR_ERR_ARG, "nesr_sdx4_create: the VAE's out_channels must be 3 (an RGB frame), got " + std::to_string(vi.cout));
    if (ti.device != ui.device || ui.device != vi.device)
        return set_error(NESR_ERR_ARG, "nesr_sdx4_create: the three contexts are on devices " + std::to_string(ti.device) + ", " + std::to_string(ui.device) + " and " +
                                           std::to_string(vi.device) + "; they must share one");
    if (ui.device < 0) return set_error(NESR_ERR_STATE, "nesr_sdx4_create: contexts without a device launch nothing");
    nesr_sdx4* p = new nesr_sdx4();
    p->text = text, p->unet = unet, p->vae = vae, p->device = ui.device, p->lc = vi.latent, p->levels = ui.levels, p->scale = 1 << (vi.blocks - 1);
    p->max_noise_level = max_noise_level, p->ddim = d, p->low_abar = low;
    *out = p;
    return NESR_OK;
}

void nesr_sdx4_destroy(nesr_sdx4* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    p->timer.destroy();
    if (p->ws_buf) (void)hipFree(p->ws_buf);
    delete p;
}

int nesr_sdx4_workspace_bytes(nesr_sdx4* p, int n, int h, int w, int tokens, size_t* bytes) {
    if (!p || !bytes) return set_error(NESR_ERR_ARG, "nesr_sdx4_workspace_bytes: null pointer");
    const int rc = check_call(p, "nesr_sdx4_workspace_bytes", n, h, w, tokens);
    if (rc) return rc;
    *bytes = plan(p, n, h, w, tokens).total;
    return NESR_OK;
}

int nesr_sdx4_upscale_u8(nesr_sdx4* p, const uint8_t* frame_dev, int h, int w, const int32_t* ids_host, int tokens, const float* noise_dev, const float* latents_dev,
                         int noise_level, int steps, double guidance_scale, uint8_t* out_dev, size_t capacity, float* latents_out_dev, void* stream) {
    const std::string e = "nesr_sdx4_upscale_u8";
    if (!p || !frame_dev || !ids_host || !noise_dev || !latents_dev || !out_dev) return set_error(NESR_ERR_ARG, e + ": null pointer");
    if (!std::isfinite(guidance_scale)) return set_error(NESR_ERR_ARG, e + ": guidance_scale must be finite");
    const int n = guidance_scale > 1.0 ? 2 : 1;      // [negative, prompt], or the prompt alone
    int rc = check_call(p, e.c_str(), n, h, w, tokens);
    if (rc) return rc;
    if (noise_level < 0 || noise_level > p->max_noise_level)
        return set_error(NESR_ERR_ARG, e + ": noise_level must be 0 .. " + std::to_string(p->max_noise_level) + " (max_noise_level), got " + std::to_string(noise_level));
    if ((rc = check_steps(e.c_str(), p->ddim, steps))) return rc;
    const Sdx4TextInfo ti = sdx4_text_info(p->text);
    if (!ti.finalized || !sdx4_unet_info(p->unet).finalized || !sdx4_vae_info(p->vae).finalized) return set_error(NESR_ERR_STATE, e + ": a context's weights are not finalized");
    for (int i = 0; i < n * tokens; ++i)
        if (ids_host[i] < 0 || ids_host[i] >= ti.vocab)
            return set_error(NESR_ERR_ARG, e + ": id " + std::to_string(ids_host[i]) + " at position " + std::to_string(i % tokens) + " of sample " + std::to_string(i / tokens) +
                                               " is outside the table of " + std::to_string(ti.vocab) + " (vocab_size)");
    const size_t need = (size_t)3 * h * p->scale * w * p->scale;
    if (capacity < need) return set_error(NESR_ERR_ARG, e + ": the output needs " + std::to_string(need) + " bytes, capacity is " + std::to_string(capacity));
    for (const void* ptr : {(const void*)noise_dev, (const void*)latents_dev, (const void*)latents_out_dev})
        if (reinterpret_cast<uintptr_t>(ptr) & 15) return set_error(NESR_ERR_ARG, e + ": the noise and latents pointers must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(frame_dev) & 3) return set_error(NESR_ERR_ARG, e + ": the frame pointer must be 4-byte aligned");
    NESR_TRY(hipSetDevice(p->device));
    const Plan pl = plan(p, n, h, w, tokens);
    if ((rc = grow(p->ws_buf, p->ws_bytes, pl.total, kName))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* text = reinterpret_cast<float*>(p->ws_buf + pl.text);
    float* sample = reinterpret_cast<float*>(p->ws_buf + pl.sample);
    float* model = reinterpret_cast<float*>(p->ws_buf + pl.model);
    float* latents = reinterpret_cast<float*>(p->ws_buf + pl.latents);
    const int hw = h * w, cin = p->lc + SDX4_IMAGE_CHANNELS;
    const int64_t before = p->timer.launches + ti.launches + sdx4_unet_info(p->unet).launches + sdx4_vae_info(p->vae).launches;

    if ((rc = nesr_clip_text_encode_f32(p->text, ids_host, n, tokens, text, (size_t)n * tokens * ti.hidden, stream))) return rc;
    // An fp16 UNet's range word is cleared once here and read once behind the last launch: the steps' forwards neither clear it nor
    // wait, so the call still has no synchronisation inside.  With an f32 UNet both calls do nothing.
    if ((rc = unet_range_begin(p->unet, s))) return rc;
    {
        Sdx4Prepare a;
        memset(&a, 0, sizeof(a));
        const double ab = p->low_abar[noise_level];
        a.frame = frame_dev, a.noise = noise_dev, a.latents = latents_dev, a.n = n, a.hw = hw, a.lc = p->lc;
        a.sa = (float)std::sqrt(ab), a.sb = (float)std::sqrt(1.0 - ab), a.sigma = 1.0f;      // DDIM's init_noise_sigma
        a.sample = sample, a.lat_out = latents;
        NESR_RUN(p->timer, kName, NESR_SDX4_GROUP_PREPARE, s, [&] { return launch_sdx4_prepare(a, s); });
    }
    for (int i = 0; i < steps; ++i) {
        int t;
        double ab, pv;
        float coef[6];
        ddim_step(p->ddim, steps, i, t, ab, pv, coef);
        // scale_model_input is the identity; the noise level is the class label
        if ((rc = unet_forward_unchecked(p->unet, sample, n, cin, h, w, (double)t, noise_level, text, tokens, model, (size_t)n * p->lc * hw, s))) return rc;
        Sdx4Step a;
        memset(&a, 0, sizeof(a));
        a.model = model, a.latents = latents, a.n = n, a.hw = hw, a.lc = p->lc, a.g = (float)guidance_scale;
        a.c0x = coef[0], a.c0m = coef[1], a.cex = coef[2], a.cem = coef[3], a.sp = coef[4], a.sq = coef[5];
        a.lat_out = latents, a.sample = sample;
        NESR_RUN(p->timer, kName, NESR_SDX4_GROUP_STEP, s, [&] { return launch_sdx4_step(a, s); });
    }
    if ((rc = nesr_vae_decode_latents_u8(p->vae, latents, 1, p->lc, h, w, out_dev, capacity, stream))) return rc;
    if (latents_out_dev) NESR_TRY(hipMemcpyAsync(latents_out_dev, latents, (size_t)p->lc * hw * 4, hipMemcpyDeviceToDevice, s));      // for the tests; after the last launch
    p->last_launches = p->timer.launches + sdx4_text_info(p->text).launches + sdx4_unet_info(p->unet).launches + sdx4_vae_info(p->vae).launches - before;
    return unet_range_end(p->unet, s, "nesr_sdx4_upscale_u8");
}

int nesr_sdx4_upscale_tiled_u8(nesr_sdx4* p, const uint8_t* frame_dev, int h, int w, const int32_t* ids_host, int tokens, const float* noise_dev, const float* latents_dev,
                               int noise_level, int steps, double guidance_scale, int tile, int tile_overlap, int vae_tile, int vae_overlap, uint8_t* out_dev, size_t capacity,
                               float* latents_out_dev, void* stream) {
    const std::string e = "nesr_sdx4_upscale_tiled_u8";
    if (!p || !frame_dev || !ids_host || !noise_dev || !latents_dev || !out_dev) return set_error(NESR_ERR_ARG, e + ": null pointer");
    if (!std::isfinite(guidance_scale)) return set_error(NESR_ERR_ARG, e + ": guidance_scale must be finite");
    const int n = guidance_scale > 1.0 ? 2 : 1;      // [negative, prompt], or the prompt alone
    Windows wd;
    int rc = check_windows(e.c_str(), h, w, 1 << (p->levels - 1), tile, tile_overlap, vae_tile, vae_overlap, wd);
    if (rc) return rc;
    {   // the three contexts' own rules, on the shapes they will see
        size_t bytes = 0;
        rc = nesr_clip_text_workspace_bytes(p->text, n, tokens, &bytes);
        if (!rc) rc = nesr_unet_workspace_bytes(p->unet, n, wd.ty, wd.tx, tokens, &bytes);
        if (!rc) rc = nesr_vae_workspace_bytes(p->vae, wd.vty, wd.vtx, &bytes);
        if (rc) return rc;
    }
    if (noise_level < 0 || noise_level > p->max_noise_level)
        return set_error(NESR_ERR_ARG, e + ": noise_level must be 0 .. " + std::to_string(p->max_noise_level) + " (max_noise_level), got " + std::to_string(noise_level));
    if ((rc = check_steps(e.c_str(), p->ddim, steps))) return rc;
    const Sdx4TextInfo ti = sdx4_text_info(p->text);
    if (!ti.finalized || !sdx4_unet_info(p->unet).finalized || !sdx4_vae_info(p->vae).finalized) return set_error(NESR_ERR_STATE, e + ": a context's weights are not finalized");
    for (int i = 0; i < n * tokens; ++i)
        if (ids_host[i] < 0 || ids_host[i] >= ti.vocab)
            return set_error(NESR_ERR_ARG, e + ": id " + std::to_string(ids_host[i]) + " at position " + std::to_string(i % tokens) + " of sample " + std::to_string(i / tokens) +
                                               " is outside the table of " + std::to_string(ti.vocab) + " (vocab_size)");
    const size_t need = (size_t)3 * h * p->scale * w * p->scale;
    if (capacity < need) return set_error(NESR_ERR_ARG, e + ": the output needs " + std::to_string(need) + " bytes, capacity is " + std::to_string(capacity));
    for (const void* ptr : {(const void*)noise_dev, (const void*)latents_dev, (const void*)latents_out_dev})
        if (reinterpret_cast<uintptr_t>(ptr) & 15) return set_error(NESR_ERR_ARG, e + ": the noise and latents pointers must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(frame_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3)) return set_error(NESR_ERR_ARG, e + ": the frame and output pointers must be 4-byte aligned");
    NESR_TRY(hipSetDevice(p->device));
    const TiledPlan pl = tiled_plan(n, p->lc, ti.hidden, p->scale, h, w, tokens, wd);
    if ((rc = grow(p->ws_buf, p->ws_bytes, pl.total, kName))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* text = reinterpret_cast<float*>(p->ws_buf + pl.text);
    float* frame = reinterpret_cast<float*>(p->ws_buf + pl.frame);
    float* acc = reinterpret_cast<float*>(p->ws_buf + pl.acc);
    float* window = reinterpret_cast<float*>(p->ws_buf + pl.window);
    float* model = reinterpret_cast<float*>(p->ws_buf + pl.model);
    const int hw = h * w, cin = p->lc + SDX4_IMAGE_CHANNELS;
    const int ky = sdx4_axis_windows(h, wd.ty, wd.r), kx = sdx4_axis_windows(w, wd.tx, wd.r);
    const int64_t before = p->timer.launches + ti.launches + sdx4_unet_info(p->unet).launches + sdx4_vae_info(p->vae).launches;

    if ((rc = nesr_clip_text_encode_f32(p->text, ids_host, n, tokens, text, (size_t)n * tokens * ti.hidden, stream))) return rc;
    if ((rc = unet_range_begin(p->unet, s))) return rc;      // as in nesr_sdx4_upscale_u8: one bracket around every window's forward
    {   // the full-frame buffer is sdx4_prepare_kernel's sample with n = 1; its second copy of the latents lands in the accumulator,
        // which is cleared behind it and then kept zero by the step kernel
        Sdx4Prepare a;
        memset(&a, 0, sizeof(a));
        const double ab = p->low_abar[noise_level];
        a.frame = frame_dev, a.noise = noise_dev, a.latents = latents_dev, a.n = 1, a.hw = hw, a.lc = p->lc;
        a.sa = (float)std::sqrt(ab), a.sb = (float)std::sqrt(1.0 - ab), a.sigma = 1.0f;
        a.sample = frame, a.lat_out = acc;
        NESR_RUN(p->timer, kName, NESR_SDX4_GROUP_PREPARE, s, [&] { return launch_sdx4_prepare(a, s); });
        NESR_TRY(hipMemsetAsync(acc, 0, (size_t)p->lc * hw * 4, s));
    }
    for (int i = 0; i < steps; ++i) {
        int t;
        double ab, pv;
        float coef[6];
        ddim_step(p->ddim, steps, i, t, ab, pv, coef);
        for (int iy = 0; iy < ky; ++iy)
            for (int ix = 0; ix < kx; ++ix) {
                const Sdx4Axis ay = sdx4_axis(h, wd.ty, wd.r, sdx4_axis_origin(h, wd.ty, wd.r, iy)), ax = sdx4_axis(w, wd.tx, wd.r, sdx4_axis_origin(w, wd.tx, wd.r, ix));
                Sdx4Gather g;
                memset(&g, 0, sizeof(g));
                g.src = frame, g.n = n, g.channels = cin, g.y = ay, g.x = ax, g.dst = window;
                NESR_RUN(p->timer, kName, NESR_SDX4_GROUP_GATHER, s, [&] { return launch_sdx4_gather(g, s); });
                if ((rc = unet_forward_unchecked(p->unet, window, n, cin, wd.ty, wd.tx, (double)t, noise_level, text, tokens, model, (size_t)n * p->lc * wd.ty * wd.tx, s))) return rc;
                Sdx4Accumulate a;
                memset(&a, 0, sizeof(a));
                a.model = model, a.n = n, a.lc = p->lc, a.y = ay, a.x = ax, a.g = (float)guidance_scale, a.acc = acc;
                NESR_RUN(p->timer, kName, NESR_SDX4_GROUP_ACCUMULATE, s, [&] { return launch_sdx4_accumulate(a, s); });
            }
        Sdx4TiledStep a;
        memset(&a, 0, sizeof(a));
        a.acc = acc, a.frame = frame, a.lc = p->lc, a.y = sdx4_axis(h, wd.ty, wd.r, 0), a.x = sdx4_axis(w, wd.tx, wd.r, 0);
        a.c0x = coef[0], a.c0m = coef[1], a.cex = coef[2], a.cem = coef[3], a.sp = coef[4], a.sq = coef[5];
        NESR_RUN(p->timer, kName, NESR_SDX4_GROUP_TILED_STEP, s, [&] { return launch_sdx4_tiled_step(a, s); });
    }
    // the final latents are channels 0 .. lc - 1 of the full-frame buffer
    if ((rc = sdx4_vae_decode_tiled(p->vae, frame, h, w, wd.vty, wd.vtx, wd.vr, p->ws_buf + pl.vae, out_dev, &p->timer, kName,
                                    Sdx4TileGroups{NESR_SDX4_GROUP_GATHER, NESR_SDX4_GROUP_BLEND_ADD, NESR_SDX4_GROUP_BLEND_FINISH}, s)))
        return rc;
    if (latents_out_dev) NESR_TRY(hipMemcpyAsync(latents_out_dev, frame, (size_t)p->lc * hw * 4, hipMemcpyDeviceToDevice, s));      // for the tests; after the last launch
    p->last_launches = p->timer.launches + sdx4_text_info(p->text).launches + sdx4_unet_info(p->unet).launches + sdx4_vae_info(p->vae).launches - before;
    return unet_range_end(p->unet, s, "nesr_sdx4_upscale_tiled_u8");
}

int nesr_sdx4_launches(const nesr_sdx4* p, int64_t* launches) {
    if (!p || !launches) return set_error(NESR_ERR_ARG, "nesr_sdx4_launches: null pointer");
    *launches = p->last_launches;
    return NESR_OK;
}

int nesr_sdx4_set_timing(nesr_sdx4* p, int enable) {
    if (!p) return set_error(NESR_ERR_ARG, "nesr_sdx4_set_timing: null context");
    p->timer.on = enable != 0;
    return NESR_OK;
}

int nesr_sdx4_kernel_time_ms(nesr_sdx4* p, double* group_ms, int n_groups, int64_t* launches) {
    if (!p) return set_error(NESR_ERR_ARG, "nesr_sdx4_kernel_time_ms: null context");
    NESR_TRY(hipSetDevice(p->device));
    double ms[NESR_SDX4_GROUPS];
    const int rc = p->timer.collect(ms, NESR_SDX4_GROUPS, launches);
    for (int i = 0; !rc && group_ms && i < n_groups && i < NESR_SDX4_GROUPS; ++i) group_ms[i] = ms[i];
    return rc;
}

// ---- single-launch test hooks: device pointers in, the launcher's struct filled field for field, one launch, no context
int nesr_sdx4_k_prepare(const uint8_t* frame_dev, const float* noise_dev, const float* latents_dev, int n, int hw, int lc, float sa, float sb, float sigma,
                        float* sample_dev, float* latents_out_dev, void* stream) {
    Sdx4Prepare a;
    memset(&a, 0, sizeof(a));
    a.frame = frame_dev, a.noise = noise_dev, a.latents = latents_dev, a.n = n, a.hw = hw, a.lc = lc, a.sa = sa, a.sb = sb, a.sigma = sigma;
    a.sample = sample_dev, a.lat_out = latents_out_dev;
    return launch_done(launch_sdx4_prepare(a, (hipStream_t)stream), "csrc/sdx4_api.h", "nesr_sdx4_k_prepare", "launch_sdx4_prepare");
}

int nesr_sdx4_k_step(const float* model_dev, const float* latents_dev, int n, int hw, int lc, float guidance, const float* coefficients, float* latents_out_dev,
                     float* sample_dev, void* stream) {
    if (!coefficients) return set_error(NESR_ERR_ARG, "nesr_sdx4_k_step: six coefficients (c0x, c0m, cex, cem, sp, sq) on the host; nothing was launched");
    Sdx4Step a;
    memset(&a, 0, sizeof(a));
    a.model = model_dev, a.latents = latents_dev, a.n = n, a.hw = hw, a.lc = lc, a.g = guidance;
    a.c0x = coefficients[0], a.c0m = coefficients[1], a.cex = coefficients[2], a.cem = coefficients[3], a.sp = coefficients[4], a.sq = coefficients[5];
    a.lat_out = latents_out_dev, a.sample = sample_dev;
    return launch_done(launch_sdx4_step(a, (hipStream_t)stream), "csrc/sdx4_api.h", "nesr_sdx4_k_step", "launch_sdx4_step");
}

// the window kernels (sdx4_tiled.hip): an axis is four integers (n, t, r, a) on the host, y first
namespace {
Sdx4Axis axis_of(const int* v) { return Sdx4Axis{v[0], v[1], v[2], v[3]}; }
const char* const kAxes = ": the axes are two rows of (n, t, r, a) on the host; nothing was launched";
}  // namespace

int nesr_sdx4_k_window_gather(const float* src_dev, int n, int channels, const int* axes, float* dst_dev, void* stream) {
    if (!axes) return set_error(NESR_ERR_ARG, std::string("nesr_sdx4_k_window_gather") + kAxes);
    Sdx4Gather a;
    memset(&a, 0, sizeof(a));
    a.src = src_dev, a.n = n, a.channels = channels, a.y = axis_of(axes), a.x = axis_of(axes + 4), a.dst = dst_dev;
    return launch_done(launch_sdx4_gather(a, (hipStream_t)stream), "csrc/sdx4_api.h", "nesr_sdx4_k_window_gather", "launch_sdx4_gather");
}

int nesr_sdx4_k_accumulate(const float* model_dev, int n, int lc, const int* axes, float guidance, float* acc_dev, void* stream) {
    if (!axes) return set_error(NESR_ERR_ARG, std::string("nesr_sdx4_k_accumulate") + kAxes);
    Sdx4Accumulate a;
    memset(&a, 0, sizeof(a));
    a.model = model_dev, a.n = n, a.lc = lc, a.y = axis_of(axes), a.x = axis_of(axes + 4), a.g = guidance, a.acc = acc_dev;
    return launch_done(launch_sdx4_accumulate(a, (hipStream_t)stream), "csrc/sdx4_api.h", "nesr_sdx4_k_accumulate", "launch_sdx4_accumulate");
}

int nesr_sdx4_k_tiled_step(float* acc_dev, float* frame_dev, int lc, const int* axes, const float* coefficients, void* stream) {
    if (!axes || !coefficients) return set_error(NESR_ERR_ARG, std::string("nesr_sdx4_k_tiled_step") + kAxes);
    Sdx4TiledStep a;
    memset(&a, 0, sizeof(a));
    a.acc = acc_dev, a.frame = frame_dev, a.lc = lc, a.y = axis_of(axes), a.x = axis_of(axes + 4);
    a.c0x = coefficients[0], a.c0m = coefficients[1], a.cex = coefficients[2], a.cem = coefficients[3], a.sp = coefficients[4], a.sq = coefficients[5];
    return launch_done(launch_sdx4_tiled_step(a, (hipStream_t)stream), "csrc/sdx4_api.h", "nesr_sdx4_k_tiled_step", "launch_sdx4_tiled_step");
}

int nesr_sdx4_k_blend_add(const float* sample_dev, const int* axes, float* acc_dev, void* stream) {
    if (!axes) return set_error(NESR_ERR_ARG, std::string("nesr_sdx4_k_blend_add") + kAxes);
    Sdx4BlendAdd a;
    memset(&a, 0, sizeof(a));
    a.sample = sample_dev, a.y = axis_of(axes), a.x = axis_of(axes + 4), a.acc = acc_dev;
    return launch_done(launch_sdx4_blend_add(a, (hipStream_t)stream), "csrc/sdx4_api.h", "nesr_sdx4_k_blend_add", "launch_sdx4_blend_add");
}

int nesr_sdx4_k_blend_finish(const float* acc_dev, const int* axes, uint8_t* out_dev, void* stream) {
    if (!axes) return set_error(NESR_ERR_ARG, std::string("nesr_sdx4_k_blend_finish") + kAxes);
    Sdx4BlendFinish a;
    memset(&a, 0, sizeof(a));
    a.acc = acc_dev, a.y = axis_of(axes), a.x = axis_of(axes + 4), a.out = out_dev;
    return launch_done(launch_sdx4_blend_finish(a, (hipStream_t)stream), "csrc/sdx4_api.h", "nesr_sdx4_k_blend_finish", "launch_sdx4_blend_finish");
}

}  // extern "C"
