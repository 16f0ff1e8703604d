"""A float64 restatement of the x4 diffusion pipeline's two schedulers and of its whole loop, composed from the three networks'
restatements (tests/clip_text_ref.py, tests/unet_ref.py, tests/vae_ref.py).  The specification of csrc/sdx4_step.hip and of the
chain csrc/sdx4_api.cpp makes.  diffusers is not installed and nothing may be fetched: every value below is recalled from the
library, not checked against it or against a file; tests/test_sdx4_host.py carries the checks that do not depend on this
transcription (the timestep tables, the closed-form identity of the step, the guidance at g = 1).

  DDIM scheduler   1000 train steps, beta 1e-4 .. 0.02 "scaled_linear" (linspace(sqrt b0, sqrt b1, T)^2), v_prediction, no clipping,
                   set_alpha_to_one false (the final alpha-bar is alpha-bar[0]), steps_offset 1, "leading" spacing, eta 0,
                   init_noise_sigma 1, scale_model_input the identity
  timesteps        (arange(N) (T // N))[::-1] + 1; the previous step of t is t - T // N, below 0 the final alpha-bar
  low-res          DDPMScheduler "squaredcos_cap_v2": beta_i = min(1 - f((i + 1) / T) / f(i / T), 0.999), f(s) = cos^2((s + 0.008) / 1.008 pi / 2);
                   add_noise(x, n, L) = sqrt(abar_L) x + sqrt(1 - abar_L) n; the noise level is also the UNet's class label
  guidance         batch order [negative, prompt]; m = m_neg + g (m_prompt - m_neg); g <= 1: the prompt alone

`fault` names one deliberate mistake (FAULTS).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import clip_text_ref as TR
from tests import unet_ref as UR
from tests import vae_ref as VR

DDIM = dict(num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="scaled_linear", prediction_type="v_prediction",
            clip_sample=False, set_alpha_to_one=False, steps_offset=1, timestep_spacing="leading")
LOW_RES = dict(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")

FAULTS = ("alpha_to_one", "no_steps_offset", "epsilon_for_v", "guidance_order_swapped", "image_not_noised", "image_scaled_by_255",
          "class_label_is_timestep", "latents_scaled_before_unet")


def ddim_alpha_bars(T=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="scaled_linear"):
    if beta_schedule == "scaled_linear":
        betas = np.linspace(math.sqrt(beta_start), math.sqrt(beta_end), T, dtype=np.float64) ** 2
    elif beta_schedule == "linear":
        betas = np.linspace(beta_start, beta_end, T, dtype=np.float64)
    else:
        raise ValueError(beta_schedule)
    return np.cumprod(1.0 - betas)


def timesteps(N, T=1000, steps_offset=1):
    return (np.arange(N) * (T // N))[::-1] + steps_offset


def low_res_alpha_bars(T=1000):
    f = lambda s: math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2
    betas = np.array([min(1.0 - f((i + 1) / T) / f(i / T), 0.999) for i in range(T)], dtype=np.float64)
    return np.cumprod(1.0 - betas)


def step_alphas(t, N, abar, T=1000, set_alpha_to_one=False):
    """(alpha-bar at t, alpha-bar at the previous step)."""
    prev = int(t) - T // N
    return float(abar[int(t)]), (float(abar[prev]) if prev >= 0 else (1.0 if set_alpha_to_one else float(abar[0])))


def ddim_step(x, m, a, p, prediction_type="v_prediction"):
    """x' of the eta = 0 step: sample x, model output m, alpha-bar a at the step and p at the previous one."""
    ra, rb = math.sqrt(a), math.sqrt(1.0 - a)
    if prediction_type == "v_prediction":
        x0, eps = ra * x - rb * m, ra * m + rb * x
    elif prediction_type == "epsilon":
        x0, eps = (x - rb * m) / ra, m
    else:
        raise ValueError(prediction_type)
    return math.sqrt(p) * x0 + math.sqrt(1.0 - p) * eps


def add_noise(x, noise, level, abar):
    return math.sqrt(abar[level]) * x + math.sqrt(1.0 - abar[level]) * noise


def guide(m, g, fault=None):
    """m [n, ...] in the order [negative, prompt] (n = 2) or the prompt alone."""
    if m.shape[0] == 1:
        return m[0]
    neg, pos = (m[1], m[0]) if fault == "guidance_order_swapped" else (m[0], m[1])
    return neg + g * (pos - neg)


def image_input(frame_u8, noise, level, abar, dtype, fault=None):
    """[3, h, w]: the frame as v / 127.5 - 1 with the low-res scheduler's noise."""
    v = frame_u8.to(dtype).permute(2, 0, 1)
    x = v / 255.0 if fault == "image_scaled_by_255" else v / 127.5 - 1.0
    return x if fault == "image_not_noised" else add_noise(x, noise.to(dtype), level, abar)


def loop(unet, frame_u8, text, noise, latents, noise_level, steps, guidance_scale, dtype=torch.float64, fault=None, model=None, scheduler=DDIM):
    """The denoising loop on the text states `text` [n, tokens, hidden] -> the final latents [1, lc, h, w] in `dtype`.  unet = (sd, cfg);
    `model` replaces the UNet (sample, t, text, label) -> [n, lc, h, w] for the checks that need a known model."""
    T = scheduler["num_train_timesteps"]
    abar = ddim_alpha_bars(T, scheduler["beta_start"], scheduler["beta_end"], scheduler["beta_schedule"])
    low = low_res_alpha_bars(LOW_RES["num_train_timesteps"])
    offset = 0 if fault == "no_steps_offset" else scheduler["steps_offset"]
    prediction = "epsilon" if fault == "epsilon_for_v" else scheduler["prediction_type"]
    n = text.shape[0]
    image = image_input(frame_u8, noise, noise_level, low, dtype, fault)
    x = latents.to(dtype).clone()                                    # init_noise_sigma = 1
    if model is None:
        sd, cfg = unet
        model = lambda sample, t, tx, label: UR.forward(sd, sample, t, tx, label, **cfg)
    for t in timesteps(steps, T, offset):
        a, p = step_alphas(t, steps, abar, T, scheduler["set_alpha_to_one"] or fault == "alpha_to_one")
        lat_in = x / math.sqrt(a) if fault == "latents_scaled_before_unet" else x      # scale_model_input is the identity
        sample = torch.cat([lat_in, image], dim=0)[None].expand(n, -1, -1, -1).contiguous()
        label = int(t) % 32 if fault == "class_label_is_timestep" else noise_level
        with torch.no_grad():
            m = model(sample, float(t), text.to(dtype), label)
        x = ddim_step(x, guide(m, guidance_scale, fault), a, p, prediction)
    return x[None]


def upscale(models, frame_u8, ids, noise, latents, noise_level, steps, guidance_scale, dtype=torch.float64, fault=None):
    """models = dict(text=(sd, cfg), unet=(sd, cfg), vae=(sd, cfg)); ids [n, tokens] in the order [negative, prompt] (n = 2 when
    guidance_scale > 1) -> (final latents [1, lc, h, w], the frame before the clamp [4h, 4w, 3]) in `dtype`."""
    tsd, tcfg = models["text"]
    with torch.no_grad():
        text = TR.forward(tsd, ids, dtype, **tcfg)
    final = loop(models["unet"], frame_u8, text, noise, latents, noise_level, steps, guidance_scale, dtype, fault)
    vsd, vcfg = models["vae"]
    return final, VR.decode_latents_float(vsd, final, dtype, **vcfg)
