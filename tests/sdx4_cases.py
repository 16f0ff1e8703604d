"""The crafted pipeline of the x4 diffusion tests: three seeded networks that fit each other and are small enough for a frame to run
in a moment, with a frame, ids, noise and latents.

  text encoder   hidden 32, 4 heads, intermediate 64, 2 layers, 50 ids, 77 positions
  UNet           two levels (32, 64), 8 groups, 2 heads, 1 layer a block, cross dim 32, 7 -> 4 channels, 32 class rows (so
                 max_noise_level is 31 here)
  VAE            widths (32, 32, 64): x4, 8 groups, 1 layer a block
  frame          16 x 24 -> 64 x 96, a smooth seeded image; 7 ids a prompt; 3 steps, noise level 5, guidance 7.5

The frame, the VAE's gain and the latents' size are chosen so that the float32 CPU restatement of the whole loop against float64
leaves few samples within 255 tol of a rounding boundary (tests/test_sdx4_host.py prints and caps the share at 2 %).
`reference(g)` computes the float64 loop once and shares it; the tolerance is 8 x max |float32 restatement - float64| of the final
latents and of the frame before the clamp, and is never written down.
"""
from __future__ import annotations

import torch

from tests import clip_text_ref as TR
from tests import sdx4_ref as R
from tests import unet_cases as UC
from tests import unet_ref as UR
from tests import vae_ref as VR

TEXT = dict(vocab_size=50, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=77, hidden_act="gelu")
UNET = UC.layout((32, 64), (True, True), (True, False), norm_num_groups=8, attention_head_dim=2, layers_per_block=1, cross_attention_dim=32)
UNET["num_class_embeds"] = 32
VAE = dict(block_out_channels=(32, 32, 64), norm_num_groups=8, layers_per_block=1)
MAX_NOISE_LEVEL = 31
H, W, TOKENS, STEPS, NOISE_LEVEL, GUIDANCE = 16, 24, 7, 3, 5, 7.5
MAX_THIN = 0.02                       # test_gpu_vae.py's cap on the share u8_check may leave out
BOS, EOS = 48, 49

_models, _refs = {}, {}


def models():
    """dict(text=(sd, cfg), unet=(sd, cfg), vae=(sd, cfg)), seeded."""
    if not _models:
        vsd = VR.seeded_state_dict(61, **VAE)
        for key in ("decoder.conv_out.weight", "decoder.conv_out.bias"):      # a gentle last conv: few samples on a rounding boundary's edge
            vsd[key] = (vsd[key] * 0.25).contiguous()
        _models.update(text=(TR.seeded_state_dict(62, **TEXT), TEXT), unet=(UR.seeded_state_dict(63, **UNET), UNET), vae=(vsd, VAE))
    return _models


def ids():
    """[2, 7]: [negative, prompt]; the negative prompt is the empty one."""
    return torch.tensor([[BOS] + [EOS] * (TOKENS - 1), [BOS, 11, 7, 11, 23, EOS, EOS]])


def frame(h=H, w=W, seed=64):
    """[h, w, 3] uint8: a smooth image with every channel's own gradient, plus a little seeded texture."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    planes = [96 + 64 * torch.sin(0.31 * x + 0.17 * y), 128 + 72 * torch.cos(0.23 * y - 0.11 * x), 40 + 6 * x + 3 * y]
    img = torch.stack(planes, dim=-1) + 6.0 * torch.randn((h, w, 3), generator=g)
    return img.round().clamp(0, 255).to(torch.uint8)


def draws(h=H, w=W, seed=65):
    """(noise [3, h, w], latents [4, h, w]) float32 unit normal, the image's noise first."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((3, h, w), generator=g), torch.randn((4, h, w), generator=g)


def reference(guidance=GUIDANCE):
    """(final latents f64 [1, 4, h, w], frame before the clamp f64 [4h, 4w, 3], tol of the latents, tol of the frame, the float32
    restatement's frame) for the crafted call at `guidance` (n = 2 above 1, else the prompt alone)."""
    if guidance not in _refs:
        noise, latents = draws()
        tok = ids() if guidance > 1.0 else ids()[1:]
        lat64, y64 = R.upscale(models(), frame(), tok, noise, latents, NOISE_LEVEL, STEPS, guidance, torch.float64)
        lat32, y32 = R.upscale(models(), frame(), tok, noise, latents, NOISE_LEVEL, STEPS, guidance, torch.float32)
        _refs[guidance] = (lat64, y64, 8.0 * float((lat32.double() - lat64).abs().max()), 8.0 * float((y32.double() - y64).abs().max()), y32)
    return _refs[guidance]
