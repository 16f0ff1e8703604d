"""A functional restatement of the decoder half of diffusers' AutoencoderKL as StableDiffusionUpscalePipeline uses it
("stabilityai/stable-diffusion-x4-upscaler"): plain torch ops on a state dict under diffusers' names, in whatever float dtype it
is handed (float64 for the reference).  The specification of csrc/vae.hip; diffusers is not a dependency of this project, so
tests/test_vae_host.py holds the restatement to a transcription built from torch's own modules (nn.GroupNorm, nn.Conv2d,
F.scaled_dot_product_attention) in float64.

What the network does and a guess would not:
  * every GroupNorm has eps 1e-6 (torch's default is 1e-5) and the biased variance;
  * a ResnetBlock's convs pad with zeros AFTER the norm and the SiLU: a tap outside the image is 0, not silu(beta - mean a);
  * conv_shortcut (1x1) exists only where a block changes the width, which is the first ResnetBlock of an up block;
  * the attention is one head of the full width, scaled by 1 / sqrt(C), softmax over the keys, added to the input from before
    the GroupNorm;
  * an upsampler is nearest x2 (out[y, x] = in[y // 2, x // 2]) and THEN a 3x3 conv;
  * the pipeline divides the latents by the scaling factor, and VaeImageProcessor computes clamp(y / 2 + 0.5, 0, 1), x 255 and
    numpy's round (half to even).

`fault` names one deliberate mistake (FAULTS); tests/test_vae_cases_host.py shows that every one of them fails a crafted case.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

DEFAULTS = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256, 512), layers_per_block=2, norm_num_groups=32,
                scaling_factor=0.08333, act_fn="silu")
EPS = 1e-6
STREAM_CHUNK = 32                    # keys of one chunk of the streamed attention (csrc/vae_api.h: VAE_ATTN_BK)
LEGACY_ATTENTION = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}
ATTENTION = "decoder.mid_block.attentions.0"

FAULTS = ("eps_1e-5", "variance_unbiased", "raw_moments_f32", "padding_normalised", "silu_before_norm", "no_shortcut_conv",
          "attention_no_residual", "scale_missing", "softmax_over_queries", "no_rescale_on_new_max", "upsample_offset",
          "upsample_after_conv", "scaling_multiplied", "post_quant_skipped", "shift_before_halving", "round_half_up")
FRAME_FAULTS = ("scaling_multiplied", "shift_before_halving")      # act around the decoder, in decode_latents_float
QUANTISER_FAULTS = ("round_half_up",)                               # acts in quantise


def config(**cfg):
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown:
        raise TypeError(f"unknown configuration field(s) {unknown}")
    c = dict(DEFAULTS)
    c.update(cfg)
    c["block_out_channels"] = tuple(c["block_out_channels"])
    return c


def spec(attention_names="current", **cfg):
    """Ordered {key: shape} of the decoder's part of AutoencoderKL(config).state_dict(): post_quant_conv and decoder.*."""
    c = config(**cfg)
    widths, lat, top = c["block_out_channels"], c["latent_channels"], c["block_out_channels"][-1]
    out = OrderedDict()

    def wb(name, wshape):
        out[name + ".weight"] = tuple(wshape)
        out[name + ".bias"] = (wshape[0],)

    def resnet(r, cin, cout):
        wb(r + ".norm1", (cin,))
        wb(r + ".conv1", (cout, cin, 3, 3))
        wb(r + ".norm2", (cout,))
        wb(r + ".conv2", (cout, cout, 3, 3))
        if cin != cout:
            wb(r + ".conv_shortcut", (cout, cin, 1, 1))

    wb("post_quant_conv", (lat, lat, 1, 1))
    wb("decoder.conv_in", (top, lat, 3, 3))
    resnet("decoder.mid_block.resnets.0", top, top)
    wb(ATTENTION + ".group_norm", (top,))
    for old, new in LEGACY_ATTENTION.items():
        wb(f"{ATTENTION}.{old if attention_names == 'legacy' else new}", (top, top))
    resnet("decoder.mid_block.resnets.1", top, top)
    prev = top
    for i, wd in enumerate(reversed(widths)):
        for j in range(c["layers_per_block"] + 1):
            resnet(f"decoder.up_blocks.{i}.resnets.{j}", prev if j == 0 else wd, wd)
        if i < len(widths) - 1:
            wb(f"decoder.up_blocks.{i}.upsamplers.0.conv", (wd, wd, 3, 3))
        prev = wd
    wb("decoder.conv_norm_out", (prev,))
    wb("decoder.conv_out", (c["out_channels"], prev, 3, 3))
    return out


def seeded_state_dict(seed, attention_names="current", **cfg):
    """Every tensor random (no GroupNorm gain of 1, no zero bias): float32, the same for a seed."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for key, shape in spec(attention_names, **cfg).items():
        r = torch.randn(shape, generator=g)
        if "norm" in key:
            t = 1.0 + 0.3 * r if key.endswith("weight") else 0.2 * r
        elif key.endswith("bias"):
            t = 0.2 * r
        else:
            t = r * (1.0 / math.sqrt(int(np.prod(shape[1:]))))
        sd[key] = t.float().contiguous()
    return sd


def seeded_latents(h, w, seed, channels=4, scaling_factor=0.08333):
    """Latents as the denoising loop leaves them: unit noise times the scaling factor."""
    return (torch.randn((1, channels, h, w), generator=torch.Generator().manual_seed(3000 + seed)) * scaling_factor).float()


# ------------------------------------------------------------------------------------------------ the pieces
def group_norm(x, groups, weight, bias, fault=None):
    """F.group_norm with eps 1e-6; the faults of its statistics are written out."""
    if fault == "eps_1e-5":
        return F.group_norm(x, groups, weight, bias, 1e-5)
    if fault not in ("variance_unbiased", "raw_moments_f32"):
        return F.group_norm(x, groups, weight, bias, EPS)
    n, c = x.shape[:2]
    xg = x.reshape(n, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    if fault == "variance_unbiased":
        var = xg.var(-1, unbiased=True, keepdim=True) if xg.shape[-1] > 1 else torch.zeros_like(mean)
    else:                                    # E[x^2] - E[x]^2 with every sum in float32
        x32 = xg.float()
        m32 = x32.mean(-1, keepdim=True)
        var = ((x32 * x32).mean(-1, keepdim=True) - m32 * m32).clamp_min(0).to(x.dtype)
        mean = m32.to(x.dtype)
    y = ((xg - mean) / torch.sqrt(var + EPS)).reshape(x.shape)
    shape = (1, c) + (1,) * (x.dim() - 2)
    return y * weight.view(shape) + bias.view(shape)


def norm_silu_conv(p, norm, conv, x, groups, fault=None):
    """conv(silu(GroupNorm(x))), 3x3 with zero padding of the activated tensor."""
    w, b = p[conv + ".weight"], p[conv + ".bias"]
    g, beta = p[norm + ".weight"], p[norm + ".bias"]
    if fault == "silu_before_norm":
        return F.conv2d(group_norm(F.silu(x), groups, g, beta, fault), w, b, padding=1)
    if fault == "padding_normalised":        # the border holds zeros BEFORE the norm: a tap outside becomes silu(beta - mean a)
        y = group_norm(x, groups, g, beta, fault)
        n, c, h, wd = x.shape
        xg = x.reshape(n, groups, -1)
        mean = xg.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(xg.var(-1, unbiased=False, keepdim=True) + EPS)
        outside = ((0 - mean) * rstd).expand(n, groups, c // groups).reshape(1, c, 1, 1) * g.view(1, c, 1, 1) + beta.view(1, c, 1, 1)
        padded = outside.expand(n, c, h + 2, wd + 2).clone()
        padded[:, :, 1:-1, 1:-1] = y
        return F.conv2d(F.silu(padded), w, b)
    return F.conv2d(F.silu(group_norm(x, groups, g, beta, fault)), w, b, padding=1)


def resnet(p, r, x, groups, fault=None):
    h = norm_silu_conv(p, r + ".norm1", r + ".conv1", x, groups, fault)
    h = norm_silu_conv(p, r + ".norm2", r + ".conv2", h, groups, fault)
    if r + ".conv_shortcut.weight" in p:
        if fault == "no_shortcut_conv":      # the input itself, cut or zero-filled to the new width
            cout, cin = h.shape[1], x.shape[1]
            x = x[:, :cout] if cin >= cout else F.pad(x, (0, 0, 0, 0, 0, cout - cin))
        else:
            x = F.conv2d(x, p[r + ".conv_shortcut.weight"], p[r + ".conv_shortcut.bias"])
    return x + h


def streamed_attention(q, k, v, scale, chunk=STREAM_CHUNK, rescale=True):
    """softmax(q k^T scale) v over key chunks with a running maximum and sum; rescale=False forgets to rescale the accumulator when
    the maximum moves (the sum is still rescaled), which is the fault no_rescale_on_new_max."""
    n = q.shape[0]
    m = torch.full((n, 1), -math.inf, dtype=q.dtype)
    l = torch.zeros((n, 1), dtype=q.dtype)
    o = torch.zeros_like(q)
    for k0 in range(0, k.shape[0], chunk):
        s = (q @ k[k0:k0 + chunk].t()) * scale
        m_new = torch.maximum(m, s.max(dim=1, keepdim=True).values)
        pr = torch.exp(s - m_new)
        alpha = torch.exp(m - m_new)
        l = l * alpha + pr.sum(dim=1, keepdim=True)
        o = (o * alpha if rescale else o) + pr @ v[k0:k0 + chunk]
        m = m_new
    return o / l


def attention(p, x, groups, fault=None, taps=None):
    a = ATTENTION
    n, c, h, w = x.shape
    t = group_norm(x, groups, p[a + ".group_norm.weight"], p[a + ".group_norm.bias"], fault).reshape(c, h * w).t()      # [h w, C]
    q = F.linear(t, p[a + ".to_q.weight"], p[a + ".to_q.bias"])
    k = F.linear(t, p[a + ".to_k.weight"], p[a + ".to_k.bias"])
    v = F.linear(t, p[a + ".to_v.weight"], p[a + ".to_v.bias"])
    s = q @ k.t() if fault == "scale_missing" else (q @ k.t()) / math.sqrt(c)
    if taps is not None:
        taps["tokens"], taps["scores"] = t, s
    if fault == "no_rescale_on_new_max":
        o = streamed_attention(q, k, v, 1.0 / math.sqrt(c), rescale=False)
    else:
        o = torch.softmax(s, dim=0 if fault == "softmax_over_queries" else 1) @ v
    o = F.linear(o, p[a + ".to_out.0.weight"], p[a + ".to_out.0.bias"]).t().reshape(1, c, h, w)
    return o if fault == "attention_no_residual" else x + o


def upsample(x, fault=None):
    if fault != "upsample_offset":
        return F.interpolate(x, scale_factor=2.0, mode="nearest")
    h, w = x.shape[2:]
    iy = ((torch.arange(2 * h) + 1) // 2).clamp(max=h - 1)
    ix = ((torch.arange(2 * w) + 1) // 2).clamp(max=w - 1)
    return x[:, :, iy][:, :, :, ix]


def current_names(sd):
    """The state dict with the attention's legacy names renamed and encoder.* / quant_conv.* dropped."""
    out = OrderedDict()
    for key, v in sd.items():
        if key.startswith(("encoder.", "quant_conv.")):
            continue
        if key.startswith(ATTENTION + "."):
            head, _, leaf = key[len(ATTENTION) + 1:].rpartition(".")
            key = f"{ATTENTION}.{LEGACY_ATTENTION.get(head, head)}.{leaf}"
        out[key] = v
    return out


def decode(sd, z, fault=None, taps=None, **cfg):
    """z [1, latent_channels, h, w] -> the sample [1, out_channels, h s, w s], in z's dtype."""
    c = config(**cfg)
    dt = z.dtype
    p = {k: v.to(dt) for k, v in current_names(sd).items()}
    groups, widths = c["norm_num_groups"], c["block_out_channels"]
    x = z if fault == "post_quant_skipped" else F.conv2d(z, p["post_quant_conv.weight"], p["post_quant_conv.bias"])
    x = F.conv2d(x, p["decoder.conv_in.weight"], p["decoder.conv_in.bias"], padding=1)
    x = resnet(p, "decoder.mid_block.resnets.0", x, groups, fault)
    x = attention(p, x, groups, fault, taps)
    x = resnet(p, "decoder.mid_block.resnets.1", x, groups, fault)
    for i in range(len(widths)):
        for j in range(c["layers_per_block"] + 1):
            x = resnet(p, f"decoder.up_blocks.{i}.resnets.{j}", x, groups, fault)
        if i < len(widths) - 1:
            up = f"decoder.up_blocks.{i}.upsamplers.0.conv"
            if fault == "upsample_after_conv":
                x = upsample(F.conv2d(x, p[up + ".weight"], p[up + ".bias"], padding=1))
            else:
                x = F.conv2d(upsample(x, fault), p[up + ".weight"], p[up + ".bias"], padding=1)
    return norm_silu_conv(p, "decoder.conv_norm_out", "decoder.conv_out", x, groups, fault)


# ------------------------------------------------------------------------------------------------ the frame-level route
def decode_latents_float(sd, latents, dtype=torch.float64, fault=None, **cfg):
    """What the pipeline computes before the clamp: decode(latents / scaling_factor) / 2 + 0.5 as [h s, w s, out_channels]."""
    sf = config(**cfg)["scaling_factor"]
    z = latents.to(dtype)
    z = z * sf if fault == "scaling_multiplied" else z / sf
    with torch.no_grad():
        y = decode(sd, z, None if fault in FRAME_FAULTS else fault, **cfg)
    y = (y + 0.5) / 2 if fault == "shift_before_halving" else y / 2 + 0.5
    return y[0].permute(1, 2, 0).contiguous()


def quantise(y, fault=None):
    """clamp to [0, 1], x 255, round half to even (numpy's round), uint8."""
    v = y.clamp(0, 1) * 255.0
    return (torch.floor(v + 0.5) if fault == "round_half_up" else v.round()).to(torch.uint8)
