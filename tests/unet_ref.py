"""A functional restatement of diffusers' UNet2DConditionModel.forward as StableDiffusionUpscalePipeline uses it
("stabilityai/stable-diffusion-x4-upscaler"): plain torch ops on a state dict under diffusers' names, in whatever float dtype it
is handed (float64 for the reference).  The specification of csrc/unet.hip; diffusers is not a dependency of this project and
nothing may be fetched, so the architecture is written out from memory and tests/test_unet_host.py holds it to a transcription
built from torch's own modules in float64.  No published checkpoint has been run through either.

What the network does and a guess would not:
  * the sinusoid is [cos | sin] (flip_sin_to_cos) with exponent i / half (freq_shift 0); the class row (the pipeline's noise
    level) is added to the time embedding; every ResnetBlock projects silu(emb) and adds it between conv1 and norm2;
  * a ResnetBlock's GroupNorm has eps 1e-5, a Transformer's GroupNorm 1e-6 and no activation; LayerNorm 1e-5;
  * attention_head_dim is the NUMBER of heads; a head is a contiguous block of columns, scaled by 1 / sqrt(its width);
  * attn1 reads the text states where only_cross_attention holds for the block, the normalised tokens otherwise;
  * the feed-forward is GEGLU: value half first, gate half second, erf GELU;
  * a downsampler is a stride-2 conv with zero padding 1 on ALL sides; an upsampler nearest x2 THEN a conv;
  * an up block's resnet reads cat(hidden, skip), hidden first, the skips popped last in first out.

`fault` names one deliberate mistake (FAULTS); tests/test_unet_cases_host.py shows that every one of them fails a crafted case.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

DEFAULTS = dict(in_channels=7, out_channels=4, block_out_channels=(256, 512, 512, 1024),
                down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", layers_per_block=2, attention_head_dim=8, cross_attention_dim=1024,
                only_cross_attention=(True, True, True, False), use_linear_projection=True, num_class_embeds=1000, norm_num_groups=32,
                norm_eps=1e-5, flip_sin_to_cos=True, freq_shift=0, downsample_padding=1, act_fn="silu", transformer_layers_per_block=1,
                dual_cross_attention=False)
TRANSFORMER_NORM_EPS = 1e-6
LAYER_NORM_EPS = 1e-5
STREAM_CHUNK = 32                    # keys of one chunk of the streamed attention (csrc/unet_api.h: UNET_ATTN_BK)

FAULTS = ("sin_cos_order", "freq_shift_1", "class_embedding_missing", "temb_without_silu", "temb_after_norm2", "resnet_eps_1e-6",
          "transformer_norm_eps_1e-5", "skip_before_hidden", "skip_order_fifo", "downsample_pad_right_bottom_only", "upsample_after_conv",
          "attn1_always_self", "attn1_always_cross", "scale_by_full_width", "heads_interleaved", "to_out_bias_missing",
          "geglu_halves_swapped", "gelu_tanh", "transformer_residual_missing", "layernorm_raw_moments_f32", "no_rescale_on_new_max")


def config(**cfg):
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown:
        raise TypeError(f"unknown configuration field(s) {unknown}")
    c = dict(DEFAULTS)
    c.update(cfg)
    for name in ("block_out_channels", "down_block_types", "up_block_types", "only_cross_attention"):
        c[name] = tuple(c[name])
    return c


def up_channels(widths, layers, i, j):
    """(hidden, skip, out) channels of resnet j of up block i: the usual diffusers bookkeeping."""
    rev = widths[::-1]
    out, before, in_ch = rev[i], rev[max(i - 1, 0)], rev[min(i + 1, len(widths) - 1)]
    return (before if j == 0 else out), (in_ch if j == layers else out), out


def spec(**cfg):
    """Ordered {key: shape} of UNet2DConditionModel(config).state_dict()."""
    c = config(**cfg)
    widths, layers, cross = c["block_out_channels"], c["layers_per_block"], c["cross_attention_dim"]
    levels, td = len(widths), 4 * widths[0]
    out = OrderedDict()

    def wb(name, wshape, bias=True):
        out[name + ".weight"] = tuple(wshape)
        if bias:
            out[name + ".bias"] = (wshape[0],)

    def resnet(r, cin, cout):
        wb(r + ".norm1", (cin,))
        wb(r + ".conv1", (cout, cin, 3, 3))
        wb(r + ".time_emb_proj", (cout, td))
        wb(r + ".norm2", (cout,))
        wb(r + ".conv2", (cout, cout, 3, 3))
        if cin != cout:
            wb(r + ".conv_shortcut", (cout, cin, 1, 1))

    def transformer(a, dim, only_cross):
        wb(a + ".norm", (dim,))
        wb(a + ".proj_in", (dim, dim))
        b = a + ".transformer_blocks.0"
        for i in (1, 2):
            kv = cross if (i == 2 or only_cross) else dim
            wb(f"{b}.norm{i}", (dim,))
            wb(f"{b}.attn{i}.to_q", (dim, dim), bias=False)
            wb(f"{b}.attn{i}.to_k", (dim, kv), bias=False)
            wb(f"{b}.attn{i}.to_v", (dim, kv), bias=False)
            wb(f"{b}.attn{i}.to_out.0", (dim, dim))
        wb(b + ".norm3", (dim,))
        wb(b + ".ff.net.0.proj", (8 * dim, dim))
        wb(b + ".ff.net.2", (dim, 4 * dim))
        wb(a + ".proj_out", (dim, dim))

    wb("conv_in", (widths[0], c["in_channels"], 3, 3))
    wb("time_embedding.linear_1", (td, widths[0]))
    wb("time_embedding.linear_2", (td, td))
    out["class_embedding.weight"] = (c["num_class_embeds"], td)
    prev = widths[0]
    for i, wd in enumerate(widths):
        if c["down_block_types"][i] == "CrossAttnDownBlock2D":
            for j in range(layers):
                transformer(f"down_blocks.{i}.attentions.{j}", wd, c["only_cross_attention"][i])
        for j in range(layers):
            resnet(f"down_blocks.{i}.resnets.{j}", prev if j == 0 else wd, wd)
        if i < levels - 1:
            wb(f"down_blocks.{i}.downsamplers.0.conv", (wd, wd, 3, 3))
        prev = wd
    for i in range(levels):
        wd = widths[levels - 1 - i]
        if c["up_block_types"][i] == "CrossAttnUpBlock2D":
            for j in range(layers + 1):
                transformer(f"up_blocks.{i}.attentions.{j}", wd, c["only_cross_attention"][levels - 1 - i])
        for j in range(layers + 1):
            hidden, skip, o = up_channels(widths, layers, i, j)
            resnet(f"up_blocks.{i}.resnets.{j}", hidden + skip, o)
        if i < levels - 1:
            wb(f"up_blocks.{i}.upsamplers.0.conv", (wd, wd, 3, 3))
    transformer("mid_block.attentions.0", widths[-1], False)
    resnet("mid_block.resnets.0", widths[-1], widths[-1])
    resnet("mid_block.resnets.1", widths[-1], widths[-1])
    wb("conv_norm_out", (widths[0],))
    wb("conv_out", (c["out_channels"], widths[0], 3, 3))
    return out


def seeded_state_dict(seed, **cfg):
    """Every tensor random (no norm gain of 1, no zero bias): float32, the same for a seed."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for key, shape in spec(**cfg).items():
        r = torch.randn(shape, generator=g)
        if ".norm" in key or key.startswith("conv_norm_out"):
            t = 1.0 + 0.3 * r if key.endswith("weight") else 0.2 * r
        elif key == "class_embedding.weight":
            t = 0.5 * r
        elif key.endswith("bias"):
            t = 0.2 * r
        else:
            t = r * (1.0 / math.sqrt(int(np.prod(shape[1:]))))
        sd[key] = t.float().contiguous()
    return sd


def seeded_inputs(n, h, w, tokens, seed, channels=7, cross=1024):
    """(sample [n, channels, h, w], text states [n, tokens, cross]) float32: unit noise, every sample its own."""
    g = torch.Generator().manual_seed(5000 + seed)
    return torch.randn((n, channels, h, w), generator=g).float(), torch.randn((n, tokens, cross), generator=g).float()


# ------------------------------------------------------------------------------------------------ the pieces
def time_embedding(p, timestep, label, width0, dtype, fault=None):
    """[1, 4 width0]: time_embedding(sinusoid(t)) + class row.  The sinusoid is formed in float64 and rounded once."""
    half = width0 // 2
    i = torch.arange(half, dtype=torch.float64)
    ang = float(timestep) * torch.exp(-math.log(10000.0) * i / (half - (1 if fault == "freq_shift_1" else 0)))
    parts = [torch.sin(ang), torch.cos(ang)] if fault == "sin_cos_order" else [torch.cos(ang), torch.sin(ang)]
    s = torch.cat(parts).to(p["time_embedding.linear_1.weight"].device, dtype)[None]
    e = F.linear(F.silu(F.linear(s, p["time_embedding.linear_1.weight"], p["time_embedding.linear_1.bias"])),
                 p["time_embedding.linear_2.weight"], p["time_embedding.linear_2.bias"])
    return e if fault == "class_embedding_missing" else e + p["class_embedding.weight"][int(label)][None]


def resnet(p, r, x, emb, groups, eps, fault=None):
    if fault == "resnet_eps_1e-6":
        eps = 1e-6
    h = F.conv2d(F.silu(F.group_norm(x, groups, p[r + ".norm1.weight"], p[r + ".norm1.bias"], eps)), p[r + ".conv1.weight"], p[r + ".conv1.bias"], padding=1)
    t = F.linear(emb if fault == "temb_without_silu" else F.silu(emb), p[r + ".time_emb_proj.weight"], p[r + ".time_emb_proj.bias"])[:, :, None, None]
    if fault == "temb_after_norm2":
        h = F.group_norm(h, groups, p[r + ".norm2.weight"], p[r + ".norm2.bias"], eps) + t
    else:
        h = F.group_norm(h + t, groups, p[r + ".norm2.weight"], p[r + ".norm2.bias"], eps)
    h = F.conv2d(F.silu(h), p[r + ".conv2.weight"], p[r + ".conv2.bias"], padding=1)
    if r + ".conv_shortcut.weight" in p:
        x = F.conv2d(x, p[r + ".conv_shortcut.weight"], p[r + ".conv_shortcut.bias"])
    return x + h


def layer_norm(x, weight, bias, fault=None):
    if fault != "layernorm_raw_moments_f32":
        return F.layer_norm(x, x.shape[-1:], weight, bias, LAYER_NORM_EPS)
    x32 = x.float()                      # E[x^2] - E[x]^2 with every sum in float32
    m = x32.mean(-1, keepdim=True)
    var = ((x32 * x32).mean(-1, keepdim=True) - m * m).clamp_min(0)
    return ((x - m.to(x.dtype)) / torch.sqrt(var.to(x.dtype) + LAYER_NORM_EPS)) * weight + bias


def streamed_attention(q, k, v, scale, chunk=STREAM_CHUNK, rescale=True):
    """softmax(q k^T scale) v over key chunks with a running maximum and sum ([..., tokens, d]); rescale=False forgets to rescale
    the accumulator when the maximum moves (the sum is still rescaled): the fault no_rescale_on_new_max."""
    m = torch.full(q.shape[:-1] + (1,), -math.inf, dtype=q.dtype)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for k0 in range(0, k.shape[-2], chunk):
        s = (q @ k[..., k0:k0 + chunk, :].transpose(-1, -2)) * scale
        m_new = torch.maximum(m, s.max(dim=-1, keepdim=True).values)
        pr = torch.exp(s - m_new)
        alpha = torch.exp(m - m_new)
        l = l * alpha + pr.sum(dim=-1, keepdim=True)
        o = (o * alpha if rescale else o) + pr @ v[..., k0:k0 + chunk, :]
        m = m_new
    return o / l


def attention(p, a, x, ctx, heads, fault=None, taps=None):
    """x [n, T, dim], ctx [n, S, .] -> to_out(softmax(q k^T / sqrt(d)) v) per head."""
    n, T, dim = x.shape
    d = dim // heads
    q, k, v = F.linear(x, p[a + ".to_q.weight"]), F.linear(ctx, p[a + ".to_k.weight"]), F.linear(ctx, p[a + ".to_v.weight"])

    def split(t):                        # [n, tokens, dim] -> [n, heads, tokens, d]
        if fault == "heads_interleaved":
            return t.reshape(n, -1, d, heads).permute(0, 3, 1, 2)
        return t.reshape(n, -1, heads, d).permute(0, 2, 1, 3)

    q, k, v = split(q), split(k), split(v)
    scale = 1.0 / math.sqrt(dim if fault == "scale_by_full_width" else d)
    if taps is not None and a in taps.get("want", ()):
        taps[a] = dict(tokens=x, scores=(q @ k.transpose(-1, -2)) * scale)
    if fault == "no_rescale_on_new_max":
        o = streamed_attention(q, k, v, scale, rescale=False)
    else:
        o = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v
    if fault == "heads_interleaved":
        o = o.permute(0, 2, 3, 1).reshape(n, T, dim)
    else:
        o = o.permute(0, 2, 1, 3).reshape(n, T, dim)
    return F.linear(o, p[a + ".to_out.0.weight"], None if fault == "to_out_bias_missing" else p[a + ".to_out.0.bias"])


def transformer(p, a, x, text, groups, heads, only_cross, fault=None, taps=None):
    n, c, h, w = x.shape
    eps = 1e-5 if fault == "transformer_norm_eps_1e-5" else TRANSFORMER_NORM_EPS
    t = F.group_norm(x, groups, p[a + ".norm.weight"], p[a + ".norm.bias"], eps).permute(0, 2, 3, 1).reshape(n, h * w, c)
    t = F.linear(t, p[a + ".proj_in.weight"], p[a + ".proj_in.bias"])
    b = a + ".transformer_blocks.0"
    y = layer_norm(t, p[b + ".norm1.weight"], p[b + ".norm1.bias"], fault)
    kv_width = p[b + ".attn1.to_k.weight"].shape[1]
    cross1 = only_cross
    if fault == "attn1_always_self" and kv_width == c:          # the faults act where the widths let them
        cross1 = False
    if fault == "attn1_always_cross" and kv_width == text.shape[-1]:
        cross1 = True
    t = t + attention(p, b + ".attn1", y, text if cross1 else y, heads, fault, taps)
    y = layer_norm(t, p[b + ".norm2.weight"], p[b + ".norm2.bias"], fault)
    t = t + attention(p, b + ".attn2", y, text, heads, fault, taps)
    y = layer_norm(t, p[b + ".norm3.weight"], p[b + ".norm3.bias"], fault)
    hg = F.linear(y, p[b + ".ff.net.0.proj.weight"], p[b + ".ff.net.0.proj.bias"])
    value, gate = hg.chunk(2, dim=-1)
    if fault == "geglu_halves_swapped":
        value, gate = gate, value
    t = t + F.linear(value * F.gelu(gate, approximate="tanh" if fault == "gelu_tanh" else "none"), p[b + ".ff.net.2.weight"], p[b + ".ff.net.2.bias"])
    t = F.linear(t, p[a + ".proj_out.weight"], p[a + ".proj_out.bias"]).reshape(n, h, w, c).permute(0, 3, 1, 2)
    return t if fault == "transformer_residual_missing" else t + x


def forward(sd, sample, timestep, text, label, fault=None, taps=None, **cfg):
    """sample [n, in_channels, h, w], text [n, tokens, cross_attention_dim] -> [n, out_channels, h, w], in sample's dtype."""
    c = config(**cfg)
    dt = sample.dtype
    p = {k: v.to(dt) for k, v in sd.items()}
    text = text.to(dt)
    widths, layers, groups, heads, eps = c["block_out_channels"], c["layers_per_block"], c["norm_num_groups"], c["attention_head_dim"], c["norm_eps"]
    levels = len(widths)
    emb = time_embedding(p, timestep, label, widths[0], dt, fault)
    x = F.conv2d(sample, p["conv_in.weight"], p["conv_in.bias"], padding=1)
    skips = [x]
    for i in range(levels):
        for j in range(layers):
            x = resnet(p, f"down_blocks.{i}.resnets.{j}", x, emb, groups, eps, fault)
            if c["down_block_types"][i] == "CrossAttnDownBlock2D":
                x = transformer(p, f"down_blocks.{i}.attentions.{j}", x, text, groups, heads, c["only_cross_attention"][i], fault, taps)
            skips.append(x)
        if i < levels - 1:
            dw, db = p[f"down_blocks.{i}.downsamplers.0.conv.weight"], p[f"down_blocks.{i}.downsamplers.0.conv.bias"]
            if fault == "downsample_pad_right_bottom_only":
                x = F.conv2d(F.pad(x, (0, 1, 0, 1)), dw, db, stride=2)
            else:
                x = F.conv2d(x, dw, db, stride=2, padding=1)
            skips.append(x)
    x = resnet(p, "mid_block.resnets.0", x, emb, groups, eps, fault)
    x = transformer(p, "mid_block.attentions.0", x, text, groups, heads, False, fault, taps)
    x = resnet(p, "mid_block.resnets.1", x, emb, groups, eps, fault)
    for i in range(levels):
        level = levels - 1 - i
        mine = [skips.pop() for _ in range(layers + 1)]      # last in, first out
        if fault == "skip_order_fifo" and len({s.shape[1] for s in mine}) == 1:      # where the widths let it: first in, first out
            mine = mine[::-1]
        for j in range(layers + 1):
            pair = [mine[j], x] if fault == "skip_before_hidden" else [x, mine[j]]
            x = resnet(p, f"up_blocks.{i}.resnets.{j}", torch.cat(pair, dim=1), emb, groups, eps, fault)
            if c["up_block_types"][i] == "CrossAttnUpBlock2D":
                x = transformer(p, f"up_blocks.{i}.attentions.{j}", x, text, groups, heads, c["only_cross_attention"][level], fault, taps)
        if i < levels - 1:
            uw, ub = p[f"up_blocks.{i}.upsamplers.0.conv.weight"], p[f"up_blocks.{i}.upsamplers.0.conv.bias"]
            if fault == "upsample_after_conv":
                x = F.interpolate(F.conv2d(x, uw, ub, padding=1), scale_factor=2.0, mode="nearest")
            else:
                x = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), uw, ub, padding=1)
    x = F.silu(F.group_norm(x, groups, p["conv_norm_out.weight"], p["conv_norm_out.bias"], eps))
    return F.conv2d(x, p["conv_out.weight"], p["conv_out.bias"], padding=1)
