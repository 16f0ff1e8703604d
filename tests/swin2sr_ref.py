"""A functional restatement of transformers-5's Swin2SRForImageSuperResolution.forward in eval mode: plain torch ops on a state
dict under transformers' names, in whatever float dtype it is handed (float64 for the reference).  The specification of
csrc/swin2sr.hip; tests/test_swin2sr_host.py holds it to transformers itself in float64.

What the installed source does and a memory of SwinIR would not (modeling_swin2sr.py):
  * the region mask is added to the scores TWICE (Swin2SRSelfAttention.forward adds `attention_mask` once inside the view and
    once more on the next line), so a pair from different regions gets -100 and -100 again, in that order;
  * window size and shift are fixed at construction from config.image_size (_compute_window_shift): with image_size >
    window_size they are the configuration's, whatever the frame; the mask comes from the run-time grid;
  * the long residual is first_convolution's output, before the patch embedding's 1x1 projection and LayerNorm;
  * the patch embedding's LayerNorm has torch's default eps, every other LayerNorm config.layer_norm_eps;
  * key has no bias; query and value have one.

`fault` names one deliberate mistake (FAULTS); tests/test_swin2sr_cases_host.py shows that every one of them fails a crafted
case.  The faults of FRAME_FAULTS are mistakes of the processor's padding and act in `process_frame`, not in the model.  Frame level: `process_frame` is Swin2SRImageProcessor (x / 255, symmetric pad right and bottom to (n // 8 + 1) * 8) and
`upscale_u8` the documented post-processing (clamp, x 255, round, uint8) of the model's output cropped to H s x W s.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

DEFAULTS = dict(image_size=64, patch_size=1, num_channels=3, num_channels_out=None, embed_dim=180, depths=(6, 6, 6, 6, 6, 6),
                num_heads=(6, 6, 6, 6, 6, 6), window_size=8, mlp_ratio=2.0, qkv_bias=True, use_absolute_embeddings=False,
                layer_norm_eps=1e-5, upscale=2, img_range=1.0, resi_connection="1conv", upsampler="pixelshuffle")
RGB_MEAN = (0.4488, 0.4371, 0.4040)
NUM_FEATURES = 64                    # the width of the pixelshuffle and nearest+conv heads
PROCESSOR_PAD = 8                    # Swin2SRImageProcessor.size_divisor

FAULTS = ("no_shift", "shift_reversed", "no_mask", "regions_at_shift_only", "key_bias", "no_clamp", "bias_unsquashed",
          "index_transposed", "pre_norm", "long_residual_after_embed", "no_stage_residual", "gelu_tanh", "shuffle_order",
          "lrelu_swapped", "symmetric_pad", "mean_not_added", "phantom_keys_unmasked", "shift_rounded_up", "ln_unbiased",
          "ln_padded_width", "embed_eps_from_config", "eps_default_everywhere", "gray_mean_kept", "single_bounce_pad")
FRAME_FAULTS = ("single_bounce_pad",)      # faults of the processor's padding: process_frame and upscale_float take them, not the model


def config(**cfg):
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown:
        raise TypeError(f"unknown Swin2SRConfig field(s) {unknown}")
    c = dict(DEFAULTS)
    c.update(cfg)
    c["depths"], c["num_heads"] = tuple(c["depths"]), tuple(c["num_heads"])
    if c["num_channels_out"] is None:
        c["num_channels_out"] = c["num_channels"]
    return c


def state_dict_spec(**cfg):
    """Ordered {key: shape} of Swin2SRForImageSuperResolution(config).state_dict()."""
    c = config(**cfg)
    C, hid, nf = c["embed_dim"], int(c["mlp_ratio"] * c["embed_dim"]), NUM_FEATURES
    spec = OrderedDict()

    def wb(name, wshape, bias=True):
        spec[name + ".weight"] = tuple(wshape)
        if bias:
            spec[name + ".bias"] = (wshape[0],)

    wb("swin2sr.first_convolution", (C, c["num_channels"], 3, 3))
    wb("swin2sr.embeddings.patch_embeddings.projection", (C, C, 1, 1))
    wb("swin2sr.embeddings.patch_embeddings.layernorm", (C,))
    for i, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
        s = f"swin2sr.encoder.stages.{i}"
        for j in range(depth):
            a = f"{s}.layers.{j}.attention.self"
            spec[a + ".logit_scale"] = (heads, 1, 1)
            wb(a + ".continuous_position_bias_mlp.0", (512, 2))
            wb(a + ".continuous_position_bias_mlp.2", (heads, 512), bias=False)
            wb(a + ".query", (C, C))
            wb(a + ".key", (C, C), bias=False)
            wb(a + ".value", (C, C))
            wb(f"{s}.layers.{j}.attention.output.dense", (C, C))
            wb(f"{s}.layers.{j}.layernorm_before", (C,))
            wb(f"{s}.layers.{j}.intermediate.dense", (hid, C))
            wb(f"{s}.layers.{j}.output.dense", (C, hid))
            wb(f"{s}.layers.{j}.layernorm_after", (C,))
        wb(s + ".conv", (C, C, 3, 3))
        wb(s + ".patch_embed.projection", (C, C, 1, 1))
    wb("swin2sr.layernorm", (C,))
    wb("swin2sr.conv_after_body", (C, C, 3, 3))
    up, scale, cout = c["upsampler"], c["upscale"], c["num_channels_out"]
    if up == "pixelshuffle":
        wb("upsample.conv_before_upsample", (nf, C, 3, 3))
        if scale & (scale - 1) == 0:
            for i in range(int(math.log2(scale))):
                wb(f"upsample.upsample.convolution_{i}", (4 * nf, nf, 3, 3))
        elif scale == 3:
            wb("upsample.upsample.convolution", (9 * nf, nf, 3, 3))
        else:
            raise ValueError(f"pixelshuffle: scale {scale}")
        wb("upsample.final_convolution", (cout, nf, 3, 3))
    elif up == "pixelshuffledirect":
        wb("upsample.conv", (scale * scale * cout, C, 3, 3))
    elif up == "nearest+conv":
        if scale != 4:
            raise ValueError("nearest+conv: scale 4 only")
        wb("upsample.conv_before_upsample", (nf, C, 3, 3))
        for name in ("conv_up1", "conv_up2", "conv_hr"):
            wb("upsample." + name, (nf, nf, 3, 3))
        wb("upsample.final_convolution", (cout, nf, 3, 3))
    else:
        raise ValueError(f"upsampler {up!r}")
    return spec


def seeded_state_dict(seed, **cfg):
    """Every tensor random (no LayerNorm gain of 1, no zero bias, no logit_scale of ln 10): float32, the same for a seed.
    logit_scale spreads over ln 100 -+ 1.2, so some heads sit above the clamp."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for key, shape in state_dict_spec(**cfg).items():
        r = torch.randn(shape, generator=g)
        if key.endswith("logit_scale"):
            t = math.log(100.0) + 1.2 * (2 * torch.rand(shape, generator=g) - 1) - 0.6
        elif key.startswith(("upsample.final_convolution", "upsample.conv.")):      # the image stays mostly inside [0, 1]
            t = (0.15 / math.sqrt(int(np.prod(shape[1:])))) * r if key.endswith("weight") else 0.05 * r
        elif "layernorm" in key:
            t = 1.0 + 0.3 * r if key.endswith("weight") else 0.2 * r
        elif key.endswith("bias"):
            t = 0.2 * r
        elif "continuous_position_bias_mlp.0" in key:
            t = 0.8 * r
        elif "continuous_position_bias_mlp.2" in key:
            t = 0.12 * r
        else:
            fan_in = int(np.prod(shape[1:]))
            t = r * (1.0 / math.sqrt(fan_in))
        sd[key] = t.float().contiguous()
    return sd


def seeded_input(h, w, seed, channels=3):
    return torch.rand((1, channels, h, w), generator=torch.Generator().manual_seed(1000 + seed)).float()


def seeded_frame(h, w, seed):
    """A uint8 RGB frame with structure (ramps and a few rectangles) plus noise."""
    rng = np.random.RandomState(2000 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255.0 / max(w - 1, 1)), (yy * 255.0 / max(h - 1, 1)), ((xx + yy) % 7) * 36.0], axis=-1)
    img += rng.uniform(-40, 40, size=img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the pieces
def coords_table_and_index(ws, dtype):
    """Swin2SRSelfAttention.create_coords_table_and_index with pretrained_window_size 0."""
    rc = torch.arange(-(ws - 1), ws, dtype=torch.int64).float()
    table = torch.stack(torch.meshgrid([rc, rc], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
    if ws > 1:
        table = table / (ws - 1)
    table = table * 8
    table = torch.sign(table) * torch.log2(torch.abs(table) + 1.0) / math.log2(8)
    c = torch.arange(ws)
    coords = torch.stack(torch.meshgrid([c, c], indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return table.to(dtype), rel.sum(-1)


def position_bias(p, a, ws, heads, fault=None):
    """16 sigmoid(MLP(table))[index] as [heads, ws^2, ws^2]: does not depend on the input."""
    dtype = p[a + ".query.weight"].dtype
    table, index = coords_table_and_index(ws, dtype)
    if fault == "index_transposed":
        index = index.t()
    t = F.linear(F.relu(F.linear(table, p[a + ".continuous_position_bias_mlp.0.weight"], p[a + ".continuous_position_bias_mlp.0.bias"])),
                 p[a + ".continuous_position_bias_mlp.2.weight"]).view(-1, heads)
    b = t[index.reshape(-1)].view(ws * ws, ws * ws, heads).permute(2, 0, 1).contiguous()
    return b if fault == "bias_unsquashed" else 16 * torch.sigmoid(b)


def region_mask(h, w, ws, shift, dtype, fault=None):
    """[windows, ws^2, ws^2]: -100 between tokens of different regions, three regions an axis."""
    def regions(n):
        i = torch.arange(n)
        if fault == "regions_at_shift_only":
            return (i >= n - shift).long()
        return (i >= n - ws).long() + (i >= n - shift).long()
    img = (regions(h)[:, None] * 3 + regions(w)[None, :]).to(dtype)
    mw = img.view(h // ws, ws, w // ws, ws).transpose(1, 2).reshape(-1, ws * ws)
    diff = mw.unsqueeze(1) - mw.unsqueeze(2)
    return torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff))


def layer_norm(t, C, weight, bias, eps, fault=None):
    """F.layer_norm over the last axis; the two faults of its statistics are written out."""
    if fault not in ("ln_unbiased", "ln_padded_width"):
        return F.layer_norm(t, (C,), weight, bias, eps)
    if fault == "ln_unbiased":
        mean = t.sum(-1, keepdim=True) / C
        var = ((t - mean) ** 2).sum(-1, keepdim=True) / (C - 1)
    else:                                    # the sums run over the C real columns, the divisor is the storage width
        cp = -(-C // 16) * 16
        mean = t.sum(-1, keepdim=True) / cp
        var = ((t - mean) ** 2).sum(-1, keepdim=True) / cp
    return (t - mean) / torch.sqrt(var + eps) * weight + bias


def window_attention(p, a, xw, mask, ws, heads, fault=None, taps=None):
    """xw [windows, ws^2, C] -> the context before output.dense."""
    nw, n, C = xw.shape
    d = C // heads
    split = lambda t: t.view(nw, n, heads, d).transpose(1, 2)
    q = split(F.linear(xw, p[a + ".query.weight"], p[a + ".query.bias"]))
    k = split(F.linear(xw, p[a + ".key.weight"], p[a + ".query.bias"] if fault == "key_bias" else None))
    v = split(F.linear(xw, p[a + ".value.weight"], p[a + ".value.bias"]))
    s = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
    ls = p[a + ".logit_scale"]
    s = s * (ls if fault == "no_clamp" else torch.clamp(ls, max=math.log(1.0 / 0.01))).exp()
    s = s + position_bias(p, a, ws, heads, fault).unsqueeze(0)
    if mask is not None:
        s = (s + mask.unsqueeze(1)) + mask.unsqueeze(1)        # twice, as the source does
    if taps is not None:
        taps.setdefault("scores", []).append(s)
    if fault == "phantom_keys_unmasked" and n % 16:
        # the window padded to a multiple of 16 tokens with zero tokens: their keys are zero (no key bias) and score 0 where
        # -inf belongs; their values are the value bias
        pad = -n % 16
        s = torch.cat([s, s.new_zeros(nw, heads, n, pad)], dim=-1)
        v = torch.cat([v, p[a + ".value.bias"].view(1, heads, 1, d).expand(nw, heads, pad, d)], dim=2)
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(nw, n, C)


def layer(p, l, x, h, w, ws, shift, heads, eps, fault=None, taps=None):
    """x [h w, C] tokens of one image -> the layer's output."""
    C = x.shape[-1]
    img = x.view(h, w, C)
    s = 0 if fault == "no_shift" else shift
    fwd = (s, s) if fault == "shift_reversed" else (-s, -s)
    if s > 0:
        img = torch.roll(img, shifts=fwd, dims=(0, 1))
    xw = img.view(h // ws, ws, w // ws, ws, C).transpose(1, 2).reshape(-1, ws * ws, C)
    mask = region_mask(h, w, ws, shift, x.dtype, fault) if (shift > 0 and fault != "no_mask") else None
    ln1 = lambda t: layer_norm(t, C, p[l + ".layernorm_before.weight"], p[l + ".layernorm_before.bias"], eps, fault)
    ln2 = lambda t: layer_norm(t, C, p[l + ".layernorm_after.weight"], p[l + ".layernorm_after.bias"], eps, fault)
    if fault == "pre_norm":
        xw = ln1(xw)
    ctx = window_attention(p, l + ".attention.self", xw, mask, ws, heads, fault, taps)
    o = F.linear(ctx, p[l + ".attention.output.dense.weight"], p[l + ".attention.output.dense.bias"])
    o = o.view(h // ws, w // ws, ws, ws, C).transpose(1, 2).reshape(h, w, C)
    if s > 0:
        o = torch.roll(o, shifts=(-fwd[0], -fwd[1]), dims=(0, 1))
    o = o.reshape(h * w, C)
    hdn = x + (o if fault == "pre_norm" else ln1(o))
    mlp = lambda t: F.linear(F.gelu(F.linear(t, p[l + ".intermediate.dense.weight"], p[l + ".intermediate.dense.bias"]),
                                    approximate="tanh" if fault == "gelu_tanh" else "none"),
                             p[l + ".output.dense.weight"], p[l + ".output.dense.bias"])
    return hdn + (mlp(ln2(hdn)) if fault == "pre_norm" else ln2(mlp(hdn)))


def pixel_shuffle(x, r, fault=None):
    if fault != "shuffle_order":
        return F.pixel_shuffle(x, r)
    n, c, h, w = x.shape                     # channels read as (r1, r2, c) instead of (c, r1, r2)
    return x.view(n, r, r, c // (r * r), h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c // (r * r), h * r, w * r)


def swin2sr_forward(sd, pixel_values, fault=None, taps=None, **cfg):
    """pixel_values [1, C, H, W] -> reconstruction [1, Cout, H s, W s], in pixel_values' dtype."""
    c = config(**cfg)
    dt = pixel_values.dtype
    p = {k: v.to(dt) for k, v in sd.items() if v.dtype.is_floating_point}
    ws, scale, eps, rng, C = c["window_size"], c["upscale"], c["layer_norm_eps"], c["img_range"], c["embed_dim"]
    conv = lambda t, name: F.conv2d(t, p[name + ".weight"], p[name + ".bias"], padding=p[name + ".weight"].shape[-1] // 2)
    _, _, H, W = pixel_values.shape
    if c["num_channels"] == 3 and c["num_channels_out"] == 3:
        mean = torch.tensor(RGB_MEAN, dtype=torch.float32).to(dt).view(1, 3, 1, 1)      # the float32 values, as the model's buffer
    else:
        mean = torch.full((1, 1, 1, 1), RGB_MEAN[0] if fault == "gray_mean_kept" else 0.0, dtype=torch.float32).to(dt)
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    x = pixel_values
    if ph or pw:
        if fault == "symmetric_pad":
            x = torch.cat([x, x.flip(3)[..., :pw]], dim=3)
            x = torch.cat([x, x.flip(2)[:, :, :ph]], dim=2)
        else:
            x = F.pad(x, (0, pw, 0, ph), "reflect")
    x = (x - mean) * rng
    first = conv(x, "swin2sr.first_convolution")
    h, w = first.shape[2:]
    pe = "swin2sr.embeddings.patch_embeddings"
    t = conv(first, pe + ".projection").flatten(2).transpose(1, 2)[0]            # [h w, C]
    eps_embed = eps if fault == "embed_eps_from_config" else 1e-5
    if fault == "eps_default_everywhere":
        eps = 1e-5
    half = (ws + 1) // 2 if fault == "shift_rounded_up" else ws // 2
    t = layer_norm(t, C, p[pe + ".layernorm.weight"], p[pe + ".layernorm.bias"], eps_embed, fault)
    long_res = t.t().reshape(1, C, h, w) if fault == "long_residual_after_embed" else first
    for i, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
        s = f"swin2sr.encoder.stages.{i}"
        res = t
        for j in range(depth):
            t = layer(p, f"{s}.layers.{j}", t, h, w, ws, 0 if j % 2 == 0 else half, heads, eps, fault, taps)
        img = conv(t.t().reshape(1, C, h, w), s + ".conv")
        t = conv(img, s + ".patch_embed.projection").flatten(2).transpose(1, 2)[0]
        if fault != "no_stage_residual":
            t = t + res
    t = layer_norm(t, C, p["swin2sr.layernorm.weight"], p["swin2sr.layernorm.bias"], eps, fault)
    y = conv(t.t().reshape(1, C, h, w), "swin2sr.conv_after_body") + long_res
    up = c["upsampler"]
    s_ps, s_nc = (0.2, 0.01) if fault == "lrelu_swapped" else (0.01, 0.2)
    if up == "pixelshuffle":
        y = F.leaky_relu(conv(y, "upsample.conv_before_upsample"), s_ps)
        if scale == 3:
            y = pixel_shuffle(conv(y, "upsample.upsample.convolution"), 3, fault)
        else:
            for i in range(int(math.log2(scale))):
                y = pixel_shuffle(conv(y, f"upsample.upsample.convolution_{i}"), 2, fault)
        y = conv(y, "upsample.final_convolution")
    elif up == "pixelshuffledirect":
        y = pixel_shuffle(conv(y, "upsample.conv"), scale, fault)
    else:
        y = F.leaky_relu(conv(y, "upsample.conv_before_upsample"), s_ps)
        y = F.leaky_relu(conv(F.interpolate(y, scale_factor=2, mode="nearest"), "upsample.conv_up1"), s_nc)
        y = F.leaky_relu(conv(F.interpolate(y, scale_factor=2, mode="nearest"), "upsample.conv_up2"), s_nc)
        y = conv(F.leaky_relu(conv(y, "upsample.conv_hr"), s_nc), "upsample.final_convolution")
    y = y / rng
    if fault != "mean_not_added":
        y = y + mean
    return y[:, :, :H * scale, :W * scale]


# ------------------------------------------------------------------------------------------------ the frame-level route
def padded_size(n):
    return (n // PROCESSOR_PAD + 1) * PROCESSOR_PAD


def process_frame(frame, dtype=torch.float64, fault=None):
    """Swin2SRImageProcessor: [H, W, 3] uint8 -> [1, 3, Hp, Wp], x / 255 then numpy's "symmetric" pad right and bottom."""
    a = np.asarray(frame).astype(np.float64) / 255.0
    h, w = a.shape[:2]
    if fault == "single_bounce_pad":         # one reflection about the far edge, then the first sample
        bounce = lambda n: np.array([i if i < n else max(2 * n - 1 - i, 0) for i in range(padded_size(n))])
        a = a[bounce(h)][:, bounce(w)]
    else:
        a = np.pad(a, ((0, padded_size(h) - h), (0, padded_size(w) - w), (0, 0)), mode="symmetric")
    return torch.from_numpy(a).permute(2, 0, 1).unsqueeze(0).to(dtype).contiguous()


def upscale_float(sd, frame, dtype=torch.float64, fault=None, **cfg):
    """The model's output on the processed frame, cropped to [H s, W s, 3] (before the clamp).  `fault`: one of FRAME_FAULTS."""
    h, w = np.asarray(frame).shape[:2]
    s = config(**cfg)["upscale"]
    with torch.no_grad():
        y = swin2sr_forward(sd, process_frame(frame, dtype, fault), **cfg)
    return y[0, :, :h * s, :w * s].permute(1, 2, 0).contiguous()


def quantise(y):
    """clamp to [0, 1], x 255, round half to even, uint8."""
    return (y.clamp(0, 1) * 255.0).round().to(torch.uint8)


def upscale_u8(sd, frame, dtype=torch.float64, **cfg):
    return quantise(upscale_float(sd, frame, dtype, **cfg))


def u8_check(got, y64, tol):
    """(excluded, wrong, n): `got` uint8 against quantise(y64) wherever clamp(y64) x 255 lies farther than 255 tol from a rounding
    boundary (k + 0.5); elsewhere it may differ by 1."""
    v = y64.double().clamp(0, 1) * 255.0
    ref = v.round().to(torch.int64)
    firm = ((v - torch.floor(v)) - 0.5).abs() > 255.0 * tol
    got = torch.as_tensor(got).cpu().to(torch.int64)
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    wrong = ((got != ref) & firm) | ((got - ref).abs() > 1)
    return int((~firm).sum()), int(wrong.sum()), ref.numel()
