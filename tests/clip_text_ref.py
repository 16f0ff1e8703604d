"""A functional restatement of transformers' CLIPTextModel(input_ids)[0] as StableDiffusionUpscalePipeline uses it
("stabilityai/stable-diffusion-x4-upscaler"): plain torch ops on a state dict under transformers-5's names, in whatever float dtype
it is asked for (float64 for the reference).  The specification of csrc/clip_text.hip and of the launches clip_text_api.cpp
chains.  transformers is installed, so tests/test_clip_text_host.py holds this restatement to the library's own CLIPTextModel in
float64; no published checkpoint has been run through either.

What the network does and a guess would not:
  * positions count from 0; the token row and the position row are added, nothing else (no scale, no LayerNorm) before layer 0;
  * pre-norm: x += out_proj(attn(layer_norm1(x))), x += fc2(act(fc1(layer_norm2(x)))); final_layer_norm on every position;
  * the mask is causal and includes the query's own key; no padding mask (the pipeline passes no attention_mask), so the ids
    after the end-of-text id are ordinary tokens for the positions that see them;
  * a head is a contiguous block of columns of q, k and v, scaled by 1 / sqrt(its width);
  * hidden_act "gelu" is the erf form; "quick_gelu" is x sigmoid(1.702 x).

`fault` names one deliberate mistake (FAULTS); tests/test_clip_text_host.py shows that every one of them fails a crafted case.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

DEFAULTS = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16,
                max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="gelu")
STREAM_CHUNK = 32                    # keys of one chunk, and queries of one block, of the causal attention (csrc/unet_api.h)

FAULTS = ("not_causal", "causal_excludes_self", "padding_masked", "quick_gelu_for_gelu", "final_norm_dropped", "positions_from_one",
          "scale_by_hidden_not_head", "post_norm", "heads_interleaved")


def config(**cfg):
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown:
        raise TypeError(f"unknown configuration field(s) {unknown}")
    c = dict(DEFAULTS)
    c.update(cfg)
    return c


def spec(**cfg):
    """Ordered {key: shape} of CLIPTextModel(config).state_dict() (transformers 5: no `text_model.` prefix, no position_ids)."""
    c = config(**cfg)
    h, inter = c["hidden_size"], c["intermediate_size"]
    out = OrderedDict()

    def wb(name, wshape):
        out[name + ".weight"] = tuple(wshape)
        out[name + ".bias"] = (wshape[0],)

    out["embeddings.token_embedding.weight"] = (c["vocab_size"], h)
    out["embeddings.position_embedding.weight"] = (c["max_position_embeddings"], h)
    for i in range(c["num_hidden_layers"]):
        layer = f"encoder.layers.{i}"
        for part in ("k_proj", "v_proj", "q_proj", "out_proj"):
            wb(f"{layer}.self_attn.{part}", (h, h))
        wb(f"{layer}.layer_norm1", (h,))
        wb(f"{layer}.mlp.fc1", (inter, h))
        wb(f"{layer}.mlp.fc2", (h, inter))
        wb(f"{layer}.layer_norm2", (h,))
    wb("final_layer_norm", (h,))
    return out


def seeded_state_dict(seed, **cfg):
    """Every tensor random, float32: LayerNorm weights about 1, biases and embeddings of a size that matters, products that keep
    the activations of unit order.  q_proj and k_proj are larger than an initialisation's, so the softmax is far from uniform."""
    g = torch.Generator().manual_seed(9000 + seed)
    sd = OrderedDict()
    for key, shape in spec(**cfg).items():
        r = torch.randn(shape, generator=g, dtype=torch.float64)
        if "layer_norm" in key:
            t = 1.0 + 0.2 * r if key.endswith("weight") else 0.2 * r
        elif key.startswith("embeddings."):
            t = 0.7 * r
        elif key.endswith("bias"):
            t = 0.2 * r
        else:
            gain = 2.0 if (".q_proj." in key or ".k_proj." in key) else 1.0
            t = r * (gain / math.sqrt(shape[1]))
        sd[key] = t.float().contiguous()
    return sd


def old_generation(sd, positions):
    """The same state dict as a published text_encoder/ file carries it: `text_model.` in front, plus the position_ids buffer."""
    out = OrderedDict((("text_model." + k), v) for k, v in sd.items())
    out["text_model.embeddings.position_ids"] = torch.arange(positions)[None]
    return out


def allowed_keys(ids, eos, fault=None):
    """[n, 1, T, T] bool: may query i read key j."""
    n, T = ids.shape
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    if fault == "not_causal":
        ok = torch.ones(T, T, dtype=torch.bool)
    elif fault == "causal_excludes_self":
        ok = (j < i) | ((i == 0) & (j == 0))        # query 0 keeps its one key: a row without keys is no softmax
    else:
        ok = j <= i
    ok = ok[None, None].expand(n, 1, T, T)
    if fault == "padding_masked":                    # a tokenizer's attention_mask: up to and including the first end-of-text id
        hit = ids == eos
        first = torch.where(hit.any(dim=1), hit.int().argmax(dim=1), torch.full((n,), T - 1))
        ok = ok & (torch.arange(T)[None, :] <= first[:, None])[:, None, None, :]
    return ok


def activation(x, name, fault=None):
    if fault == "quick_gelu_for_gelu":
        name = "gelu" if name == "quick_gelu" else "quick_gelu"
    if name == "gelu":
        return F.gelu(x)
    if name == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    raise ValueError(f"hidden_act {name!r}")


def attention(p, a, x, ok, heads, fault=None, taps=None):
    """x [n, T, h] -> out_proj(softmax over the allowed keys of q k^T / sqrt(d)) v) per head."""
    n, T, h = x.shape
    d = h // heads
    q, k, v = (F.linear(x, p[f"{a}.{part}.weight"], p[f"{a}.{part}.bias"]) for part in ("q_proj", "k_proj", "v_proj"))

    def split(t):                        # [n, T, h] -> [n, heads, T, d]
        if fault == "heads_interleaved":
            return t.reshape(n, T, d, heads).permute(0, 3, 1, 2)
        return t.reshape(n, T, heads, d).permute(0, 2, 1, 3)

    q, k, v = split(q), split(k), split(v)
    scale = 1.0 / math.sqrt(h if fault == "scale_by_hidden_not_head" else d)
    s = (q @ k.transpose(-1, -2)) * scale
    if taps is not None:
        taps[a] = dict(q=q, k=k, v=v, scores=s)
    o = torch.softmax(s.masked_fill(~ok, -math.inf), dim=-1) @ v
    o = o.permute(0, 2, 3, 1).reshape(n, T, h) if fault == "heads_interleaved" else o.permute(0, 2, 1, 3).reshape(n, T, h)
    return F.linear(o, p[a + ".out_proj.weight"], p[a + ".out_proj.bias"])


def forward(sd, ids, dtype=torch.float64, fault=None, taps=None, **cfg):
    """ids [n, T] integers -> last_hidden_state [n, T, hidden_size] in `dtype`."""
    c = config(**cfg)
    p = {k: v.to(dtype) for k, v in sd.items()}
    ids = torch.as_tensor(ids, dtype=torch.int64)
    n, T = ids.shape
    h, heads, eps = c["hidden_size"], c["num_attention_heads"], c["layer_norm_eps"]
    positions = torch.arange(T)
    if fault == "positions_from_one":
        positions = (positions + 1) % c["max_position_embeddings"]
    x = p["embeddings.token_embedding.weight"][ids] + p["embeddings.position_embedding.weight"][positions][None]
    ok = allowed_keys(ids, c["vocab_size"] - 1, fault)
    norm = lambda t, name: F.layer_norm(t, (h,), p[name + ".weight"], p[name + ".bias"], eps)
    for i in range(c["num_hidden_layers"]):
        l = f"encoder.layers.{i}"
        mlp = lambda t: F.linear(activation(F.linear(t, p[l + ".mlp.fc1.weight"], p[l + ".mlp.fc1.bias"]), c["hidden_act"], fault),
                                 p[l + ".mlp.fc2.weight"], p[l + ".mlp.fc2.bias"])
        if fault == "post_norm":
            x = norm(x + attention(p, l + ".self_attn", x, ok, heads, fault, taps), l + ".layer_norm1")
            x = norm(x + mlp(x), l + ".layer_norm2")
        else:
            x = x + attention(p, l + ".self_attn", norm(x, l + ".layer_norm1"), ok, heads, fault, taps)
            x = x + mlp(norm(x, l + ".layer_norm2"))
    return x if fault == "final_norm_dropped" else norm(x, "final_layer_norm")
