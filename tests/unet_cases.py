"""Crafted cases of the UNet: seeded configurations small enough to run in seconds, each built for a shape the kernels of
csrc/unet.hip can get wrong.  Every tensor is random (tests/unet_ref.py: seeded_state_dict) unless the case says otherwise.

  published_layout   four levels with the published block types and only_cross_attention pattern: widths (16, 32, 32, 64), 8
                     groups, 2 heads, 2 layers, cross dim 32, 7 tokens, 16 x 24 latents (the lowest level is 2 x 3), t = 487.25
  wide               widths (256, 512), 4 heads (head widths 64 and 128), cross dim 1024, 77 tokens, 1 layer, 4 x 6 latents: the
                     1024-channel concatenated conv input, the 2048-wide GEGLU (K tiled through LDS), the 1024-wide K | V product
  ragged_heads       width 48 with 2 heads: head width 24, no tile multiple; 8 groups of 6 channels; cross dim 24, no tile multiple
  seam_groups        widths (8, 16), 8 groups: an up-block resnet sees 16 + 8 = 24 channels, the group 15..17 straddles the seam
  self_many_tokens   two levels, the second with only_cross_attention False; 18 x 30 latents: 135 self-attention tokens, the last
                     query block and key chunk ragged
  late_maxima        the same frame; the mid block's attn1 has to_q and to_k crafted so that a key of the last chunk scores highest
                     for most queries: the running maximum moves in the last chunk and the accumulator has to be rescaled there
  one_text_token     1 text state
  many_text_tokens   80 text states: past two key chunks
  batch_two          n = 2 with different samples and text states
  timestep_lo / _hi  t = 0, label 0; t = 999, the last label
  offset_stats       a resnet's conv1.bias and a block's attn1.to_out.0.bias are 1000 + noise: GroupNorm and LayerNorm see a mean a
                     thousand deviations out
  small_variance     conv_in, and the resnet in front of a Transformer, scaled by 0.003: variances of the order of the eps
  smallest           two levels, 2 x 2 latents: the lowest level is one pixel and its self-attention has one token
  thin               2 x 34 latents

`reference(name)` computes the float64 restatement once and shares it; the tolerance of a case is 8 x max |float32 restatement -
float64| and is never written down.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from tests import unet_ref as R

Case = namedtuple("Case", "name cfg sd sample text timestep label")
LAST_CHUNK_SHARE = 0.5                # late_maxima: the share of queries whose best key lies in the last chunk, at least
LATE_ATTENTION = "mid_block.attentions.0.transformer_blocks.0.attn1"


def layout(widths, attention, only_cross, **more):
    """The configuration of a UNet with `widths`; attention[i]: level i has Transformers (down block i and its mirror)."""
    down = tuple("CrossAttnDownBlock2D" if a else "DownBlock2D" for a in attention)
    up = tuple("CrossAttnUpBlock2D" if a else "UpBlock2D" for a in reversed(attention))
    return dict(dict(block_out_channels=tuple(widths), down_block_types=down, up_block_types=up, only_cross_attention=tuple(only_cross),
                     num_class_embeds=10), **more)


SMALL = layout((16, 32), (True, True), (True, False), norm_num_groups=4, attention_head_dim=2, layers_per_block=1, cross_attention_dim=40)
MANY = layout((16, 64), (False, True), (False, False), norm_num_groups=8, attention_head_dim=2, layers_per_block=1, cross_attention_dim=64)

# which case must expose which fault (tests/test_unet_cases_host.py)
FAULT_CASE = {"sin_cos_order": "published_layout", "freq_shift_1": "published_layout", "class_embedding_missing": "published_layout",
              "temb_without_silu": "published_layout", "temb_after_norm2": "published_layout", "resnet_eps_1e-6": "small_variance",
              "transformer_norm_eps_1e-5": "small_variance", "skip_before_hidden": "seam_groups", "skip_order_fifo": "published_layout",
              "downsample_pad_right_bottom_only": "published_layout", "upsample_after_conv": "published_layout",
              "attn1_always_self": "published_layout", "attn1_always_cross": "self_many_tokens", "scale_by_full_width": "published_layout",
              "heads_interleaved": "published_layout", "to_out_bias_missing": "published_layout", "geglu_halves_swapped": "published_layout",
              "gelu_tanh": "published_layout", "transformer_residual_missing": "published_layout", "layernorm_raw_moments_f32": "offset_stats",
              "no_rescale_on_new_max": "late_maxima"}

_cases, _refs = {}, {}


def _make(name, seed, hw, cfg, tokens=7, n=1, timestep=487.25, label=3):
    c = R.config(**cfg)
    sample, text = R.seeded_inputs(n, hw[0], hw[1], tokens, seed, c["in_channels"], c["cross_attention_dim"])
    return Case(name, cfg, R.seeded_state_dict(seed, **cfg), sample, text, timestep, label)


def late_taps(case):
    """The tokens attn1 of the mid block reads and its scores [n, heads, queries, keys], in float64."""
    taps = {"want": (LATE_ATTENTION,)}
    with torch.no_grad():
        R.forward(case.sd, case.sample.double(), case.timestep, case.text, case.label, taps=taps, **case.cfg)
    return taps[LATE_ATTENTION]


def _late_maxima():
    """to_k = 2 I + noise and to_q = (g d) u^T + small noise: u is the vector with t . u = 1 for every token t (the tokens are
    LayerNorm outputs, which do not depend on this attention's weights), so every query is g d, and head by head d is the
    ridge-regression direction that tells the last token from the others; g puts it 8 above the runner-up."""
    base = _make("late_maxima", 37, (18, 30), MANY, tokens=9)
    tokens = late_taps(base)["tokens"][0]                       # [135, 64]
    n, c = tokens.shape
    heads = MANY["attention_head_dim"]
    d = c // heads
    u = torch.linalg.lstsq(tokens, torch.ones(n, 1, dtype=torch.float64)).solution[:, 0]
    assert float((tokens @ u - 1).abs().max()) < 1e-6
    target = torch.zeros(n, dtype=torch.float64)
    target[-1] = 1.0
    gd = torch.zeros(c, dtype=torch.float64)
    for h in range(heads):
        th = tokens[:, h * d:(h + 1) * d]
        centred = th - th.mean(0)
        dh = torch.linalg.solve(centred.t() @ centred + 0.1 * torch.eye(d, dtype=torch.float64), centred.t() @ target)
        best = (th @ dh).topk(2).values
        gd[h * d:(h + 1) * d] = dh * (8.0 * math.sqrt(d) / (2.0 * float(best[0] - best[1])))
    g = torch.Generator().manual_seed(370)
    base.sd[LATE_ATTENTION + ".to_k.weight"] = (2.0 * torch.eye(c) + 0.05 * torch.randn((c, c), generator=g)).contiguous()
    base.sd[LATE_ATTENTION + ".to_q.weight"] = (torch.outer(gd, u).float() + (0.1 / math.sqrt(c)) * torch.randn((c, c), generator=g)).contiguous()
    return base


def _build(name):
    if name == "published_layout":
        return _make(name, 31, (16, 24), layout((16, 32, 32, 64), (False, True, True, True), (True, True, True, False), norm_num_groups=8,
                                                attention_head_dim=2, layers_per_block=2, cross_attention_dim=32))
    if name == "wide":
        return _make(name, 32, (4, 6), layout((256, 512), (True, True), (True, True), norm_num_groups=32, attention_head_dim=4, layers_per_block=1,
                                              cross_attention_dim=1024), tokens=77)
    if name == "ragged_heads":
        return _make(name, 33, (6, 10), layout((48, 48), (True, True), (True, False), norm_num_groups=8, attention_head_dim=2, layers_per_block=1,
                                               cross_attention_dim=24), tokens=5)
    if name == "seam_groups":
        return _make(name, 34, (6, 10), layout((8, 16), (False, True), (False, True), norm_num_groups=8, attention_head_dim=2, layers_per_block=1,
                                               cross_attention_dim=40))
    if name == "self_many_tokens":
        return _make(name, 35, (18, 30), MANY, tokens=9)
    if name == "late_maxima":
        return _late_maxima()
    if name == "one_text_token":
        return _make(name, 38, (6, 10), SMALL, tokens=1)
    if name == "many_text_tokens":
        return _make(name, 39, (6, 10), SMALL, tokens=80)
    if name == "batch_two":
        return _make(name, 40, (6, 10), SMALL, n=2)
    if name == "timestep_lo":
        return _make(name, 41, (6, 10), SMALL, timestep=0, label=0)
    if name == "timestep_hi":
        return _make(name, 42, (6, 10), SMALL, timestep=999, label=SMALL["num_class_embeds"] - 1)
    if name == "offset_stats":
        case = _make(name, 43, (6, 10), SMALL)
        case.sd["down_blocks.0.resnets.0.conv1.bias"] += 1000.0
        case.sd["down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_out.0.bias"] += 1000.0
        return case
    if name == "small_variance":
        case = _make(name, 44, (6, 10), SMALL)
        for key in ("conv_in", "down_blocks.1.resnets.0.conv2", "down_blocks.1.resnets.0.conv_shortcut"):
            case.sd[key + ".weight"] *= 0.003
            case.sd[key + ".bias"] *= 0.003
        return case
    if name == "smallest":
        return _make(name, 45, (2, 2), SMALL)
    if name == "thin":
        return _make(name, 46, (2, 34), SMALL)
    raise KeyError(name)


NAMES = ("published_layout", "wide", "ragged_heads", "seam_groups", "self_many_tokens", "late_maxima", "one_text_token", "many_text_tokens",
         "batch_two", "timestep_lo", "timestep_hi", "offset_stats", "small_variance", "smallest", "thin")


def by_name(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def reference(name):
    """(y64, tol): the float64 restatement on the float32 inputs, and 8 x the float32 restatement's error."""
    if name not in _refs:
        case = by_name(name)
        with torch.no_grad():
            y64 = R.forward(case.sd, case.sample.double(), case.timestep, case.text, case.label, **case.cfg)
            y32 = R.forward(case.sd, case.sample, case.timestep, case.text, case.label, **case.cfg)
        _refs[name] = (y64, 8.0 * float((y32.double() - y64).abs().max()))
    return _refs[name]
