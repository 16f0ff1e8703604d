"""Crafted cases of the VAE decoder: seeded configurations small enough to run in seconds, each built for a shape the kernels of
csrc/vae.hip can get wrong.  Every tensor is random (tests/vae_ref.py: seeded_state_dict) unless the case says otherwise.

  published_width   (128, 256, 512), 32 groups, 5 x 7 latents: the published shape; eight K chunks and four output blocks a conv
  two_levels        (16, 32), 4 groups, layers_per_block 1: every ResnetBlock of an up block has a shortcut
  four_levels       (8, 16, 16, 32): a four-level decoder, x8, with an up block that keeps its width (no shortcut)
  odd_groups        (24, 48), 8 groups: 3 channels a group at width 24, groups that straddle a 16-channel tile
  many_chunks       9 x 15 latents, 135 tokens: five key chunks and five query blocks, the last of each ragged (7 tokens)
  late_maxima       the same frame; to_q and to_k crafted so that the last token scores highest for most queries: the running
                    maximum moves in the last chunk and the accumulator has to be rescaled there
  offset_stats      mid_block.resnets.0.conv1's bias is 1000 + noise: the second GroupNorm sees a mean a thousand deviations out
  small_variance    conv_in scaled by 0.003: the first GroupNorm's variance is of the order of eps
  one_pixel         1 x 1 latents: a group of the first norms is its cpg channels of a single pixel
  thin              1 x 17 latents: one row, two tiles wide
  rounding_ties     conv_out's weights zero and its biases chosen so that every sample x 255 is k + 0.5 exactly in float32

`reference(name)` and `frame_reference(name)` compute the float64 restatement once and share it; the tolerance of a case is
8 x max |float32 restatement - float64| and is never written down.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from tests import vae_ref as R

Case = namedtuple("Case", "name cfg sd latents")
MAX_THIN = 0.02                       # share of a frame's samples that may lie within 255 tol of a rounding boundary
SMALL = dict(block_out_channels=(16, 32), norm_num_groups=4, layers_per_block=1)
LAST_CHUNK_SHARE = 0.5                # late_maxima: the share of queries whose best key lies in the last chunk, at least
TIE_LEVELS = (100, 101, 200)          # rounding_ties: sample x 255 is k + 0.5 for these k, one per channel

# which case must expose which fault (tests/test_vae_cases_host.py)
FAULT_CASE = {"eps_1e-5": "small_variance", "variance_unbiased": "one_pixel", "raw_moments_f32": "offset_stats",
              "padding_normalised": "two_levels", "silu_before_norm": "two_levels", "no_shortcut_conv": "two_levels",
              "attention_no_residual": "many_chunks", "scale_missing": "many_chunks", "softmax_over_queries": "many_chunks",
              "no_rescale_on_new_max": "late_maxima", "upsample_offset": "four_levels", "upsample_after_conv": "four_levels",
              "scaling_multiplied": "two_levels", "post_quant_skipped": "two_levels", "shift_before_halving": "two_levels",
              "round_half_up": "rounding_ties"}
FRAME_CASES = ("published_width", "four_levels", "many_chunks")      # at least 1000 samples each; the u8 route is checked on these

_cases, _refs, _frame_refs = {}, {}, {}


def _make(name, seed, hw, cfg):
    c = R.config(**cfg)
    return Case(name, cfg, R.seeded_state_dict(seed, **cfg), R.seeded_latents(hw[0], hw[1], seed, c["latent_channels"], c["scaling_factor"]))


def _late_maxima():
    """to_k = 2 I + noise, to_q = small noise with the bias g d: every query scores key j at about 2 g d . t_j / sqrt(C) (t the
    normalised tokens, which do not depend on the attention's weights).  d is the ridge-regression direction that tells the last
    token from the others (the tokens of a smooth frame are far from orthogonal, so t_last itself would not do), and g puts the
    last token 8 above the runner-up."""
    base = _make("late_maxima", 17, (9, 15), SMALL)
    taps = {}
    with torch.no_grad():
        R.decode(base.sd, (base.latents.double() / R.config(**SMALL)["scaling_factor"]), taps=taps, **SMALL)
    tokens = taps["tokens"]
    centred = tokens - tokens.mean(0)
    n, c = tokens.shape
    target = torch.zeros(n, dtype=torch.float64)
    target[-1] = 1.0
    d = torch.linalg.solve(centred.t() @ centred + 0.1 * torch.eye(c, dtype=torch.float64), centred.t() @ target)
    best = (tokens @ d).topk(2).values
    gain = 8.0 * math.sqrt(c) / (2.0 * float(best[0] - best[1]))
    sd, a = base.sd, R.ATTENTION
    g = torch.Generator().manual_seed(170)
    sd[a + ".to_k.weight"] = (2.0 * torch.eye(c) + 0.05 * torch.randn((c, c), generator=g)).contiguous()
    sd[a + ".to_k.bias"] = 0.05 * torch.randn((c,), generator=g)
    sd[a + ".to_q.weight"] = (0.1 / math.sqrt(c)) * torch.randn((c, c), generator=g)
    sd[a + ".to_q.bias"] = (gain * d).float().contiguous()
    return base


def _tie_bias(k):
    """A float32 b with float32(float32(b / 2 + 0.5) * 255) == k + 0.5 exactly."""
    u0 = np.float32((k + 0.5) / 255.0)
    for step in range(-4, 5):
        u = np.float32(u0)
        for _ in range(abs(step)):
            u = np.nextafter(u, np.float32(2.0 if step > 0 else -2.0), dtype=np.float32)
        b = np.float32((u - np.float32(0.5)) * np.float32(2.0))
        if np.float32(np.float32(b / np.float32(2.0) + np.float32(0.5)) * np.float32(255.0)) == np.float32(k + 0.5):
            return float(b)
    raise AssertionError(f"no float32 bias gives the tie {k} + 0.5")


def _build(name):
    if name == "published_width":
        return _make(name, 11, (5, 7), {})
    if name == "two_levels":
        return _make(name, 12, (5, 7), SMALL)
    if name == "four_levels":
        return _make(name, 13, (3, 4), dict(block_out_channels=(8, 16, 16, 32), norm_num_groups=4, layers_per_block=1))
    if name == "odd_groups":
        return _make(name, 14, (5, 7), dict(block_out_channels=(24, 48), norm_num_groups=8, layers_per_block=2))
    if name == "many_chunks":
        return _make(name, 15, (9, 15), SMALL)
    if name == "late_maxima":
        return _late_maxima()
    if name == "offset_stats":
        case = _make(name, 16, (5, 7), SMALL)
        case.sd["decoder.mid_block.resnets.0.conv1.bias"] += 1000.0
        return case
    if name == "small_variance":
        case = _make(name, 18, (5, 7), SMALL)
        case.sd["decoder.conv_in.weight"] *= 0.003
        case.sd["decoder.conv_in.bias"] *= 0.003
        return case
    if name == "one_pixel":
        return _make(name, 19, (1, 1), dict(block_out_channels=(24, 48), norm_num_groups=8, layers_per_block=1))
    if name == "thin":
        return _make(name, 20, (1, 17), SMALL)
    if name == "rounding_ties":
        case = _make(name, 21, (3, 5), SMALL)
        case.sd["decoder.conv_out.weight"].zero_()
        case.sd["decoder.conv_out.bias"] = torch.tensor([_tie_bias(k) for k in TIE_LEVELS], dtype=torch.float32)
        return case
    raise KeyError(name)


NAMES = ("published_width", "two_levels", "four_levels", "odd_groups", "many_chunks", "late_maxima", "offset_stats", "small_variance",
         "one_pixel", "thin", "rounding_ties")


def by_name(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def z_of(case, dtype=torch.float64):
    """The decoder's input of a case: its latents divided by the scaling factor (in float64, then rounded to `dtype`)."""
    return (case.latents.double() / R.config(**case.cfg)["scaling_factor"]).to(dtype)


def reference(name):
    """(z float32, y64, tol) of `decode`: the float64 restatement on the float32 z, and 8 x the float32 restatement's error."""
    if name not in _refs:
        case = by_name(name)
        z = z_of(case, torch.float32)
        with torch.no_grad():
            y64 = R.decode(case.sd, z.double(), **case.cfg)
            y32 = R.decode(case.sd, z, **case.cfg)
        _refs[name] = (z, y64, 8.0 * float((y32.double() - y64).abs().max()))
    return _refs[name]


def frame_reference(name):
    """(latents, y64 [h s, w s, 3] before the clamp, tol) of `decode_latents_u8`."""
    if name not in _frame_refs:
        case = by_name(name)
        y64 = R.decode_latents_float(case.sd, case.latents, torch.float64, **case.cfg)
        y32 = R.decode_latents_float(case.sd, case.latents, torch.float32, **case.cfg)
        _frame_refs[name] = (case.latents, y64, 8.0 * float((y32.double() - y64).abs().max()))
    return _frame_refs[name]


def ties_expected_frame(case):
    """rounding_ties: the frame every sample of which is the tie of its channel rounded half to even, as float32 computes it."""
    h, w = case.latents.shape[2:]
    s = 2 ** (len(R.config(**case.cfg)["block_out_channels"]) - 1)
    b = case.sd["decoder.conv_out.bias"].numpy().astype(np.float32)
    v = (b / np.float32(2.0) + np.float32(0.5)).astype(np.float32) * np.float32(255.0)
    assert [float(x) for x in v] == [k + 0.5 for k in TIE_LEVELS]
    row = np.rint(v).astype(np.uint8)      # numpy rounds half to even
    return torch.from_numpy(np.broadcast_to(row, (h * s, w * s, 3)).copy())
