"""Crafted Swin2SR cases: tiny configurations with every tensor random (tests/swin2sr_ref.seeded_state_dict), each built to expose
one part of csrc/swin2sr.hip and named for the faults (swin2sr_ref.FAULTS) it is there to show.

  reconstruction   max |got - f64| <= tol,  tol = 8 x max |f32 CPU restatement - f64|, per case; nothing is fixed in advance
  u8 frame         got == the float64 route's u8 wherever the float64 value x 255 lies farther than 255 tol from a rounding
                   boundary, off by at most 1 elsewhere; at most MAX_THIN of the samples are left out (a condition on the seeds,
                   checked on the CPU by test_swin2sr_cases_host.py)

tests/test_swin2sr_cases_host.py checks on the CPU that the float32 restatement passes every case and that each fault, applied to
the float32 restatement, fails a case named for it by 10 x that case's tolerance; tests/test_gpu_swin2sr_cases.py runs the kernels
through the same criterion.

The later cases reach what the published shape (window 8, 180 channels, RGB) does not: windows of 2, 5, 6, 7 and 10, whose
token count is no multiple of 16 (phantom rows and keys in the attention kernel), odd windows, head dims of 4, 16 and 48, the
x3 and x4 direct heads, one channel, and a layer_norm_eps that differs from the patch embedding's.  SMALL_FRAMES are frames
shorter than the processor's padding; `rounding_ties` pins the u8 route's rounding mode exactly.

`window_12_frame` is the one case transformers itself cannot run (its patch_unembed is handed the unpadded size): a frame the
processor pads to 16 x 24 meets a window of 12, so the model's own reflect padding acts after the processor's symmetric one.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from tests import swin2sr_ref as R

MAX_THIN = 0.02
FRAMES = ((13, 18), (8, 8))          # upscale: both paddings and the crop; a multiple of 8, which the processor still pads by 8
# frames shorter than the processor's padding: the symmetric extension bounces more than once (1 x 1: every sample is the pixel)
SMALL_FRAMES = ((1, 1), (2, 3), (3, 17))
SMALL_FRAME_CASES = ("window_12_frame", "published_width")      # 8 x 8 -> 12 x 12 by the model's reflect padding; window 8


class Case:
    """name; cfg (Swin2SRConfig fields); sd (seeded state dict); x (pixel_values [1, num_channels, h, w] float32, h and w multiples
    of the window) or, for via == "upscale", frame ([h, w, 3] uint8 ndarray); faults: the faults the case is named for."""

    def __init__(self, name, cfg, sd, x=None, frame=None, faults=(), note=""):
        self.name, self.cfg, self.sd, self.x, self.frame = name, cfg, sd, x, frame
        self.faults, self.note = tuple(faults), note
        self.via = "upscale" if frame is not None else "forward"

    def pixel_values(self):
        return R.process_frame(self.frame, torch.float32) if self.via == "upscale" else self.x

    def __repr__(self):
        return self.name


def _cfg(embed, heads, depths, window, upsampler, upscale, image_size=64, mlp_ratio=2.0, img_range=1.0, num_channels=None, layer_norm_eps=None):
    cfg = dict(embed_dim=embed, num_heads=tuple(heads), depths=tuple(depths), window_size=window, upsampler=upsampler, upscale=upscale,
               image_size=image_size, mlp_ratio=mlp_ratio, img_range=img_range)
    if num_channels is not None:
        cfg["num_channels"] = num_channels
    if layer_norm_eps is not None:
        cfg["layer_norm_eps"] = layer_norm_eps
    return cfg


def _case(name, cfg, seed, h, w, faults, note):
    return Case(name, cfg, R.seeded_state_dict(seed, **cfg), x=R.seeded_input(h, w, seed, channels=cfg.get("num_channels", 3)), faults=faults,
                note=note)


def _clamp_and_bias():
    """One layer, one head.  logit_scale = ln 100 + 2: without the clamp every score is e^2 times too large.  The position-bias
    MLP's last weights are large, so 16 sigmoid(.) spans (0, 16) and an unsquashed bias is tens of units off; q and k weights are
    scaled down so that the cosines stay moderate and the softmax is not one-hot either way."""
    cfg = _cfg(32, (1,), (1,), 8, "pixelshuffledirect", 2, image_size=16)
    sd = R.seeded_state_dict(36, **cfg)
    a = "swin2sr.encoder.stages.0.layers.0.attention.self."
    sd[a + "logit_scale"].fill_(math.log(100.0) + 2.0)
    sd[a + "continuous_position_bias_mlp.2.weight"].mul_(4.0)
    return Case("clamp_and_bias", cfg, sd, x=R.seeded_input(8, 8, 36), faults=["no_clamp", "bias_unsquashed", "index_transposed"],
                note="8x8 tokens, one window; logit_scale ln 100 + 2; 16 sigmoid spans (0, 16)")


def _window_12_frame():
    cfg = _cfg(24, (2,), (2,), 12, "pixelshuffledirect", 2, image_size=24)
    sd = R.seeded_state_dict(37, **cfg)
    return Case("window_12_frame", cfg, sd, frame=R.seeded_frame(13, 18, 37), faults=["symmetric_pad", "single_bounce_pad"],
                note="upscale: 13x18 -> 16x24 (symmetric) -> 24x24 (reflect), window 12 (144 tokens a window)")


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        _case("small_shift", _cfg(24, (2, 2), (2, 2), 4, "pixelshuffle", 2, image_size=16), 31, 12, 20,
              ["no_shift", "shift_reversed", "no_mask", "regions_at_shift_only", "key_bias", "pre_norm", "long_residual_after_embed",
               "no_stage_residual", "gelu_tanh", "shuffle_order", "mean_not_added", "lrelu_swapped"],
              "12x20 tokens, 3x5 windows of 4, both axes masked; two stages"),
        _case("one_window_high", _cfg(60, (6,), (2,), 8, "pixelshuffledirect", 2), 32, 8, 24,
              ["no_shift", "shift_reversed", "no_mask", "regions_at_shift_only", "shuffle_order"],
              "8x24 tokens, 1x3 windows of 8: the roll wraps one window row onto itself; head dim 10"),
        _case("published_width", _cfg(180, (6, 6), (2, 2), 8, "nearest+conv", 4), 33, 16, 24,
              ["lrelu_swapped", "key_bias", "gelu_tanh", "no_stage_residual", "ln_unbiased", "ln_padded_width", "single_bounce_pad"],
              "16x24 tokens; embed 180 (head dim 30), hidden 360; nearest+conv x4"),
        _case("odd_depth_x4", _cfg(36, (3,), (3,), 4, "pixelshuffle", 4), 34, 8, 12,
              ["shuffle_order", "shift_reversed", "pre_norm"],
              "8x12 tokens; depth 3 (ends unshifted after a shifted layer); two shuffle steps"),
        _case("x3_range255", _cfg(32, (4,), (2,), 4, "pixelshuffle", 3, img_range=255.0), 35, 8, 8,
              ["shuffle_order", "mean_not_added", "long_residual_after_embed"],
              "8x8 tokens; the 9C shuffle; img_range 255"),
        _clamp_and_bias(),
        _window_12_frame(),
        # windows whose token count is no multiple of 16 (phantom rows and keys), odd windows, head dims below 8, of 16 and above 32
        _case("window_6_wide", _cfg(128, (4,), (2,), 6, "pixelshuffledirect", 3, image_size=32), 40, 12, 18,
              ["phantom_keys_unmasked", "no_mask", "shuffle_order"],
              "12x18 tokens, 2x3 windows of 6: 36 tokens in 48 rows, three m-tiles against eight n-tiles; x3 direct, 27 channels in 32"),
        _case("window_7_odd", _cfg(40, (5,), (3,), 7, "pixelshuffle", 2, image_size=32), 41, 14, 21,
              ["shift_rounded_up", "phantom_keys_unmasked", "shift_reversed", "ln_padded_width"],
              "14x21 tokens, 2x3 windows of 7: 49 tokens in 64 rows; shift 3; head dim 8"),
        _case("window_10_one_high", _cfg(64, (4,), (2,), 10, "pixelshuffledirect", 4, image_size=32), 42, 10, 20,
              ["phantom_keys_unmasked", "no_mask", "shuffle_order"],
              "10x20 tokens, 1x2 windows of 10: 100 tokens in 112 rows, seven m-tiles (4 + 3); head dim 16; x4 direct, 48 channels"),
        _case("window_5_one_head", _cfg(48, (1,), (2,), 5, "pixelshuffledirect", 2, image_size=32, mlp_ratio=1.5), 43, 10, 15,
              ["phantom_keys_unmasked", "shift_rounded_up"],
              "10x15 tokens, 2x3 windows of 5: 25 tokens in 32 rows; one head of 48; hidden 72 in 80"),
        _case("window_2_many_heads", _cfg(24, (6,), (2,), 2, "pixelshuffledirect", 2, image_size=32), 44, 6, 4,
              ["phantom_keys_unmasked", "no_shift", "ln_unbiased"],
              "6x4 tokens, 3x2 windows of 2: 4 tokens in 16 rows; shift 1; head dim 4"),
        _case("one_window_shifted", _cfg(32, (2,), (2,), 8, "pixelshuffledirect", 2, image_size=32), 45, 8, 8,
              ["no_mask"],
              "8x8 tokens, one window of 8 with a shifted layer: the roll wraps it onto itself on both axes, four regions inside it"),
        _case("gray", _cfg(24, (2,), (2,), 4, "pixelshuffle", 2, image_size=32, num_channels=1), 46, 8, 12,
              ["gray_mean_kept", "ln_unbiased", "ln_padded_width"],
              "8x12 tokens; one input and one output channel, zero mean"),
        _case("eps_1e-2", _cfg(24, (2,), (2,), 4, "pixelshuffledirect", 2, image_size=32, layer_norm_eps=1e-2), 47, 8, 12,
              ["embed_eps_from_config", "eps_default_everywhere"],
              "8x12 tokens; layer_norm_eps 1e-2 against the patch embedding's 1e-5"),
    ]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)


def forward_cases():
    return tuple(c for c in cases() if c.via == "forward")


def frame_cases():
    """The cases whose configuration takes an RGB frame: nesr_swin2sr_upscale_u8 refuses any other channel count."""
    return tuple(c for c in cases() if c.cfg.get("num_channels", 3) == 3)


# ------------------------------------------------------------------------------------------------ rounding ties of the u8 route
# [channel][r1][r2]: the k of a sample that lands on k + 0.5 exactly, even and odd; "low" and "high" leave [0, 1] for the clamp
TIE_K = (((64, 101), (200, "low")), ((77, 128), (253, 150)), ((41, 96), (187, "high")))


def _neighbours(v, steps=4):
    out, lo, hi = [v], v, v
    for _ in range(steps):
        lo, hi = np.nextafter(lo, np.float32(-9)), np.nextafter(hi, np.float32(9))
        out += [lo, hi]
    return out


def tie_bias(k, cc):
    """A float32 bias b with float32(float32(b + mean[cc]) x 255) == k + 0.5 exactly, or None: a float32 search among the
    neighbours of (k + 0.5) / 255 and of their difference to the mean."""
    mean = np.float32(R.RGB_MEAN[cc])
    for v in _neighbours(np.float32((k + 0.5) / 255.0)):
        if np.float32(v * np.float32(255.0)) != np.float32(k + 0.5):
            continue
        for b in _neighbours(np.float32(v - mean)):
            if np.float32(b + mean) == v:
                return float(b)
    return None


@functools.lru_cache(maxsize=None)
def rounding_ties():
    """Not one of cases(): upsample.conv.weight is zero, so every output sample is its bias: (bias + mean) x 255 is k + 0.5 exactly
    in float32 (TIE_K), where round-half-to-even and round-half-up part.  case.expected: the u8 value [3][2][2] of each channel and
    sub-pixel: k for an even k, k + 1 for an odd one, 0 and 255 behind the clamp."""
    cfg = _cfg(24, (2,), (1,), 4, "pixelshuffledirect", 2, image_size=16)
    sd = R.seeded_state_dict(48, **cfg)
    sd["upsample.conv.weight"].zero_()
    bias, expected = sd["upsample.conv.bias"], torch.zeros(3, 2, 2, dtype=torch.uint8)
    for cc in range(3):
        for r1 in range(2):
            for r2 in range(2):
                k = TIE_K[cc][r1][r2]
                if isinstance(k, str):
                    b, want = (-0.75, 0) if k == "low" else (0.875, 255)
                else:
                    b, want = tie_bias(k, cc), k + (k & 1)
                    assert b is not None, (k, cc)
                bias[(cc * 2 + r1) * 2 + r2] = b
                expected[cc, r1, r2] = want
    case = Case("rounding_ties", cfg, sd, frame=R.seeded_frame(5, 7, 48), note="5x7 frame; every sample a rounding tie or clamped")
    case.expected = expected
    return case


def ties_expected_frame(case):
    """[2 h, 2 w, 3] uint8: case.expected laid out by the PixelShuffle."""
    h, w = case.frame.shape[:2]
    return case.expected.permute(1, 2, 0).repeat(h, w, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the criterion
@functools.lru_cache(maxsize=None)
def reference(case):
    """(float64 reconstruction, the float32 CPU restatement's, tol = 8 x max |f32 - f64|), computed once per case."""
    x = case.pixel_values()
    with torch.no_grad():
        y64 = R.swin2sr_forward(case.sd, x.double(), **case.cfg)
        y32 = R.swin2sr_forward(case.sd, x, **case.cfg)
    return y64, y32, 8 * float((y32.double() - y64).abs().max())


def error(got, case):
    """(max |got - f64|, tol)."""
    y64, _, tol = reference(case)
    assert tuple(got.shape) == tuple(y64.shape), (tuple(got.shape), tuple(y64.shape))
    return float((got.double().cpu() - y64).abs().max()), tol


@functools.lru_cache(maxsize=None)
def frame_reference(name, hw):
    """The frame-level route of case `name`'s configuration on the seeded frame of size hw: (frame uint8 ndarray, float64 output
    [H s, W s, 3] before the clamp, tol = 8 x max |f32 - f64| of that output)."""
    case = by_name(name)
    frame = case.frame if (case.via == "upscale" and hw == tuple(case.frame.shape[:2])) else R.seeded_frame(hw[0], hw[1], 50 + hw[0])
    y64 = R.upscale_float(case.sd, frame, torch.float64, **case.cfg)
    y32 = R.upscale_float(case.sd, frame, torch.float32, **case.cfg)
    return frame, y64, 8 * float((y32.double() - y64).abs().max())
