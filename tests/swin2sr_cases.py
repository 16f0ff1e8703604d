"""Crafted Swin2SR cases: tiny configurations with every tensor random (tests/swin2sr_ref.seeded_state_dict), each built to expose
one part of csrc/swin2sr.hip and named for the faults (swin2sr_ref.FAULTS) it is there to show.

  reconstruction   max |got - f64| <= tol,  tol = 8 x max |f32 CPU restatement - f64|, per case; nothing is fixed in advance
  u8 frame         got == the float64 route's u8 wherever the float64 value x 255 lies farther than 255 tol from a rounding
                   boundary, off by at most 1 elsewhere; at most MAX_THIN of the samples are left out (a condition on the seeds,
                   checked on the CPU by test_swin2sr_cases_host.py)

tests/test_swin2sr_cases_host.py checks on the CPU that the float32 restatement passes every case and that each fault, applied to
the float32 restatement, fails a case named for it by 10 x that case's tolerance; tests/test_gpu_swin2sr_cases.py runs the kernels
through the same criterion.

`window_12_frame` is the one case transformers itself cannot run (its patch_unembed is handed the unpadded size): a frame the
processor pads to 16 x 24 meets a window of 12, so the model's own reflect padding acts after the processor's symmetric one.
"""
from __future__ import annotations

import functools
import math

import torch

from tests import swin2sr_ref as R

MAX_THIN = 0.02
FRAMES = ((13, 18), (8, 8))          # upscale: both paddings and the crop; a multiple of 8, which the processor still pads by 8


class Case:
    """name; cfg (Swin2SRConfig fields); sd (seeded state dict); x (pixel_values [1, 3, h, w] float32, h and w multiples of the
    window) or, for via == "upscale", frame ([h, w, 3] uint8 ndarray); faults: the faults the case is named for."""

    def __init__(self, name, cfg, sd, x=None, frame=None, faults=(), note=""):
        self.name, self.cfg, self.sd, self.x, self.frame = name, cfg, sd, x, frame
        self.faults, self.note = tuple(faults), note
        self.via = "upscale" if frame is not None else "forward"

    def pixel_values(self):
        return R.process_frame(self.frame, torch.float32) if self.via == "upscale" else self.x

    def __repr__(self):
        return self.name


def _cfg(embed, heads, depths, window, upsampler, upscale, image_size=64, mlp_ratio=2.0, img_range=1.0):
    return dict(embed_dim=embed, num_heads=tuple(heads), depths=tuple(depths), window_size=window, upsampler=upsampler, upscale=upscale,
                image_size=image_size, mlp_ratio=mlp_ratio, img_range=img_range)


def _case(name, cfg, seed, h, w, faults, note):
    return Case(name, cfg, R.seeded_state_dict(seed, **cfg), x=R.seeded_input(h, w, seed), faults=faults, note=note)


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
    return Case("window_12_frame", cfg, sd, frame=R.seeded_frame(13, 18, 37), faults=["symmetric_pad"],
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
              ["lrelu_swapped", "key_bias", "gelu_tanh", "no_stage_residual"],
              "16x24 tokens; embed 180 (head dim 30), hidden 360; nearest+conv x4"),
        _case("odd_depth_x4", _cfg(36, (3,), (3,), 4, "pixelshuffle", 4), 34, 8, 12,
              ["shuffle_order", "shift_reversed", "pre_norm"],
              "8x12 tokens; depth 3 (ends unshifted after a shifted layer); two shuffle steps"),
        _case("x3_range255", _cfg(32, (4,), (2,), 4, "pixelshuffle", 3, img_range=255.0), 35, 8, 8,
              ["shuffle_order", "mean_not_added", "long_residual_after_embed"],
              "8x8 tokens; the 9C shuffle; img_range 255"),
        _clamp_and_bias(),
        _window_12_frame(),
    ]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)


def forward_cases():
    return tuple(c for c in cases() if c.via == "forward")


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
