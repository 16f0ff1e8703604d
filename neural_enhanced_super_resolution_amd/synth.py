"""Seeded synthetic weights and frames.

No checkpoint ships with the reference (models/weights/RealESRGAN_x2plus.pth is stripped,
/root/reference/.MISSING_LARGE_BLOBS) and there is no network, so benches, smoke and parity
tests use weights drawn from a seeded numpy PCG64 stream (bit-reproducible across hosts)
with upstream's init statistics: basicsr ``default_init_weights(scale=0.1)`` = kaiming-normal
x 0.1 for the dense-block convs, torch's default Conv2d init elsewhere.  ``rdb_gain`` scales the
dense-block weights so that the 23-block trunk contributes visibly to the output (the parity
tests would be blind to trunk errors with an all-but-identity trunk).

Frames follow SURVEY.md section 8(d): uint8 noise smoothed by a 5x5 box.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

from .rrdbnet import rrdbnet_state_dict_spec


def synthetic_state_dict(seed=0, num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23,
                         num_grow_ch=32, rdb_gain=0.1 * 4.0, bias_std=0.02):
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    spec = rrdbnet_state_dict_spec(num_in_ch, num_out_ch, scale, num_feat, num_block, num_grow_ch)
    for key, shape in spec.items():
        if key.endswith(".weight"):
            fan_in = shape[1] * 9
            if key.startswith("body."):
                std = rdb_gain * math.sqrt(2.0 / fan_in)          # kaiming_normal_(a=0) * scale
                w = rng.standard_normal(shape, dtype=np.float32) * np.float32(std)
            else:
                bound = 1.0 / math.sqrt(fan_in)                    # kaiming_uniform_(a=sqrt(5))
                w = rng.uniform(-bound, bound, size=shape).astype(np.float32)
            sd[key] = torch.from_numpy(w)
        else:
            sd[key] = torch.from_numpy((rng.standard_normal(shape, dtype=np.float32) * np.float32(bias_std)))
    if num_out_ch == 3:
        # centre the output in the displayable range so clamp/quantise paths see real variation
        sd["conv_last.bias"] = sd["conv_last.bias"] + 0.5
    return sd


def synthetic_frame(h, w, seed=0, channels=3):
    """uint8 HWC BGR frame: uniform noise smoothed by a 5x5 box (edge-replicated)."""
    rng = np.random.default_rng(1000 + seed)
    shape = (h, w, channels) if channels else (h, w)
    x = rng.integers(0, 256, size=shape, dtype=np.uint8).astype(np.float32)
    pad = [(2, 2), (2, 2)] + ([(0, 0)] if channels else [])
    xp = np.pad(x, pad, mode="edge")
    acc = np.zeros_like(x)
    for dy in range(5):
        for dx in range(5):
            acc += xp[dy:dy + h, dx:dx + w]
    # stretch back to a wide range: box-filtered noise has std ~ 74/5
    y = (acc / 25.0 - 127.5) * 4.0 + 127.5
    return np.clip(np.rint(y), 0, 255).astype(np.uint8)


def synthetic_compact_state_dict(seed=0, num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type="prelu",
                                 slope_range=(0.1, 0.3), bias_std=0.02, tail_gain=0.25):
    """Seeded weights for SRVGGNetCompact (upstream key names).  torch's default init shrinks the signal about 5x in
    variance per PReLU layer, which would leave the tests blind to errors in a 32-layer body; here every conv is
    kaiming-normal for its activation's negative slope (the body keeps its scale), PReLU slopes are drawn per channel in
    `slope_range`, the weights are zero-mean (about half of every layer's pre-activations are negative, so the slope path
    runs), and the tail is kaiming x `tail_gain` so the learned residual is clearly visible on top of the upsampled input."""
    from .srvgg import srvgg_state_dict_spec
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    spec = srvgg_state_dict_spec(num_in_ch, num_out_ch, num_feat, num_conv, upscale, act_type)
    last = f"body.{2 * (num_conv + 1)}.weight"
    slope = {"prelu": 0.5 * (slope_range[0] + slope_range[1]), "relu": 0.0, "leakyrelu": 0.1}[act_type]
    for key, shape in spec.items():
        if len(shape) == 4:
            fan_in = shape[1] * 9
            std = math.sqrt(2.0 / ((1.0 + slope * slope) * fan_in))
            if key == last:
                std = tail_gain * math.sqrt(1.0 / fan_in)
            sd[key] = torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * np.float32(std))
        elif key.endswith(".bias"):
            sd[key] = torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * np.float32(bias_std))
        else:   # PReLU slopes
            sd[key] = torch.from_numpy(rng.uniform(slope_range[0], slope_range[1], size=shape).astype(np.float32))
    return sd
