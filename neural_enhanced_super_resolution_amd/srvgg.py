"""``SRVGGNetCompact`` drop-in: same constructor, state_dict key names and call signature as upstream
``realesrgan.archs.srvgg_arch.SRVGGNetCompact``, the network of the realesr-general-x4v3 (with its -wdn twin for denoise
strength) and realesr-animevideov3 checkpoints the reference fetches (standalone/download-x3-model.py:77-116)::

    body = conv3x3(in, F), act, (conv3x3(F, F), act) x num_conv, conv3x3(F, out * s * s)
    out  = pixel_shuffle(body(x), s) + nearest_upsample(x, s)

As with :class:`RRDBNet`, the module owns ordinary torch Parameters under upstream's names (``body.{2i}.weight/bias`` for
the convs, ``body.{2i+1}.weight`` [F] for each PReLU) and its ``forward`` is the HIP path in libnesr_hip.so
(srvgg_compact.hip, one launch per layer).  There is no torch/CPU implementation of forward here: a non-CUDA input raises.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch
from torch import nn

from . import _lib
from ._contexts import _HipNet
from .rrdbnet import _ConvParams

ACT_TYPES = {"prelu": _lib.ACT_PRELU, "relu": _lib.ACT_RELU, "leakyrelu": _lib.ACT_LEAKYRELU}


def srvgg_state_dict_spec(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type="prelu"):
    """Ordered {key: shape} of an SRVGGNetCompact checkpoint (101 tensors for x4v3, 53 for animevideov3)."""
    if act_type not in ACT_TYPES:
        raise ValueError(f"act_type {act_type!r}: expected one of {sorted(ACT_TYPES)}")
    spec = OrderedDict()
    i = 0

    def conv(cin, cout):
        nonlocal i
        spec[f"body.{i}.weight"] = (cout, cin, 3, 3)
        spec[f"body.{i}.bias"] = (cout,)
        i += 1

    def act():
        nonlocal i
        if act_type == "prelu":
            spec[f"body.{i}.weight"] = (num_feat,)
        i += 1

    conv(num_in_ch, num_feat)
    act()
    for _ in range(num_conv):
        conv(num_feat, num_feat)
        act()
    conv(num_feat, num_out_ch * upscale * upscale)
    return spec


class _PReLUParams(nn.Module):
    """Parameter holder of one PReLU (``weight`` [F], torch's default 0.25).  Not callable."""

    def __init__(self, num_feat):
        super().__init__()
        self.weight = nn.Parameter(torch.full((num_feat,), 0.25), requires_grad=False)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("_PReLUParams holds weights only; SRVGGNetCompact.forward runs in libnesr_hip.so")


class _NoParams(nn.Module):
    """ReLU / LeakyReLU(0.1): no tensors, but they take a body index as upstream's modules do."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("SRVGGNetCompact.forward runs in libnesr_hip.so")


class SRVGGNetCompact(_HipNet):
    """Compact VGG-style super-resolution network (Real-ESRGAN's realesr-*-v3 models).

    Args mirror upstream: num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type='prelu'.
    Extra keyword ``compute_dtype``: "f32" (default; operands as f16 pairs, three f16 MFMAs per product, values beyond
    +-65504 raise NesrRangeError), "bf16" (what ``.half()`` / ``.to(torch.bfloat16)`` select, as for RRDBNet) or "fp16"
    (f16 storage and MFMA operands, f32 accumulation: upstream's half=True numerics at one MFMA per product.  Opt-in: a
    model built with it stays fp16 through ``.half()`` / ``.to(torch.float16)`` / ``RealESRGANer(half=True)``, any other
    model keeps turning bf16 there.  The range contract of "f32" holds: a weight beyond +-65504 is refused at upload, an
    input or activation beyond it makes the float output NaN and raises NesrRangeError at check_range()).  The spelling
    is "fp16" only: "f16", which RRDBNet also takes, stays a ValueError here.
    The HIP path supports num_feat 64, num_in_ch == num_out_ch == 3 and upscale 2 or 4.
    The contexts, replicas, forward calls and range checks are _HipNet's (the C ABI is RRDBNet's; only creation differs).
    """

    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type="prelu", compute_dtype="f32"):
        super().__init__()
        if act_type not in ACT_TYPES:
            raise ValueError(f"act_type {act_type!r}: expected one of {sorted(ACT_TYPES)}")
        self.num_in_ch = num_in_ch
        self.num_out_ch = num_out_ch
        self.num_feat = num_feat
        self.num_conv = num_conv
        self.upscale = upscale
        self.act_type = act_type
        self.compute_dtype = compute_dtype
        self._dtype_code()   # a bad compute_dtype fails here, not at the first forward
        mods = [_ConvParams(num_in_ch, num_feat), self._act()]
        for _ in range(num_conv):
            mods += [_ConvParams(num_feat, num_feat), self._act()]
        mods.append(_ConvParams(num_feat, num_out_ch * upscale * upscale))
        self.body = nn.ModuleList(mods)

    def _act(self):
        return _PReLUParams(self.num_feat) if self.act_type == "prelu" else _NoParams()

    def _dtype_code(self):
        if self.compute_dtype in ("f32", "fp32", torch.float32, "f32-split", "split"):
            return _lib.DTYPE_F32_SPLIT
        if self.compute_dtype in ("bf16", torch.bfloat16, "half", torch.float16):
            return _lib.DTYPE_BF16
        if self.compute_dtype == "fp16":
            return _lib.DTYPE_F16               # f16 operands on the f16 matrix cores, range-checked (|x| <= 65504)
        raise ValueError(f"compute_dtype {self.compute_dtype!r}: expected 'f32', 'bf16' or 'fp16'")

    def _to_bf16(self):
        """As _HipNet's, but a model built with compute_dtype="fp16" stays fp16 (upstream's fp16 run)."""
        if self.compute_dtype != "fp16":
            self.compute_dtype = "bf16"

    def _create(self, index, code):
        handle = ctypes.c_void_p()
        _lib.check(_lib.load().nesr_create_compact(ctypes.byref(handle), index, self.num_in_ch, self.num_out_ch, self.num_feat,
                                                   self.num_conv, self.upscale, ACT_TYPES[self.act_type], code), "nesr_create_compact")
        return handle

    def out_scale(self):
        return self.upscale

    def forward_flops(self, n, h, w):
        """Algorithmic FLOPs (2 x MACs) of one forward on [n, *, h, w]."""
        f = self.num_feat
        macs = 9 * (self.num_in_ch * f + self.num_conv * f * f + f * self.num_out_ch * self.upscale ** 2)
        return 2.0 * macs * n * h * w
