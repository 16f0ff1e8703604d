"""The specification of Swin2SR's fp16 compute form (``Swin2SR(compute_dtype="fp16")``, csrc/swin2sr.hip): tests/swin2sr_ref.py run
unchanged under a hook that rounds both operands of every GEMM to 16 bits and leaves everything else in the dtype it is handed.

The hook is a ``TorchFunctionMode``.  It rounds (to nearest even, ``t.to(rounding).to(t.dtype)``) the input and the weight of
``F.linear``, of ``F.conv2d`` with more than 4 input channels (the frame-loading first convolution stays unrounded) and both
operands of ``matmul`` (q^ k^T: q^ and k^ are normalised first, then rounded; P V: P is the softmax, then rounded).  Biases, the
normalisation, temperature, bias table, mask, softmax, GELU, LayerNorm and the residuals are untouched; ``position_bias`` (an
F.linear MLP that does not depend on the input and is computed on the host in double) runs with the hook off.  Products of two
16-bit values are exact in float32, so in float64 the emulation is the form's exact arithmetic with exact sums, and in float32 it
is the same with float32 sums in torch's order.

``rounding=torch.float64`` changes nothing: the result has swin2sr_ref's bits (tests/test_swin2sr_f16_host.py).

FAULTS name deliberate departures from the specification; each must fail a (case, part) named for it:
  unrounded              no operand is rounded (the f32 form)
  bf16                   operands rounded to bfloat16
  weights_unrounded      the weights of F.linear / F.conv2d stay unrounded
  activations_unrounded  only those weights are rounded
  qk_unrounded           scores from the unrounded q^ and k^
  p_unrounded            P V from the unrounded softmax (V still rounded)
  gelu_unrounded         fc2 takes the unrounded GELU output
  first_conv_rounded     the first convolution's operands rounded too

The three parts are one launch each of the kernels (``Swin2SR.part``): an attention block, an MLP block, a stage's 3x3 conv, on
tokens [N, H, W, C]; `layer_in_two_parts` shows that attention then mlp is swin2sr_ref.layer.
"""
from __future__ import annotations

import contextlib
import functools

import torch
import torch.nn.functional as F
from torch.overrides import TorchFunctionMode

from tests import swin2sr_ref as R

FAULTS = ("unrounded", "bf16", "weights_unrounded", "activations_unrounded", "qk_unrounded", "p_unrounded", "gelu_unrounded", "first_conv_rounded")
PARTS = ("attention", "mlp", "stage_conv")
_MATMULS = (torch.matmul, torch.Tensor.matmul, torch.Tensor.__matmul__)


class Rounding(TorchFunctionMode):
    def __init__(self, rounding=torch.float16, fault=None):
        super().__init__()
        assert fault is None or fault in FAULTS, fault
        if fault == "unrounded":
            rounding = None
        elif fault == "bf16":
            rounding = torch.bfloat16
        self.rounding, self.fault, self.on = rounding, fault, True
        self.matmuls = 0            # even: q^ k^T, odd: P V (swin2sr_ref has no other matmul)
        self.gelu_out = None

    def rnd(self, t):
        return t if self.rounding is None else t.to(self.rounding).to(t.dtype)

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if not self.on:
            return func(*args, **kwargs)
        act = (lambda t: t) if self.fault == "activations_unrounded" else self.rnd
        wgt = (lambda t: t) if self.fault == "weights_unrounded" else self.rnd
        if func is F.gelu:
            self.gelu_out = func(*args, **kwargs)
            return self.gelu_out
        if func is F.linear:
            x, w, *rest = args
            if self.fault == "gelu_unrounded" and x is self.gelu_out:
                return func(x, wgt(w), *rest, **kwargs)
            return func(act(x), wgt(w), *rest, **kwargs)
        if func is F.conv2d:
            x, w, *rest = args
            if w.shape[1] > 4 or self.fault == "first_conv_rounded":
                return func(act(x), wgt(w), *rest, **kwargs)
            return func(*args, **kwargs)
        if func in _MATMULS:
            a, b = args
            pv = self.matmuls % 2 == 1
            self.matmuls += 1
            if self.fault == "qk_unrounded" and not pv:
                return func(a, b)
            if self.fault == "p_unrounded" and pv:
                return func(a, act(b))
            return func(act(a), act(b))
        return func(*args, **kwargs)


@contextlib.contextmanager
def hooked(rounding=torch.float16, fault=None):
    """swin2sr_ref under the rounding hook; position_bias runs with the hook off."""
    mode = Rounding(rounding, fault)
    plain = R.position_bias

    def position_bias(*a, **k):
        mode.on = False
        try:
            return plain(*a, **k)
        finally:
            mode.on = True

    R.position_bias = position_bias
    try:
        with torch.no_grad(), mode:
            yield mode
    finally:
        R.position_bias = plain


def forward(sd, pixel_values, rounding=torch.float16, fault=None, **cfg):
    """swin2sr_ref.swin2sr_forward in pixel_values' dtype with the GEMM operands rounded."""
    with hooked(rounding, fault):
        return R.swin2sr_forward(sd, pixel_values, **cfg)


def upscale_float(sd, frame, dtype=torch.float64, rounding=torch.float16, fault=None, **cfg):
    with hooked(rounding, fault):
        return R.upscale_float(sd, frame, dtype, **cfg)


def _params(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items() if v.dtype.is_floating_point}


def _attention(p, l, x, h, w, ws, shift, heads, eps):
    """The first half of swin2sr_ref.layer: x [h w, C] -> x + LayerNorm(output.dense(window attention))."""
    C = x.shape[-1]
    img = x.view(h, w, C)
    if shift > 0:
        img = torch.roll(img, shifts=(-shift, -shift), dims=(0, 1))
    xw = img.view(h // ws, ws, w // ws, ws, C).transpose(1, 2).reshape(-1, ws * ws, C)
    mask = R.region_mask(h, w, ws, shift, x.dtype) if shift > 0 else None
    ctx = R.window_attention(p, l + ".attention.self", xw, mask, ws, heads)
    o = F.linear(ctx, p[l + ".attention.output.dense.weight"], p[l + ".attention.output.dense.bias"])
    o = o.view(h // ws, w // ws, ws, ws, C).transpose(1, 2).reshape(h, w, C)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(0, 1))
    return x + R.layer_norm(o.reshape(h * w, C), C, p[l + ".layernorm_before.weight"], p[l + ".layernorm_before.bias"], eps)


def _mlp(p, l, x, eps):
    """The second half: x + LayerNorm(fc2(GELU(fc1(x))))."""
    C = x.shape[-1]
    y = F.linear(F.gelu(F.linear(x, p[l + ".intermediate.dense.weight"], p[l + ".intermediate.dense.bias"])), p[l + ".output.dense.weight"],
                 p[l + ".output.dense.bias"])
    return x + R.layer_norm(y, C, p[l + ".layernorm_after.weight"], p[l + ".layernorm_after.bias"], eps)


def part(name, sd, stage, layer, tokens, rounding=torch.float16, fault=None, **cfg):
    """What Swin2SR.part(name, stage, layer, tokens) computes: tokens [N, H, W, C] in any float dtype -> the same shape."""
    assert name in PARTS, name
    c = R.config(**cfg)
    n, h, w, C = tokens.shape
    ws, heads, eps = c["window_size"], c["num_heads"][stage], c["layer_norm_eps"]
    p = _params(sd, tokens.dtype)
    s = f"swin2sr.encoder.stages.{stage}"
    l = f"{s}.layers.{layer}"
    out = []
    with hooked(rounding, fault):
        for i in range(n):
            x = tokens[i].reshape(h * w, C)
            if name == "attention":
                y = _attention(p, l, x, h, w, ws, ws // 2 if layer % 2 else 0, heads, eps)
            elif name == "mlp":
                y = _mlp(p, l, x, eps)
            else:
                y = F.conv2d(x.t().reshape(1, C, h, w), p[s + ".conv.weight"], p[s + ".conv.bias"], padding=1).flatten(2).transpose(1, 2)[0]
            out.append(y.reshape(h, w, C))
    return torch.stack(out)


def layer_in_two_parts(sd, stage, layer, tokens, **cfg):
    """(attention then mlp by `part`, swin2sr_ref.layer) on tokens [1, H, W, C], nothing rounded: the same bits."""
    c = R.config(**cfg)
    _, h, w, C = tokens.shape
    two = part("mlp", sd, stage, layer, part("attention", sd, stage, layer, tokens, torch.float64, **cfg), torch.float64, **cfg)
    l = f"swin2sr.encoder.stages.{stage}.layers.{layer}"
    with torch.no_grad():
        one = R.layer(_params(sd, tokens.dtype), l, tokens[0].reshape(h * w, C), h, w, c["window_size"], c["window_size"] // 2 if layer % 2 else 0,
                      c["num_heads"][stage], c["layer_norm_eps"])
    return two[0].reshape(h * w, C), one


def first_conv(sd, pixel_values, rounding=torch.float16, fault=None, **cfg):
    """first_convolution on the normalised input (H, W multiples of the window), which the form leaves unrounded: [1, C, H, W]."""
    c = R.config(**cfg)
    dt = pixel_values.dtype
    rgb = c["num_channels"] == 3 and c["num_channels_out"] == 3
    mean = torch.tensor(R.RGB_MEAN if rgb else (0.0,), dtype=torch.float32).to(dt).view(1, -1, 1, 1)
    with hooked(rounding, fault):
        return F.conv2d((pixel_values - mean) * c["img_range"], sd["swin2sr.first_convolution.weight"].to(dt), sd["swin2sr.first_convolution.bias"].to(dt),
                        padding=1)


# ------------------------------------------------------------------------------------------------ the criterion
def part_layer(case, name):
    """The layer a case's part is checked on: the second (shifted) attention block where the stage has one, the first MLP."""
    return min(1, case.cfg["depths"][0] - 1) if name == "attention" else 0


@functools.lru_cache(maxsize=None)
def part_reference(case, name):
    """(tokens [1, h, w, C] float32, layer, the float64 emulation, tol = 8 x max |emulation in float32 - emulation in float64|) of
    part `name` of stage 0 on the case's seeded tokens; "first_conv" takes the case's pixel values instead."""
    if name == "first_conv":
        e64, e32 = first_conv(case.sd, case.x.double(), **case.cfg), first_conv(case.sd, case.x, **case.cfg)
        return case.x, 0, e64, 8 * float((e32.double() - e64).abs().max())
    tokens, layer = seeded_tokens(case), part_layer(case, name)
    e64 = part(name, case.sd, 0, layer, tokens.double(), **case.cfg)
    e32 = part(name, case.sd, 0, layer, tokens, **case.cfg)
    return tokens, layer, e64, 8 * float((e32.double() - e64).abs().max())


def part_fault(case, name, fault):
    """max |the faulty emulation in float32 - the float64 emulation| of a (case, part)."""
    tokens, layer, e64, _ = part_reference(case, name)
    if name == "first_conv":
        y = first_conv(case.sd, tokens, fault=fault, **case.cfg)
    else:
        y = part(name, case.sd, 0, layer, tokens, fault=fault, **case.cfg)
    return float((y.double() - e64).abs().max())


@functools.lru_cache(maxsize=None)
def network_reference(case):
    """(float64 unrounded reconstruction, the float64 emulation, bound) of the whole network on the case's input, where
    bound = max |emulation64 - unrounded64| + 8 x max |emulation32 - emulation64|: the form's own distance from the exact
    network plus the float32 noise of evaluating it.  A bound, not a pin: an activation within a float32 error of an f16 rounding
    boundary rounds the other way and the layers after it amplify the flip, so no per-value pin of the whole network holds."""
    x = case.pixel_values()
    with torch.no_grad():
        y64 = R.swin2sr_forward(case.sd, x.double(), **case.cfg)
    e64, e32 = forward(case.sd, x.double(), **case.cfg), forward(case.sd, x, **case.cfg)
    return y64, e64, float((e64 - y64).abs().max()) + 8 * float((e32.double() - e64).abs().max())


def seeded_tokens(case, seed=7, n=1):
    """N(0, 1) tokens [n, h, w, C] float32 of the case's token grid, the same for a seed."""
    _, _, h, w = case.x.shape
    return torch.randn((n, h, w, case.cfg["embed_dim"]), generator=torch.Generator().manual_seed(seed)).float()
