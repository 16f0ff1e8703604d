"""The specification of the UNet's fp16 compute form (``UNet2DCondition(compute_dtype="fp16")``, csrc/unet_f16.hip):
tests/unet_ref.py's forward, unchanged, under a hook that rounds both operands of the form's products to f16 and leaves
everything else in the dtype it is handed.

The hook is a ``TorchFunctionMode``.  It rounds (to nearest even, ``t.to(rounding).to(t.dtype)``) the input and the weight of every
``F.conv2d`` and of those ``F.linear`` calls whose weight is one of the GEMM weights it is given (by key of the state dict:
every weight matrix except ``time_embedding.*`` and ``*.time_emb_proj.*``, which are M = 1 products on plain FMAs).  The ``@`` of
the attention is not intercepted; biases, residuals, GEGLU's product, the norms and the embedding are untouched.  unet_ref applies
GroupNorm (+ SiLU) and LayerNorm before the product's call, so the activation is rounded after its prologue, and F.conv2d pads
with zeros after that.  Products of two f16 values are exact in float32, so in float64 the emulation is the form's exact
arithmetic with exact sums, and in float32 it is the same with float32 sums in torch's order.

``rounding=torch.float64`` changes nothing: the result has unet_ref's bits (tests/test_unet_f16_host.py).
``subnormals="flushed"`` replaces an operand that rounded to an f16 subnormal (below 2^-14 in magnitude) by zero.

`launch` is the same hook around ONE launch's dense restatement of tests/unet_kernel_ref.py (conv, rows; attention and temb
for the faults that concern them), which is what the per-launch GPU tests compare with.

FAULTS name deliberate departures from the specification; each must miss a (case, launch) named for it (FAULT_CASE) by 10 x that
launch's tolerance:
  unrounded              no operand is rounded (the f32 form)
  bf16                   operands rounded to bfloat16
  weights_unrounded      the weights stay unrounded
  activations_unrounded  only the weights are rounded
  rounded_before_norm    the activation is rounded before its GroupNorm / LayerNorm prologue, not after
  padding_through_norm   a conv's padding taps go through GroupNorm + SiLU instead of being 0
  bias_rounded           the bias is rounded to f16
  residual_rounded       the residual is rounded to f16
  geglu_product_rounded  GEGLU's value and gate (with their biases) are rounded before (h + b_h) gelu(g + b_g)
  attention_rounded      q, k and v of the attention are rounded
  temb_rounded           time_emb_proj's operands are rounded
  k_tail_dropped         a source's K tail of 16 (K = 48, 80) is not run
  second_source_offset   source 1's weight rows start at c0, the real width of source 0, not at its padded K (which IS cs0 in
                         this layout, so the fault as the f32 suite names it, `cs0 instead of the padded K0`, cannot exist here)
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch.overrides import TorchFunctionMode

from tests import unet_kernel_ref as K
from tests import unet_ref as R

FAULTS = ("unrounded", "bf16", "weights_unrounded", "activations_unrounded", "rounded_before_norm", "padding_through_norm", "bias_rounded",
          "residual_rounded", "geglu_product_rounded", "attention_rounded", "temb_rounded", "k_tail_dropped", "second_source_offset")
_MATMULS = (torch.matmul, torch.Tensor.matmul, torch.Tensor.__matmul__)
F16_MIN_NORMAL = 2.0 ** -14


def gemm_keys(sd):
    """The keys of the weights whose products the form runs on the f16 matrix cores."""
    return tuple(k for k, v in sd.items() if k.endswith(".weight") and v.dim() >= 2 and not k.startswith(("time_embedding.", "class_embedding."))
                 and ".time_emb_proj." not in k)


def round_to(t, rounding, subnormals="kept"):
    if rounding is None:
        return t
    h = t.to(rounding)
    if subnormals == "flushed" and rounding == torch.float16:
        h = torch.where(h.abs() < F16_MIN_NORMAL, torch.zeros_like(h), h)
    return h.to(t.dtype)


class Rounding(TorchFunctionMode):
    """weights: the GEMM weight tensors themselves (compared by identity), or None: every F.linear is a GEMM."""

    def __init__(self, weights=None, rounding=torch.float16, fault=None, subnormals="kept", temb_weights=()):
        super().__init__()
        assert fault is None or fault in FAULTS, fault
        assert subnormals in ("kept", "flushed"), subnormals
        if fault == "unrounded":
            rounding = None
        elif fault == "bf16":
            rounding = torch.bfloat16
        self.rounding, self.fault, self.subnormals = rounding, fault, subnormals
        self.weights = None if weights is None else {id(w) for w in weights}
        self.temb = {id(w) for w in temb_weights}
        self.keep = (weights, temb_weights)      # the ids stay valid

    def rnd(self, t):
        return round_to(t, self.rounding, self.subnormals)

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        act = (lambda t: t) if self.fault in ("activations_unrounded", "rounded_before_norm") else self.rnd
        wgt = (lambda t: t) if self.fault == "weights_unrounded" else self.rnd
        bias = self.rnd if self.fault == "bias_rounded" else (lambda t: t)
        if func is F.conv2d or func is F.linear:
            x, w, *rest = args
            if func is F.linear and self.weights is not None and id(w) not in self.weights:
                if self.fault == "temb_rounded" and id(w) in self.temb:
                    return func(self.rnd(x), self.rnd(w), *rest, **kwargs)
                return func(*args, **kwargs)
            b = rest[0] if rest else kwargs.pop("bias", None)
            return func(act(x), wgt(w), None if b is None else bias(b), *rest[1:], **kwargs)
        if self.fault == "rounded_before_norm" and (func is F.group_norm or func is F.layer_norm):
            return func(self.rnd(args[0]), *args[1:], **kwargs)
        if self.fault == "attention_rounded" and func in _MATMULS:
            return func(self.rnd(args[0]), self.rnd(args[1]))
        return func(*args, **kwargs)


def forward(sd, sample, timestep, text, label, rounding=torch.float16, fault=None, subnormals="kept", **cfg):
    """unet_ref.forward in sample's dtype with the GEMM operands rounded.  The state dict is cast first, so that unet_ref's own
    cast returns the same tensors and the hook knows the GEMM weights by identity."""
    assert fault in (None, "unrounded", "bf16", "weights_unrounded", "activations_unrounded", "rounded_before_norm", "bias_rounded", "attention_rounded",
                     "temb_rounded"), f"{fault}: a fault of one launch (see `launch`)"
    p = {k: v.to(sample.dtype) for k, v in sd.items()}
    mode = Rounding([p[k] for k in gemm_keys(p)], rounding, fault, subnormals, temb_weights=[v for k, v in p.items() if k.endswith(".time_emb_proj.weight")])
    with torch.no_grad(), mode:
        return R.forward(p, sample, timestep, text, label, **cfg)


# ------------------------------------------------------------------------------------------------ one launch
def _padded_through_norm(d, dtype, mode):
    """The conv with its padding ring sent through GroupNorm + SiLU: pad first, then the loader's affine map and SiLU, then no padding."""
    parts = []
    for x, nm in ((d["x0"], d.get("norm0")), (d.get("x1"), d.get("norm1"))):
        if x is not None:
            parts.append(K._affine_silu(F.pad(x.to(dtype), (1, 1, 1, 1)), nm, dtype))
    with mode:
        return F.conv2d(torch.cat(parts, 1), d["w"].to(dtype), d["b"].to(dtype), stride=d.get("stride", 1))


def launch(family, dense, dtype=torch.float64, rounding=torch.float16, fault=None, subnormals="kept"):
    """One launch's dense restatement (tests/unet_kernel_ref.py: conv, rows, attention, temb) on `dense` in `dtype` with the form's
    roundings; attention and temb are not rounded by the form (only by their faults)."""
    d = dict(dense)
    mode = Rounding(None, rounding, fault, subnormals)
    rnd = mode.rnd
    with torch.no_grad():
        if family == "attention":
            if fault == "attention_rounded":
                d.update({k: rnd(d[k].to(dtype)) for k in "qkv"})
            return K.attention(d, dtype)
        if family == "temb":
            if fault == "temb_rounded":
                d["semb"] = rnd(d["semb"].to(dtype))
                d["resnets"] = [(rnd(w.to(dtype)), b, cb) for w, b, cb in d["resnets"]]
            return torch.cat(K.temb(d, dtype))
        assert family in ("conv", "rows"), family
        if fault == "rounded_before_norm":
            d["x0"] = rnd(d["x0"].to(dtype))
            if d.get("x1") is not None:
                d["x1"] = rnd(d["x1"].to(dtype))
        if fault == "residual_rounded":
            d["res"] = rnd(d["res"].to(dtype))
        if fault in ("k_tail_dropped", "second_source_offset"):
            w = d["w"].clone()
            c0 = d["x0"].shape[1] if family == "conv" else d["x0"].shape[2]
            widths = [c0, w.shape[1] - c0]
            if fault == "k_tail_dropped":
                at = 0
                for c in widths:
                    if c % 32:
                        w[:, at + c - c % 32:at + c] = 0.0      # the source's last 16: never multiplied
                    at += c
            else:
                pad = K.up16(c0) - c0                           # source 1's channel j reads the row of channel j - pad, or the zero padding
                w1 = w[:, c0:].clone()
                w[:, c0:] = 0.0
                if pad < widths[1]:
                    w[:, c0 + pad:] = w1[:, :widths[1] - pad]
            d["w"] = w
        if fault == "padding_through_norm" and family == "conv":
            return _padded_through_norm(d, dtype, mode)
        if fault == "geglu_product_rounded" and family == "rows":
            with mode:
                y = K.rows(dict(d, geglu=False, res=None), dtype)
            value, gate = y.chunk(2, dim=-1)
            return rnd(value) * F.gelu(rnd(gate))
        with mode:
            return (K.conv if family == "conv" else K.rows)(d, dtype)


class _Operand(TorchFunctionMode):
    """Keeps the activation handed to the launch's product."""

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if func is F.conv2d or func is F.linear:
            self.x = args[0]
        return func(*args, **(kwargs or {}))


def without_subnormal_operands(family, dense):
    """`dense` (a conv or rows case without `up`) changed so that the launch's float64 emulation is a pin the hardware can be held to:

      * no operand of the product rounds to an f16 subnormal: every element of x0, x1 and w below 2^-13 in magnitude is set to 0,
        and an input whose value after the prologue lands below 2^-13 is moved by 2^-6 (the norms are given to a launch, so they do
        not move with it).  On the result the two subnormal switches give the same bits (tests/test_unet_f16_host.py);
      * no value a prologue computes lies within 2^-8 of an f16 ulp of a rounding boundary: such an input is moved by 2^-6 too.
        The kernel evaluates the prologue in float32, the emulation in float64; they differ by a few float32 ulps, 2^-13 of an
        f16 ulp, and a value that close to a boundary would round the other way and miss the emulation by a whole f16 ulp times
        the weight, with either of them right.  A case without a prologue rounds its inputs themselves and needs none of this.

    Under one element in fifty moves (asserted there)."""
    d = dict(dense)
    for k in ("x0", "x1", "w"):
        if d.get(k) is not None:
            d[k] = torch.where(d[k].abs() < 2.0 ** -13, torch.zeros_like(d[k]), d[k])
    if d.get("prologue") is None and d.get("norm0") is None:
        return d
    ch = 1 if family == "conv" else 2
    c0 = d["x0"].shape[ch]
    for _ in range(16):
        seen = _Operand()
        with torch.no_grad(), seen:
            (K.conv if family == "conv" else K.rows)(d, torch.float64)
        h = seen.x.to(torch.float16).double()
        ulp = torch.ldexp(torch.ones_like(h), torch.frexp(h.abs().clamp_min(2.0 ** -14))[1] - 11)      # of the f16 value, normal
        tiny = ((seen.x.abs() < 2.0 ** -13) & (seen.x != 0)) | ((seen.x - h).abs() > (0.5 - 2.0 ** -8) * ulp)
        tiny = tiny.float()
        if not bool(tiny.any()):
            return d
        assert tiny.shape[ch] == c0 + (d["x1"].shape[ch] if d.get("x1") is not None else 0) and tiny.shape[0] == d["x0"].shape[0]
        d["x0"] = d["x0"] + 2.0 ** -6 * tiny.narrow(ch, 0, c0).reshape(d["x0"].shape)
        if d.get("x1") is not None:
            d["x1"] = d["x1"] + 2.0 ** -6 * tiny.narrow(ch, c0, tiny.shape[ch] - c0).reshape(d["x1"].shape)
    raise AssertionError("an operand stays subnormal or on a rounding boundary")


def launch_reference(family, dense):
    """(the float64 emulation of the launch, tol = 8 x max |emulation in float32 - emulation in float64|)."""
    e64, e32 = launch(family, dense), launch(family, dense, torch.float32)
    return e64, 8.0 * float((e32.double() - e64).abs().max())


_network = {}


def network_case(name):
    """The case `name` of tests/unet_cases.py with every GEMM weight below 2^-13 in magnitude set to 0 (a handful of a random
    matrix): no weight rounds to an f16 subnormal, so the verdict on a case does not hang on what the hardware does with one."""
    from tests import unet_cases as C
    case = C.by_name(name)
    keys = set(gemm_keys(case.sd))
    sd = type(case.sd)((k, torch.where(v.abs() < 2.0 ** -13, torch.zeros_like(v), v) if k in keys else v) for k, v in case.sd.items())
    return case._replace(sd=sd)


def network_reference(name):
    """(float64 unrounded result, float64 emulation, bound) of network_case(name), computed once, where bound = max |emulation64 -
    unrounded64| + 8 x max |emulation32 - emulation64|: the form's own distance from the exact network plus the float32 noise of
    evaluating it.  A bound, not a pin: an activation within a float32 error of an f16 rounding boundary rounds the other way."""
    if name not in _network:
        case = network_case(name)
        with torch.no_grad():
            y64 = R.forward(case.sd, case.sample.double(), case.timestep, case.text, case.label, **case.cfg)
        e64 = forward(case.sd, case.sample.double(), case.timestep, case.text, case.label, **case.cfg)
        e32 = forward(case.sd, case.sample, case.timestep, case.text, case.label, **case.cfg)
        _network[name] = (y64, e64, float((e64 - y64).abs().max()) + 8.0 * float((e32.double() - e64).abs().max()))
    return _network[name]


# ------------------------------------------------------------------------------------------------ the fault cases
def _gen(seed):
    return torch.Generator().manual_seed(21000 + seed)


def _n(g, shape, scale=1.0):
    return (scale * torch.randn(shape, generator=g)).float()


def _rows_case(seed, n, rps, c0, c1, nout, prologue=None, geglu=False, res=False):
    """N(0, 1) inputs; weights N(0, 1 / K), biases N(0, 1) (a rounded bias must show)."""
    from tests import unet_kernels as UK
    g = _gen(seed)
    c = c0 + c1
    x = _n(g, (n, rps, c))
    d = dict(x0=x[..., :c0].contiguous(), x1=x[..., c0:].contiguous() if c1 else None, w=_n(g, ((2 if geglu else 1) * nout, c), 1.0 / math.sqrt(c)),
             b=_n(g, ((2 if geglu else 1) * nout,)), prologue=prologue, geglu=geglu)
    if prologue == "layernorm":
        d.update(ln=tuple(t.reshape(n, rps) for t in UK.given_ln(x.reshape(n * rps, c))), ln_g=1.0 + 0.3 * _n(g, (c,)), ln_b=0.2 * _n(g, (c,)))
    if res:
        d["res"] = _n(g, (n, rps, nout))
    return d


def _conv_case(seed, n, c0, c1, cout, h, w, normed=False):
    from tests import unet_kernels as UK
    g = _gen(seed)
    c = c0 + c1
    x = _n(g, (n, c, h, w))
    d = dict(x0=x[:, :c0].contiguous(), x1=x[:, c0:].contiguous() if c1 else None, w=_n(g, (cout, c, 3, 3), 1.0 / math.sqrt(9 * c)), b=_n(g, (cout,)))
    if normed:
        nm = UK.given_norm(x, 4, 1.0 + 0.3 * _n(g, (c,)), 2.0 + 0.2 * _n(g, (c,)), 1e-5)      # beta near 2: a padding tap through the norm is silu(beta - mean a)
        d["norm0"] = (nm[0][:, :c0], nm[1][:, :c0], nm[2][:c0])
        if c1:
            d["norm1"] = (nm[0][:, c0:], nm[1][:, c0:], nm[2][c0:])
    return d


def _attn_case(seed):
    g = _gen(seed)
    return dict(q=_n(g, (1, 2, 33, 24)), k=_n(g, (1, 2, 33, 24)), v=_n(g, (1, 2, 33, 24)), layout="text")


def _temb_case(seed):
    g = _gen(seed)
    return dict(semb=_n(g, (64,)), resnets=[(_n(g, (c, 64), 0.125), _n(g, (c,)), _n(g, (c,))) for c in (24, 48)])


FAULT_CASES = {      # name: (family, builder)
    "rows_ln_96": ("rows", lambda: _rows_case(1, 1, 33, 96, 0, 40, "layernorm")),
    "rows_res_64": ("rows", lambda: _rows_case(2, 2, 17, 64, 0, 40, res=True)),
    "rows_geglu_64": ("rows", lambda: _rows_case(3, 1, 33, 64, 0, 48, "layernorm", geglu=True)),
    "rows_k48": ("rows", lambda: _rows_case(4, 1, 33, 48, 0, 24)),
    "rows_k80": ("rows", lambda: _rows_case(5, 1, 33, 80, 0, 24)),
    "rows_cat_6_10": ("rows", lambda: _rows_case(6, 1, 33, 6, 10, 24)),
    "conv_gn_24_8": ("conv", lambda: _conv_case(7, 2, 24, 8, 20, 5, 17, normed=True)),
    "conv_cat_6_10": ("conv", lambda: _conv_case(8, 1, 6, 10, 16, 4, 5)),
    "attn_d24": ("attention", lambda: _attn_case(9)),
    "temb_2": ("temb", lambda: _temb_case(10)),
}
# which (case, launch) must expose which fault
FAULT_CASE = {"unrounded": ("rows_ln_96", "conv_gn_24_8"), "bf16": ("rows_ln_96", "conv_gn_24_8"), "weights_unrounded": ("rows_ln_96", "conv_gn_24_8"),
              "activations_unrounded": ("rows_ln_96", "conv_gn_24_8"), "rounded_before_norm": ("rows_ln_96", "conv_gn_24_8"),
              "padding_through_norm": ("conv_gn_24_8",), "bias_rounded": ("rows_res_64", "conv_gn_24_8"), "residual_rounded": ("rows_res_64",),
              "geglu_product_rounded": ("rows_geglu_64",), "attention_rounded": ("attn_d24",), "temb_rounded": ("temb_2",),
              "k_tail_dropped": ("rows_k48", "rows_k80"), "second_source_offset": ("rows_cat_6_10", "conv_cat_6_10")}
_fault_cases = {}


def fault_case(name):
    if name not in _fault_cases:
        family, build = FAULT_CASES[name]
        _fault_cases[name] = (family, build())
    return _fault_cases[name]


def fault_ratio(fault, name):
    """max |the faulty emulation in float32 - the float64 emulation| / the launch's tolerance."""
    family, dense = fault_case(name)
    e64, tol = launch_reference(family, dense)
    y = launch(family, dense, torch.float32, fault=fault)
    return float((y.double() - e64).abs().max()) / tol
