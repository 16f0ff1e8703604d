"""The per-value pin of one 16-bit conv layer (bf16 or f16 operands and storage, f32 accumulation), shared by the per-layer
tests of both 16-bit kernels (test_gpu_conv.py, test_gpu_conv_xl.py, xl_layer_child.py) -- the bf16 twin of
test_one_layer_rounding_pin in test_gpu_f16.py.

Reference: operands already rounded to the storage type, the float64 conv (+ nearest x2 of the input, + LeakyReLU(0.2)) with
the float32 bias, rounded once to the storage type (ref16).

  per value   |y - ref16| <= ulp(ref16), or, where one 16-bit ulp is smaller than what f32 accumulation of K = 9 cin products
              may be off by (sums that cancel), |y - ref| <= K 2^-24 conv(|x|, |w|, |b|) + ulp
  bitwise     the share of values that are not ref16's bits: a correctly rounded store misses only where the f32 sum and the
              float64 value straddle a rounding boundary (torch's f32 conv as the kernel's stand-in: 0.4e-4 .. 1.0e-4 of the
              values for bf16, none outside the per-value condition); a store that rounds toward zero misses about half.
              The cap is 0.01 for bf16 and 0.05 for f16 (three more bits: the boundaries are 8x denser, most misses near zero)
"""
import math

import torch
import torch.nn.functional as F

STORE = {"bf16": torch.bfloat16, "f16": torch.float16}
MISS_CAP = {"bf16": 0.01, "f16": 0.05}
MANT = {"bf16": 7, "f16": 10}            # stored significand bits
MIN_EXP = {"bf16": -126, "f16": -14}     # below 2^MIN_EXP the spacing is the subnormal one


def miss_allowance(values, dtype):
    """Values of one case that may differ from ref16's bits: the cap's share of the case, and one value where the case is so
    small (under 100 values for bf16) that a single straddled rounding boundary is already more than that share."""
    return max(1, math.floor(MISS_CAP[dtype] * values))


def ulp16(v, dtype):
    """Spacing of the storage type at |v| (v float64, already a storage-type value): 2^(floor(log2|v|) - mantissa bits)."""
    a = v.abs().clamp_min(2.0 ** MIN_EXP[dtype])
    return torch.exp2(torch.floor(torch.log2(a)) - MANT[dtype])


def make_case(cin, cout, h, w, dtype, seed, n=2):
    """randn inputs, weights randn / sqrt(9 cin), bias 0.1 randn; x and w rounded to the storage type, bias float32."""
    g = torch.Generator().manual_seed(seed)
    st = STORE[dtype]
    x = torch.randn(n, cin, h, w, generator=g).to(st).float()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / math.sqrt(9 * cin))).to(st).float()
    b = torch.randn(cout, generator=g) * 0.1
    return x, wt, b


def conv_f64(x, wt, b, up=False):
    """(float64 conv before the activation, sum of |products|): the part of the reference that lrelu on / off share."""
    xd = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up else x.double()
    pre = F.conv2d(xd, wt.double(), b.double(), padding=1)
    mag = F.conv2d(xd.abs(), wt.double().abs(), b.double().abs(), padding=1)
    return pre, mag


def reference16(pre, lrelu, dtype):
    """(ref, ref16): the float64 value and the same rounded once to the storage type, both float64."""
    ref = F.leaky_relu(pre, 0.2) if lrelu else pre
    return ref, ref.to(STORE[dtype]).double()


def pin(y, pre, mag, cin, lrelu, dtype):
    """Figures of one case: y the kernel's NCHW float32 output.  {"values", "outside", "worst", "miss"}."""
    y = y.double()
    ref, ref16 = reference16(pre, lrelu, dtype)
    ulp = ulp16(ref16, dtype)
    e_acc = 9 * cin * 2.0 ** -24 * mag
    diff = (y - ref16).abs()
    within = (diff <= ulp) | ((ulp < e_acc) & ((y - ref).abs() <= e_acc + ulp))
    return {"values": y.numel(), "outside": int((~within).sum()), "worst": float(diff.max()), "worst_ulps": float((diff / ulp).max()),
            "missed": int((diff > 0).sum()), "miss": float((diff > 0).double().mean()), "finite": bool(torch.isfinite(y).all())}


def assert_pin(fig, dtype, what=""):
    assert fig["finite"], what
    assert fig["outside"] == 0, f"{what}: {fig['outside']} of {fig['values']} values more than one {dtype} ulp off, worst {fig['worst']:.3e}"
    assert fig["missed"] <= miss_allowance(fig["values"], dtype), \
        f"{what}: {fig['missed']} of {fig['values']} values ({fig['miss']:.3e}) are not the rounded float64 value's bits"


class MissPool:
    """The bitwise-miss cap once more over the pooled values of several cases, on top of the cap of every case."""

    def __init__(self):
        self.values, self.missed = {}, {}

    def add(self, dtype, fig):
        self.values[dtype] = self.values.get(dtype, 0) + fig["values"]
        self.missed[dtype] = self.missed.get(dtype, 0) + fig["missed"]

    def shares(self):
        return {d: self.missed[d] / self.values[d] for d in self.values}

    def check(self):
        for d, share in self.shares().items():
            assert share <= MISS_CAP[d], f"{d}: {share:.3e} of {self.values[d]} pooled values are not the rounded float64 value's bits"


def one_hot_case(cin, cout, h, w, tap):
    """Small integers (exact in bf16 and f16): one input channel and one tap per output channel, bias = the channel index."""
    x = ((torch.arange(cin * h * w, dtype=torch.float32).reshape(1, cin, h, w) * 7) % 61).contiguous()
    wt = torch.zeros(cout, cin, 3, 3)
    for o in range(cout):
        wt[o, (o * 5 + tap) % cin, tap // 3, tap % 3] = 1.0
    b = torch.arange(cout, dtype=torch.float32)
    return x, wt, b, F.conv2d(x, wt, b, padding=1)
