"""GPU: the bodies csrc/vae.hip and csrc/unet.hip share (csrc/f32_rows_device.h: the conv's patch loader and tap loop, the GroupNorm
partial sums and moments, the attention's scores, softmax step and P V) give the same bits through both front ends.  Each case
makes one launch through a nesr_vae_k_* hook and one through the matching nesr_unet_k_* hook on the same dense input and weights,
the UNet's with one sample, one source and stride 1, and the results must be equal: no tolerance anywhere.  The shapes are the
smallest at which a body takes each of its paths; what the values must be is the business of tests/test_gpu_vae_kernels.py and
tests/test_gpu_unet_kernels.py, this file fails when the two front ends drift apart.
"""
import math

import pytest
import torch

from tests import unet_kernels as K
from tests import vae_kernels as V

pytestmark = pytest.mark.gpu


def _conv(seed, cin, cout, h, w, up=False, norm=False, res=False):
    """h x w: the SOURCE grid."""
    g = K.gen(seed)
    x = K.rnd(g, (1, cin, h, w)) + 0.5
    d = dict(x=x, w=K.rnd(g, (cout, cin, 3, 3), 1.0 / math.sqrt(9 * cin)), b=K.rnd(g, (cout,), 0.2), up=up)
    if norm:
        d["norm"] = K.given_norm(x, 4, 1.0 + 0.3 * K.rnd(g, (cin,)), 2.0 + 0.2 * K.rnd(g, (cin,)), 1e-6)
    if res:
        d["res"] = K.rnd(g, (1, cout, 2 * h if up else h, 2 * w if up else w))
    return d


CONVS = {
    # one K chunk of a 16-step and a 4-step tail; the second column tile half padded; 2 x 2 tiles, ragged both ways; residual of stride coutp
    "cin20_cout24_5x18_norm_res": lambda: _conv(500, 20, 24, 5, 18, norm=True, res=True),
    "cin20_cout24_up_6x18_norm_res": lambda: _conv(501, 20, 24, 3, 9, up=True, norm=True, res=True),
    "cin72_cout16_4x16": lambda: _conv(502, 72, 16, 4, 16),      # two K chunks, 64 + 8
}


@pytest.mark.parametrize("name", tuple(CONVS))
def test_conv_is_the_same_through_both_front_ends(name):
    d = CONVS[name]()
    va = V.pack_conv(d)
    ua = K.pack_conv(dict(x0=d["x"], w=d["w"], b=d["b"], up=d["up"], norm0=d.get("norm"), res=d.get("res")))
    assert va["res"] is None or va["cs_res"] == va["coutp"]
    (vy,), vpad = V.unpack("conv", va, V.launch("conv", va)[0])
    (uy,), upad = K.unpack("conv", ua, K.launch("conv", ua))
    assert vpad and upad and bool(torch.isfinite(vy).all())
    print(f"{name}: {vy.numel()} values, {int((vy != uy).sum())} differ")
    assert torch.equal(vy, uy)


GROUP_NORMS = {"c32_4groups_m600": (32, 4, 600),      # two partial blocks, the second ragged
               "c24_in_cs32_3groups_m5": (24, 3, 5)}    # the padded channels get the zero VaeNorm


@pytest.mark.parametrize("name", tuple(GROUP_NORMS))
def test_group_norm_is_the_same_through_both_front_ends(name):
    c, groups, m = GROUP_NORMS[name]
    g = K.gen(510 + c)
    d = dict(x0=K.rnd(g, (1, c, m)) + 0.5 * K.rnd(g, (1, c, 1)), groups=groups, gamma=1.0 + 0.3 * K.rnd(g, (c,)), beta=0.2 * K.rnd(g, (c,)), eps=1e-6)
    va, ua = V.pack_group_norm(d), K.pack_group_norm(d)
    vo, uo = V.launch("group_norm", va)[0], K.launch("group_norm", ua)
    assert V.unpack("group_norm", va, vo)[1] and K.unpack("group_norm", ua, uo)[1]
    vn, un = (o["norm0"].reshape(va["cs0"], 4) for o in (vo, uo))      # (mean hi, mean lo, a, beta) per channel
    assert bool(torch.isfinite(vn).all())
    assert torch.equal(vn.view(torch.int32), un.view(torch.int32))


@pytest.mark.parametrize("n", (40, 32))      # two key chunks, the second ragged, and two query blocks; one full chunk
def test_attention_is_the_same_through_both_front_ends(n):
    g = K.gen(520 + n)
    d = dict(q=K.rnd(g, (1, 1, n, 64)), k=K.rnd(g, (1, 1, n, 64)), v=K.rnd(g, (1, 1, n, 64)), layout="fused")
    va, ua = V.pack_attention(d), K.pack_attention(d)
    assert torch.equal(ua["qbuf"], va["qkv"]) and (ua["ldq"], ua["ldkv"], ua["ldo"]) == (3 * va["cs"], 3 * va["cs"], va["cs"])
    (vy,), vpad = V.unpack("attention", va, V.launch("attention", va)[0])
    (uy,), upad = K.unpack("attention", ua, K.launch("attention", ua))
    assert vpad and upad and bool(torch.isfinite(vy).all()) and bool(torch.isfinite(uy).all())
    assert torch.equal(vy, uy.reshape(vy.shape))
