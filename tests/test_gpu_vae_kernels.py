"""GPU: every kernel of csrc/vae.hip, one launch (or one short chain) at a time through the nesr_vae_k_* test hooks, against a plain
float64 torch restatement of the same operation (tests/vae_kernel_ref.py), at the pixel counts (to 20000), widths, ragged extents
and arguments no whole-decode case of tests/vae_cases.py reaches.  tests/vae_kernels.py holds the cases and the packing.

Exact cases carry small integers (the u8 case integers x 2^-7), so every partial sum is an exact float32 in any order
(tests/test_vae_kernels_host.py asserts the premise): the result must equal the float64 reference bit for bit, the u8 frame with no
sample left out.  The selector cases of the attention are exact the same way: the softmax is one-hot in float32, the output is the
selected integer V row.  Toleranced cases carry random floats; their tolerance is the project's rule per launch, 8 x max |float32
restatement - float64| per compared quantity, computed here, never derived from the GPU's output, and `err / tol` is printed per
case.  A statistics launch's mean is also held to 2^-38 max |x|, and to the exact double mean where the inputs are integers.

Every output buffer lies between guards of sentinels (asserted) and is itself filled with the sentinel before the launch, so what
csrc/vae_api.h says of padded columns is asserted, not assumed: the conv's and the row product's zero columns, the attention's
columns past c, the zero VaeNorm of padded channels, the zero columns past the latents' channels.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from neural_enhanced_super_resolution_amd import _lib
from tests import vae_kernel_ref as R
from tests import vae_kernels as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", V.NAMES)
def test_a_launch_against_the_float64_restatement(name):
    case = V.by_name(name)
    ref64, ref32 = V.references(name)
    got, pads = V.unpack(case.family, case.args, V.launch(case.family, case.args)[0])
    assert len(got) == len(ref64) and all(g.shape == r.shape and bool(torch.isfinite(g).all()) for g, r in zip(got, ref64))
    assert pads, "a padded column does not hold what csrc/vae_api.h documents"
    if case.kind == "exact":
        wrong = sum(int((g.float() != r.float()).sum()) for g, r in zip(got, ref64))
        print(f"{name}: exact, {sum(g.numel() for g in got)} values, {wrong} differ")
        assert V.is_exact(got, ref64)
    else:
        rs = V.ratios(got, ref64, ref32)
        print(f"{name}: err / tol {max(rs):.3f} ({', '.join(f'{r:.3f}' for r in rs)})")
        assert max(rs) <= 1.0
    if case.family == "group_norm":      # the double sums and the (hi, lo) pair: far inside the tolerance
        err, bound = float((got[0] - ref64[0]).abs().max()), V.mean_bound(case)
        print(f"{name}: |mean error| {err:.2e}, bound {bound:.2e}")
        assert err <= bound
        if case.dense["integer"]:
            assert torch.equal(got[0], V.split_mean(ref64[0])), "the mean of integers is exact in double"


def chain_stats_conv():
    """The statistics launch writes the VaeNorm that the NEAREST2 conv's loader reads: conv2d(silu(group_norm(nearest x2(x))))."""
    g = V.gen(400)
    x, gamma, beta, eps = V.rnd(g, (1, 32, 3, 5)) + 0.5, 1.0 + 0.3 * V.rnd(g, (32,)), 1.0 + 0.2 * V.rnd(g, (32,)), 1e-6
    w, b = V.rnd(g, (24, 32, 3, 3), 1.0 / math.sqrt(288)), V.rnd(g, (24,), 0.2)
    _, norm = V.launch("group_norm", V.pack_group_norm(dict(x0=x.reshape(1, 32, 15), groups=8, gamma=gamma, beta=beta, eps=eps)))
    a = dict(V.pack_conv(dict(x=x, up=True, w=w, b=b)), norm=norm["norm0"])
    got, pads = V.unpack("conv", a, V.launch("conv", a)[0])
    ref = [F.conv2d(F.silu(F.group_norm(F.interpolate(x.to(t), scale_factor=2.0, mode="nearest"), 8, gamma.to(t), beta.to(t), eps)), w.to(t), b.to(t), padding=1)
           for t in (torch.float64, torch.float32)]
    return got, pads, ref


def chain_attention_block():
    """The whole attention block at width 40 in rows of 48, 70 tokens: statistics -> q | k | v product with the norm in its loader ->
    attention -> output product + the block's input."""
    g = V.gen(401)
    n, c, cs = 70, 40, 48
    x, gamma, beta, eps = V.rnd(g, (n, c)) + 0.3, 1.0 + 0.3 * V.rnd(g, (c,)), 0.2 * V.rnd(g, (c,)), 1e-6
    ws, bs = [V.rnd(g, (c, c), 1.0 / math.sqrt(c)) for _ in range(4)], [V.rnd(g, (c,), 0.2) for _ in range(4)]
    xdev = V.pad_cols(x, cs).reshape(-1).to("cuda:0")      # the statistics' input, the first product's input, the last product's residual
    gn = dict(V.pack_group_norm(dict(x0=x.t()[None], groups=8, gamma=gamma, beta=beta, eps=eps)), in0=xdev)
    _, norm = V.launch("group_norm", gn)
    wt, bt = torch.zeros((cs, 3 * cs)), torch.zeros(3 * cs)
    for j in range(3):
        wt[:c, j * cs:j * cs + c], bt[j * cs:j * cs + c] = ws[j].t(), bs[j]
    qkv = dict(m=n, cs_in=cs, np=3 * cs, norm=norm["norm0"], w=wt.reshape(-1), b=bt, res=None, out=V.sentinels(n * 3 * cs), **{"in": xdev})
    _, qkv_dev = V.launch("rows", qkv)
    attn = dict(n=n, c=c, cs=cs, qkv=qkv_dev["out"], out=V.sentinels(n * cs))
    _, o_dev = V.launch("attention", attn)
    last = dict(V.pack_rows(dict(x=torch.zeros((n, c)), w=ws[3], b=bs[3])), res=xdev, **{"in": o_dev["out"]})
    got, pads = V.unpack("rows", last, V.launch("rows", last)[0])
    ref = []
    for t in (torch.float64, torch.float32):
        h = F.group_norm(x.to(t).t()[None], 8, gamma.to(t), beta.to(t), eps)[0].t()
        q, k, v = (F.linear(h, ws[j].to(t), bs[j].to(t)) for j in range(3))
        ref.append(F.linear(torch.softmax((q @ k.t()) / math.sqrt(c), dim=-1) @ v, ws[3].to(t), bs[3].to(t)) + x.to(t))
    return got, pads, ref


def chain_head():
    """The decoder's head: latents / scaling factor -> post_quant_conv (1x1) -> conv_in (3x3)."""
    g = V.gen(402)
    z, div = V.rnd(g, (4, 35)), 0.18215
    w1, b1, w3, b3 = V.rnd(g, (4, 4), 0.5), V.rnd(g, (4,), 0.2), V.rnd(g, (32, 4, 3, 3), 1.0 / 6.0), V.rnd(g, (32,), 0.2)
    _, rows0 = V.launch("in", V.pack_in(dict(z=z, divisor=div)))
    pq = dict(V.pack_rows(dict(x=torch.zeros((35, 4)), w=w1, b=b1)), **{"in": rows0["out"]})
    _, rows1 = V.launch("rows", pq)
    a = dict(V.pack_conv(dict(x=torch.zeros((1, 4, 5, 7)), w=w3, b=b3)), **{"in": rows1["out"]})
    got, pads = V.unpack("conv", a, V.launch("conv", a)[0])
    ref = []
    for t in (torch.float64, torch.float32):
        h = F.linear(R.vin(dict(z=z, divisor=div), t), w1.to(t), b1.to(t))      # [35, 4]
        ref.append(F.conv2d(h.t().reshape(1, 4, 5, 7), w3.to(t), b3.to(t), padding=1))
    return got, pads, ref


CHAINS = {"statistics_then_the_nearest2_conv_loader": chain_stats_conv, "the_attention_block_at_width_48": chain_attention_block,
          "in_then_rows_then_conv": chain_head}


@pytest.mark.parametrize("name", tuple(CHAINS))
def test_a_short_chain_on_the_same_buffers(name):
    """Each launch reads what the launch before left on the device; nothing is copied through the host in between."""
    with torch.no_grad():
        got, pads, ref = CHAINS[name]()
    rs = V.ratios(got, (ref[0],), (ref[1],))
    print(f"{name}: err / tol {rs[0]:.3f}")
    assert pads and got[0].shape == ref[0].shape and rs[0] <= 1.0


def _aliased(a, out, src):
    b = dict(a)
    b[out] = b[src]
    return b


REFUSALS = {      # name: (family, the arguments, the launcher that refuses)
    "conv_nearest2_with_odd_H": lambda: ("conv", dict(V.by_name("conv_up_6x34").args, H=5), "launch_vae_conv"),
    "conv_f32_with_res": lambda: ("conv", dict(V.by_name("conv_f32_cout3").args, res=V.by_name("conv_f32_cout3").args["in"], cs_res=16), "launch_vae_conv"),
    "conv_rows_with_cs_out_not_coutp": lambda: ("conv", dict(V.by_name("conv_cin6_1x1").args, cs_out=32), "launch_vae_conv"),
    "conv_cs_res_below_coutp": lambda: ("conv", dict(V.by_name("conv_res_wide").args, cs_res=16), "launch_vae_conv"),
    "rows_in_place_with_np_not_cs_in": lambda: ("rows", _aliased(V.by_name("rows_m31_16_80").args, "out", "in"), "launch_vae_rows"),
    "statistics_c_not_a_multiple_of_groups": lambda: ("group_norm", dict(V.by_name("gn_c24_cs32").args, groups=7), "launch_vae_stats_partial"),
    "attention_past_the_token_limit": lambda: ("attention", dict(V.by_name("attn_random_16_16_33").args, n=R.MAX_TOKENS + 1), "launch_vae_attn"),
    "in_divisor_0": lambda: ("in", dict(V.by_name("in_c4_m15").args, divisor=0.0), "launch_vae_in"),
}


@pytest.mark.parametrize("name", tuple(REFUSALS))
def test_a_refusal_writes_nothing(name):
    """NESR_ERR_ARG, the launcher named, and nothing written: every output buffer as it was (the guards are asserted by launch)."""
    family, a, launcher = REFUSALS[name]()
    outs, _ = V.launch(family, a, expect_rc=_lib.ERR_ARG)
    text = _lib.load().nesr_last_error().decode()
    assert launcher in text and "nesr_vae_k_" in text
    for key, got in outs.items():
        assert torch.equal(got, a[key]), f"a refused launch wrote `{key}`"
