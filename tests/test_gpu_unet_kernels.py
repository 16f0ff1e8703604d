"""GPU: every kernel of csrc/unet.hip, one launch (or one short chain) at a time through the nesr_unet_k_* test hooks, against a
plain float64 torch restatement of the same operation (tests/unet_kernel_ref.py), at the widths (to 1024), sample counts (n = 2)
and edges no whole-network case of tests/unet_cases.py reaches.  tests/unet_kernels.py holds the cases and the packing.

Exact cases carry small integers, so every partial sum is an exact float32 in any order (tests/test_unet_kernels_host.py asserts
the premise): the result must equal the float64 reference bit for bit.  The selector cases of the attention are exact the same way:
the softmax is one-hot in float32, the output is the selected integer V row.  Toleranced cases carry random floats; their tolerance
is the project's rule per launch, 8 x max |float32 restatement - float64| per compared quantity, computed here, never derived from
the GPU's output, and `err / tol` is printed per case.

Every output buffer lies between guards of sentinels (asserted) and is itself filled with the sentinel before the launch, so what
csrc/unet_api.h says of padded columns is asserted, not assumed: the conv's and the row product's zero columns, the attention's
columns past heads d, the zero VaeNorm of padded channels, a time-embedding row written to its coutp and not past it.
"""
import pytest
import torch
import torch.nn.functional as F

from neural_enhanced_super_resolution_amd import _lib
from tests import unet_kernel_ref as R
from tests import unet_kernels as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", K.NAMES)
def test_a_launch_against_the_float64_restatement(name):
    case = K.by_name(name)
    ref64, ref32 = K.references(name)
    got, pads = K.unpack(case.family, case.args, K.launch(case.family, case.args))
    assert len(got) == len(ref64) and all(g.shape == r.shape and bool(torch.isfinite(g).all()) for g, r in zip(got, ref64))
    assert pads, "a padded column does not hold what csrc/unet_api.h documents"
    if case.kind == "exact":
        wrong = sum(int((g.float() != r.float()).sum()) for g, r in zip(got, ref64))
        print(f"{name}: exact, {sum(g.numel() for g in got)} values, {wrong} differ")
        assert K.is_exact(got, ref64)
    else:
        rs = K.ratios(got, ref64, ref32)
        print(f"{name}: err / tol {max(rs):.3f} ({', '.join(f'{r:.3f}' for r in rs)})")
        assert max(rs) <= 1.0
    if case.family in R.EXTRA_FAULTS["mean_lo_dropped"]:      # the double sums and the (hi, lo) pair: far inside the tolerance
        err, bound = float((got[0] - ref64[0]).abs().max()), K.mean_bound(case)
        print(f"{name}: |mean error| {err:.2e}, bound {bound:.2e}")
        assert err <= bound


def test_group_norm_then_the_conv_loader():
    """A short chain: the statistics launch writes the VaeNorm that the conv's loader reads.  conv2d(silu(group_norm(cat)))."""
    case = K.by_name("conv_gn_loader_5x17")
    d = case.dense
    g = K.gen(41)
    gamma, beta, eps = 1.0 + 0.3 * K.rnd(g, (32,)), 2.0 + 0.2 * K.rnd(g, (32,)), 1e-5
    gn = K.pack_group_norm(dict(x0=d["x0"].reshape(2, 24, -1), x1=d["x1"].reshape(2, 8, -1), groups=8, gamma=gamma, beta=beta, eps=eps))
    norms = K.launch("group_norm", gn)
    a = dict(case.args, norm0=norms["norm0"], norm1=norms["norm1"])
    got, pads = K.unpack("conv", a, K.launch("conv", a))
    ref = [F.conv2d(F.silu(F.group_norm(torch.cat([d["x0"], d["x1"]], 1).to(t), 8, gamma.to(t), beta.to(t), eps)), d["w"].to(t), d["b"].to(t), padding=1)
           for t in (torch.float64, torch.float32)]
    rs = K.ratios(got, (ref[0],), (ref[1],))
    print(f"group_norm -> conv: err / tol {rs[0]:.3f}")
    assert pads and rs[0] <= 1.0


def test_layer_norm_stats_then_the_row_product():
    """A short chain: the statistics launch writes the float4 rows that the row product's prologue reads.  linear(layer_norm(x))."""
    case = K.by_name("rows_layernorm_1000")
    d = case.dense
    x = d["x0"].reshape(-1, d["x0"].shape[-1])
    st = K.launch("layer_norm_stats", K.pack_layer_norm_stats(dict(x=x, eps=1e-5)))
    a = dict(case.args, ln=st["out"])
    got, pads = K.unpack("rows", a, K.launch("rows", a))
    ref = [F.linear(F.layer_norm(d["x0"].to(t), (x.shape[-1],), d["ln_g"].to(t), d["ln_b"].to(t), 1e-5), d["w"].to(t), d["b"].to(t)) for t in (torch.float64, torch.float32)]
    rs = K.ratios(got, (ref[0],), (ref[1],))
    print(f"layer_norm_stats -> rows: err / tol {rs[0]:.3f}")
    assert pads and rs[0] <= 1.0


def test_the_embedding_then_every_resnets_projection():
    """A short chain: silu(emb) of the embedding launch is what the time-embedding launch projects."""
    emb, tb = K.by_name("emb_16_t487"), K.by_name("temb_30_resnets")      # both 64 wide
    semb = K.launch("embedding", emb.args)["out"]
    a = dict(tb.args, semb=semb)
    got, pads = K.unpack("temb", a, K.launch("temb", a))
    ref = [R.temb(dict(tb.dense, semb=R.embedding(emb.dense, t)), t) for t in (torch.float64, torch.float32)]
    rs = K.ratios(got, ref[0], ref[1])
    print(f"embedding -> temb: err / tol {max(rs):.3f}")
    assert pads and max(rs) <= 1.0


def refused(family, a, text):
    """NESR_ERR_ARG, the launcher named, and nothing written: every output buffer as it was (the guards are asserted by launch)."""
    outs = K.launch(family, a, expect_rc=_lib.ERR_ARG)
    assert text in _lib.load().nesr_last_error().decode()
    for name, got in outs.items():
        assert torch.equal(got, a[name]), f"a refused launch wrote `{name}`"


def test_refusals_write_nothing():
    rows = dict(K.by_name("rows_res_in_place").args, res=None)
    rows["out"] = rows["in0"]                                                      # cs0 = np = 48: a.out == a.in
    refused("rows", rows, "launch_unet_rows")
    up = K.by_name("conv_up_6x20").args
    refused("conv", dict(up, H=5), "launch_unet_conv")                             # up with odd H
    refused("conv", dict(up, stride=2), "launch_unet_conv")                        # stride 2 with up
    nchw = K.by_name("conv_out_nchw").args
    refused("conv", dict(nchw, res=nchw["in0"]), "launch_unet_conv")               # out_nchw with res
    attn = K.by_name("attn_selector_d24_h5_text").args
    refused("attention", dict(attn, ldo=attn["ldo"] + 16), "launch_unet_attn")     # ldo - heads d >= 16
    refused("attention", dict(attn, d=12, heads=10), "launch_unet_attn")           # d not a multiple of 8
