"""GPU: every launch of csrc/unet_f16.hip on its own, through nesr_unet_k_conv_f16 and nesr_unet_k_rows_f16 (tests/unet_f16_kernels.py).

  exact       integer activations in [-3, 3] and weights in {-1, 0, 1} are f16 values and every sum is below 2^24: the result is the
              float64 reference bit for bit, and the f32 hook's result on the same input bit for bit
  toleranced  random floats within 8 x max |emulation in float32 - emulation in float64| of the float64 emulation of that launch
              (tests/unet_f16_emu.py), computed here
  blocks      the column block the launcher picks is the one the shape selects (a returned value), and 1024 columns are right at each
  subnormals  weights of +-2^-20: the result is one of the two emulations bit for bit; which one is DESIGN section 21's finding
  refusals    what the f32 launchers refuse, the f16 launchers refuse
  range       7e4 raises the word, 65504 does not, a NaN does, a value the prologue brings back into range does not
Guards and the zero padding of every output are asserted in every launch.
"""
import pytest
import torch

from neural_enhanced_super_resolution_amd import _lib
from tests import unet_f16_emu as E
from tests import unet_f16_kernels as K16
from tests import unet_kernels as UK
from tests.test_unet_f16_host import subnormal_case

pytestmark = pytest.mark.gpu


def run(name):
    family, kind, dense, a = K16.by_name(name)
    outs, word, block = K16.launch16(family, a)
    got, padded_ok = UK.unpack(family, a, outs)
    assert padded_ok, f"{name}: a padded column does not hold what csrc/unet_api.h documents"
    return family, dense, a, got[0], word, block


@pytest.mark.parametrize("name", [n for n in K16.NAMES if K16.kind(n) == "exact"])
def test_an_exact_case_is_float64_and_the_f32_launch_bit_for_bit(name):
    family, dense, a, got, word, block = run(name)
    ref = UK.as_tuple(UK.REF[family](dense, torch.float64))[0]
    bound = max(float(t.max()) for t in UK.as_tuple(UK.REF[family]({k: (v.abs() if torch.is_tensor(v) else v) for k, v in dense.items()}, torch.float64)))
    assert bound < 2 ** 24
    assert got.shape == ref.shape and torch.equal(got, ref.float()), f"{name}: max |gpu - f64| {float((got.double() - ref).abs().max())}"
    assert word == 0
    f32 = UK.unpack(family, a, UK.launch(family, a))[0][0]
    assert torch.equal(got, f32)
    if K16.expected_block(name) is not None:
        assert block == K16.expected_block(name)


@pytest.mark.parametrize("name", [n for n in K16.NAMES if K16.kind(n) == "tol"])
def test_a_toleranced_case_is_within_eight_float32_errors_of_the_emulation(name):
    family, dense, a, got, word, block = run(name)
    e64, tol = E.launch_reference(family, dense)
    err = float((got.double() - e64).abs().max())
    print(f"{name}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.3f}, block {block}")
    assert got.shape == e64.shape and err <= tol
    assert word == 0
    if K16.expected_block(name) is not None:
        assert block == K16.expected_block(name)


def test_every_block_width_is_reached_by_both_launchers_and_geglu():
    seen = {(K16.family(n), "geglu" in n, K16.expected_block(n)) for n in K16.NAMES if K16.expected_block(n)}
    assert {("rows", False, b) for b in (32, 64, 128)} | {("rows", True, b) for b in (32, 64, 128)} | {("conv", False, b) for b in (32, 64, 128)} <= seen


def test_f16_subnormal_weights_are_one_of_the_two_emulations_bit_for_bit():
    d = subnormal_case()
    a = K16.packed("rows", d)
    got = UK.unpack("rows", a, K16.launch16("rows", a)[0])[0][0]
    kept, flushed = E.launch("rows", d).float(), E.launch("rows", d, subnormals="flushed").float()
    assert not torch.equal(kept, flushed)
    which = "kept" if torch.equal(got, kept) else "flushed" if torch.equal(got, flushed) else None
    print(f"f16 subnormal operands on this device: {which}")
    assert which is not None
    assert which == "kept"      # DESIGN section 21 and include/nesr_hip.h state it


def bad_arguments(family, a):
    """(what, arguments) the f32 launcher refuses for reasons that do not concern the weight pointer."""
    def change(**kw):
        return dict(a, **kw)
    if family == "rows":
        yield "m = 0", change(m=0)
        yield "cs0 no multiple of 16", change(cs0=a["cs0"] + 4)
        yield "np = 8", change(np=8, ldw=8)
        yield "ldw != np", change(ldw=a["ldw"] + 16)
        yield "out is in0", change(out=a["in0"])
        yield "a prologue that does not exist", change(prologue=3)
        yield "GroupNorm without a norm", change(prologue=1, norm0=None)
        yield "LayerNorm without statistics", change(prologue=2, ln=None)
        yield "no bias", change(b=None)
    else:
        yield "n = 3", change(n=3)
        yield "H = 0", change(H=0)
        yield "stride 3", change(stride=3)
        yield "stride 2 and up", change(stride=2, up=1)
        yield "up on an odd grid", change(up=1, H=3)
        yield "coutp not cout rounded up", change(coutp=a["coutp"] + 16)
        yield "cs0 below c0", change(cs0=a["c0"] - 16 if a["c0"] > 16 else 0)
        yield "out_nchw with a residual", change(out_nchw=1, res=a["in0"])
        yield "no bias", change(bias=None)


@pytest.mark.parametrize("name", ["rows_res_in_place", "conv_res"])
def test_the_refusals_are_the_f32_launchers(name):
    family, _, _, a = K16.by_name(name)
    for what, bad in bad_arguments(family, a):
        print(what)
        UK.launch(family, bad, expect_rc=_lib.ERR_ARG)           # refused by the f32 launcher (asserted inside)
        K16.launch16(family, bad, expect_rc=_lib.ERR_ARG)        # and by the f16 one; the sentinels are untouched
    K16.launch16(family, dict(a, w16=None), expect_rc=_lib.ERR_ARG)
    K16.launch16(family, a, with_range=False)                                                    # the range word is optional


def range_word(family, dense):
    return K16.launch16(family, K16.packed(family, dense))[1]


def test_the_range_word():
    g = UK.gen(300)
    rows = dict(x0=UK.rnd(g, (1, 33, 48)), x1=None, w=UK.rnd(g, (24, 48), 0.1), b=UK.rnd(g, (24,)))
    conv = dict(x0=UK.rnd(g, (1, 24, 5, 7)), x1=None, w=UK.rnd(g, (16, 24, 3, 3), 0.1), b=UK.rnd(g, (16,)))
    for family, d, at in (("rows", rows, (0, 32, 47)), ("conv", conv, (0, 23, 4, 6))):
        assert range_word(family, d) == 0
        for value, want in ((7e4, 1), (-7e4, 1), (65504.0, 0), (-65504.0, 0), (65520.0, 1), (float("nan"), 1), (float("inf"), 1)):
            x = d["x0"].clone()
            x[at] = value
            assert range_word(family, dict(d, x0=x)) == want, (family, value)


def test_a_value_the_prologue_brings_back_into_range_does_not_raise_the_word():
    g = UK.gen(301)
    x = 1e5 + 100.0 * UK.rnd(g, (1, 33, 48))      # every input is beyond 65504; LayerNorm brings them to N(0, 1)
    d = dict(x0=x, x1=None, w=UK.rnd(g, (24, 48), 0.1), b=UK.rnd(g, (24,)), prologue="layernorm", ln=tuple(t.reshape(1, 33) for t in UK.given_ln(x.reshape(33, 48))),
             ln_g=1.0 + 0.3 * UK.rnd(g, (48,)), ln_b=0.2 * UK.rnd(g, (48,)))
    assert range_word("rows", d) == 0
    assert range_word("rows", dict(d, prologue=None)) == 1
    xc = 1e5 + 100.0 * UK.rnd(g, (1, 24, 5, 7))
    nm = UK.given_norm(xc, 4, 1.0 + 0.3 * UK.rnd(g, (24,)), 0.2 * UK.rnd(g, (24,)), 1e-5)
    c = dict(x0=xc, x1=None, w=UK.rnd(g, (16, 24, 3, 3), 0.1), b=UK.rnd(g, (16,)), norm0=nm)
    assert range_word("conv", c) == 0
    assert range_word("conv", dict(c, norm0=None)) == 1
