"""CPU: the 16-bit specification of RRDBNet (tests/rrdbnet_emu16.py) and the sharpness of the conditions that the GPU tests
(test_gpu_rrdb_emu16.py) put on the kernels against it.

  (c)      one layer of the float64 variant is, bit for bit, the reference of the per-layer pins (tests/conv_pin.py)
  sharp    wrong kernels, played by mutated emulations that accumulate in float32 as a kernel does, must break a condition on
           the 33 x 47 trunk (x2plus, 66 x 94 input, one RRDB, bf16); the unmutated float32 variants must pass all of them:
             (i)   16-bit stores that truncate              -> (a), (b), (b'), (b")
             (ii)  a lost halo column at the tile seam x = 32 in one dense-block conv  -> (b')
             (iii) the second residual applied after an intermediate 16-bit rounding   -> (b'), (b")
             (iv)  x3 and x4 swapped in one block's conv5   -> (a), (b'), (b")
           In f16 the float32 accumulation error is of the size of the 16-bit rounding itself, and (ii) and (iii) -- one column,
           one more rounding per RRDB -- stay inside what accumulation order alone produces: no statistic of the output
           separates them there, so the mutants are bf16's (the figures of both are printed)."""
import pytest
import torch

from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
from tests import conv_pin
from tests.rrdbnet_emu16 import RRDBNetEmu16, conditions, describe, oracle_f64


# ------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("cin,cout,lrelu,up", [(64, 32, True, False), (192, 64, False, False), (16, 64, True, True), (64, 3, False, False)])
def test_one_layer_of_the_specification_is_the_pin_reference(dtype, cin, cout, lrelu, up):
    x, w, b = conv_pin.make_case(cin, cout, 19, 37, dtype, seed=cin * 7 + cout)
    emu = RRDBNetEmu16({}, 4, 0, conv_pin.STORE[dtype])
    got = emu.one_layer(x, w, b, lrelu=lrelu, upsample=up)
    pre, _ = conv_pin.conv_f64(x, w, b, up)
    _, ref16 = conv_pin.reference16(pre, lrelu, dtype)
    assert torch.equal(got.double(), ref16)
    # ... and the float32 variants meet the pin as a kernel must
    for acc in (torch.float32, "f32-chunked"):
        y = RRDBNetEmu16({}, 4, 0, conv_pin.STORE[dtype], accumulate=acc).one_layer(x, w, b, lrelu=lrelu, upsample=up)
        fig = conv_pin.pin(y, pre, conv_pin.conv_f64(x, w, b, up)[1], cin, lrelu, dtype)
        conv_pin.assert_pin(fig, dtype, f"{acc}")


# ------------------------------------------------------------------------------------------------------------ mutants
class Truncating(RRDBNetEmu16):
    """(i) 16-bit stores round toward zero."""

    def store(self, x):
        if self.store_type == torch.bfloat16:
            return (x.contiguous().view(torch.int32) & ~0xffff).view(torch.float32)
        r = x.to(torch.float16)
        toward = torch.nextafter(r, torch.zeros_like(r)).float()
        return torch.where(r.float().abs() > x.abs(), toward, r.float())


class LostHalo(RRDBNetEmu16):
    """(ii) the tile of columns 0..31 reads zeros for its halo column x = 32 in one conv."""
    layer = "body.0.rdb2.conv3"

    def conv(self, x, name, lrelu=False):
        out = super().conv(x, name, lrelu)
        if name == self.layer and x.shape[-1] > 32:
            lost = x.clone()
            lost[..., 32] = 0
            out[..., :32] = super().conv(lost, name, lrelu)[..., :32]
        return out


class LateSecondResidual(RRDBNetEmu16):
    """(iii) the third block stores x5 * 0.2 + x0 in 16 bits before the RRDB's residual is applied."""

    def dense_block(self, x0, prefix, rrdb_in=None):
        v = super().dense_block(x0, prefix, None)
        return v if rrdb_in is None else self.store(v * 0.2 + rrdb_in)


class SwappedGrowth(RRDBNetEmu16):
    """(iv) conv5 of one block reads x4 where x3 belongs and x3 where x4 does."""
    block = "body.0.rdb2"

    def conv(self, x, name, lrelu=False):
        if name == self.block + ".conv5":
            x = torch.cat([x[:, :128], x[:, 160:192], x[:, 128:160]], 1)
        return super().conv(x, name, lrelu)


MUTANTS = {"truncating store": Truncating, "lost halo": LostHalo, "late second residual": LateSecondResidual, "x3/x4 swapped": SwappedGrowth}
_cache = {}


def _case(dtype):
    if dtype not in _cache:
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=1)
        x = torch.rand(1, 3, 66, 94, generator=torch.Generator().manual_seed(201))
        st = conv_pin.STORE[dtype]
        _cache[dtype] = (sd, x, st, RRDBNetEmu16(sd, 2, 1, st)(x), RRDBNetEmu16(sd, 2, 1, st, accumulate=torch.float32)(x), oracle_f64(sd, 2, 1, x))
    return _cache[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_unmutated_float32_variants_meet_every_condition(dtype):
    sd, x, st, emu64, emu32, exact = _case(dtype)
    for acc in (torch.float32, "f32-chunked"):
        fig = conditions(RRDBNetEmu16(sd, 2, 1, st, accumulate=acc)(x), emu64, emu32, exact)
        print(f"{dtype} {acc}: {describe(fig)}")
        assert fig["a"] and fig["b"] and fig["b_band"] and fig["b_mean"], describe(fig)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_every_wrong_kernel_breaks_a_condition(name):
    sd, x, st, emu64, emu32, exact = _case("bf16")
    fig = conditions(MUTANTS[name](sd, 2, 1, st, accumulate="f32-chunked")(x), emu64, emu32, exact)
    print(f"bf16 {name}: {describe(fig)}")
    sd, x, st, e64, e32, ex = _case("f16")
    print(f"f16  {name}: {describe(conditions(MUTANTS[name](sd, 2, 1, st, accumulate='f32-chunked')(x), e64, e32, ex))}")
    assert not (fig["a"] and fig["b"] and fig["b_band"] and fig["b_mean"]), f"{name} passes for a correct kernel: {describe(fig)}"
