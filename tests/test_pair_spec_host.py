"""CPU: the pair specification of the default f32 form (tests/pair_spec.py) and the sharpness of the conditions that the GPU
tests (test_gpu_pair_spec.py) put on the kernels against it.

  split    pair(x) == x for every x of <= 22 significant bits in the normal f16 range; |x - pair(x)| <= 2^-22 |x| on
           6.1e-5 <= |x| <= 65504 and <= 2^-35 below; the join is exact in float32; the staging encode has its inverse
  exact    one-hot and small-integer cases: the float64 specification, the float32 stand-ins and torch agree bit for bit
  sharp    wrong kernels, played by mutants of the specification that accumulate in float32 as a kernel does, must break a
           condition by a ratio >= 8 (twice the threshold 4); the unmutated stand-ins must pass every condition.
           One layer (2 x 19 x 37; 64->32, 192->64, 16->64; activations scaled by 1 and by 1e-3) and one dense block
           (synthetic weights, the 23 x 47 conv_first output of a rand image).  Ratios measured here, (b) max / (b') band /
           (b") mean; layer: range over the six cases, block: in conv3 (vi: conv5) of the first block:
             (i)   x_lo of one tap of one 16-channel chunk dropped        layer 74..253 / 97..424 / 86..376     block 3 / 20 / 18
             (ii)  x_lo of the halo column x = 32 lost to the tile of columns 0..31
                                                                          layer 232..394 / 571..736 / 16..21    block 9 / 60 / 5
             (iii) w_lo of one tap dropped                                layer 209..255 / 356..424 / 332..383
             (iv)  the cross sum scaled by 2^-10 instead of 2^-11         layer 802..956 / 1497..1823 / 1410..1698
             (v)   the output's lo plane zero in column 31                layer 704..1021 / 855..1080 / 24..30
             (vi)  conv5's residual x0 taken from its hi half alone       block 2046 / 10420 / 9264
           (test_table_of_mutants prints the table; DESIGN.md, "The pair specification of the f32 form", holds a copy).

Known blind spots, not tests -- no statistic of the output separates them from accumulation order (measured with mutants of the
same kind, (b) / (b') / (b")):
  adding the lo x lo term (w_lo x_lo 2^-22)     layer 1.00 / 1.10..1.15 / 1.02..1.04, block 1.00 / 1.22 / 1.00: it is 2^-22 of a
                                                product, the size of one f32 rounding of the sum
  truncating the lo half of every store         layer 1.00 / 1.10..1.15 / 1.02..1.03, block 1.00 / 2.26 / 1.85: one unit of lo is
                                                2^-21 of hi's unit, below the f32 rounding of the value that is split
Seen, but weakly:
  v * s + res as ONE fma instead of two roundings   first block 1.00 / 1.24 / 1.03; third block of an RRDB (two residuals, the
                                                order figures five times smaller behind the second 0.2) 2.0 / 2.96 / 2.37.  The
                                                kernels did exactly this (the compiler fused __fmul_rn / __fadd_rn) and showed
                                                2.5 .. 2.9 in the mean and 3.1 .. 4.3 in the bands on the GPU, one case beyond 4,
                                                until scale_add_2r (f16x2_common.h); now 1.1 .. 1.3 and 1.6 .. 2.5."""
import pytest
import torch
import torch.nn.functional as F

from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
from tests import conv_pin
from tests.pair_spec import (STANDINS, PairRRDBNet, PairSpec, conditions, describe, fold_restated, join, make_case, pair, pair_bytes,
                             pair_values, split, worst_ratio)


# ------------------------------------------------------------------------------------------------------------ split
def test_values_of_22_significant_bits_are_their_pair():
    g = torch.Generator().manual_seed(1)
    m = torch.randint(1 << 21, 1 << 22, (20000,), generator=g).double()              # 22-bit significands
    e = torch.randint(-14 - 21, 15 - 21 + 1, (20000,), generator=g).double()         # values in [2^-14, 2^16): the normal f16 range
    x = (m * torch.exp2(e)).float()
    x = torch.cat([x[x.abs() <= 65504.0], -x[x.abs() <= 65504.0], torch.tensor([0.0, 1.0, 65504.0, 2.0 ** -14])])
    assert torch.equal(pair(x), x.double())


def test_pair_error_bounds_and_exact_join():
    g = torch.Generator().manual_seed(2)
    x = torch.exp(torch.empty(200000).uniform_(-9.7, 11.08, generator=g)) * (torch.randint(0, 2, (200000,), generator=g) * 2 - 1)
    x = x[(x.abs() >= 6.1e-5) & (x.abs() <= 65504.0)].float()
    err = (x.double() - pair(x)).abs()
    assert bool((err <= 2.0 ** -22 * x.double().abs()).all()), float((err / x.double().abs()).max())
    small = torch.exp(torch.empty(100000).uniform_(-40.0, -9.71, generator=g)).float()
    small = torch.cat([small, -small, torch.tensor([2.0 ** -24, 2.0 ** -25, 3e-8])])
    assert float((small.double() - pair(small)).abs().max()) <= 2.0 ** -35
    for v in (x, small):
        hi, lo = split(v)
        joined = torch.addcmul(hi, lo, torch.tensor(1.0 / 2048.0))                    # float32 arithmetic
        assert torch.equal(joined.double(), join((hi, lo)))                           # exact in float32


def test_staging_bytes_have_their_inverse():
    x = torch.randn(1, 64, 5, 7, generator=torch.Generator().manual_seed(3)) * 3.0
    raw = pair_bytes(x)
    assert raw.dtype == torch.uint8 and raw.numel() == 5 * 7 * 64 * 4
    assert torch.equal(pair_values(raw, 5, 7), pair(x))
    # the layout: chunk 1, row 2, column 3 -> 16 hi halves, then 16 scaled-lo halves of channels 16..31
    at = ((1 * 5 + 2) * 7 + 3) * 64
    hi, lo = split(x)
    assert torch.equal(raw[at:at + 32].view(torch.float16).float(), hi[0, 16:32, 2, 3])
    assert torch.equal(raw[at + 32:at + 64].view(torch.float16).float(), lo[0, 16:32, 2, 3])


# ------------------------------------------------------------------------------------------------------------ exact cases
ACCS = (torch.float64,) + STANDINS + ("f32-steps",)


@pytest.mark.parametrize("tap", range(9))
def test_one_hot_cases_agree_bit_for_bit(tap):
    x, w, b, ref = conv_pin.one_hot_case(32, 64, 9, 35, tap)
    for acc in ACCS:
        assert torch.equal(PairSpec(acc).one_layer(x, w, b), ref.double()), f"{acc} tap {tap}"
    up = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1).double()
    for acc in ACCS:
        for form in ("3x3", "2x2"):
            assert torch.equal(PairSpec(acc).one_layer(x, w, b, upsample=True, upconv=form), up), f"{acc} {form} tap {tap}"


def test_small_integer_case_agrees_bit_for_bit():
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-9, 10, (2, 48, 10, 37), generator=g).float()
    w = torch.randint(-3, 4, (32, 48, 3, 3), generator=g).float()
    b = torch.randint(-5, 6, (32,), generator=g).float()
    ref = F.conv2d(x, w, b, padding=1)
    lre = F.leaky_relu(ref.double(), 0.5).float()                                   # (the spec's slope is 0.2f: checked on ref >= 0 only)
    up = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    for acc in ACCS:
        s = PairSpec(acc)
        assert torch.equal(s.one_layer(x, w, b), ref.double()), acc
        got = s.one_layer(x, w, b, lrelu=True)
        assert torch.equal(got[ref >= 0], lre.double()[ref >= 0]), acc
        for form in ("3x3", "2x2"):
            assert torch.equal(s.one_layer(x, w, b, upsample=True, upconv=form), up.double()), (acc, form)


def test_the_restated_fold_is_the_librarys():
    from neural_enhanced_super_resolution_amd.rrdbnet import fold_upconv_weights
    w = torch.randn(5, 7, 3, 3, generator=torch.Generator().manual_seed(6))
    assert torch.equal(fold_restated(w), fold_upconv_weights(w))


# ------------------------------------------------------------------------------------------------------------ mutants
class Mutant(PairRRDBNet):
    target = "_one"          # the layer it strikes: the single layer, or one conv of the dense block


class DroppedTapChunkLo(Mutant):
    """(i) x_lo of tap (0, 2) of the second 16-channel chunk (the first if there is one only) never meets w_hi."""

    def sums(self, xp, wp, name, pad=1, wh_x=None):
        if name == self.target:
            wh_x = wp[0].clone()
            c = 16 if wh_x.shape[1] > 16 else 0
            wh_x[:, c:c + 16, 0, 2] = 0
        return super().sums(xp, wp, name, pad, wh_x)


class LostHaloLo(Mutant):
    """(ii) the tile of columns 0..31 reads zeros for the lo halves of its halo column x = 32."""

    def sums(self, xp, wp, name, pad=1, wh_x=None):
        main, cross = super().sums(xp, wp, name, pad, wh_x)
        if name == self.target and xp[0].shape[-1] > 32:
            lost = xp[1].clone()
            lost[..., 32] = 0
            cross[..., :32] = super().sums((xp[0], lost), wp, name, pad, wh_x)[1][..., :32]
        return main, cross


class DroppedTapWeightLo(Mutant):
    """(iii) w_lo of tap (1, 0) is zero."""

    def sums(self, xp, wp, name, pad=1, wh_x=None):
        if name == self.target:
            wl = wp[1].clone()
            wl[:, :, 1, 0] = 0
            wp = (wp[0], wl)
        return super().sums(xp, wp, name, pad, wh_x)


class CrossScaledWrong(Mutant):
    """(iv) the cross sum enters with 2^-10."""

    def combine(self, main, cross, bias):
        return super().combine(main, cross * 2.0, bias)


class OutputLoColumnZero(Mutant):
    """(v) the stored lo plane is zero in column 31."""

    def store(self, v):
        hi, lo = super().store(v)
        lo[..., 31] = 0
        return hi, lo


class ResidualFromHi(Mutant):
    """(vi) conv5 adds x0's hi half alone."""

    def layer(self, xp, wp, bias, name="", **kw):
        if name == self.target:
            kw["res1"] = (kw["res1"][0], torch.zeros_like(kw["res1"][1]))
        return super().layer(xp, wp, bias, name, **kw)


LAYER_MUTANTS = {"(i) tap-chunk x_lo": DroppedTapChunkLo, "(ii) halo column x_lo": LostHaloLo, "(iii) tap w_lo": DroppedTapWeightLo,
                 "(iv) cross 2^-10": CrossScaledWrong, "(v) output lo column": OutputLoColumnZero}
BLOCK_MUTANTS = {"(i) tap-chunk x_lo": (DroppedTapChunkLo, "conv3"), "(ii) halo column x_lo": (LostHaloLo, "conv3"),
                 "(vi) residual from hi": (ResidualFromHi, "conv5")}
LAYERS = [(64, 32), (192, 64), (16, 64)]
SCALES = [1.0, 1e-3]
_cache = {}


def _layer_case(cin, cout, scale):
    k = (cin, cout, scale)
    if k not in _cache:
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        x, w, b = make_case(cin, cout, 19, 37, seed=cin * 11 + cout, scale=scale)
        _cache[k] = (x, w, b, PairSpec().one_layer(x, w, b, lrelu=True), [PairSpec(a).one_layer(x, w, b, lrelu=True) for a in STANDINS])
    return _cache[k]


def _block_case():
    if "block" not in _cache:
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=4, num_block=1)
        x = torch.rand(1, 3, 23, 47, generator=torch.Generator().manual_seed(401))
        x0 = PairRRDBNet(sd, 4, 1).first(x)
        run = lambda net: join(net.dense_block(x0, "body.0.rdb1"))      # noqa: E731
        _cache["block"] = (sd, x0, run, run(PairRRDBNet(sd, 4, 1)), [run(PairRRDBNet(sd, 4, 1, accumulate=a)) for a in STANDINS])
    return _cache["block"]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("cin,cout", LAYERS)
def test_unmutated_stand_ins_meet_every_condition_on_a_layer(cin, cout, scale):
    x, w, b, spec64, spec32 = _layer_case(cin, cout, scale)
    for acc in STANDINS + ("f32-steps",):
        fig = conditions(PairSpec(acc).one_layer(x, w, b, lrelu=True), spec64, spec32)
        print(f"layer {cin}->{cout} x{scale:g} {acc}: {describe(fig)}")
        assert fig["ok"], describe(fig)


def test_unmutated_stand_ins_meet_every_condition_on_a_block():
    sd, x0, run, spec64, spec32 = _block_case()
    for acc in STANDINS + ("f32-steps",):
        fig = conditions(run(PairRRDBNet(sd, 4, 1, accumulate=acc)), spec64, spec32)
        print(f"block {acc}: {describe(fig)}")
        assert fig["ok"], describe(fig)


@pytest.mark.parametrize("name", list(LAYER_MUTANTS))
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("cin,cout", LAYERS)
def test_every_wrong_layer_breaks_a_condition_by_twice_the_threshold(cin, cout, scale, name):
    x, w, b, spec64, spec32 = _layer_case(cin, cout, scale)
    fig = conditions(LAYER_MUTANTS[name]({}, 4, 0, accumulate="f32-chunked").one_layer(x, w, b, lrelu=True), spec64, spec32)
    print(f"layer {cin}->{cout} x{scale:g} {name}: {describe(fig)}")
    assert worst_ratio(fig) >= 8, f"{name} is not told from a correct kernel: {describe(fig)}"


@pytest.mark.parametrize("name", list(BLOCK_MUTANTS))
def test_every_wrong_block_breaks_a_condition_by_twice_the_threshold(name):
    sd, x0, run, spec64, spec32 = _block_case()
    cls, conv = BLOCK_MUTANTS[name]
    net = cls(sd, 4, 1, accumulate="f32-chunked")
    net.target = f"body.0.rdb1.{conv}"
    fig = conditions(run(net), spec64, spec32)
    print(f"block {name} in {conv}: {describe(fig)}")
    assert worst_ratio(fig) >= 8, f"{name} is not told from a correct kernel: {describe(fig)}"


def test_table_of_mutants():
    """The table of DESIGN.md: per mutant and level the range of each condition's ratio (asserted above; printed here)."""
    rows = []
    for name, cls in LAYER_MUTANTS.items():
        figs = [conditions(cls({}, 4, 0, accumulate="f32-chunked").one_layer(c[0], c[1], c[2], lrelu=True), c[3], c[4])
                for c in (_layer_case(ci, co, s) for ci, co in LAYERS for s in SCALES)]
        rows.append((f"layer {name}", figs))
    sd, x0, run, spec64, spec32 = _block_case()
    for name, (cls, conv) in BLOCK_MUTANTS.items():
        net = cls(sd, 4, 1, accumulate="f32-chunked")
        net.target = f"body.0.rdb1.{conv}"
        rows.append((f"block {name}", [conditions(run(net), spec64, spec32)]))
    for what, figs in rows:
        cells = [f"{k} {min(f[k] for f in figs):.0f}..{max(f[k] for f in figs):.0f}" for k in ("ratio", "band_ratio", "mean_ratio")]
        print(f"{what:32s} max {cells[0][6:]:>12s} | band {cells[1][11:]:>12s} | mean {cells[2][11:]:>12s}")
        assert all(worst_ratio(f) >= 8 for f in figs), what
