"""CPU: the per-layer pins and the whole-network conditions that the GPU tests put on SRVGGNetCompact's 16-bit kernels
(tests/srvgg_pin.py; test_gpu_srvgg_pin.py, test_gpu_srvgg_emu16.py), checked without a kernel.

  exact     the specification in float64 (SRVGGEmu16, the slope as the kernel applies it), run through each construction of
            srvgg_pin, gives bit for bit the directly computed float32(ref16 + x): generator, pass-through and read-out
            isolate a layer and lose nothing
  margin    the kernel-order stand-in (accumulate="f32-kernel-order": a serial f32 sum in srvgg_compact.hip's order) meets
            every pin and every condition that the GPU tests assert; srvgg_pin.asserted, which the GPU test reads, is computed
            from it
  sharp     wrong kernels, played by mutated stand-ins, each fail the criterion named for them in PLAYS
  at depth  the same faults in one layer of the 16-layer network against (a), (b), (b'), (b"): a misplaced operand (tap,
            channel, halo, residual, sub-pixel) breaks (b) and (b'); a misplaced rounding in one layer (a truncating store
            among them) breaks none of (b), (b'), (b") and moves (a) by a few per cent of a bound that a correct kernel meets
            by a tenth -- which is why the per-layer pins exist"""
import pytest
import torch

from tests import conv_pin, srvgg_pin
from tests.rrdbnet_emu16 import describe
from tests.srvgg_fp16_emu import KERNEL_ORDER, SRVGGEmu16

DTYPES = ["bf16", "f16"]
SEAMS = (2, 17, 33)          # the smallest shape with a second tile row (row 16) and a second tile column (column 32)


# ------------------------------------------------------------------------------------------------------------ mutants
class Mutant(SRVGGEmu16):
    layer = 2                # index in body of the conv whose layer is wrong

    def __init__(self, *a, **k):
        super().__init__(*a, accumulate=KERNEL_ORDER, **k)


class TruncatingStore(Mutant):
    def store(self, t, idx=None):
        if idx != self.layer:
            return super().store(t, idx)
        t = t.float()
        if self.store_type == torch.bfloat16:
            return (t.contiguous().view(torch.int32) & ~0xffff).view(torch.float32)
        r = t.to(torch.float16)
        toward = torch.nextafter(r, torch.zeros_like(r)).float()
        return torch.where(r.float().abs() > t.abs(), toward, r.float())


class UnroundedWeights(Mutant):
    def weight(self, m, idx):
        return m.weight.to(self.work) if idx == self.layer else super().weight(m, idx)


class SlopeAfterStore(Mutant):
    def act(self, v, m, idx):
        return super().act(self.store(v) if idx == self.layer else v, m, idx)


class BiasAfterRounding(Mutant):
    def conv(self, x, m, idx):
        v = super().conv(x, m, idx)
        if idx != self.layer:
            return v
        b = m.bias.float().view(1, -1, 1, 1)
        return self.store(v - b) + b


class TapsTransposed(Mutant):
    def weight(self, m, idx):
        w = super().weight(m, idx)
        return w.transpose(2, 3).contiguous() if idx == self.layer else w


class ChannelsSwapped(Mutant):
    """Input channels 0 and 1 (of one 8-channel group) change places."""

    def weight(self, m, idx):
        w = super().weight(m, idx)
        return torch.cat([w[:, 1:2], w[:, 0:1], w[:, 2:]], 1) if idx == self.layer else w


class TopHaloLost(Mutant):
    """The tiles of rows 16..31 read zeros for their halo row 15."""

    def conv(self, x, m, idx):
        out = super().conv(x, m, idx)
        if idx == self.layer and x.shape[2] > 16:
            lost = x.clone()
            lost[:, :, 15] = 0
            out[:, :, 16:32] = super().conv(lost, m, idx)[:, :, 16:32]
        return out


class LeftHaloLost(Mutant):
    """The tiles of columns 32..63 read zeros for their halo column 31."""

    def conv(self, x, m, idx):
        out = super().conv(x, m, idx)
        if idx == self.layer and x.shape[3] > 32:
            lost = x.clone()
            lost[..., 31] = 0
            out[..., 32:64] = super().conv(lost, m, idx)[..., 32:64]
        return out


class UnroundedImage(Mutant):
    def image(self, x):
        return x.to(self.work)


class RoundedResidual(Mutant):
    def tail(self, v, x):
        return super().tail(v, self.store(x.to(self.work)))


class FlippedResidual(Mutant):
    def tail(self, v, x):
        return super().tail(v, x.flip(1))


class ShuffleSwapped(Mutant):
    """Tail channel c s^2 + i s + j lands on sub-pixel (j, i)."""

    def tail(self, v, x):
        n, c, h, w = v.shape
        s = self.upscale
        return super().tail(v.view(n, 3, s, s, h, w).transpose(2, 3).reshape(n, c, h, w), x)


class PadChannelsWritten(Mutant):
    """x2: the zero-padded tail channels 12..15 are written as image channel 3, which is channel 0 of the next image."""

    def tail(self, v, x):
        y = super().tail(v, x)
        assert self.upscale == 2 and y.shape[0] > 1
        y[1:, 0] = 0
        return y


def runner(cls, s, dtype, layer=None, **kw):
    def run(sd, x):
        m = cls(num_conv=1, upscale=s, act_type="prelu", store=conv_pin.STORE[dtype], **kw)
        if layer is not None:
            m.layer = layer
        m.load_state_dict(sd)
        with torch.no_grad():
            return m(x)
    return run


def failures(fig, dtype):
    out = set()
    if fig["outside"]:
        out.add("outside")
    if fig["missed"] > conv_pin.miss_allowance(fig["values"], dtype):
        out.add("miss")
    return out


# ------------------------------------------------------------------------------------------------------------ exact, margin
def _shapes():
    return [(4, sh) for sh in srvgg_pin.SHAPES] + [(2, sh) for sh in srvgg_pin.SHAPES_X2]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["feature", "first"])
def test_constructions_lose_nothing(kind, dtype):
    for s, shape in _shapes():
        fig = srvgg_pin.CASES[kind](runner(SRVGGEmu16, s, dtype, slope_f32=True), s, dtype, shape)
        assert fig["finite"] and fig["missed"] == 0 and fig["outside"] == 0, (s, shape, fig)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pass_through_passes_through_and_the_generator_is_known(dtype):
    x = srvgg_pin.grid_image(*SEAMS, seed=1)
    gen = srvgg_pin.generator(2)
    m = SRVGGEmu16(num_conv=1, upscale=4, act_type="prelu", store=conv_pin.STORE[dtype], accumulate=KERNEL_ORDER)
    m.load_state_dict(srvgg_pin.state_dict(gen[:3], srvgg_pin.passthrough(), srvgg_pin.readout(list(range(48)), 4)))
    feats = []
    with torch.no_grad():
        m(x, features=feats)
    a = srvgg_pin.generated(x, gen)
    assert torch.equal(feats[0], a) and torch.equal(feats[1], a)
    assert len({t for t in gen[3]}) == 64 and sorted(sum(srvgg_pin.selections(2), [])[:60]) == list(range(60))
    assert {c for sel in srvgg_pin.selections(2) for c in sel} == set(range(64)) == {c for sel in srvgg_pin.selections(4) for c in sel}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(srvgg_pin.CASES))
def test_kernel_order_stand_in_meets_every_pin(kind, dtype):
    worst = 0.0
    for s, shape in _shapes():
        fig = srvgg_pin.CASES[kind](runner(SRVGGEmu16, s, dtype, accumulate=KERNEL_ORDER), s, dtype, shape)
        conv_pin.assert_pin(fig, dtype, f"{kind} x{s} {shape}")
        worst = max(worst, fig["miss"])
    print(f"stand-in {kind} {dtype}: worst miss share {worst:.2e} (cap {conv_pin.MISS_CAP[dtype]})")
    assert worst <= conv_pin.MISS_CAP[dtype] / 10          # the reference sits well inside the cap it sets for the kernel


@pytest.mark.parametrize("name", list(srvgg_pin.NETWORKS))
def test_kernel_order_stand_in_meets_every_asserted_condition(name):
    rule = srvgg_pin.asserted(name)
    for dtype in DTYPES:
        spec = srvgg_pin.network_spec(name, dtype)
        fig = srvgg_pin.judge(spec["standin"], spec, srvgg_pin.NETWORKS[name]["upscale"])
        print(f"stand-in {name} {dtype}: {describe(fig)}; asserted {sorted(rule)}")
        assert all(fig[c] for c in rule), describe(fig)
    deep = srvgg_pin.NETWORKS[name]["num_conv"] >= 16
    assert {"b", "b_mean"} <= rule and ("b_band" in rule) == deep and ("a" in rule) == (srvgg_pin.NETWORKS[name]["num_conv"] <= 16)


# ------------------------------------------------------------------------------------------------------------ sharp
# (mutant, isolation, upscale, conv under test, the criterion it must fail)
PLAYS = [(TruncatingStore, "feature", 4, 2, "miss"), (UnroundedWeights, "feature", 4, 2, "miss"), (SlopeAfterStore, "feature", 4, 2, "miss"),
         (BiasAfterRounding, "feature", 4, 2, "miss"), (TapsTransposed, "feature", 4, 2, "outside"), (ChannelsSwapped, "feature", 4, 2, "outside"),
         (TopHaloLost, "feature", 4, 2, "outside"), (LeftHaloLost, "feature", 4, 2, "outside"),
         (TruncatingStore, "first", 4, 0, "miss"), (UnroundedWeights, "first", 4, 0, "miss"), (TapsTransposed, "first", 4, 0, "outside"),
         (ChannelsSwapped, "first", 4, 0, "outside"), (TopHaloLost, "first", 4, 0, "outside"), (LeftHaloLost, "first", 4, 0, "outside"),
         (UnroundedImage, "first", 4, 0, "miss"), (RoundedResidual, "first", 4, 0, "miss"), (FlippedResidual, "first", 4, 0, "outside"),
         (FlippedResidual, "feature", 2, 2, "outside"), (ShuffleSwapped, "feature", 4, 2, "outside"), (ShuffleSwapped, "first", 2, 0, "outside"),
         (PadChannelsWritten, "feature", 2, 2, "outside"), (PadChannelsWritten, "tail", 2, 4, "outside"),
         (TapsTransposed, "tail", 4, 4, "outside"), (ChannelsSwapped, "tail", 2, 4, "outside"), (TopHaloLost, "tail", 4, 4, "outside"),
         (LeftHaloLost, "tail", 2, 4, "outside"), (ShuffleSwapped, "tail", 4, 4, "outside"), (UnroundedWeights, "tail", 4, 4, "outside"),
         (FlippedResidual, "tail", 4, 4, "outside")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant,kind,s,layer,criterion", PLAYS, ids=[f"{p[0].__name__}-{p[1]}-x{p[2]}" for p in PLAYS])
def test_every_wrong_kernel_fails_its_criterion(mutant, kind, s, layer, criterion, dtype):
    fig = srvgg_pin.CASES[kind](runner(mutant, s, dtype, layer=layer), s, dtype, SEAMS)
    print(f"{mutant.__name__} on {kind} x{s} {dtype}: {srvgg_pin.describe(fig)}")
    assert criterion in failures(fig, dtype), srvgg_pin.describe(fig)
    if mutant is TruncatingStore:
        assert 0.4 < fig["miss"] < 0.6, fig["miss"]


# ------------------------------------------------------------------------------------------------------------ at depth
DEEP = "16-prelu-x4"
DEEP_LAYER = 16              # body.16: the eighth of the 16 feature convs
STRUCTURAL = [TapsTransposed, ChannelsSwapped, TopHaloLost, LeftHaloLost, FlippedResidual, ShuffleSwapped]
ROUNDING = [TruncatingStore, UnroundedWeights, SlopeAfterStore, BiasAfterRounding, UnroundedImage, RoundedResidual]


def _deep(mutant, dtype):
    spec = srvgg_pin.network_spec(DEEP, dtype)
    m = mutant(**srvgg_pin.NETWORKS[DEEP], store=conv_pin.STORE[dtype])
    m.layer = DEEP_LAYER
    m.load_state_dict(spec["sd"])
    with torch.no_grad():
        fig = srvgg_pin.judge(m(spec["x"].double()), spec, srvgg_pin.NETWORKS[DEEP]["upscale"])
    print(f"{mutant.__name__} in body.{DEEP_LAYER} of {DEEP} {dtype}: {describe(fig)}")
    return {c for c in ("a", "b", "b_band", "b_mean") if not fig[c]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", STRUCTURAL, ids=[m.__name__ for m in STRUCTURAL])
def test_a_misplaced_operand_in_one_layer_of_16_breaks_the_local_conditions(mutant, dtype):
    """A wrong tap, channel, halo row or column, residual or sub-pixel: (b) and (b') by a factor of 5 and more beyond the
    bound, where the lost halos move the image-wide mean of (b") least."""
    broken = _deep(mutant, dtype)
    assert {"b", "b_band"} <= broken and broken & srvgg_pin.asserted(DEEP), broken


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", ROUNDING, ids=[m.__name__ for m in ROUNDING])
def test_a_misplaced_rounding_in_one_layer_of_16_breaks_no_local_condition(mutant, dtype):
    """One layer's store rounding toward zero, weights left unrounded, the slope or the bias on the wrong side of the store, the
    image unrounded into the first conv or rounded into the residual: 15 correct layers bury it.  None of (b), (b'), (b") sees
    it, and (a), which the stand-in itself meets by a tenth, sees it or not by a few per cent (printed).  Each of them fails
    its per-layer pin (PLAYS): that is what the pins are for."""
    broken = _deep(mutant, dtype)
    assert not broken & {"b", "b_band", "b_mean"}, broken
