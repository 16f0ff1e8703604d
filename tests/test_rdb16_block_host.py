"""CPU: the per-block tests of the 16-bit dense block (tests/rdb16_block.py, test_gpu_rdb16_block.py) checked against themselves.

  staging   rows16_bytes / rows16_values round-trip and are the layout band_api.cpp documents
  exact     every exact case of the GPU file has one answer (rdb16_block.exactness)
  sharp     wrong kernels, played by mutated emulations that accumulate in the kernels' chunk order, differ from `expected`
            in at least one value, in bf16 and in f16, on the smallest shape where the defect can show
  random    the two rules of the random-weights part accept each correct float32 stand-in judged by the other alone, and
            refuse the mutants; F (rdb16_block.FLOOR) is the measured figure and stays below a quarter of the mildest mutant"""
import pytest
import torch

from tests import conv_pin
from tests import rdb16_block as B
from tests.rrdbnet_emu16 import RRDBNetEmu16
from tests.test_rrdb_emu16_host import Truncating

DTYPES = ["bf16", "f16"]


# ------------------------------------------------------------------------------------------------------------ staging
@pytest.mark.parametrize("dtype", DTYPES)
def test_staging_round_trips(dtype):
    h, w = 3, 5
    x = torch.randn(1, 64, h, w, generator=torch.Generator().manual_seed(1)).to(conv_pin.STORE[dtype]).float()
    raw = B.rows16_bytes(x, dtype)
    assert raw.dtype == torch.uint8 and raw.numel() == h * w * 64 * 2
    assert torch.equal(B.rows16_values(raw, h, w, dtype), x)
    # [chunk][row][column][16 elements]: element 7 of chunk 2 at (row 1, column 4) is channel 39
    at = ((2 * h + 1) * w + 4) * 16 + 7
    assert float(raw.view(conv_pin.STORE[dtype])[at]) == float(x[0, 39, 1, 4])


# ------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_exact_case_has_one_answer(dtype, signed):
    """Non-negative cases meet the plain criterion (every partial sum of every conv a float32 value: span < 2^24).  Signed
    cases cannot: LeakyReLU'd negatives that nearly cancel leave values of 2^-20 beside sums of hundreds (span up to 2^30 in
    bf16, 2^34 in f16); there every value is decided per output value, by span_local or by the monotone-interval argument."""
    worst = {"span": 0.0, "span_local": 0.0, "top": 0.0, "wide": 0}
    f64_equal = True
    for hw in B.SHAPES + B.SEG_SHAPES:
        for r in (0, 1, 2):
            sd, x0, rrdb_in = B.exact_case(hw, r, signed, dtype)
            assert not torch.equal(x0, rrdb_in)
            fig = B.exactness(sd, x0, r, rrdb_in, dtype)
            assert fig["span"] < 2.0 ** 53, (hw, r, fig)
            assert fig["undecided"] == 0, (hw, r, fig)
            if not signed:
                assert fig["span"] < 2.0 ** 24 and fig["wide"] == 0, (hw, r, fig)
                assert fig["f64_equal"], (hw, r)
            assert fig["standins_equal"], (hw, r)
            assert fig["top"] < 2.0 ** 11, (hw, r, fig)          # nothing near f16's range
            f64_equal &= fig["f64_equal"]
            for k in worst:
                worst[k] = max(worst[k], fig[k])
    print(f"{dtype} {'signed' if signed else 'nonneg'}: span 2^{torch.log2(torch.tensor(worst['span'])):.1f}, per value 2^"
          f"{torch.log2(torch.tensor(worst['span_local'])):.1f}, at most {worst['wide']} values decided by the interval, "
          f"largest |value| {worst['top']:.0f}, float64 variant equal everywhere: {f64_equal}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_tag_bound_cases_have_one_answer(dtype):
    """The two tall shapes of test_gpu_strip_queue.py (256 and 257 positions, 17 columns), non-negative, r = 0 and 2: the plain
    criterion, as for every non-negative case above."""
    for hw in B.TAG_SHAPES:
        for r in (0, 2):
            sd, x0, rrdb_in = B.exact_case(hw, r, False, dtype)
            assert not torch.equal(x0, rrdb_in)
            fig = B.exactness(sd, x0, r, rrdb_in, dtype)
            assert fig["span"] < 2.0 ** 24 and fig["wide"] == 0 and fig["undecided"] == 0, (hw, r, fig)
            assert fig["f64_equal"] and fig["standins_equal"], (hw, r)
            assert fig["top"] < 2.0 ** 11, (hw, r, fig)


# ------------------------------------------------------------------------------------------------------------ mutants
class LostHalo(RRDBNetEmu16):
    """The strip of columns 0..15 reads zeros for its halo column x = 16 in one of conv1..conv4."""
    k = 3

    def conv(self, x, name, lrelu=False):
        out = super().conv(x, name, lrelu)
        if name.endswith(f".conv{self.k}") and x.shape[-1] > 16:
            lost = x.clone()
            lost[..., 16] = 0
            out[..., :16] = super().conv(lost, name, lrelu)[..., :16]
        return out


class LostHalo1(LostHalo):
    k = 1


class StaleRow(RRDBNetEmu16):
    """conv4 reads row 0 of x3 where row 12 belongs (a circular row window one slot off)."""

    def conv(self, x, name, lrelu=False):
        if name.endswith(".conv4") and x.shape[2] > 12:
            x = x.clone()
            x[:, 128:160, 12] = x[:, 128:160, 0]
        return super().conv(x, name, lrelu)


class LateSecondResidual(RRDBNetEmu16):
    """The third block stores x5 * 0.2 + x0 in 16 bits before the RRDB's residual is applied."""

    def dense_block(self, x0, prefix, rrdb_in=None):
        v = super().dense_block(x0, prefix, None)
        return v if rrdb_in is None else self.store(v * 0.2 + rrdb_in)


class SwappedGrowth(RRDBNetEmu16):
    """conv5 reads x4 where x3 belongs and x3 where x4 does."""

    def conv(self, x, name, lrelu=False):
        if name.endswith(".conv5"):
            x = torch.cat([x[:, :128], x[:, 160:192], x[:, 128:160]], 1)
        return super().conv(x, name, lrelu)


class Residuals(RRDBNetEmu16):
    """The block with its residual arithmetic spelled out, for the two mutants below."""
    res_scale = 0.2

    def residual(self, v, res):
        return v * self.res_scale + res

    def dense_block(self, x0, prefix, rrdb_in=None):
        feats = [x0]
        for k in range(1, 5):
            feats.append(self.store(self.conv(torch.cat(feats, 1), f"{prefix}.conv{k}", lrelu=True)))
        v = self.residual(self.conv(torch.cat(feats, 1), f"{prefix}.conv5"), x0)
        return self.store(v if rrdb_in is None else self.residual(v, rrdb_in))


class FusedResidual(Residuals):
    """v * 0.2f + res as one fused multiply-add: the product (24 x 24 bits, exact in float64) is not rounded to float32."""

    def residual(self, v, res):
        return (v.double() * float(torch.tensor(0.2, dtype=torch.float32)) + res.double()).float()


class Quarter(Residuals):
    """0.25 in place of 0.2 in the residuals."""
    res_scale = 0.25


class QuarterSlope(RRDBNetEmu16):
    """0.25 in place of 0.2 in LeakyReLU (signed cases only: the non-negative ones never take that branch)."""

    def conv(self, x, name, lrelu=False):
        out = super().conv(x, name, False)
        return torch.where(out > 0, out, out * 0.25) if lrelu else out


# name -> (class, smallest shape where it can show, the r it needs or None, needs a signed case)
MUTANTS = {"truncating store": (Truncating, (5, 15), None, False),
           "lost halo, conv3": (LostHalo, (12, 17), None, False),
           "lost halo, conv1": (LostHalo1, (12, 17), None, False),
           "stale row": (StaleRow, (13, 33), None, False),
           "late second residual": (LateSecondResidual, (5, 15), 2, False),
           "x3/x4 swapped": (SwappedGrowth, (5, 15), None, False),
           "fused multiply-add": (FusedResidual, (5, 15), None, False),
           "0.25 for 0.2": (Quarter, (5, 15), None, False),
           "slope 0.25": (QuarterSlope, (5, 15), None, True)}


def test_the_residual_spelled_out_is_the_specification():
    """(the base of two mutants must itself be `expected`)"""
    sd, x0, rrdb_in = B.exact_case((5, 15), 2, True, "bf16")
    assert torch.equal(B.block(B.emu(sd, "bf16", "f32-chunked", Residuals), x0, 2, rrdb_in), B.expected(sd, x0, 2, rrdb_in, "bf16"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(MUTANTS))
def test_wrong_kernels_break_equality(name, dtype):
    """One mutant shows in the signed cases only, the fused multiply-add.  On non-negative integers the residual is c / 5 + x0
    with c an integer: for c no multiple of 5 the sum is at least 1 / (5 * 2^10) from any 16-bit rounding boundary, far more
    than a float32 rounding, and for c a multiple of 5 the unfused product rounds to the integer c / 5 itself, a boundary only
    from 256 (bf16) or 2048 (f16) on.  In the signed cases c * 0.2f cancels against x0 here and there: the two roundings give 0
    where the fused form keeps c * (0.2f - 1 / 5)."""
    cls, hw, need_r, need_signed = MUTANTS[name]
    differing = {}
    for signed in ([True] if need_signed else [False, True]):
        for r in ([need_r] if need_r is not None else [0, 1, 2]):
            sd, x0, rrdb_in = B.exact_case(hw, r, signed, dtype)
            want = B.expected(sd, x0, r, rrdb_in, dtype)
            got = B.block(B.emu(sd, dtype, "f32-chunked", cls), x0, r, rrdb_in)
            differing[("signed" if signed else "nonneg", r)] = int((got != want).sum())
    print(f"{name} {dtype} {hw}: values that differ of {64 * hw[0] * hw[1]}: {differing}")
    if name == "fused multiply-add":
        differing = {k: v for k, v in differing.items() if k[0] == "signed"}
    assert all(differing.values()), differing


# ------------------------------------------------------------------------------------------------------------ random weights
_random = {}


def _random_case(hw, r, dtype, seed=B.RANDOM_SEED):
    key = (hw, r, dtype, seed)
    if key not in _random:
        x0, rrdb_in = B.random_inputs(hw[0], hw[1], dtype, seed)
        _random[key] = (x0, rrdb_in) + B.specs(B.random_state_dict(), x0, r, rrdb_in, dtype)
    return _random[key]


CASES = [(hw, r, dtype) for hw in sorted({hw for hw, _ in B.RANDOM_CASES}) for r in (0, 2) for dtype in DTYPES]
DRAWS = [0, 1, 2, 3]          # input draws over which F is measured; the GPU file's is B.RANDOM_SEED


def test_random_rules_accept_each_standin_judged_by_the_other():
    """On the GPU file's cases each stand-in passes both rules with the other as the only stand-in.  F is twice the largest count
    that one stand-in shows where the other shows none, over these cases and the same cases with three more input draws (one
    draw holds too few such cases: 0 to 10 was seen per draw).  On the other draws the size rule is printed, not asserted: with a
    single stand-in that happens to flip nothing near a cancelling output, it refuses the other's cluster of 2 to 3 ulps
    (DESIGN.md has the figures)."""
    assert B.RANDOM_SEED in DRAWS
    lonely = 0
    for seed in DRAWS:
        for hw, r, dtype in CASES:
            x0, rrdb_in, spec64, standins = _random_case(hw, r, dtype, seed)
            for me, other in ((0, 1), (1, 0)):
                fig = B.share_and_size(standins[me], spec64, [standins[other]], dtype)
                print(f"draw {seed} {hw} r {r} {dtype} stand-in {B.STANDINS[me]}: {B.describe(fig)}")
                if seed == B.RANDOM_SEED:
                    assert fig["share"] and fig["size"], B.describe(fig)
                if fig["standin_counts"][0] == 0:
                    lonely = max(lonely, fig["count"])
    print(f"largest count beside a stand-in that shows none: {lonely}")
    assert B.FLOOR == 2 * lonely, f"F = {B.FLOOR}, measured twice {lonely}"


@pytest.mark.parametrize("name", list(MUTANTS))
def test_random_rules_refuse_the_mutants(name):
    """Each mutant, judged as the kernel with both stand-ins, fails a rule on every case that has what it loses (every shape
    here is wider than a strip and higher than a position; the late residual needs r = 2).  F stays below a quarter of the
    mildest mutant's count on the smallest case.  The fused multiply-add is the exception: one rounding fewer in float32 moves a
    value by half a float32 ulp, which crosses a 16-bit boundary once in 2^16 (bf16) or 2^13 (f16) values -- fewer than another
    summation order flips -- and randn values do not cancel exactly as the integers do.  No rule on one block's output with
    random weights can tell it from a correct kernel (its figures are printed); the signed exact cases do."""
    cls, _, need_r, _ = MUTANTS[name]
    smallest = min(hw for hw, _ in B.RANDOM_CASES)
    for hw, r, dtype in CASES:
        if need_r is not None and r != need_r:
            continue
        x0, rrdb_in, spec64, standins = _random_case(hw, r, dtype)
        got = B.block(B.emu(B.random_state_dict(), dtype, "f32-chunked", cls), x0, r, rrdb_in)
        fig = B.share_and_size(got, spec64, standins, dtype)
        print(f"{name} {hw} r {r} {dtype}: {B.describe(fig)}")
        if name == "fused multiply-add":
            continue
        assert not (fig["share"] and fig["size"]), f"{name} passes for a correct kernel: {B.describe(fig)}"
        if hw == smallest:
            assert B.FLOOR < fig["count"] / 4, f"F = {B.FLOOR} against the mutant's {fig['count']}"
