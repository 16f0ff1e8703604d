"""The crafted cases of tests/vae_cases.py without a GPU: what each case is built for really holds (the key chunks, the late
maxima, the offset statistics, the ties), every named fault of tests/vae_ref.py fails the case named for it by at least ten
tolerances when it is applied to the float32 restatement, and the frames of the u8 criterion keep their thin samples under the cap."""
import math

import numpy as np
import pytest
import torch

from tests import vae_cases as C
from tests import vae_ref as R
from tests.swin2sr_ref import u8_check


def test_every_fault_has_a_case():
    assert set(C.FAULT_CASE) == set(R.FAULTS) and set(C.FAULT_CASE.values()) <= set(C.NAMES)


@pytest.mark.parametrize("name", C.NAMES)
def test_cases_are_seeded_and_finite(name):
    case = C.by_name(name)
    assert list(case.sd) == list(R.spec(**case.cfg)) and all(v.dtype == torch.float32 for v in case.sd.values())
    z, y64, tol = C.reference(name)
    s = 2 ** (len(R.config(**case.cfg)["block_out_channels"]) - 1)
    assert tuple(y64.shape) == (1, 3, z.shape[2] * s, z.shape[3] * s) and bool(torch.isfinite(y64).all())
    assert tol > 0 or name == "rounding_ties"      # zero weights: the float32 route is exact there
    again = C._build(name)
    assert all(torch.equal(again.sd[k], case.sd[k]) for k in case.sd) and torch.equal(again.latents, case.latents)


@pytest.mark.parametrize("fault", [f for f in R.FAULTS if f not in R.QUANTISER_FAULTS])
def test_fault_fails_its_case_by_ten_tolerances(fault):
    name = C.FAULT_CASE[fault]
    case = C.by_name(name)
    with torch.no_grad():
        if fault in R.FRAME_FAULTS:
            latents, y64, tol = C.frame_reference(name)
            got = R.decode_latents_float(case.sd, latents, torch.float32, fault=fault, **case.cfg)
        else:
            z, y64, tol = C.reference(name)
            got = R.decode(case.sd, z, fault=fault, **case.cfg)
    err = float((got.double() - y64).abs().max())
    print(f"{fault} on {name}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.1f}")
    assert tol > 0 and err >= 10 * tol


def test_round_half_up_fails_the_ties():
    """The quantiser's fault acts on samples that are ties in float32: channel 0 (100.5) and channel 2 (200.5) round down to even."""
    case = C.by_name("rounding_ties")
    want = C.ties_expected_frame(case)
    assert want[0, 0].tolist() == [100, 102, 200] and tuple(want.shape) == (6, 10, 3)
    y32 = R.decode_latents_float(case.sd, case.latents, torch.float32, **case.cfg)
    assert torch.equal(R.quantise(y32), want)
    wrong = R.quantise(y32, fault="round_half_up")
    assert wrong[0, 0].tolist() == [101, 102, 201] and int((wrong != want).sum()) == 2 * 6 * 10


def test_many_chunks_has_a_ragged_last_chunk():
    n = int(np.prod(C.by_name("many_chunks").latents.shape[2:]))
    assert n == 135 and math.ceil(n / R.STREAM_CHUNK) == 5 and n % R.STREAM_CHUNK == 7 and n % 16 == 7


def test_late_maxima_lie_in_the_last_chunk():
    case = C.by_name("late_maxima")
    taps = {}
    with torch.no_grad():
        R.decode(case.sd, C.z_of(case), taps=taps, **case.cfg)
    s = taps["scores"]
    n = s.shape[0]
    last0 = (n - 1) // R.STREAM_CHUNK * R.STREAM_CHUNK
    share = float((s.argmax(dim=1) >= last0).double().mean())
    gap = (s[:, last0:].max(dim=1).values - s[:, :last0].max(dim=1).values)
    print(f"late_maxima: {100 * share:.0f} % of the rows have their maximum in the last chunk; it lies {float(gap.median()):.2f} above the earlier ones (median)")
    assert share >= C.LAST_CHUNK_SHARE and float(gap.median()) > 1.0      # exp(-gap) is what a missing rescale gets wrong by


def test_streamed_attention_is_the_softmax():
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn((45, 16), generator=g, dtype=torch.float64) for _ in range(3))
    want = torch.softmax(q @ k.t() * 0.25, dim=1) @ v
    assert float((R.streamed_attention(q, k, v, 0.25) - want).abs().max()) < 1e-12
    assert float((R.streamed_attention(q, k, v, 0.25, rescale=False) - want).abs().max()) > 1e-3


def test_offset_stats_puts_the_mean_far_out():
    case = C.by_name("offset_stats")
    bias = case.sd["decoder.mid_block.resnets.0.conv1.bias"]
    assert float(bias.mean()) > 900 and float(bias.std()) < 1.0


@pytest.mark.parametrize("name", C.FRAME_CASES)
def test_thin_samples_stay_under_the_cap(name):
    """The u8 criterion leaves out the samples whose float64 value x 255 lies within 255 tol of a rounding boundary; the cases are
    chosen so that these are at most 2 % of at least 1000 samples, and the float32 restatement meets the criterion itself."""
    case = C.by_name(name)
    latents, y64, tol = C.frame_reference(name)
    y32 = R.decode_latents_float(case.sd, latents, torch.float32, **case.cfg)
    excluded, wrong, n = u8_check(R.quantise(y32), y64, tol)
    clamped = float(((y64 <= 0) | (y64 >= 1)).double().mean())
    print(f"{name}: tol {tol:.3e}, {excluded} of {n} samples thin ({100.0 * excluded / n:.2f} %), {wrong} wrong (f32 CPU), {100 * clamped:.1f} % on the clamp")
    assert n >= 1000 and excluded <= C.MAX_THIN * n and wrong == 0
    assert 0.02 < clamped < 0.5      # the clamp acts, and does not decide most samples
