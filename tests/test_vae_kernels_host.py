"""CPU: proof that the per-launch cases of tests/vae_kernels.py bite, and that their premises hold.

  * The float64 emulation of each kernel's indexing (tests/vae_kernel_ref.py), run on the PACKED arguments and unpacked again,
    gives the dense reference: bit for bit on the exact cases, within the case's tolerance on the toleranced ones, with every
    padded column as csrc/vae_api.h documents and nothing stored behind the buffer.  That is the round trip of the packing helpers.
  * Every named fault of the emulation fails the case that FAULT_CASE assigns to it: an exact case is no longer bit-equal (or a
    padded column, a sentinel or the memory behind the buffer is wrong); a toleranced case has err / tol > 1 (or a pad is wrong:
    there is no tolerance on a pad).  The smallest toleranced miss is printed.
  * Exact cases: sum_k |x_k| |w_k| (+ |bias| + |residual|) < 2^24 in units of the case's grid, so every partial sum is an exact
    float32 in any order.  Selector cases: every query's best key leads the runner-up by at least 120 in scaled score, at least a
    quarter of the queries select a key of the first chunk and at least a quarter one of the last.
  * Every toleranced quantity has a tolerance above 0, but a copy (beta) and the mean of integer inputs, which float32 restates exactly.
"""
import math

import pytest
import torch

from tests import vae_kernel_ref as R
from tests import vae_kernels as V

ISSUE_FAULTS = ("k_tail_dropped", "chunk_weight_offset_ignores_c0", "weight_rows_by_cs_not_cinp", "z_block_channel_offset_dropped", "absent_tile_stored",
                "edge_store_unguarded", "padding_normalised", "nearest2_source_width_not_halved", "res_stride_is_coutp", "f32_plane_stride", "u8_round_half_up",
                "u8_no_clamp", "last_block_not_clamped", "finish_first_trip_only", "cpg_over_256_unwritten", "idle_pixel_lane_counted", "variance_unbiased",
                "raw_moments_f32", "padded_channels_not_zero", "ragged_rows_written", "norm_with_silu", "res_dropped", "tiles_past_the_fourth_dropped",
                "scale_by_cs_not_c", "ragged_keys_score_zero", "no_rescale_on_new_max", "sum_not_rescaled", "tiles_past_the_first_round_dropped",
                "multiplied_not_divided", "plane_stride", "columns_past_c_not_zero")
FAULT_FAMILY = {fault: family for family, faults in R.FAULTS.items() for fault in faults}
misses = {}


def emulate(case, fault=None):
    """(the compared quantities, pads as documented, nothing stored behind the buffer)"""
    with torch.no_grad():
        outs = R.EMU[case.family](case.args, fault)
    got, pads = V.unpack(case.family, case.args, outs)
    return got, pads, bool((outs["past"] == R.SENT).all())


def test_every_fault_has_a_case():
    assert sorted(FAULT_FAMILY) == sorted(ISSUE_FAULTS) == sorted(V.FAULT_CASE)
    for fault, name in V.FAULT_CASE.items():
        assert V.BUILDERS[name][0] == FAULT_FAMILY[fault], (fault, name)


@pytest.mark.parametrize("name", V.NAMES)
def test_packed_emulated_and_unpacked_is_the_reference(name):
    case = V.by_name(name)
    ref64, ref32 = V.references(name)
    got, pads, behind = emulate(case)
    assert pads, "a padded column of the emulated output is not what csrc/vae_api.h documents"
    assert behind
    assert len(got) == len(ref64) and all(g.shape == r.shape for g, r in zip(got, ref64))
    if case.kind == "exact":
        assert V.is_exact(got, ref64)
    else:
        worst = max(V.ratios(got, ref64, ref32))
        print(f"{name}: emulation err / tol {worst:.3f}")
        assert worst <= 1.0
        tols = [8.0 * float((r32.double() - r64).abs().max()) for r64, r32 in zip(ref64, ref32)]
        must = [tols[1]] + ([] if case.dense["integer"] else [tols[0]]) if case.family == "group_norm" else tols
        assert all(t > 0.0 for t in must), tols


@pytest.mark.parametrize("fault", ISSUE_FAULTS)
def test_a_fault_fails_its_case(fault):
    case = V.by_name(V.FAULT_CASE[fault])
    ref64, ref32 = V.references(case.name)
    got, pads, behind = emulate(case, fault)
    clean = pads and behind
    if case.kind == "exact":
        print(f"{fault}: {case.name} (exact), pads {'as documented' if pads else 'wrong'}, behind the buffer {'nothing' if behind else 'a store'}")
        assert not clean or not V.is_exact(got, ref64)
    else:
        worst = max(V.ratios(got, ref64, ref32))
        print(f"{fault}: {case.name}, err / tol {worst:.1f}, pads {'as documented' if pads else 'wrong'}")
        assert not clean or worst > 1.0
        if clean:
            misses[fault] = worst
            print(f"smallest toleranced miss so far: {min(misses.values()):.1f} ({min(misses, key=misses.get)})")


@pytest.mark.parametrize("name", V.STATISTICS)
def test_the_means_own_bound_sees_a_dropped_mean_lo(name):
    """The float32 restatement's tolerance on a mean is wider than mean_hi's rounding, so the statistics' mean is also held to
    V.mean_bound: the emulation keeps it, and without mean_lo misses it where the mean is not a float32 to begin with.  The mean of
    integer inputs is exact in double: the emulation's is the reference's, split to (hi, lo)."""
    case = V.by_name(name)
    ref64, _ = V.references(name)
    bound = V.mean_bound(case)
    kept_mean = emulate(case)[0][0]
    kept = float((kept_mean - ref64[0]).abs().max())
    dropped = float((emulate(case, R.MEAN_FAULT)[0][0] - ref64[0]).abs().max())
    print(f"{name}: bound {bound:.2e}, |mean error| {kept:.2e}, without mean_lo {dropped:.2e}")
    assert kept <= bound
    if case.dense["integer"]:
        assert torch.equal(kept_mean, V.split_mean(ref64[0]))
    if bool((ref64[0] != ref64[0].float().double()).any()):
        assert bound < dropped


@pytest.mark.parametrize("name", V.EXACT_SUMS)
def test_exact_cases_stay_below_2_to_the_24(name):
    case = V.by_name(name)
    unit = case.dense.get("unit", 1.0)
    tensors = [t for t in case.dense.values() if torch.is_tensor(t)]
    assert all(bool((t / unit == (t / unit).round()).all()) for t in tensors), "an exact case carries integers of its grid only"
    bound = V.exact_bound(case)
    print(f"{name}: max sum |x| |w| = {bound:.0f}")
    assert bound < 2.0 ** 24


def test_the_u8_cases_reach_both_clamps_the_tie_and_a_spread():
    k = V.u8_levels(V.by_name("conv_u8_exact"))
    between = set(k[(k > -128) & (k < 128)].tolist())
    print(f"conv_u8_exact: k from {int(k.min())} to {int(k.max())}, {len(between)} levels between the clamps")
    assert float(k.min()) < -128 and float(k.max()) > 128 and 0.0 in between and len(between) >= 64
    ties = V.by_name("conv_u8_ties")
    b = ties.dense["b"]
    assert [float(x) for x in (b / 2.0 + 0.5) * 255.0] == [lv + 0.5 for lv in V.TIE_LEVELS]      # in float32
    assert V.references("conv_u8_ties")[0][0][0, 0].tolist() == [100.0, 102.0, 200.0]


@pytest.mark.parametrize("name", V.SELECTORS)
def test_selector_cases_lead_by_120_and_spread_over_the_chunks(name):
    case = V.by_name(name)
    lead = V.K.selector_lead(case)      # the minimum over EVERY query
    q, k, v = (case.dense[x][0, 0] for x in "qkv")
    chunks = V.selected_chunks(case)
    last = (k.shape[0] - 1) // R.ATTN_BK
    first_share, last_share = float((chunks == 0).float().mean()), float((chunks == last).float().mean())
    print(f"{name}: smallest lead {lead:.1f}, first chunk {first_share:.2f}, last chunk {last_share:.2f}")
    assert lead >= V.SELECTOR_LEAD and first_share >= 0.25 and last_share >= 0.25
    assert bool((v == v.round()).all())
    p = torch.softmax((q @ k.t()) / math.sqrt(q.shape[-1]), dim=-1)      # in float32, as the kernel
    assert bool(((p == 0) | (p == 1)).all()), "the float32 softmax is exactly one-hot"
    assert float(torch.exp(torch.tensor(-V.SELECTOR_LEAD))) == 0.0
