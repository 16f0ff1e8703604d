"""CPU: proof that the per-launch cases of tests/unet_kernels.py bite, and that their premises hold.

  * The float64 emulation of each kernel's indexing (tests/unet_kernel_ref.py), run on the PACKED arguments and unpacked again,
    gives the dense reference: bit for bit on the exact cases, within the case's tolerance on the toleranced ones, with every
    padded column as csrc/unet_api.h documents.  That is the round trip of the packing helpers, checked against the reference.
  * Every named fault of the emulation fails the case that FAULT_CASE assigns to it: an exact case is no longer bit-equal (or a
    padded column or sentinel is wrong); a toleranced case misses by at least 10 tolerances, or leaves a padded column that must
    read 0 (`padded_norm_left`: an exact check, there is no tolerance on a pad).
  * Exact cases: sum_k |x_k| |w_k| (+ |bias| + |residual|) < 2^24 for every output, so every partial sum is an exact float32 in
    any order.  Selector cases: every query's best key leads the runner-up by at least 120 in scaled score (float64).
"""
import math

import pytest
import torch

from tests import unet_kernel_ref as R
from tests import unet_kernels as K

ISSUE_FAULTS = ("sample_ignores_channel_blocks", "weight_offset_by_cs_not_cinp", "k_tail_dropped", "up_reads_gx_not_halved", "stride2_pad_right_bottom",
                "norm_on_padding_taps", "second_tile_of_ragged_block_kept", "gate_tile_mispaired", "norm_of_sample_0_for_all_rows",
                "second_source_weight_row_offset", "seam_group_split_at_cs", "last_partial_block_full", "padded_norm_left", "mean_over_cs", "one_pass_f32",
                "no_rescale_on_new_max", "ragged_chunk_unmasked", "head_offset_by_dp", "pad_columns_left", "kv_stride_of_q", "sin_cos_order",
                "class_row_of_label_0")
FAULT_FAMILY = {fault: family for family, faults in R.FAULTS.items() for fault in faults}
MISS = 10.0


def emulate(case, fault=None):
    with torch.no_grad():
        outs = R.EMU[case.family](case.args, fault)
    return K.unpack(case.family, case.args, outs)


def test_every_fault_has_a_case():
    assert sorted(FAULT_FAMILY) == sorted(ISSUE_FAULTS) == sorted(K.FAULT_CASE)
    for fault, name in K.FAULT_CASE.items():
        assert K.BUILDERS[name][0] == FAULT_FAMILY[fault], (fault, name)


@pytest.mark.parametrize("name", K.NAMES)
def test_packed_emulated_and_unpacked_is_the_reference(name):
    case = K.by_name(name)
    ref64, ref32 = K.references(name)
    got, pads = emulate(case)
    assert pads, "a padded column of the emulated output is not what csrc/unet_api.h documents"
    assert len(got) == len(ref64) and all(g.shape == r.shape for g, r in zip(got, ref64))
    if case.kind == "exact":
        assert K.is_exact(got, ref64)
    else:
        worst = max(K.ratios(got, ref64, ref32))
        print(f"{name}: emulation err / tol {worst:.3f}")
        assert worst <= 1.0


@pytest.mark.parametrize("fault", ISSUE_FAULTS)
def test_a_fault_fails_its_case(fault):
    case = K.by_name(K.FAULT_CASE[fault])
    ref64, ref32 = K.references(case.name)
    got, pads = emulate(case, fault)
    if case.kind == "exact":
        print(f"{fault}: {case.name} (exact), pads {'as documented' if pads else 'wrong'}")
        assert not pads or not K.is_exact(got, ref64)
    else:
        worst = max(K.ratios(got, ref64, ref32))
        print(f"{fault}: {case.name}, err / tol {worst:.1f}, pads {'as documented' if pads else 'wrong'}")
        assert not pads or worst >= MISS


STATISTICS = tuple(n for n in K.NAMES if K.BUILDERS[n][0] in R.EXTRA_FAULTS["mean_lo_dropped"])


@pytest.mark.parametrize("name", STATISTICS)
def test_the_means_own_bound_sees_a_dropped_mean_lo(name):
    """The float32 restatement's tolerance on a mean is wider than mean_hi's rounding, so the statistics' mean is also held to
    K.mean_bound: the emulation keeps it, and without mean_lo misses it where the mean is not a float32 to begin with."""
    case = K.by_name(name)
    ref64, _ = K.references(name)
    bound = K.mean_bound(case)
    kept = float((emulate(case)[0][0] - ref64[0]).abs().max())
    dropped = float((emulate(case, "mean_lo_dropped")[0][0] - ref64[0]).abs().max())
    print(f"{name}: bound {bound:.2e}, |mean error| {kept:.2e}, without mean_lo {dropped:.2e}")
    assert kept <= bound < dropped


@pytest.mark.parametrize("name", K.EXACT_SUMS)
def test_exact_cases_stay_below_2_to_the_24(name):
    case = K.by_name(name)
    tensors = [t for t in case.dense.values() if torch.is_tensor(t)] + [t for r in case.dense.get("resnets", ()) for t in r]
    assert all(bool((t == t.round()).all()) for t in tensors), "an exact case carries integers only"
    bound = K.exact_bound(case)
    print(f"{name}: max sum |x| |w| = {bound:.0f}")
    assert bound < 2.0 ** 24


@pytest.mark.parametrize("name", K.SELECTORS)
def test_selector_cases_lead_by_120(name):
    case = K.by_name(name)
    lead = K.selector_lead(case)      # the minimum over EVERY query of every head and sample
    print(f"{name}: smallest lead {lead:.1f}")
    assert lead >= K.SELECTOR_LEAD
    assert bool((case.dense["v"] == case.dense["v"].round()).all())
    p = torch.softmax((case.dense["q"] @ case.dense["k"].transpose(-1, -2)) / math.sqrt(case.dense["q"].shape[-1]), dim=-1)      # in float32, as the kernel
    assert bool(((p == 0) | (p == 1)).all()), "the float32 softmax is exactly one-hot"


def test_selector_winners_lie_in_the_first_a_middle_and_the_last_chunk():
    case = K.by_name("attn_selector_d24_h1_text")      # 256 keys: eight chunks
    q, k = case.dense["q"].double(), case.dense["k"].double()
    chunks = set(((q @ k.transpose(-1, -2)).argmax(-1) // R.ATTN_BK).reshape(-1).tolist())
    assert chunks == {0, 4, 7}
    ragged = K.by_name("attn_selector_d24_h5_text")     # 33 keys: the last chunk holds one
    q, k = ragged.dense["q"].double(), ragged.dense["k"].double()
    assert 32 in set((q @ k.transpose(-1, -2)).argmax(-1).reshape(-1).tolist())
