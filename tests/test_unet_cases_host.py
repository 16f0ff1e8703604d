"""The crafted cases of tests/unet_cases.py without a GPU: what each case is built for really holds (the seam group, the key
chunks, the late maxima, the offset statistics), and every named fault of tests/unet_ref.py fails the case named for it by at least
ten tolerances when it is applied to the float32 restatement."""
import math

import pytest
import torch

from tests import unet_cases as C
from tests import unet_ref as R


def test_every_fault_has_a_case():
    assert set(C.FAULT_CASE) == set(R.FAULTS) and set(C.FAULT_CASE.values()) <= set(C.NAMES)


@pytest.mark.parametrize("name", C.NAMES)
def test_cases_are_seeded_and_finite(name):
    case = C.by_name(name)
    assert list(case.sd) == list(R.spec(**case.cfg)) and all(v.dtype == torch.float32 for v in case.sd.values())
    y64, tol = C.reference(name)
    n, _, h, w = case.sample.shape
    assert tuple(y64.shape) == (n, 4, h, w) and bool(torch.isfinite(y64).all()) and tol > 0
    again = C._build(name)
    assert all(torch.equal(again.sd[k], case.sd[k]) for k in case.sd) and torch.equal(again.sample, case.sample) and torch.equal(again.text, case.text)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_fault_fails_its_case_by_ten_tolerances(fault):
    name = C.FAULT_CASE[fault]
    case = C.by_name(name)
    y64, tol = C.reference(name)
    with torch.no_grad():
        got = R.forward(case.sd, case.sample, case.timestep, case.text, case.label, fault=fault, **case.cfg)
    err = float((got.double() - y64).abs().max())
    print(f"{fault} on {name}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.1f}")
    assert tol > 0 and err >= 10 * tol


def test_seam_group_straddles_the_concatenation():
    cfg = R.config(**C.by_name("seam_groups").cfg)
    hidden, skip, _ = R.up_channels(cfg["block_out_channels"], cfg["layers_per_block"], 1, 0)
    per = (hidden + skip) // cfg["norm_num_groups"]
    assert (hidden, skip, per) == (16, 8, 3) and any(g * per < hidden < (g + 1) * per for g in range(cfg["norm_num_groups"]))


def test_shapes_the_cases_reach():
    wide = R.config(**C.by_name("wide").cfg)
    assert [w // wide["attention_head_dim"] for w in wide["block_out_channels"]] == [64, 128] and wide["cross_attention_dim"] == 1024
    assert sum(R.up_channels(wide["block_out_channels"], 1, 0, 0)[:2]) == 1024 and 4 * 512 == 2048
    ragged = R.config(**C.by_name("ragged_heads").cfg)
    assert 48 // ragged["attention_head_dim"] == 24 and ragged["cross_attention_dim"] % 16 != 0
    n = C.by_name("self_many_tokens").sample.shape[2] * C.by_name("self_many_tokens").sample.shape[3] // 4
    assert n == 135 and math.ceil(n / R.STREAM_CHUNK) == 5 and n % R.STREAM_CHUNK == 7
    assert C.by_name("many_text_tokens").text.shape[1] == 80 > 2 * R.STREAM_CHUNK and C.by_name("one_text_token").text.shape[1] == 1
    assert C.by_name("batch_two").sample.shape[0] == 2 and not torch.equal(C.by_name("batch_two").text[0], C.by_name("batch_two").text[1])
    assert tuple(C.by_name("smallest").sample.shape[2:]) == (2, 2)


def test_late_maxima_lie_in_the_last_chunk():
    s = C.late_taps(C.by_name("late_maxima"))["scores"]                # [1, heads, 135, 135]
    n = s.shape[-1]
    last0 = (n - 1) // R.STREAM_CHUNK * R.STREAM_CHUNK
    share = float((s.argmax(dim=-1) >= last0).double().mean())
    gap = (s[..., last0:].max(dim=-1).values - s[..., :last0].max(dim=-1).values)
    print(f"late_maxima: {100 * share:.0f} % of the rows have their maximum in the last chunk; it lies {float(gap.median()):.2f} above the earlier ones (median)")
    assert share >= C.LAST_CHUNK_SHARE and float(gap.median()) > 1.0      # exp(-gap) is what a missing rescale gets wrong by


def test_streamed_attention_is_the_softmax():
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn((2, 3, 45, 16), generator=g, dtype=torch.float64) for _ in range(3))
    want = torch.softmax(q @ k.transpose(-1, -2) * 0.25, dim=-1) @ v
    assert float((R.streamed_attention(q, k, v, 0.25) - want).abs().max()) < 1e-12
    assert float((R.streamed_attention(q, k, v, 0.25, rescale=False) - want).abs().max()) > 1e-3


def test_offset_stats_puts_the_means_far_out():
    case = C.by_name("offset_stats")
    for key in ("down_blocks.0.resnets.0.conv1.bias", "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_out.0.bias"):
        assert float(case.sd[key].mean()) > 900 and float(case.sd[key].std()) < 1.0
