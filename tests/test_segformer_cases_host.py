"""CPU: the crafted SegFormer cases of tests/segformer_cases.py, checked without a kernel.

  clean     the float32 restatement passes every case under the criterion the GPU test applies, and the positions with a thin
            float64 margin stay inside segformer_ref.MAX_THIN
  sharp     every fault of segformer_ref.FAULTS and MAP_FAULTS, injected into the float64 restatement, fails at least one case
            named for it by 10 x that case's tolerance (a class-map fault: wrong labels at positions whose margin is 10 x the
            margin the criterion asks for); the fault x case table is printed
  built     each construction does what its docstring says: the score maxima lie in the chunk they are meant to, the scores of
            the padding case are all negative, the variances are about 1e-4, fc1's outputs spread beyond +-3
  sizes     the grid SegFormer allocates (nesr_segformer_output_size, no device) is the restatement's logits' grid
  cover     the key counts, query counts and widths the cases are there for

Everything here is measured on the CPU; test_gpu_segformer_cases.py runs the kernels."""
import pytest
import torch

from neural_enhanced_super_resolution_amd import SegFormer
from tests import segformer_cases as C
from tests import segformer_ref as R

CASES = C.cases()
NAMES = [c.name for c in CASES]
REJECT = 10.0


@pytest.mark.parametrize("name", NAMES)
def test_f32_restatement_is_clean(name):
    case = C.by_name(name)
    l64, l32, tol = C.reference(case)
    err, _ = C.logits_error(l32, case)
    excluded, wrong, n = C.map_check(C.restatement_map(case, l32), case)
    print(f"{name}: logits {tuple(l64.shape)}, max |logit| {float(l64.abs().max()):.2f}, tol {tol:.3e} (CPU), f32 err / tol {err / tol:.3f}, "
          f"{excluded} of {n} positions thin, {wrong} wrong")
    assert torch.isfinite(l64).all() and tol > 0
    assert err <= tol and wrong == 0
    assert excluded <= R.MAX_THIN * n
    h, w = case.frame.shape[:2] if case.via == "segment" else case.x.shape[2:]
    assert h <= 96 and w <= 128


def fault_ratio(case, fault):
    """How far the float64 restatement with `fault` misses `case`: max |logit change| / tol, or for a class-map fault the number of
    wrong labels among the positions whose float64 margin is REJECT x the criterion's.  None where the fault changes the shape."""
    l64, _, tol = C.reference(case)
    if fault in R.MAP_FAULTS:
        return float(C.map_check(C.restatement_map(case, l64, fault=fault), case, factor=REJECT)[1])
    with torch.no_grad():
        lf = R.segformer_forward(case.sd, case.pixel_values().double(), fault=fault, **case.cfg)
    if lf.shape != l64.shape:
        return None
    return float((lf - l64).abs().max()) / tol


def test_every_fault_fails_a_case_named_for_it():
    table = {}
    for fault in R.FAULTS + R.MAP_FAULTS:
        for case in CASES:
            if (fault in R.MAP_FAULTS) == (case.via == "segment"):      # the 512 x 512 cases are there for the class map alone
                table[fault, case.name] = fault_ratio(case, fault)
    width = max(len(f) for f in R.FAULTS + R.MAP_FAULTS)
    print("\nfault x case (CPU, float64 restatement with the fault): max |logit change| / tol; class-map faults: wrong labels at firm "
          "positions; * = the case is named for the fault")
    for i, name in enumerate(NAMES):
        print(f"  [{i:2d}] {name}: {C.by_name(name).note}")
    print(" " * (width + 2) + "".join(f"{'[%d]' % i:>11s}" for i in range(len(NAMES))))
    for fault in R.FAULTS + R.MAP_FAULTS:
        cells = []
        for case in CASES:
            r = table.get((fault, case.name), "-")
            cell = "-" if r == "-" else ("shape" if r is None else f"{r:.3g}")
            cells.append(f"{cell + ('*' if fault in case.faults else ''):>11s}")
        print(f"  {fault:<{width}s}" + "".join(cells))
    for fault in R.FAULTS + R.MAP_FAULTS:
        named = [c for c in CASES if fault in c.faults]
        assert named, f"no case is named for {fault}"
        best = max((table[fault, c.name] or 0.0) for c in named)
        assert best >= (1 if fault in R.MAP_FAULTS else REJECT), (fault, best)
    for case in CASES:
        assert set(case.faults) <= set(R.FAULTS + R.MAP_FAULTS)


# ------------------------------------------------------------------------------------------------ the constructions
@pytest.mark.parametrize("name", [c.name for c in CASES if c.want_max])
def test_score_maxima_lie_in_the_chunk_they_are_built_for(name):
    case = C.by_name(name)
    s = C.scores_of(case)
    keys = s.shape[-1]
    assert keys > C.KCH and keys == C.key_counts(case.cfg, *case.x.shape[2:])[0]
    last0 = (keys - 1) // C.KCH * C.KCH
    if case.want_max == "last":
        gap = s[..., last0:].max(dim=-1).values - s[..., :last0].max(dim=-1).values
    else:
        gap = s[..., :C.KCH].max(dim=-1).values - s[..., C.KCH:].max(dim=-1).values
    print(f"{name}: {keys} keys; the {case.want_max} chunk's best score leads the others' by {float(gap.min()):.2f} .. {float(gap.max()):.2f} (CPU)")
    assert C.max_chunk_share(case) == 1.0
    assert float(gap.min()) >= 1.0        # exp(-1): without the rescale a row's sum is off by a factor, not by rounding


def test_padding_case_has_negative_scores_only():
    case = C.by_name("negative_scores_12_keys")
    taps = {}
    with torch.no_grad():
        R.segformer_forward(case.sd, case.x.double(), taps=taps, **case.cfg)
    assert len(taps["scores"]) == 3
    for s in taps["scores"]:
        assert s.shape[-1] == 12 and float(s.max()) < -0.25
    for c in CASES:
        if "argmax_pad_label" in c.faults:
            assert float(C.reference(c)[0].max()) < 0


def test_small_variance_case_has_small_variances():
    case = C.by_name("small_variance")
    p = {k: v.double() for k, v in case.sd.items() if v.dtype.is_floating_point}
    s0 = "segformer.stages.0."
    rows = torch.nn.functional.conv2d(case.x.double(), p[s0 + "patch_embeddings.proj.weight"], p[s0 + "patch_embeddings.proj.bias"], stride=4, padding=3)
    var = rows.flatten(2).var(dim=1, unbiased=False)
    print(f"patch conv rows: variance {float(var.min()):.2e} .. {float(var.max()):.2e}; running_var "
          f"{float(p['decode_head.batch_norm.running_var'].min()):.2e} .. {float(p['decode_head.batch_norm.running_var'].max()):.2e}")
    assert 1e-5 < float(var.min()) and float(var.max()) < 2e-3
    g = p[s0 + "patch_embeddings.layer_norm.weight"]
    assert 2e-5 < float((g * g).mean()) < 5e-4                       # the variance of a row of the residual stream
    assert float(p["decode_head.batch_norm.running_var"].max()) < 2e-4


def test_gelu_case_spreads_beyond_three():
    case = C.by_name("gelu_wide")
    b = "segformer.stages.0.blocks.0.mlp."
    seen = {}
    real = torch.nn.functional.gelu

    def spy(t, approximate="none"):
        seen["pre"] = t
        return real(t, approximate=approximate)

    torch.nn.functional.gelu = spy
    try:
        with torch.no_grad():
            R.segformer_forward(case.sd, case.x.double(), **case.cfg)
    finally:
        torch.nn.functional.gelu = real
    pre = seen["pre"]
    assert case.sd[b + "fc1.weight"].shape == (32, 32)
    assert float(pre.min()) < -3 and float(pre.max()) > 3 and float((pre.abs() > 2).double().mean()) > 0.1


# ------------------------------------------------------------------------------------------------ sizes and coverage
@pytest.mark.parametrize("name", NAMES)
def test_allocated_grid_is_the_restatements(name):
    """What SegFormer.forward and segment allocate comes from nesr_segformer_output_size, which needs no device."""
    case = C.by_name(name)
    m = SegFormer(**case.cfg)
    h, w = case.pixel_values().shape[2:]
    assert m.output_size(h, w) == tuple(C.reference(case)[0].shape[2:]) == C.grid(case.cfg, h, w)[0]


def test_output_size_of_b0_and_of_other_strides():
    assert SegFormer().output_size(512, 512) == (128, 128) and SegFormer().output_size(96, 160) == (24, 40)
    two = dict(num_encoder_blocks=1, depths=(1,), sr_ratios=(1,), hidden_sizes=(32,), num_attention_heads=(1,), mlp_ratios=(1,))
    assert SegFormer(patch_sizes=(3,), strides=(2,), **two).output_size(96, 128) == (48, 64)
    assert SegFormer(patch_sizes=(7,), strides=(8,), **two).output_size(96, 128) == (12, 16)
    with pytest.raises(Exception, match="strides"):
        SegFormer(patch_sizes=(7,), strides=(9,), **two).output_size(96, 128)


def test_cases_cover_the_shapes_they_are_there_for():
    keys, queries, hidden, mlp8_at_256, dec, labels, stages, depths, wide_q = set(), set(), set(), False, set(), set(), set(), set(), False
    for c in CASES:
        h, w = c.pixel_values().shape[2:]
        cfg = c.cfg
        keys.update(C.key_counts(cfg, h, w))
        queries.update(gh * gw for gh, gw in C.grid(cfg, h, w))
        hidden.update(cfg["hidden_sizes"])
        mlp8_at_256 |= any(ch == 256 and m == 8 for ch, m in zip(cfg["hidden_sizes"], cfg["mlp_ratios"]))
        wide_q |= any(ch == 256 and sr > 1 for ch, sr in zip(cfg["hidden_sizes"], cfg["sr_ratios"]))
        dec.add(cfg["decoder_hidden_size"])
        labels.add(cfg["num_labels"])
        stages.add(cfg["num_encoder_blocks"])
        depths.update(cfg["depths"])
    assert any(k <= 31 for k in keys) and 256 in keys and 512 in keys and any(k > 512 for k in keys)
    assert any(256 < k < 512 and k % 32 for k in keys)
    for count in (k for k in keys if k > 256):      # each count above one chunk: the maximum in the first chunk, and in the last
        for where in ("first", "last"):
            assert any(c.want_max == where and C.key_counts(c.cfg, *c.x.shape[2:])[0] == count for c in CASES if c.want_max), (count, where)
    assert any(q < 32 for q in queries) and any(q % 32 for q in queries if q > 32)
    assert {32, 96, 256} <= hidden and mlp8_at_256 and wide_q
    assert any(1 in c.cfg["mlp_ratios"] for c in CASES)
    assert {32, 256} <= dec and {1, 5, 33, 256} <= labels and {1, 3} <= stages and 3 in depths
    assert any(c.cfg["strides"][0] == 2 for c in CASES) and any(c.cfg["strides"][0] == 8 and c.via == "forward" for c in CASES)
    assert {c.cfg["num_labels"] for c in CASES if c.via == "segment"} == {1, 5, 33}
