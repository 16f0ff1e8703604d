"""CPU: the crafted Swin2SR cases of tests/swin2sr_cases.py, checked without a kernel.

  clean     the float32 restatement passes every case under the criterion the GPU test applies (trivially: the tolerance is 8 x
            its own error; what is asserted is that the reference is finite, the tolerance positive and the case as large as its
            note says)
  sharp     every fault of swin2sr_ref.FAULTS, applied to the float32 restatement, fails at least one case named for it by
            10 x that case's tolerance; the fault x case table is printed
  built     the constructions do what their docstrings say: some logit_scale entries sit above ln 100, the bias of
            clamp_and_bias spans (0, 16), the masked cases have all three regions on both axes (or inside one window); token counts
            that are no multiple of 16, an odd window, head dims 4, 16 and 48; the rounding ties are exact in float32

One fault of the list cannot fail any case, here or anywhere: `regions_at_shift_only`.  The boundary it drops, n - window, is a
window boundary whenever n is a multiple of the window (the model's contract, and what its own padding guarantees), so within a
window the two-region and the three-region labelling separate the same pairs and the mask is bit for bit the same.  The test
asserts exactly that, instead of a failure that does not exist.

`single_bounce_pad` is a fault of the processor's padding (swin2sr_ref.FRAME_FAULTS), so its column of the table is the frame-level
route: upscale_float with the fault on SMALL_FRAMES against frame_reference's tolerance, for the configurations of
SMALL_FRAME_CASES.  It fails the 2 x 3 and the 3 x 17 frame; on the 1 x 1 frame it is provably the same padding (every sample is
the one pixel either way), which is asserted as an equality.

`one_window_shifted` cannot hold nine regions: with a grid as large as the window, n - window is 0, every token has the first
cut behind it and an axis carries two labels, not three.  The only window then holds four regions, which the roll moves as
blocks; the test asserts the four, and that the case rejects `no_mask`.
"""
import math

import pytest
import torch

from tests import swin2sr_cases as C
from tests import swin2sr_ref as R

CASES = C.cases()
NAMES = [c.name for c in CASES]
REJECT = 10.0
EQUIVALENT = ("regions_at_shift_only",)


@pytest.mark.parametrize("name", NAMES)
def test_f32_restatement_is_clean(name):
    case = C.by_name(name)
    y64, y32, tol = C.reference(case)
    err, _ = C.error(y32, case)
    print(f"{name}: {tuple(y64.shape)}, max |out| {float(y64.abs().max()):.3f}, tol {tol:.3e} (CPU), f32 err / tol {err / tol:.3f}; {case.note}")
    assert torch.isfinite(y64).all() and tol > 0 and err <= tol
    h, w = case.pixel_values().shape[2:]
    assert h <= 24 and w <= 24


def frame_fault_ratio(name, hw, fault):
    frame, y64, tol = C.frame_reference(name, hw)
    case = C.by_name(name)
    yf = R.upscale_float(case.sd, frame, torch.float32, fault=fault, **case.cfg)
    return float((yf.double() - y64).abs().max()) / tol


def fault_ratio(case, fault):
    if fault in R.FRAME_FAULTS:      # the frame-level route on the small frames, for the configurations that run them
        return max(frame_fault_ratio(case.name, hw, fault) for hw in C.SMALL_FRAMES) if case.name in C.SMALL_FRAME_CASES else 0.0
    y64, _, tol = C.reference(case)
    with torch.no_grad():
        yf = R.swin2sr_forward(case.sd, case.pixel_values(), fault=fault, **case.cfg)
    return float((yf.double() - y64).abs().max()) / tol


def test_every_fault_fails_a_case_named_for_it():
    table = {(f, c.name): fault_ratio(c, f) for f in R.FAULTS for c in CASES}
    width = max(len(f) for f in R.FAULTS)
    print("\nfault x case (CPU, float32 restatement with the fault): max |out - f64| / tol; * = the case is named for the fault")
    for i, c in enumerate(CASES):
        print(f"  [{i}] {c.name}: {c.note}")
    print(" " * (width + 2) + "".join(f"{'[%d]' % i:>11s}" for i in range(len(CASES))))
    for f in R.FAULTS:
        print(f"  {f:<{width}s}" + "".join(f"{'%.3g' % table[f, c.name] + ('*' if f in c.faults else ''):>11s}" for c in CASES))
    for f in R.FAULTS:
        named = [c for c in CASES if f in c.faults]
        assert named, f"no case is named for {f}"
        best = max(table[f, c.name] for c in named)
        if f in EQUIVALENT:
            continue
        assert best >= REJECT, (f, best)
    for c in CASES:
        assert set(c.faults) <= set(R.FAULTS)


@pytest.mark.parametrize("name", C.SMALL_FRAME_CASES)
def test_single_bounce_padding_fails_the_small_frames(name):
    """One reflection and a clamp is numpy's "symmetric" up to twice the frame's side: the frames of FRAMES cannot tell them apart,
    the 2 x 3 and 3 x 17 frames do, and on a 1 x 1 frame both give the pixel everywhere."""
    for hw in C.FRAMES:
        frame = C.frame_reference(name, hw)[0]
        assert torch.equal(R.process_frame(frame, torch.float64), R.process_frame(frame, torch.float64, fault="single_bounce_pad"))
    for hw in C.SMALL_FRAMES:
        frame = C.frame_reference(name, hw)[0]
        same = torch.equal(R.process_frame(frame, torch.float64), R.process_frame(frame, torch.float64, fault="single_bounce_pad"))
        ratio = frame_fault_ratio(name, hw, "single_bounce_pad")
        print(f"{name} {hw}: single_bounce_pad {ratio:.3g} x tol")
        assert same == (hw == (1, 1))
        assert ratio >= REJECT or same


@pytest.mark.parametrize("hw,ws", [((12, 20), 4), ((8, 24), 8), ((16, 24), 8), ((24, 24), 12)])
def test_two_region_labelling_gives_the_same_mask(hw, ws):
    """See the module docstring: n - window is a window boundary, so cutting at n - shift alone separates the same pairs."""
    want = R.region_mask(hw[0], hw[1], ws, ws // 2, torch.float64)
    got = R.region_mask(hw[0], hw[1], ws, ws // 2, torch.float64, fault="regions_at_shift_only")
    assert torch.equal(want, got) and float(want.min()) == -100.0 and float(want.max()) == 0.0
    for c in CASES:
        y64, y32, _ = C.reference(c)
        with torch.no_grad():
            assert torch.equal(R.swin2sr_forward(c.sd, c.pixel_values(), fault="regions_at_shift_only", **c.cfg), y32)
        break


def test_constructions():
    above = below = 0
    for c in CASES:
        for k, v in c.sd.items():
            if k.endswith("logit_scale"):
                above += int((v > math.log(100.0)).sum())
                below += int((v < math.log(100.0)).sum())
            assert float(v.abs().max()) > 0 and (v.numel() == 1 or float(v.std()) > 0), k      # nothing at its default
    assert above >= 5 and below >= 5
    c = C.by_name("clamp_and_bias")
    a = "swin2sr.encoder.stages.0.layers.0.attention.self"
    assert float(c.sd[a + ".logit_scale"].min()) == pytest.approx(math.log(100.0) + 2.0)
    b = R.position_bias({k: v.double() for k, v in c.sd.items()}, a, 8, 1)
    print(f"clamp_and_bias: 16 sigmoid(bias) spans {float(b.min()):.2f} .. {float(b.max()):.2f}")
    assert float(b.min()) < 2.0 and float(b.max()) > 14.0
    taps = {}
    with torch.no_grad():
        R.swin2sr_forward(c.sd, c.x.double(), taps=taps, **c.cfg)
    s = taps["scores"][0]
    top2 = s.topk(2, dim=-1).values
    assert float((top2[..., 0] - top2[..., 1]).median()) < 8.0      # the softmax is not one-hot: the bias and the clamp both move it
    one = C.by_name("one_window_high")
    assert one.x.shape[2] == one.cfg["window_size"] and one.cfg["embed_dim"] // one.cfg["num_heads"][0] == 10
    wide = C.by_name("published_width")
    assert wide.cfg["embed_dim"] == 180 and wide.cfg["embed_dim"] // wide.cfg["num_heads"][0] == 30
    small = C.by_name("small_shift")
    m = R.region_mask(12, 20, 4, 2, torch.float64)
    assert m.shape[0] == 15 and int((m.view(15, -1).min(dim=1).values < 0).sum()) == 3 + 5 - 1      # the last window row and column
    assert small.cfg["depths"] == (2, 2)
    # the later cases: token counts that are no multiple of 16, an odd window, the head dims, the widths of the direct heads
    tokens = {c.name: c.cfg["window_size"] ** 2 for c in CASES}
    head_dim = {c.name: c.cfg["embed_dim"] // c.cfg["num_heads"][0] for c in CASES}
    assert [tokens[n] for n in ("window_6_wide", "window_7_odd", "window_10_one_high", "window_5_one_head", "window_2_many_heads")] == [36, 49, 100, 25, 4]
    assert all(tokens[n] % 16 for n in ("window_6_wide", "window_7_odd", "window_10_one_high", "window_5_one_head", "window_2_many_heads"))
    assert C.by_name("window_7_odd").cfg["window_size"] % 2 == 1 and C.by_name("window_5_one_head").cfg["window_size"] % 2 == 1
    assert (head_dim["window_2_many_heads"], head_dim["window_7_odd"], head_dim["window_10_one_high"], head_dim["window_5_one_head"]) == (4, 8, 16, 48)
    wide = C.by_name("window_6_wide")            # three m-tiles against eight n-tiles in output.dense: the 3-tile branch with 8 waves
    assert (tokens["window_6_wide"] + 15) // 16 == 3 and wide.cfg["embed_dim"] // 16 == 8
    assert (tokens["window_10_one_high"] + 15) // 16 == 7
    assert wide.sd["upsample.conv.weight"].shape[0] == 27 and C.by_name("window_10_one_high").sd["upsample.conv.weight"].shape[0] == 48
    one_head = C.by_name("window_5_one_head")
    assert one_head.sd["swin2sr.encoder.stages.0.layers.0.intermediate.dense.weight"].shape[0] == 72
    for c in C.forward_cases():
        h, w = c.x.shape[2:]
        assert h % c.cfg["window_size"] == 0 and w % c.cfg["window_size"] == 0 and c.cfg["image_size"] > c.cfg["window_size"]
    gray = C.by_name("gray")
    assert gray.x.shape[1] == 1 and gray.sd["upsample.final_convolution.weight"].shape[0] == 1 and C.reference(gray)[0].shape[1] == 1
    assert gray not in C.frame_cases() and len(C.frame_cases()) == len(CASES) - 1
    assert C.by_name("eps_1e-2").cfg["layer_norm_eps"] == 1e-2
    # one_window_shifted: the grid is the window, so an axis has the labels 1 and 2 only and the window holds 2 x 2 regions
    ows = C.by_name("one_window_shifted")
    m = R.region_mask(8, 8, 8, 4, torch.float64)
    assert m.shape[0] == 1 and ows.cfg["depths"] == (2,)
    labels = {tuple((m[0, i] == 0).nonzero().flatten().tolist()) for i in range(64)}
    assert len(labels) == 4 and all(len(g) == 16 for g in labels)
    many = R.region_mask(12, 20, 4, 2, torch.float64)[-1]          # the last window of a larger grid holds four as well: never nine
    assert len({tuple((many[i] == 0).nonzero().flatten().tolist()) for i in range(16)}) == 4


def test_rounding_ties_are_exact_in_float32():
    """(bias + mean) x 255 is k + 0.5 exactly for ten (channel, sub-pixel) slots, k even and odd; two slots leave [0, 1]."""
    case = C.rounding_ties()
    assert float(case.sd["upsample.conv.weight"].abs().max()) == 0.0
    y32 = R.upscale_float(case.sd, case.frame, torch.float32, **case.cfg)
    assert y32.dtype == torch.float32 and tuple(y32.shape) == (10, 14, 3)
    v = y32.clamp(0, 1) * 255.0
    ks, odd, even = [], 0, 0
    for cc in range(3):
        for r1 in range(2):
            for r2 in range(2):
                k, got = C.TIE_K[cc][r1][r2], v[r1::2, r2::2, cc]
                assert float(got.min()) == float(got.max())          # the same value at every position
                if isinstance(k, str):
                    raw = float(y32[r1, r2, cc])
                    assert raw < 0 if k == "low" else raw > 1
                    continue
                assert float(got[0, 0]) == k + 0.5, (cc, r1, r2, k, float(got[0, 0]))
                ks.append(k)
                odd, even = odd + (k & 1), even + 1 - (k & 1)
    assert len(ks) == 10 and odd >= 4 and even >= 4 and len({cc for cc in range(3) for r in C.TIE_K[cc] for k in r if k != "low" and k != "high" and k & 1}) == 3
    want = C.ties_expected_frame(case)
    assert torch.equal(R.quantise(y32), want)                         # torch rounds half to even
    half_up = torch.floor(v + 0.5).to(torch.uint8)
    assert int((half_up != want).sum()) == sum(k & 1 == 0 for k in ks) * 5 * 7      # round-half-up differs on every even k
