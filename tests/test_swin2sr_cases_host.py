"""CPU: the crafted Swin2SR cases of tests/swin2sr_cases.py, checked without a kernel.

  clean     the float32 restatement passes every case under the criterion the GPU test applies (trivially: the tolerance is 8 x
            its own error; what is asserted is that the reference is finite, the tolerance positive and the case as large as its
            note says)
  sharp     every fault of swin2sr_ref.FAULTS, applied to the float32 restatement, fails at least one case named for it by
            10 x that case's tolerance; the fault x case table is printed
  built     the constructions do what their docstrings say: some logit_scale entries sit above ln 100, the bias of
            clamp_and_bias spans (0, 16), the masked cases have all three regions on both axes (or inside one window)

One fault of the list cannot fail any case, here or anywhere: `regions_at_shift_only`.  The boundary it drops, n - window, is a
window boundary whenever n is a multiple of the window (the model's contract, and what its own padding guarantees), so within a
window the two-region and the three-region labelling separate the same pairs and the mask is bit for bit the same.  The test
asserts exactly that, instead of a failure that does not exist.
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


def fault_ratio(case, fault):
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
