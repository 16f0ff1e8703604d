"""GPU: the crafted cases of tests/segformer_cases.py through SegFormer(**cfg) on the HIP path (csrc/segformer.hip), each a tiny
non-B0 configuration built so that one fused stage dominates the logits; test_segformer_cases_host.py shows on the CPU that a
plausible fault in that stage fails its case by 10 x the tolerance.

  logits   max |gpu - f64| <= tol = 8 x max |f32 CPU restatement - f64|, per case (printed as err / tol)
  map      the argmax of the logits, and for the cases about the argmax the u8 class map of `segment` (the ARGMAX output mode),
           equals the float64 argmax, lowest index among equals, wherever the float64 top-2 margin is >= 2 tol
"""
import pytest
import torch

from neural_enhanced_super_resolution_amd import SegFormer
from tests import segformer_cases as C
from tests import segformer_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [c.name for c in C.cases()]
_cache = {}


def model(case):
    if case.name not in _cache:
        m = SegFormer(**case.cfg).to(DEV)
        m.load_state_dict(case.sd)
        _cache[case.name] = m
    return _cache[case.name]


def logits_of(case):
    key = ("logits", case.name)
    if key not in _cache:
        got = model(case)(case.pixel_values().to(DEV))
        torch.cuda.synchronize()
        _cache[key] = got.cpu()
    return _cache[key]


@pytest.mark.parametrize("name", NAMES)
def test_logits_against_float64(name):
    case = C.by_name(name)
    got = logits_of(case)
    l64, _, _ = C.reference(case)
    assert got.shape == l64.shape and got.dtype == torch.float32      # the restatement's grid, whatever the strides
    err, tol = C.logits_error(got, case)
    print(f"{name}: logits {tuple(got.shape)}, max |gpu - f64| = {err:.3e}, tol {tol:.3e}, err / tol = {err / tol:.3f}")
    assert torch.isfinite(got).all()
    assert err <= tol


@pytest.mark.parametrize("name", NAMES)
def test_argmax_of_logits_under_the_margin_rule(name):
    case = C.by_name(name)
    got = logits_of(case)
    if case.tie is not None:      # bit-equal classifier rows give bit-equal logits: the columns of one MFMA share a summation order
        assert torch.equal(got[:, case.tie[0]], got[:, case.tie[1]])
    excluded, wrong, n = C.map_check(R.class_map(got), case)
    print(f"{name}: argmax of the logits, {excluded} of {n} positions thin, {wrong} wrong")
    assert wrong == 0 and excluded <= R.MAX_THIN * n


@pytest.mark.parametrize("name", ["keys_336_stride_2_max_last", "three_stages_stride_8", "small_variance"])
def test_c_entry_writes_the_size_it_reports(name):
    """nesr_segformer_forward_f32 takes no capacity: it writes num_labels x nesr_segformer_output_size floats and not one more
    (first-stage strides 2, 8 and 4).  The buffer here is larger than anything the entry may write; the floats behind the reported
    size keep their sentinel."""
    import ctypes

    from neural_enhanced_super_resolution_amd import _lib
    case = C.by_name(name)
    m = model(case)
    x = case.x.to(DEV)
    h, w = x.shape[2:]
    oh, ow = m.output_size(h, w)
    n = case.cfg["num_labels"] * oh * ow
    guard = max(n, case.cfg["num_labels"] * (h // 2) * (w // 2))      # room for the largest grid any stride gives
    buf = torch.full((n + guard,), -7.0, dtype=torch.float32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().nesr_segformer_forward_f32(m._context(x.device), ctypes.c_void_p(x.data_ptr()), 1, 3, h, w, ctypes.c_void_p(buf.data_ptr()),
                                                      stream), "nesr_segformer_forward_f32")
    torch.cuda.synchronize()
    assert torch.equal(buf[:n].view(1, -1, oh, ow).cpu(), logits_of(case))
    assert bool((buf[n:] == -7.0).all())


@pytest.mark.parametrize("name", [c.name for c in C.cases() if c.via == "segment"])
def test_segment_class_map(name):
    case = C.by_name(name)
    m = model(case)
    got = m.segment(torch.from_numpy(case.frame).to(DEV))
    l64, _, _ = C.reference(case)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == tuple(l64.shape[2:]) == (64, 64)
    excluded, wrong, n = C.map_check(got, case)
    print(f"{name}: segment, labels {sorted(int(v) for v in torch.unique(got))[:8]}, {excluded} of {n} positions thin, {wrong} wrong")
    assert int(got.max()) < case.cfg["num_labels"]      # never a padded label column
    assert wrong == 0 and excluded <= R.MAX_THIN * n
    frame = torch.from_numpy(case.frame).to(DEV)
    assert torch.equal(got.cpu().long(), R.class_map(m(m.pixel_values(frame)).cpu()))      # the fused argmax: the same logits, the lowest index
