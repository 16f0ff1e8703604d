"""GPU: `UNet2DCondition.forward` on every crafted case of tests/unet_cases.py against the float64 restatement, within the case's
own tolerance (8 x the float32 restatement's error, computed here).  The result is written into the middle of a buffer of
sentinels (the guards are asserted), a second forward on the same context gives the same bits, and the two samples of `batch_two`
equal two forwards of one sample each, bit for bit."""
import ctypes

import pytest
import torch

from neural_enhanced_super_resolution_amd import UNet2DCondition, _lib
from tests import unet_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
_cache = {}


def model(name):
    if name not in _cache:
        case = C.by_name(name)
        m = UNet2DCondition(**case.cfg).to(DEV)
        m.load_state_dict(case.sd)
        _cache[name] = m
    return _cache[name]


def guarded_forward(m, sample, timestep, text, label):
    """nesr_unet_forward_f32 into the middle of a buffer of sentinels: the result on the host; the guards are asserted."""
    n, ch, h, w = sample.shape
    count = n * int(m.config["out_channels"]) * h * w
    buf = torch.full((GUARD + count + GUARD,), -777.0, dtype=torch.float32, device=DEV)
    src, txt = sample.to(DEV).contiguous(), text.to(DEV).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().nesr_unet_forward_f32(m._context(src.device), ctypes.c_void_p(src.data_ptr()), n, ch, h, w, float(timestep), int(label),
                                                 ctypes.c_void_p(txt.data_ptr()), txt.shape[1], ctypes.c_void_p(buf.data_ptr() + 4 * GUARD), count, stream),
               "nesr_unet_forward_f32")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == -777.0).all()) and bool((buf[GUARD + count:] == -777.0).all()), "the entry wrote outside the result it reports"
    return buf[GUARD:GUARD + count].view(n, -1, h, w).cpu()


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_against_the_float64_restatement(name):
    m, case = model(name), C.by_name(name)
    y64, tol = C.reference(name)
    got = guarded_forward(m, case.sample, case.timestep, case.text, case.label)
    assert got.shape == y64.shape and bool(torch.isfinite(got).all())
    err = float((got.double() - y64).abs().max())
    print(f"{name}: {tuple(y64.shape)}, err {err:.3e}, tol {tol:.3e}, err / tol {err / tol if tol else 0.0:.3f}")
    assert err <= tol
    again = m(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label)
    assert again.is_cuda and again.dtype == torch.float32 and torch.equal(again.cpu(), got)      # a repeated forward: the same bits


def test_a_sample_does_not_depend_on_its_batch():
    m, case = model("batch_two"), C.by_name("batch_two")
    both = m(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label).cpu()
    for i in range(2):
        alone = m(case.sample[i:i + 1].to(DEV), case.timestep, case.text[i:i + 1].to(DEV), case.label).cpu()
        assert torch.equal(alone[0], both[i]), f"sample {i} alone differs from sample {i} of two"
    assert not torch.equal(both[0], both[1])
