"""GPU: `VaeDecoder.decode` on every crafted case of tests/vae_cases.py against the float64 restatement, within the case's own
tolerance (8 x the float32 restatement's error, computed here).  The sample is written into the middle of a buffer of sentinels
(the guards are asserted), and a second forward on the same context gives the same bits."""
import ctypes

import pytest
import torch

from neural_enhanced_super_resolution_amd import VaeDecoder, _lib
from tests import vae_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
_cache = {}


def model(name):
    if name not in _cache:
        case = C.by_name(name)
        m = VaeDecoder(**case.cfg).to(DEV)
        m.load_state_dict(case.sd)
        _cache[name] = m
    return _cache[name]


def guarded_decode(m, z):
    """nesr_vae_decode_f32 into the middle of a buffer of sentinels: the sample on the host; the guards are asserted."""
    _, ch, h, w = z.shape
    oh, ow = m.output_size(h, w)
    n = int(m.config["out_channels"]) * oh * ow
    buf = torch.full((GUARD + n + GUARD,), -777.0, dtype=torch.float32, device=DEV)
    src = z.to(DEV).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().nesr_vae_decode_f32(m._context(src.device), ctypes.c_void_p(src.data_ptr()), 1, ch, h, w,
                                               ctypes.c_void_p(buf.data_ptr() + 4 * GUARD), n, stream), "nesr_vae_decode_f32")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == -777.0).all()) and bool((buf[GUARD + n:] == -777.0).all()), "the entry wrote outside the sample it reports"
    return buf[GUARD:GUARD + n].view(1, -1, oh, ow).cpu()


@pytest.mark.parametrize("name", C.NAMES)
def test_decode_against_the_float64_restatement(name):
    m = model(name)
    z, y64, tol = C.reference(name)
    got = guarded_decode(m, z)
    assert got.shape == y64.shape and bool(torch.isfinite(got).all())
    err = float((got.double() - y64).abs().max())
    print(f"{name}: {tuple(y64.shape)}, err {err:.3e}, tol {tol:.3e}, err / tol {err / tol if tol else 0.0:.3f}")
    assert err <= tol
    again = m.decode(z.to(DEV))
    assert again.is_cuda and again.dtype == torch.float32 and torch.equal(again.cpu(), got)      # a repeated forward: the same bits
    assert torch.equal(m(z.to(DEV)).cpu(), got)                                                   # __call__ is decode
