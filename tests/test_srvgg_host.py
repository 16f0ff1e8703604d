"""CPU: SRVGGNetCompact's parameters, state-dict spec, shim import, argument checks and the synthetic weights
(no kernel runs here; the forward is tests/test_gpu_srvgg.py)."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import SRVGGNetCompact, srvgg_state_dict_spec
from neural_enhanced_super_resolution_amd.synth import synthetic_compact_state_dict, synthetic_frame
from tests.srvgg_ref import SRVGGRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(nc, act, s) for nc in (16, 32) for act in ("prelu", "relu", "leakyrelu") for s in (2, 4)]


@pytest.mark.parametrize("num_conv,act,up", CONFIGS)
def test_spec_matches_reference_state_dict(num_conv, act, up):
    ref = SRVGGRef(num_conv=num_conv, upscale=up, act_type=act).state_dict()
    spec = srvgg_state_dict_spec(3, 3, 64, num_conv, up, act)
    assert list(spec) == list(ref)
    assert [tuple(v.shape) for v in ref.values()] == list(spec.values())
    ours = SRVGGNetCompact(num_conv=num_conv, upscale=up, act_type=act).state_dict()
    assert list(ours) == list(ref) and [tuple(v.shape) for v in ours.values()] == list(spec.values())


def test_tensor_counts_of_the_released_models():
    assert len(srvgg_state_dict_spec(num_conv=32, upscale=4, act_type="prelu")) == 101     # realesr-general-x4v3
    assert len(srvgg_state_dict_spec(num_conv=16, upscale=4, act_type="prelu")) == 53      # realesr-animevideov3


def test_load_state_dict_round_trips():
    sd = synthetic_compact_state_dict(seed=3, num_conv=16)
    m = SRVGGNetCompact(num_conv=16)
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        SRVGGNetCompact(num_conv=32).load_state_dict(sd, strict=True)


def test_shim_import_resolves_to_the_class(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "dropin"))
    for m in [m for m in sys.modules if m.split(".")[0] == "realesrgan"]:
        monkeypatch.delitem(sys.modules, m)
    importlib.invalidate_caches()
    from realesrgan.archs.srvgg_arch import SRVGGNetCompact as shim
    assert shim is SRVGGNetCompact


def test_bad_arguments_raise():
    with pytest.raises(ValueError):
        SRVGGNetCompact(compute_dtype="f16")
    with pytest.raises(ValueError):
        SRVGGNetCompact(act_type="gelu")
    with pytest.raises(ValueError):
        srvgg_state_dict_spec(act_type="swish")


def test_half_selects_bf16():
    assert SRVGGNetCompact().half().compute_dtype == "bf16"
    assert SRVGGNetCompact().to(torch.bfloat16).compute_dtype == "bf16"
    assert SRVGGNetCompact().eval().compute_dtype == "f32"


def test_cpu_input_raises():
    m = SRVGGNetCompact(num_conv=1)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(1, 3, 4, 4))


def test_create_rejects_bad_arguments_without_touching_a_device():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    bad = [(0, 3, 3, 48, 16, 4, 0, 3), (0, 3, 3, 64, 16, 3, 0, 3), (0, 1, 1, 64, 16, 4, 0, 3), (0, 3, 3, 64, 0, 4, 0, 3),
           (0, 3, 3, 64, 16, 4, 7, 3), (0, 3, 3, 64, 16, 4, 0, 0), (0, 3, 3, 64, 16, 4, 0, 2)]
    for args in bad:
        assert lib.nesr_create_compact(ctypes.byref(h), *args) == -1, args
        assert lib.nesr_last_error()
        assert h.value is None


def test_synthetic_weights_are_reproducible_and_keep_the_body_scale():
    a = synthetic_compact_state_dict(seed=5, num_conv=32)
    b = synthetic_compact_state_dict(seed=5, num_conv=32)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["body.2.weight"], synthetic_compact_state_dict(seed=6, num_conv=32)["body.2.weight"])
    slopes = torch.cat([v for k, v in a.items() if v.dim() == 1 and int(k.split(".")[1]) % 2 == 1])
    assert 0.1 <= float(slopes.min()) and float(slopes.max()) <= 0.3
    ref = SRVGGRef(num_conv=32)
    ref.load_state_dict(a)
    x = torch.from_numpy(synthetic_frame(48, 48, seed=1)).permute(2, 0, 1)[None].float() / 255
    pre = []
    with torch.no_grad():
        y = ref(x, pre)
    stds = [float(p.std()) for p in pre]
    assert min(stds[8:]) > 0.5 * stds[1] and max(stds) < 4 * stds[1]           # no collapse or blow-up over 33 activations
    neg = [float((p < 0).double().mean()) for p in pre]
    assert min(neg) > 0.3 and max(neg) < 0.7                                   # the slope path runs on every layer
    residual = y - torch.nn.functional.interpolate(x, scale_factor=4, mode="nearest")
    assert 0.05 < float(residual.std()) < 0.5                                  # the body's contribution is visible
