"""CPU: the fp16 compute form of SRVGGNetCompact (compute_dtype="fp16", NESR_DTYPE_F16) without a kernel: the spelling and
what .half() does to it, nesr_create_compact's argument checks for dtype 4, and the form's specification
(tests/srvgg_fp16_emu.py) against the float64 network -- the three extra mantissa bits over bf16."""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import SRVGGNetCompact
from neural_enhanced_super_resolution_amd.synth import synthetic_compact_state_dict, synthetic_frame
from tests.srvgg_fp16_emu import SRVGGEmu16
from tests.srvgg_ref import SRVGGRef

CONFIGS = [dict(num_conv=32, upscale=4, act_type="prelu"),       # realesr-general-x4v3
           dict(num_conv=16, upscale=4, act_type="prelu"),       # realesr-animevideov3
           dict(num_conv=16, upscale=2, act_type="relu")]


def test_fp16_spelling_is_accepted_and_f16_is_not():
    from neural_enhanced_super_resolution_amd import _lib
    m = SRVGGNetCompact(compute_dtype="fp16")
    assert m.compute_dtype == "fp16" and m._dtype_code() == _lib.DTYPE_F16 == 4
    with pytest.raises(ValueError, match="fp16"):
        SRVGGNetCompact(compute_dtype="f16")


def test_half_keeps_fp16():
    assert SRVGGNetCompact(num_conv=1, compute_dtype="fp16").half().compute_dtype == "fp16"
    assert SRVGGNetCompact(num_conv=1, compute_dtype="fp16").to(torch.float16).compute_dtype == "fp16"
    assert SRVGGNetCompact(num_conv=1, compute_dtype="fp16").to(torch.bfloat16).compute_dtype == "fp16"
    assert SRVGGNetCompact(num_conv=1, compute_dtype="fp16").eval().compute_dtype == "fp16"


def test_a_default_model_still_turns_bf16():
    from neural_enhanced_super_resolution_amd import _lib
    m = SRVGGNetCompact(num_conv=1).half()
    assert m.compute_dtype == "bf16" and m._dtype_code() == _lib.DTYPE_BF16
    assert SRVGGNetCompact(num_conv=1).to(torch.float16).compute_dtype == "bf16"
    assert SRVGGNetCompact(num_conv=1, compute_dtype="bf16").half().compute_dtype == "bf16"


def test_create_with_dtype_4_rejects_bad_shapes_without_touching_a_device():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    bad = [(0, 3, 3, 48, 16, 4, 0, 4), (0, 3, 3, 64, 16, 3, 0, 4), (0, 1, 1, 64, 16, 4, 0, 4), (0, 3, 3, 64, 0, 4, 0, 4),
           (0, 3, 3, 64, 16, 4, 7, 4), (0, 3, 3, 64, 16, 4, 0, 5)]
    for args in bad:
        assert lib.nesr_create_compact(ctypes.byref(h), *args) == -1, args
        assert lib.nesr_last_error()
        assert h.value is None
    # the refusal of an unknown dtype names the form as one it takes
    assert b"NESR_DTYPE_F16" in lib.nesr_last_error()


def _psnr(a, b):
    return 10 * np.log10(1.0 / max(float(((a.double() - b.double()) ** 2).mean()), 1e-30))


@pytest.mark.parametrize("cfg", CONFIGS)
def test_fp16_storage_is_12_db_closer_to_float64_than_bf16(cfg):
    """Operands and stored activations in f16 carry 11 significant bits against bf16's 8: 18 dB.  Asked for: 12 dB, two of the
    three bits."""
    sd = synthetic_compact_state_dict(seed=0, **cfg)
    x = torch.stack([torch.from_numpy(synthetic_frame(67, 93, seed=3 + i)).permute(2, 0, 1).double() / 255 for i in range(2)])
    ref = SRVGGRef(**cfg)
    ref.load_state_dict(sd)
    out = {}
    pre = []
    with torch.no_grad():
        want = ref(x)
        for name, store in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            emu = SRVGGEmu16(**cfg, store=store)
            emu.load_state_dict(sd)
            out[name] = emu(x, pre if name == "fp16" else None)
    p16, pbf = _psnr(out["fp16"], want), _psnr(out["bf16"], want)
    top = max(float(p.abs().max()) for p in pre)
    print(f"{cfg}: fp16 storage {p16:.2f} dB, bf16 storage {pbf:.2f} dB, largest pre-activation {top:.2f}")
    assert p16 >= pbf + 12.0, (p16, pbf)
    assert top < 65504 / 100                        # the released shapes sit far inside f16's range
