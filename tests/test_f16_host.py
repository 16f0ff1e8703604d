"""CPU: the f16 compute form (NESR_DTYPE_F16) at the Python and header level -- the dtype strings and codes, and that it is
opt-in: .half(), torch.float16 and half=True keep meaning bf16 for every model that did not ask for f16."""
import os
import re

import pytest
import torch

from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, SRVGGNetCompact, _lib
from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(dtype, **kw):
    return RRDBNet(3, 3, scale=2, num_block=1, compute_dtype=dtype, **kw)


def test_f16_dtype_strings_map_to_the_f16_code():
    assert _lib.DTYPE_F16 == 4
    for s in ("f16", "fp16"):
        net = _net(s)
        assert net.compute_dtype == "f16"                  # "fp16" is an alias
        assert net._dtype_code() == _lib.DTYPE_F16


@pytest.mark.parametrize("dtype,code", [("bf16", _lib.DTYPE_BF16), ("half", _lib.DTYPE_BF16), (torch.float16, _lib.DTYPE_BF16),
                                        (torch.bfloat16, _lib.DTYPE_BF16), ("f32", _lib.DTYPE_F32_SPLIT),
                                        ("f32-winograd", _lib.DTYPE_F32_WINOGRAD), ("f32-direct", _lib.DTYPE_F32)])
def test_existing_dtype_strings_keep_their_codes(dtype, code):
    assert _net(dtype)._dtype_code() == code


def test_unknown_dtype_still_raises():
    with pytest.raises(ValueError):
        _net("f8")._dtype_code()


def test_half_keeps_an_f16_model_f16_and_gives_bf16_otherwise():
    assert _net("f16").half().compute_dtype == "f16"
    assert _net("fp16").half().compute_dtype == "f16"
    assert _net("f32").half().compute_dtype == "bf16"
    assert RRDBNet(3, 3, scale=2, num_block=1).half().compute_dtype == "bf16"


def test_apply_to_fp16_tensors_keeps_an_f16_model_f16():
    net = _net("f16").to(torch.float16)
    assert net.compute_dtype == "f16" and net._dtype_code() == _lib.DTYPE_F16
    net = _net("f32").to(torch.float16)
    assert net.compute_dtype == "bf16"
    net = _net("f32").to(torch.bfloat16)
    assert net.compute_dtype == "bf16"


def test_realesrganer_half_with_an_f16_model_is_fp16_and_ragged():
    """RealESRGANer(half=True, model=RRDBNet(..., compute_dtype="f16")) is upstream's fp16 run: the model stays f16, and a tiling
    wrapper makes it size-independent (its tiles run as ragged batches through the strip kernel, as bf16's do)."""
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=1)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=_net("f16"), tile=512, tile_pad=10, pre_pad=0, half=True,
                      device="cpu")
    assert up.model.compute_dtype == "f16" and up.model._dtype_code() == _lib.DTYPE_F16
    assert up.model.size_independent
    assert up.model.strip_kernel_active() == (os.environ.get("NESR_STRIP", "-1") != "0")
    default = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=1), tile=512, tile_pad=10,
                           pre_pad=0, half=True, device="cpu")
    assert default.model.compute_dtype == "bf16"


def test_srvgg_still_rejects_f16():
    with pytest.raises(ValueError):
        SRVGGNetCompact(num_conv=2, upscale=4, compute_dtype="f16")._dtype_code()


def test_header_enum_matches_lib():
    text = open(os.path.join(ROOT, "include", "nesr_hip.h")).read()
    m = re.search(r"NESR_DTYPE_F16\s*=\s*(\d+)", text)
    assert m, "include/nesr_hip.h does not declare NESR_DTYPE_F16"
    assert int(m.group(1)) == _lib.DTYPE_F16
    for name in ("F32", "BF16", "F32_WINOGRAD", "F32_SPLIT"):
        assert int(re.search(rf"NESR_DTYPE_{name}\s*=\s*(\d+)", text).group(1)) == getattr(_lib, f"DTYPE_{name}")
