"""Swin2SR without a GPU: the restatement of tests/swin2sr_ref.py pinned to ``transformers`` in float64 on every crafted case, its
frame-level route to transformers' image processor, the key set against transformers' own state_dict, nesr_swin2sr_output_size,
the new symbols, the strictness of the loader, the configuration checks of nesr_swin2sr_create that come before any device, and
the thin-sample condition of the u8 criterion for the committed seeds."""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

from neural_enhanced_super_resolution_amd import Swin2SR, _lib, swin2sr_state_dict_spec
from neural_enhanced_super_resolution_amd import nesr_adapter
from tests import swin2sr_cases as C
from tests import swin2sr_ref as R

FORWARD = [c.name for c in C.forward_cases()]
NAMES = [c.name for c in C.cases()]
FRAME_NAMES = [c.name for c in C.frame_cases()]      # the RGB configurations: the frame-level route takes no other


def hf_model(cfg):
    transformers = pytest.importorskip("transformers")
    config = transformers.Swin2SRConfig(**{k: list(v) if isinstance(v, tuple) else v for k, v in cfg.items()})
    return transformers.Swin2SRForImageSuperResolution(config).eval()


@pytest.mark.parametrize("name", FORWARD)
def test_restatement_matches_transformers_f64(name):
    case = C.by_name(name)
    model = hf_model(case.cfg).double()
    assert list(model.state_dict()) == list(case.sd)
    model.load_state_dict({k: v.double() for k, v in case.sd.items()})
    with torch.no_grad():
        want = model(pixel_values=case.x.double()).reconstruction
    got = C.reference(case)[0]
    assert got.shape == want.shape
    err, bound = float((got - want).abs().max()), 1e-9 * max(1.0, float(want.abs().max()))
    print(f"restatement vs transformers f64, {name}: {tuple(want.shape)}, max |diff| = {err:.3e}, bound {bound:.3e}, max |out| = {float(want.abs().max()):.3f}")
    assert err <= bound


@pytest.mark.parametrize("name", NAMES + ["default"])
def test_state_dict_spec_is_transformers_own(name):
    cfg = {} if name == "default" else C.by_name(name).cfg
    if name == "default":
        cfg = dict(depths=(1, 1), num_heads=(6, 6))      # the configuration class's defaults at a depth that builds quickly
    want = OrderedShapes(hf_model(cfg).state_dict())
    assert list(swin2sr_state_dict_spec(**cfg).items()) == want
    assert list(R.state_dict_spec(**cfg).items()) == want
    m = Swin2SR(**cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want


def OrderedShapes(sd):
    return [(k, tuple(v.shape)) for k, v in sd.items()]


def test_transformers_renames_no_swin2sr_key():
    """One key generation: the loader takes transformers' names as they are."""
    pytest.importorskip("transformers")
    import inspect

    from transformers import conversion_mapping
    assert "swin2sr" not in inspect.getsource(conversion_mapping).lower()


@pytest.mark.parametrize("hw", [(13, 18), (8, 8), (5, 7), (1, 1), (2, 3)])
def test_process_frame_is_the_image_processor(hw):
    pytest.importorskip("transformers")
    try:
        from transformers.models.swin2sr.image_processing_pil_swin2sr import Swin2SRImageProcessorPil as Proc
    except Exception:
        Proc = pytest.importorskip("transformers").Swin2SRImageProcessor
    frame = R.seeded_frame(hw[0], hw[1], 3)
    want = Proc()(frame, return_tensors="pt", input_data_format="channels_last")["pixel_values"]
    got = R.process_frame(frame, torch.float32)
    assert tuple(got.shape) == tuple(want.shape) == (1, 3, R.padded_size(hw[0]), R.padded_size(hw[1]))
    assert float((got - want.float()).abs().max()) <= 1e-7


@pytest.mark.parametrize("name", FRAME_NAMES)
@pytest.mark.parametrize("hw", C.FRAMES, ids=lambda hw: "%dx%d" % hw)
def test_thin_samples_stay_under_the_cap(name, hw):
    """The u8 criterion leaves out the samples whose float64 value x 255 lies within 255 tol of a rounding boundary; the seeds are
    chosen so that these are at most 2 % (a condition the GPU test relies on), and the float32 restatement meets the criterion."""
    case = C.by_name(name)
    frame, y64, tol = C.frame_reference(name, hw)
    s = case.cfg["upscale"]
    assert tuple(y64.shape) == (hw[0] * s, hw[1] * s, 3) and tol > 0
    y32 = R.upscale_float(case.sd, frame, torch.float32, **case.cfg)
    excluded, wrong, n = R.u8_check(R.quantise(y32), y64, tol)
    inside = float(((y64 > 0) & (y64 < 1)).double().mean())
    print(f"{name} {hw}: tol {tol:.3e}, {excluded} of {n} samples thin ({100.0 * excluded / n:.2f} %), {wrong} wrong (f32 CPU), {100 * inside:.0f} % inside (0, 1)")
    assert excluded <= C.MAX_THIN * n and wrong == 0
    assert inside > 0.5      # the clamp does not decide most samples


@pytest.mark.parametrize("name", C.SMALL_FRAME_CASES)
@pytest.mark.parametrize("hw", C.SMALL_FRAMES, ids=lambda hw: "%dx%d" % hw)
def test_thin_samples_stay_under_the_cap_on_small_frames(name, hw):
    """The same condition on the frames shorter than the processor's padding (a 1 x 1 frame has 12 s^2 samples: none may be thin)."""
    test_thin_samples_stay_under_the_cap(name, hw)


def test_output_size_needs_no_device():
    assert Swin2SR(depths=(1,), num_heads=(6,)).output_size(13, 18) == (26, 36)
    assert Swin2SR(depths=(1,), num_heads=(6,), upscale=4, upsampler="nearest+conv").output_size(8, 8) == (32, 32)
    oh, ow = ctypes.c_int(0), ctypes.c_int(0)
    lib = _lib.load()
    assert lib.nesr_swin2sr_output_size(3, 7, 9, ctypes.byref(oh), ctypes.byref(ow)) == 0 and (oh.value, ow.value) == (21, 27)
    assert lib.nesr_swin2sr_output_size(0, 7, 9, ctypes.byref(oh), ctypes.byref(ow)) == _lib.ERR_ARG
    assert lib.nesr_swin2sr_output_size(2, 0, 9, ctypes.byref(oh), ctypes.byref(ow)) == _lib.ERR_ARG


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in ("create", "destroy", "num_tensors", "load_weight", "finalize", "output_size", "forward_f32", "upscale_u8", "set_timing", "kernel_time_ms"):
        assert getattr(lib, "nesr_swin2sr_" + name) is not None
    assert callable(nesr_adapter.swin2sr_stage)


def test_load_state_dict_is_strict():
    case = C.by_name("small_shift")
    m = Swin2SR(**case.cfg)
    m.load_state_dict(case.sd)
    sd = dict(case.sd)
    first = next(iter(sd))
    del sd[first]
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict(sd)
    sd = dict(case.sd, extra=torch.zeros(1))
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict(sd)
    sd = dict(case.sd)
    sd[first] = torch.zeros(5)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict(sd)
    # what older checkpoints carry is accepted and ignored
    a = "swin2sr.encoder.stages.0.layers.1.attention.self."
    m.load_state_dict(dict(case.sd, **{a + "relative_position_index": torch.zeros(16, 16), a + "relative_coords_table": torch.zeros(1, 7, 7, 2),
                                       "swin2sr.encoder.stages.0.layers.1.attn_mask": torch.zeros(15, 16, 16)}))
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        m(torch.zeros(1, 3, 8, 8))
    with pytest.raises(FileNotFoundError):
        Swin2SR.from_checkpoint("caidas/swin2SR-classical-sr-x2-64")


BASE = dict(embed_dim=24, num_heads=(2,), depths=(1,), window_size=4, image_size=16)
UNSUPPORTED = [
    ("upsampler", dict(upsampler="pixelshuffle_aux")),
    ("upsampler", dict(upsampler="")),
    ("resi_connection", dict(resi_connection="3conv")),
    ("use_absolute_embeddings", dict(use_absolute_embeddings=True)),
    ("patch_size", dict(patch_size=2)),
    ("qkv_bias", dict(qkv_bias=False)),
    ("image_size", dict(image_size=4)),
    ("num_heads", dict(num_heads=(2, 3), depths=(1, 1))),
    ("num_heads", dict(num_heads=(5,))),
    ("upscale", dict(upsampler="pixelshuffle", upscale=5)),
    ("upscale", dict(upsampler="nearest+conv", upscale=2)),
    ("window_size", dict(window_size=16, image_size=64, embed_dim=180, num_heads=(6,))),
]


@pytest.mark.parametrize("field,change", UNSUPPORTED, ids=[f"{f}-{i}" for i, (f, _) in enumerate(UNSUPPORTED)])
def test_unsupported_configurations_name_the_field_before_any_device(field, change):
    m = Swin2SR(**dict(BASE, **change))
    with pytest.raises(_lib.NesrUnsupportedError, match=field):
        m._create(0)
