"""Swin2SR's fp16 compute form without a GPU: the emulation of tests/swin2sr_f16_emu.py changes nothing but the rounding, every
named fault fails the (case, part)s named for it by 10 x that pair's tolerance, and the C ABI's refusals that need no device: the
dtypes nesr_swin2sr_set_dtype takes, its place between create and finalize, and a weight f16 cannot carry at finalize.

The tolerance of a (case, part) is 8 x max |emulation in float32 - emulation in float64|, computed here; the tokens are N(0, 1),
seed 7.  Measured ratio (fault's error / tolerance) of every named pair, by this file's own print:
  unrounded 3131, 315, 137; bf16 14802, 3719, 1314; weights_unrounded 3142, 325, 98; activations_unrounded 2251, 188, 101;
  qk_unrounded 1271, 1094, 38; p_unrounded 329, 145; gelu_unrounded 140, 25; first_conv_rounded 240, 215 (on the first convolution alone)."""
import ctypes

import pytest
import torch

from neural_enhanced_super_resolution_amd import Swin2SR, _lib
from neural_enhanced_super_resolution_amd._contexts import _invoke
from tests import swin2sr_cases as C
from tests import swin2sr_f16_emu as E
from tests import swin2sr_ref as R

FORWARD = [c.name for c in C.forward_cases()]
_GEMMS = [("x3_range255", "attention"), ("window_2_many_heads", "mlp"), ("window_6_wide", "stage_conv")]
NAMED = {
    "unrounded": _GEMMS,
    "bf16": _GEMMS,
    "weights_unrounded": _GEMMS,
    "activations_unrounded": _GEMMS,
    "qk_unrounded": [("x3_range255", "attention"), ("window_2_many_heads", "attention"), ("gray", "attention")],
    "p_unrounded": [("x3_range255", "attention"), ("window_2_many_heads", "attention")],
    "gelu_unrounded": [("window_2_many_heads", "mlp"), ("window_5_one_head", "mlp")],
    "first_conv_rounded": [("small_shift", "first_conv"), ("published_width", "first_conv")],
}


def test_every_fault_is_named():
    assert set(NAMED) == set(E.FAULTS)


@pytest.mark.parametrize("name", ["small_shift", "window_7_odd", "gray"])
def test_float64_rounding_changes_nothing(name):
    case = C.by_name(name)
    for x in (case.x, case.x.double()):
        with torch.no_grad():
            plain = R.swin2sr_forward(case.sd, x, **case.cfg)
        assert torch.equal(E.forward(case.sd, x, torch.float64, **case.cfg), plain)


def test_the_hook_sees_every_matmul_and_restores_the_module():
    case = C.by_name("small_shift")
    plain = R.position_bias
    with E.hooked() as mode:
        R.swin2sr_forward(case.sd, case.x, **case.cfg)
    assert mode.matmuls == 2 * sum(case.cfg["depths"]) and R.position_bias is plain


@pytest.mark.parametrize("name", ["small_shift", "window_5_one_head", "one_window_shifted"])
def test_attention_then_mlp_is_the_layer(name):
    case = C.by_name(name)
    for layer in range(2):
        two, one = E.layer_in_two_parts(case.sd, 0, layer, E.seeded_tokens(case).double(), **case.cfg)
        assert torch.equal(two, one)


def test_the_form_differs_from_f32_and_rounds_what_it_says():
    case = C.by_name("small_shift")
    tokens, layer, e64, tol = E.part_reference(case, "mlp")
    plain = E.part("mlp", case.sd, 0, layer, tokens.double(), torch.float64, **case.cfg)
    assert float((plain - e64).abs().max()) > 10 * tol
    # rounded inputs and weights given to the unrounded part give the emulation's fc1; GELU's rounding is inside, so not the whole
    x16 = tokens.half().double()
    assert not torch.equal(E.part("mlp", case.sd, 0, layer, x16, torch.float64, **case.cfg), e64)


@pytest.mark.parametrize("fault", E.FAULTS)
def test_fault_fails_its_named_cases(fault):
    for name, part in NAMED[fault]:
        case = C.by_name(name)
        tol = E.part_reference(case, part)[3]
        err = E.part_fault(case, part, fault)
        print(f"{fault}: {name} / {part}: error {err:.3e}, tolerance {tol:.3e}, ratio {err / tol:.1f}")
        assert tol > 0 and err > 10 * tol, (fault, name, part, err, tol)


@pytest.mark.parametrize("name", FORWARD)
def test_float32_emulation_passes_every_part(name):
    """The criterion accepts the float32 evaluation of the specification itself (by construction 1/8 of the tolerance), and the
    whole-network bound holds for it."""
    case = C.by_name(name)
    for part in E.PARTS:
        tokens, layer, e64, tol = E.part_reference(case, part)
        e32 = E.part(part, case.sd, 0, layer, tokens, **case.cfg)
        assert torch.isfinite(e32).all() and float((e32.double() - e64).abs().max()) <= tol
    y64, e64, bound = E.network_reference(case)
    e32 = E.forward(case.sd, case.pixel_values(), **case.cfg)
    assert float((e32.double() - y64).abs().max()) <= bound


# ------------------------------------------------------------------------------------------------ Python and the C ABI, no device
def test_compute_dtype_is_a_keyword_of_the_model_not_of_the_configuration():
    cfg = C.by_name("small_shift").cfg
    m = Swin2SR(compute_dtype="fp16", **cfg)
    assert m.compute_dtype == "fp16" and "compute_dtype" not in m.config
    assert Swin2SR(**cfg).compute_dtype == "f32"
    assert Swin2SR(**cfg).half().compute_dtype == "f32"      # .half() does not select the form
    with pytest.raises(ValueError, match="bf16"):
        Swin2SR(compute_dtype="bf16", **cfg)
    with pytest.raises(ValueError, match="part"):
        m.part("softmax", 0, 0, torch.zeros(1, 4, 4, cfg["embed_dim"]))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        m.part("mlp", 0, 0, torch.zeros(1, 4, 4, cfg["embed_dim"]))


def test_set_dtype_refusals_need_no_context():
    lib = _lib.load()
    assert lib.nesr_swin2sr_set_dtype(None, _lib.DTYPE_BF16) == _lib.ERR_UNSUPPORTED
    assert b"significand" in lib.nesr_last_error()
    for dtype in (_lib.DTYPE_F32_WINOGRAD, _lib.DTYPE_F32_SPLIT, 5, -1):
        assert lib.nesr_swin2sr_set_dtype(None, dtype) == _lib.ERR_ARG
    assert lib.nesr_swin2sr_set_dtype(None, _lib.DTYPE_F16) == _lib.ERR_ARG      # a form it takes, but no context


def _host_context(model, sd):
    """A context without a device (NESR_SWIN2SR_NO_DEVICE) given `sd`; the caller finalizes and destroys it."""
    handle = model._create(-1)
    for key, t in sd.items():
        t = t.detach().float().contiguous()
        shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
        _invoke("nesr_swin2sr_load_weight", None, handle, (key.encode(), t, shape, t.dim()))
    return handle


ERR_STATE = -3
RANGE_KEYS = ["swin2sr.encoder.stages.0.layers.1.attention.self.key.weight", "swin2sr.encoder.stages.1.layers.0.output.dense.weight",
              "swin2sr.encoder.stages.0.conv.weight", "swin2sr.embeddings.patch_embeddings.projection.weight", "upsample.final_convolution.weight"]


@pytest.mark.parametrize("key", RANGE_KEYS)
@pytest.mark.parametrize("value", [65520.0, -7e4, float("inf"), float("nan")])
def test_a_weight_f16_cannot_carry_is_refused_at_finalize(key, value):
    case = C.by_name("small_shift")
    lib = _lib.load()
    sd = {k: v.clone() for k, v in case.sd.items()}
    sd[key].view(-1)[3] = value
    handle = _host_context(Swin2SR(compute_dtype="fp16", **case.cfg), sd)
    try:
        assert lib.nesr_swin2sr_finalize(handle) == _lib.ERR_RANGE
        assert key.encode() in lib.nesr_last_error()
    finally:
        lib.nesr_swin2sr_destroy(handle)
    handle = _host_context(Swin2SR(**case.cfg), sd)      # the f32 form carries it
    try:
        assert lib.nesr_swin2sr_finalize(handle) == 0
    finally:
        lib.nesr_swin2sr_destroy(handle)


def test_the_largest_f16_passes_and_the_form_is_fixed_at_finalize():
    case = C.by_name("small_shift")
    lib = _lib.load()
    sd = {k: v.clone() for k, v in case.sd.items()}
    sd[RANGE_KEYS[0]].view(-1)[0] = 65504.0
    sd["swin2sr.first_convolution.weight"].view(-1)[0] = 1e6      # not a GEMM of the form: stays f32
    sd["swin2sr.encoder.stages.0.layers.0.layernorm_after.weight"][0] = 1e5
    handle = _host_context(Swin2SR(compute_dtype="fp16", **case.cfg), sd)
    try:
        assert lib.nesr_swin2sr_set_dtype(handle, _lib.DTYPE_F32) == 0 and lib.nesr_swin2sr_set_dtype(handle, _lib.DTYPE_F16) == 0
        assert lib.nesr_swin2sr_set_dtype(handle, _lib.DTYPE_BF16) == _lib.ERR_UNSUPPORTED
        assert lib.nesr_swin2sr_finalize(handle) == 0
        assert lib.nesr_swin2sr_set_dtype(handle, _lib.DTYPE_F32) == ERR_STATE
        assert b"between" in lib.nesr_last_error()
        # no device: nothing that would launch
        assert lib.nesr_swin2sr_part_f32(handle, 0, 0, 0, ctypes.c_void_p(64), 1, 4, 4, ctypes.c_void_p(64), 1 << 20, None) == ERR_STATE
        n = ctypes.c_int64(7)      # nor a timing to collect: refused as the other networks' entries refuse it, before any device call
        assert lib.nesr_swin2sr_kernel_time_ms(handle, None, 0, ctypes.byref(n)) == ERR_STATE and n.value == 7
        assert lib.nesr_last_error() == b"nesr_swin2sr_kernel_time_ms: a context without a device launches nothing"
    finally:
        lib.nesr_swin2sr_destroy(handle)


def test_new_symbols_are_exported():
    lib = _lib.load()
    assert lib.nesr_swin2sr_set_dtype is not None and lib.nesr_swin2sr_part_f32 is not None
