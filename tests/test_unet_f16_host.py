"""CPU: the specification of the UNet's fp16 compute form (tests/unet_f16_emu.py) and the host side of the form in the library.

  emulation   with rounding=float64 it is tests/unet_ref.py bit for bit, on every case of tests/unet_cases.py
  faults      every named departure from the specification misses the (case, launch) named for it by 10 x that launch's tolerance
  subnormals  the two subnormal switches agree on every toleranced shape the GPU tests use, and differ on the one exact case
              that carries weights of 2^-20
  finalize    a context without a device (NESR_UNET_NO_DEVICE): the range check of the GEMM weights, the order of set_dtype
  packing     the library's f16 packing against a packer written here from csrc/unet_api.h's comment alone
"""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import UNet2DCondition, _lib
from tests import unet_cases as C
from tests import unet_f16_emu as E
from tests.unet_kernel_ref import up16

NO_DEVICE = -1      # NESR_UNET_NO_DEVICE
ERR_STATE = -3      # NESR_ERR_STATE


# ------------------------------------------------------------------------------------------------ the emulation
@pytest.mark.parametrize("name", C.NAMES)
def test_rounding_to_float64_is_the_reference_bit_for_bit(name):
    case = C.by_name(name)
    y64, _ = C.reference(name)
    e = E.forward(case.sd, case.sample.double(), case.timestep, case.text, case.label, rounding=torch.float64, **case.cfg)
    assert e.dtype == torch.float64 and torch.equal(e, y64)


def test_the_gemm_weights_are_every_matrix_but_the_embedding_path():
    case = C.by_name("published_layout")
    keys = set(E.gemm_keys(case.sd))
    assert "conv_in.weight" in keys and "mid_block.attentions.0.transformer_blocks.0.ff.net.2.weight" in keys
    assert "down_blocks.1.resnets.0.conv_shortcut.weight" in keys and "mid_block.attentions.0.transformer_blocks.0.attn2.to_k.weight" in keys
    assert not any(k.startswith(("time_embedding.", "class_embedding.")) or ".time_emb_proj." in k or ".norm" in k or k.endswith(".bias") for k in keys)
    matrices = {k for k, v in case.sd.items() if v.dim() >= 2}
    assert matrices - keys == {k for k in matrices if k.startswith(("time_embedding.", "class_embedding.")) or ".time_emb_proj." in k}


def test_the_emulation_rounds_something():
    case = C.by_name("seam_groups")
    y64, _ = C.reference("seam_groups")
    e64 = E.forward(case.sd, case.sample.double(), case.timestep, case.text, case.label, **case.cfg)
    assert 1e-5 < float((e64 - y64).abs().max()) < 1e-1


@pytest.mark.parametrize("fault,name", [(f, n) for f in E.FAULTS for n in E.FAULT_CASE[f]])
def test_a_fault_misses_its_launch_by_ten_tolerances(fault, name):
    ratio = E.fault_ratio(fault, name)
    print(f"{fault} on {name}: {ratio:.1f} x tol")
    assert ratio > 10.0


def test_every_fault_has_a_case():
    assert set(E.FAULT_CASE) == set(E.FAULTS) and all(n in E.FAULT_CASES for names in E.FAULT_CASE.values() for n in names)


def test_the_subnormal_switches_agree_wherever_a_tolerance_is_used():
    """The toleranced launches of the GPU tests (tests/unet_kernels.py's through E.without_subnormal_operands) carry no operand that
    rounds to an f16 subnormal: the two emulations give the same bits.  The exact case of 2^-20 weights is where they part."""
    from tests import unet_kernels as UK
    for name in UK.NAMES:
        family, kind, _ = UK.BUILDERS[name]
        if family in ("conv", "rows") and kind == "tol":
            d = E.without_subnormal_operands(family, UK.by_name(name).dense)
            assert torch.equal(E.launch(family, d, subnormals="flushed"), E.launch(family, d)), name
            moved = sum(int((d[k] != UK.by_name(name).dense[k]).sum()) for k in ("x0", "x1", "w") if d.get(k) is not None)
            assert moved <= 2e-2 * sum(d[k].numel() for k in ("x0", "x1", "w") if d.get(k) is not None), name      # the case is still the case
    d = subnormal_case()
    kept, flushed = E.launch("rows", d), E.launch("rows", d, subnormals="flushed")
    assert bool((flushed == d["b"].double()).all()) and float((kept - flushed).abs().max()) > 0


@pytest.mark.parametrize("name", C.NAMES)
def test_the_subnormal_switches_agree_on_a_network_case(name):
    """The network cases of the GPU test are tests/unet_cases.py's with the GEMM weights below 2^-13 zeroed (E.network_case).  An
    activation can still round to a subnormal; flushing one moves an operand by at most 6.1e-5, and what reaches the output is
    that perturbation amplified as any float32 error is (the bound is no pin for this reason).  The two emulations must agree to a
    quarter of the bound, the share the bound's own 8 x float32 term leaves to such noise."""
    case = E.network_case(name)
    assert all(torch.equal(v, C.by_name(name).sd[k]) or k in E.gemm_keys(case.sd) for k, v in case.sd.items())
    kept = E.forward(case.sd, case.sample.double(), case.timestep, case.text, case.label, **case.cfg)
    flushed = E.forward(case.sd, case.sample.double(), case.timestep, case.text, case.label, subnormals="flushed", **case.cfg)
    y64, _, bound = E.network_reference(name)
    diff = float((kept - flushed).abs().max())
    print(f"{name}: kept - flushed {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound / 4


def subnormal_case():
    """Weights of +-2^-20 (an f16 subnormal: 2^-20 = 16 x 2^-24), integer activations in [-3, 3], integer bias: every product and
    sum is exact in float32, so the result is one of the two emulations bit for bit."""
    g = torch.Generator().manual_seed(777)
    sign = torch.randint(0, 2, (24, 48), generator=g).float() * 2.0 - 1.0
    return dict(x0=torch.randint(-3, 4, (1, 33, 48), generator=g).float(), x1=None, w=sign * 2.0 ** -20, b=torch.randint(-3, 4, (24,), generator=g).float())


# ------------------------------------------------------------------------------------------------ finalize without a device
def context(sd, cfg, dtype=_lib.DTYPE_F16):
    """A context without a device given `sd`; the caller finalizes and destroys it."""
    lib = _lib.load()
    h = UNet2DCondition(**cfg)._create(NO_DEVICE)
    assert lib.nesr_unet_set_dtype(h, dtype) == 0 and lib.nesr_unet_dtype(h) == dtype
    for key, t in sd.items():
        t = t.detach().to(torch.float32).contiguous()
        shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
        assert lib.nesr_unet_load_weight(h, key.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()) == 0, lib.nesr_last_error()
    return h


def finalize(sd, cfg):
    lib = _lib.load()
    h = context(sd, cfg)
    try:
        rc = lib.nesr_unet_finalize(h)
        return rc, (lib.nesr_last_error() or b"").decode()
    finally:
        lib.nesr_unet_destroy(h)


@pytest.mark.parametrize("value", [7e4, -7e4, float("nan"), float("inf")])
@pytest.mark.parametrize("key", ["down_blocks.1.resnets.0.conv2.weight", "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj.weight",
                                 "up_blocks.0.resnets.1.conv_shortcut.weight", "down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_v.weight"])
def test_a_gemm_weight_f16_cannot_carry_is_a_range_error_naming_the_key(key, value):
    case = C.by_name("one_text_token")
    sd = {k: v.clone() for k, v in case.sd.items()}
    sd[key].view(-1)[-1] = value
    rc, msg = finalize(sd, case.cfg)
    assert rc == _lib.ERR_RANGE and key in msg, (rc, msg)


@pytest.mark.parametrize("key", ["time_embedding.linear_1.weight", "down_blocks.0.resnets.0.time_emb_proj.weight", "conv_in.bias", "class_embedding.weight"])
def test_the_same_value_outside_the_gemms_is_accepted(key):
    case = C.by_name("one_text_token")
    sd = {k: v.clone() for k, v in case.sd.items()}
    sd[key].view(-1)[0] = 7e4
    assert finalize(sd, case.cfg)[0] == 0
    sd[key].view(-1)[0] = 65504.0
    assert finalize(sd, case.cfg)[0] == 0


def test_65504_in_a_gemm_weight_is_accepted_and_the_f32_form_takes_anything():
    lib, case = _lib.load(), C.by_name("one_text_token")
    sd = {k: v.clone() for k, v in case.sd.items()}
    sd["conv_out.weight"].view(-1)[3] = -65504.0
    assert finalize(sd, case.cfg)[0] == 0
    sd["conv_out.weight"].view(-1)[3] = 7e4
    h = context(sd, case.cfg, _lib.DTYPE_F32)
    try:
        assert lib.nesr_unet_finalize(h) == 0
    finally:
        lib.nesr_unet_destroy(h)


def test_set_dtype_order_and_values():
    lib, case = _lib.load(), C.by_name("one_text_token")
    h = context(case.sd, case.cfg)
    try:
        assert lib.nesr_unet_set_dtype(h, _lib.DTYPE_BF16) == _lib.ERR_UNSUPPORTED and b"BF16" in lib.nesr_last_error()
        assert lib.nesr_unet_set_dtype(h, 17) == _lib.ERR_UNSUPPORTED and b"17" in lib.nesr_last_error()
        assert lib.nesr_unet_set_dtype(h, _lib.DTYPE_F32) == 0 and lib.nesr_unet_dtype(h) == _lib.DTYPE_F32
        assert lib.nesr_unet_set_dtype(h, _lib.DTYPE_F16) == 0 and lib.nesr_unet_dtype(h) == _lib.DTYPE_F16
        assert lib.nesr_unet_finalize(h) == 0
        for dtype in (_lib.DTYPE_F32, _lib.DTYPE_F16):
            assert lib.nesr_unet_set_dtype(h, dtype) == ERR_STATE and b"nesr_unet_finalize" in lib.nesr_last_error()
        assert lib.nesr_unet_dtype(h) == _lib.DTYPE_F16
    finally:
        lib.nesr_unet_destroy(h)


def test_the_fp16_form_holds_half_the_gemm_bytes():
    lib, case = _lib.load(), C.by_name("one_text_token")
    sizes = {}
    for dtype in (_lib.DTYPE_F32, _lib.DTYPE_F16):
        h = context(case.sd, case.cfg, dtype)
        try:
            assert lib.nesr_unet_finalize(h) == 0
            n = ctypes.c_size_t(0)
            assert lib.nesr_unet_weight_bytes(h, ctypes.byref(n)) == 0
            sizes[dtype] = n.value
        finally:
            lib.nesr_unet_destroy(h)
    assert sizes[_lib.DTYPE_F16] < 0.75 * sizes[_lib.DTYPE_F32]      # the GEMM weights dominate; their f32 copy is not kept


def test_python_refuses_other_spellings():
    for bad in ("f16", "bf16", "float16", None):
        with pytest.raises(ValueError, match="compute_dtype"):
            UNet2DCondition(compute_dtype=bad, **C.SMALL)
    assert UNet2DCondition(**C.SMALL).compute_dtype == "f32" and UNet2DCondition(compute_dtype="fp16", **C.SMALL).compute_dtype == "fp16"


# ------------------------------------------------------------------------------------------------ the packing
def pack_linear(w, k0, k1):
    """csrc/unet_api.h: W16[ldw][K], K = cs0 + cs1, k contiguous; source 1's k after source 0's cs0."""
    n = w.shape[0]
    cs0, cs1 = up16(k0), up16(k1) if k1 else 0
    out = torch.zeros((up16(n), cs0 + cs1), dtype=torch.float16)
    out[:n, :k0] = w[:, :k0].half()
    out[:n, cs0:cs0 + k1] = w[:, k0:].half()
    return out


def pack_conv(w, c0, c1):
    """csrc/unet_api.h: W16[coutp][9][cs0 + cs1]: per output channel and tap source 0's cs0 channels, then source 1's cs1."""
    n = w.shape[0]
    cs0, cs1 = up16(c0), up16(c1) if c1 else 0
    taps = w.reshape(n, c0 + c1, 9).permute(0, 2, 1)      # [n][tap][cin]
    out = torch.zeros((up16(n), 9, cs0 + cs1), dtype=torch.float16)
    out[:n, :, :c0] = taps[:, :, :c0].half()
    out[:n, :, cs0:cs0 + c1] = taps[:, :, c0:].half()
    return out


@pytest.mark.parametrize("n,k0,k1", [(24, 80, 48), (16, 16, 0), (272, 32, 0), (5, 6, 10), (40, 1000, 0)])
def test_the_linear_packing_is_the_headers(n, k0, k1):
    lib = _lib.load()
    w = torch.randn((n, k0 + k1), generator=torch.Generator().manual_seed(n)).float().contiguous()
    want = pack_linear(w, k0, k1)
    got = np.full(want.numel(), 0x7777, np.uint16)
    assert lib.nesr_unet_pack_linear_f16(ctypes.c_void_p(w.data_ptr()), n, k0, k1, got.ctypes.data_as(ctypes.c_void_p), got.size) == 0
    got = torch.from_numpy(got.view(np.float16)).reshape(want.shape)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    cs0 = up16(k0)      # and back: the two sources come out of their places, the padding is zero
    assert torch.equal(torch.cat([got[:n, :k0], got[:n, cs0:cs0 + k1]], 1), w.half()) and int((got != 0).sum()) == int((w.half() != 0).sum())
    assert lib.nesr_unet_pack_linear_f16(ctypes.c_void_p(w.data_ptr()), n, k0, k1, got.numpy().ctypes.data_as(ctypes.c_void_p), got.numel() - 1) == _lib.ERR_ARG


@pytest.mark.parametrize("n,c0,c1", [(16, 6, 10), (20, 24, 8), (4, 32, 0), (32, 7, 0)])
def test_the_conv_packing_is_the_headers(n, c0, c1):
    lib = _lib.load()
    w = torch.randn((n, c0 + c1, 3, 3), generator=torch.Generator().manual_seed(n)).float().contiguous()
    want = pack_conv(w, c0, c1)
    got = np.full(want.numel(), 0x7777, np.uint16)
    assert lib.nesr_unet_pack_conv_f16(ctypes.c_void_p(w.data_ptr()), n, c0, c1, got.ctypes.data_as(ctypes.c_void_p), got.size) == 0
    assert torch.equal(torch.from_numpy(got.view(np.int16)).reshape(want.shape), want.view(torch.int16))
    w.view(-1)[5] = 1e5
    assert lib.nesr_unet_pack_conv_f16(ctypes.c_void_p(w.data_ptr()), n, c0, c1, got.ctypes.data_as(ctypes.c_void_p), got.size) == _lib.ERR_RANGE
