"""GPU: the UNet's fp16 compute form, whole network (``UNet2DCondition(compute_dtype="fp16")``).

Every case of tests/unet_cases.py (as tests/unet_f16_emu.py's network_case hands it on) must satisfy
max |gpu - f64| <= max |emu64 - f64| + 8 max |emu32 - emu64|: DESIGN section 17's bound, not a pin.  A repeated forward gives the same
bits, a sample alone gives the bits it gives as one of two, the launch count is the f32 form's, an activation beyond 65504 raises
NesrRangeError and leaves the context clean, and the default form still gives the bits and the launch count recorded on the
commit before this form existed.
"""
import hashlib

import pytest
import torch

from neural_enhanced_super_resolution_amd import UNet2DCondition, _lib
from neural_enhanced_super_resolution_amd.unet import launches_per_forward
from tests import unet_cases as C
from tests import unet_f16_emu as E
from tests.test_gpu_unet_cases import DEV, guarded_forward

pytestmark = pytest.mark.gpu
_cache = {}

# recorded on the parent commit (the f32 form before this one existed): sha256 of the output's float32 bytes, launches of a forward
PARENT_F32 = {"published_layout": ("cca8abf50e85eb31607e023232125c9dc102b4777824a59d618ff169233edf2c", 438),
              "seam_groups": ("4099614ae5c257d6085c02407a1d38401addd85c4e608d159e3451dd193fd6ad", 134),
              "batch_two": ("d17fa24985b484fe00274ad541851cee05be7454031b6583d8dca8ba34f81cfb", 182)}


def model(name, compute_dtype="fp16", case=None):
    key = (name, compute_dtype, case is not None)
    if key not in _cache:
        case = case or E.network_case(name)
        m = UNet2DCondition(compute_dtype=compute_dtype, **case.cfg).to(DEV)
        m.load_state_dict(case.sd)
        _cache[key] = m
    return _cache[key]


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_within_the_forms_own_bound(name):
    m, case = model(name), E.network_case(name)
    y64, e64, bound = E.network_reference(name)
    got = guarded_forward(m, case.sample, case.timestep, case.text, case.label)
    assert got.shape == y64.shape and bool(torch.isfinite(got).all())
    err, own = float((got.double() - y64).abs().max()), float((got.double() - e64).abs().max())
    print(f"{name}: {tuple(y64.shape)}, err {err:.3e}, bound {bound:.3e}, err / bound {err / bound:.3f}, |gpu - emu64| {own:.3e}")
    assert err <= bound
    again = m(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label)
    assert again.is_cuda and again.dtype == torch.float32 and torch.equal(again.cpu(), got)      # a repeated forward: the same bits


def test_a_sample_does_not_depend_on_its_batch():
    m, case = model("batch_two"), E.network_case("batch_two")
    both = m(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label).cpu()
    for i in range(2):
        alone = m(case.sample[i:i + 1].to(DEV), case.timestep, case.text[i:i + 1].to(DEV), case.label).cpu()
        assert torch.equal(alone[0], both[i]), f"sample {i} alone differs from sample {i} of two"
    assert not torch.equal(both[0], both[1])


@pytest.mark.parametrize("name", ["published_layout", "batch_two"])
def test_the_launch_count_is_the_f32_forms(name):
    m, case = model(name), E.network_case(name)
    m.set_kernel_timing(True)
    try:
        m.kernel_time_ms()
        m(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label)
        t = m.kernel_time_ms()
    finally:
        m.set_kernel_timing(False)
    assert t["launches"] == launches_per_forward(**case.cfg) == PARENT_F32[name][1]


def test_the_form_is_not_the_f32_form_and_holds_fewer_bytes():
    case = E.network_case("seam_groups")
    f16, f32 = model("seam_groups"), model("seam_groups", "f32")
    a = f16(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label)
    b = f32(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label)
    assert not torch.equal(a, b) and float((a - b).abs().max()) < 0.1
    assert f16.weight_bytes(DEV) < 0.75 * f32.weight_bytes(DEV)


def test_an_activation_beyond_f16_raises_and_the_next_forward_is_clean():
    m, case = model("batch_two"), E.network_case("batch_two")
    good = m(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label).cpu()
    with pytest.raises(_lib.NesrRangeError, match="65504"):
        m(torch.full_like(case.sample, 1e5).to(DEV), case.timestep, case.text.to(DEV), case.label)
    with pytest.raises(_lib.NesrRangeError):
        m(case.sample.to(DEV), case.timestep, torch.full_like(case.text, float("nan")).to(DEV), case.label)
    assert torch.equal(m(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label).cpu(), good)
    f32 = model("batch_two", "f32")
    out = f32(torch.full_like(case.sample, 1e5).to(DEV), case.timestep, case.text.to(DEV), case.label)      # the f32 form neither checks nor raises
    assert out.shape == good.shape


@pytest.mark.parametrize("name", sorted(PARENT_F32))
def test_the_default_form_is_untouched(name):
    case = C.by_name(name)      # the case as it is, not network_case
    m = model(name, "f32", case)
    assert m.compute_dtype == "f32" and UNet2DCondition(**case.cfg).compute_dtype == "f32"
    m.set_kernel_timing(True)
    try:
        m.kernel_time_ms()
        y = m(case.sample.to(DEV), case.timestep, case.text.to(DEV), case.label).cpu()
        t = m.kernel_time_ms()
    finally:
        m.set_kernel_timing(False)
    sha, launches = PARENT_F32[name]
    assert hashlib.sha256(y.contiguous().numpy().tobytes()).hexdigest() == sha
    assert t["launches"] == launches
