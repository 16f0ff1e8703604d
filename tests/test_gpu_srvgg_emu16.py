"""GPU: whole SRVGGNetCompact networks in bf16 and fp16 against their exact 16-bit specification on the CPU
(tests/srvgg_fp16_emu.py, store = bfloat16 | float16), judged by rrdbnet_emu16.conditions as RRDBNet's are
(test_gpu_rrdb_emu16.py), with band_px the upscale: one feature pixel.

No measured constant is asserted: with emu64 the specification, emu32 the same with torch's f32 conv and `exact` the float64
network, all computed here on the same input,
  (a)  mean |kernel - emu64| < mean |emu64 - exact|
  (b)  max |kernel - emu64| <= 4 max |emu32 - emu64|
  (b') per band of rows / columns one feature pixel wide: mean |kernel - emu64| <= 4 mean over the image |emu32 - emu64|
  (b") over the image: mean |kernel - emu64| <= 4 mean |emu32 - emu64|
Which of them is asserted on a network is srvgg_pin.asserted's rule, computed from the kernel-order stand-in on the CPU
(test_srvgg_pin_host.py): (b) and (b") everywhere, (b') at num_conv >= 16, (a) up to num_conv 16; every ratio is printed.
test_srvgg_pin_host.py plays wrong kernels against them: a lost halo row or column in one of 16 layers breaks (b) and (b')
twentyfold while the image-wide mean moves little.  The measured ratios are in DESIGN.md section 8, "The 16-bit
specification of SRVGGNetCompact"."""
import pytest
import torch

from neural_enhanced_super_resolution_amd import SRVGGNetCompact
from tests import srvgg_pin
from tests.rrdbnet_emu16 import describe

pytestmark = pytest.mark.gpu

FORM = {"bf16": "bf16", "f16": "fp16"}


@pytest.mark.parametrize("dtype", list(FORM))
@pytest.mark.parametrize("name", list(srvgg_pin.NETWORKS))
def test_network_against_its_16_bit_specification(cuda_device, name, dtype):
    cfg = srvgg_pin.NETWORKS[name]
    spec = srvgg_pin.network_spec(name, dtype)
    rule = srvgg_pin.asserted(name)
    net = SRVGGNetCompact(**cfg, compute_dtype=FORM[dtype]).to(cuda_device)
    net.load_state_dict(spec["sd"])
    got = net(spec["x"].to(cuda_device)).cpu()
    net.check_status()
    assert got.shape == spec["emu64"].shape and bool(torch.isfinite(got).all())
    fig = srvgg_pin.judge(got, spec, cfg["upscale"])
    print(f"emu16 {name} {dtype}: {describe(fig)} | (a) ratio {fig['mean_to_spec'] / fig['spec_to_exact']:.3f} | asserted {sorted(rule)}")
    for c in sorted(rule):
        assert fig[c], f"{c}: {describe(fig)}"
