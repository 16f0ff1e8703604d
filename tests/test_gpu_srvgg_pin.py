"""GPU: every layer kind of SRVGGNetCompact's bf16 and fp16 kernels (srvgg_compact.hip: the 16 x 32 tile, the layer's weights
resident in LDS across a persistent tile walk, the 16-bit staging and store) pinned per value to the rounded float64 value --
what test_gpu_conv.py does for RRDBNet's single layers.  A compact context has no single-layer entry, so a layer is isolated
through the ordinary forward of SRVGGNetCompact(num_conv=1) with crafted weights: tests/srvgg_pin.py has the construction and
the criterion, test_srvgg_pin_host.py shows on the CPU that the construction loses nothing, that a serial f32 sum in the
kernel's order meets the pins 100 times inside the miss cap, and which wrong kernel fails which pin.

  feature   body.2 (64 -> 64, CIN = 64): every value within one 16-bit ulp of ref16, at most conv_pin.MISS_CAP not its bits
  first     body.0 (3 -> 64, CIN = 32): the same; the conv reads the rounded image, the residual adds the unrounded one
  tail      body.4 (64 -> 3 s^2, shuffle, residual, float32): every value within f32 accumulation's bound of the float64 conv
Shapes: 1 x 1, 3 x 5, one tile exactly, one row and column more, one less, 37 x 53; x2 (NCB = 1, 12 of 16 tail channels
live) on three of them; and the feature layer on 1 x 264 x 528, where every workgroup walks several tiles on resident
weights.  The measured figures are in DESIGN.md section 8, "The 16-bit specification of SRVGGNetCompact"."""
import pytest
import torch

from neural_enhanced_super_resolution_amd import SRVGGNetCompact
from tests import conv_pin, srvgg_pin

pytestmark = pytest.mark.gpu

FORM = {"bf16": "bf16", "f16": "fp16"}          # conv_pin's name of the storage type -> compute_dtype
CASES = [(4, sh) for sh in srvgg_pin.SHAPES] + [(2, sh) for sh in srvgg_pin.SHAPES_X2]
_models = {}
pool = conv_pin.MissPool()


def runner(s, dtype):
    """run(state_dict, x) of one live model per (upscale, form): load_state_dict re-finalises the weights."""
    if (s, dtype) not in _models:
        _models[(s, dtype)] = SRVGGNetCompact(num_conv=1, upscale=s, act_type="prelu", compute_dtype=FORM[dtype]).to("cuda:0")
    model = _models[(s, dtype)]

    def run(sd, x):
        model.load_state_dict(sd)
        y = model(x.to("cuda:0")).cpu()
        model.check_status()
        return y
    return run


@pytest.mark.parametrize("dtype", list(FORM))
@pytest.mark.parametrize("s,shape", CASES, ids=[f"x{s}-{'x'.join(map(str, sh))}" for s, sh in CASES])
@pytest.mark.parametrize("kind", list(srvgg_pin.CASES))
def test_layer_is_the_rounded_float64_value(cuda_device, kind, s, shape, dtype):
    fig = srvgg_pin.CASES[kind](runner(s, dtype), s, dtype, shape)
    print(f"pin {kind} x{s} {shape} {dtype}: {srvgg_pin.describe(fig)}")
    conv_pin.assert_pin(fig, dtype, f"{kind} x{s} {shape}")
    if kind != "tail":
        pool.add(dtype, fig)
        pool.check()


@pytest.mark.parametrize("dtype", list(FORM))
def test_feature_layer_on_resident_weights_over_many_tiles(cuda_device, dtype):
    """289 tiles, more than the device has compute units: the second and later tiles of a workgroup, on the weights it
    staged once, are pinned per value."""
    n, h, w = srvgg_pin.MANY_TILES
    assert n * -(-h // 16) * -(-w // 32) > torch.cuda.get_device_properties(0).multi_processor_count
    fig = srvgg_pin.feature_case(runner(4, dtype), 4, dtype, (n, h, w), seed=20)
    print(f"pin feature x4 {(n, h, w)} {dtype}: {srvgg_pin.describe(fig)}")
    conv_pin.assert_pin(fig, dtype, f"feature x4 {(n, h, w)}")
