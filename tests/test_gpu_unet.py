"""GPU: the UNet's edges.

  workspace     it grows with the frame and is reused: a small frame after a large one gives the bits of a fresh context
  launches      kernel_time_ms()["launches"] of a forward is the same at two frame sizes and at n = 2, and is DESIGN section 19's formula
  weights       a changed weight is picked up after load_state_dict
  refusals      every configuration and argument the entries refuse raises, and the message names the field or argument
"""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from neural_enhanced_super_resolution_amd import UNet2DCondition, _lib
from neural_enhanced_super_resolution_amd.unet import KERNEL_GROUPS, _config, launches_per_forward
from tests import unet_cases as C
from tests import unet_ref as R
from tests.test_gpu_unet_cases import DEV, model

pytestmark = pytest.mark.gpu


def inputs(n, h, w, tokens, seed, cfg=C.SMALL):
    c = R.config(**cfg)
    sample, text = R.seeded_inputs(n, h, w, tokens, seed, c["in_channels"], c["cross_attention_dim"])
    return sample.to(DEV), text.to(DEV)


def create(cfg):
    """nesr_unet_create for a configuration alone: no module, so no parameters of a width the library refuses anyway."""
    return UNet2DCondition._create(SimpleNamespace(config=_config(cfg)), 0)


def test_workspace_grows_and_is_reused():
    case = C.by_name("thin")
    used, fresh = UNet2DCondition(**case.cfg).to(DEV), UNet2DCondition(**case.cfg).to(DEV)
    used.load_state_dict(case.sd)
    fresh.load_state_dict(case.sd)
    big, small = inputs(2, 22, 38, 33, 81), inputs(1, 4, 6, 5, 82)
    y_big, y_small, y_again = used(big[0], 10.5, big[1], 1).cpu(), used(small[0], 10.5, small[1], 1).cpu(), used(big[0], 10.5, big[1], 1).cpu()
    assert bool(torch.isfinite(y_big).all()) and torch.equal(y_big, y_again)
    assert torch.equal(y_small, fresh(small[0], 10.5, small[1], 1).cpu()) and torch.equal(fresh(big[0], 10.5, big[1], 1).cpu(), y_big)
    assert used.workspace_bytes(2, 22, 38, 33) > used.workspace_bytes(1, 4, 6, 5) > 0
    assert used.calls == 3


@pytest.mark.parametrize("name", ["thin", "published_layout", "seam_groups"])
def test_launch_count_is_the_formula_at_any_frame(name):
    m, case = model(name), C.by_name(name)
    div = 2 ** (len(m.config["block_out_channels"]) - 1)
    m.set_kernel_timing(True)
    counts = []
    for n, h, w, tokens in ((1, div, 2 * div, 3), (2, 3 * div, 5 * div, 40)):
        sample, text = inputs(n, h, w, tokens, 90 + n, case.cfg)
        m.kernel_time_ms()
        m(sample, 3.0, text, 2)
        t = m.kernel_time_ms()
        counts.append(t["launches"])
    m.set_kernel_timing(False)
    assert counts[0] == counts[1] == launches_per_forward(**case.cfg)
    assert tuple(t["groups"]) == KERNEL_GROUPS and all(v > 0 for v in t["groups"].values())


def test_changed_weight_is_picked_up():
    case = C.by_name("smallest")
    m = UNet2DCondition(**case.cfg).to(DEV)
    m.load_state_dict(case.sd)
    sample, text = case.sample.to(DEV), case.text.to(DEV)
    before = m(sample, case.timestep, text, case.label).cpu()
    sd = dict(case.sd)
    sd["conv_out.bias"] = sd["conv_out.bias"] + 1.0
    m.load_state_dict(sd)
    after = m(sample, case.timestep, text, case.label).cpu()
    assert float((after - before - 1.0).abs().max()) < 1e-5


@pytest.mark.parametrize("field, value, match", [
    ("down_block_types", ("AttnDownBlock2D", "CrossAttnDownBlock2D"), "down_block_types"),
    ("up_block_types", ("CrossAttnUpBlock2D", "AttnUpBlock2D"), "up_block_types"),
    ("mid_block_type", "UNetMidBlock2DSimpleCrossAttn", "mid_block_type"),
    ("use_linear_projection", False, "use_linear_projection"),
    ("transformer_layers_per_block", 2, "transformer_layers_per_block"),
    ("dual_cross_attention", True, "dual_cross_attention"),
    ("act_fn", "gelu", "act_fn"),
    ("block_out_channels", (16, 30), "norm_num_groups"),
    ("block_out_channels", (16, 2048), "block_out_channels"),
    ("attention_head_dim", 3, "attention_head_dim"),
    ("attention_head_dim", 8, "attention_head_dim"),                    # a head width of 2
    ("attention_head_dim", 1, None),                                    # widths 16 and 32 as one head: fine
    ("cross_attention_dim", 2048, "cross_attention_dim"),
    ("layers_per_block", 4, "layers_per_block"),
    ("flip_sin_to_cos", False, "flip_sin_to_cos"),
    ("freq_shift", 1, "freq_shift"),
    ("downsample_padding", 0, "downsample_padding"),
])
def test_configurations_the_kernels_do_not_take(field, value, match):
    if match is None:
        _lib.load().nesr_unet_destroy(create(dict(C.SMALL, **{field: value})))
        return
    with pytest.raises(_lib.NesrUnsupportedError, match=match):
        create(dict(C.SMALL, **{field: value}))


def test_five_levels_and_one_level_are_refused():
    for widths in ((16,), (16, 16, 16, 16, 16)):
        cfg = C.layout(widths, (True,) * len(widths), (True,) * len(widths), norm_num_groups=4, attention_head_dim=2, cross_attention_dim=40)
        with pytest.raises(_lib.NesrUnsupportedError, match="block_out_channels"):
            create(cfg)


def test_arguments_the_forward_refuses():
    m = model("thin")
    sample, text = inputs(1, 4, 6, 5, 83)
    with pytest.raises(_lib.NesrHipError, match="n is 1 or 2"):
        m(torch.zeros(3, 7, 4, 6, device=DEV), 1.0, torch.zeros(3, 5, 40, device=DEV), 0)
    with pytest.raises(_lib.NesrHipError, match="multiples of 2"):
        m(torch.zeros(1, 7, 5, 6, device=DEV), 1.0, text, 0)
    with pytest.raises(_lib.NesrHipError, match="in_channels"):
        m(torch.zeros(1, 4, 4, 6, device=DEV), 1.0, text, 0)
    with pytest.raises(_lib.NesrHipError, match="tokens must be 1 .. 256"):
        m(sample, 1.0, torch.zeros(1, 257, 40, device=DEV), 0)
    with pytest.raises(_lib.NesrHipError, match="class_label"):
        m(sample, 1.0, text, 10)
    with pytest.raises(_lib.NesrHipError, match="class_label"):
        m(sample, 1.0, text, -1)
    with pytest.raises(_lib.NesrHipError, match="self-attention of level 1"):
        m.workspace_bytes(1, 516, 516, 5)
    with pytest.raises(ValueError, match="encoder_hidden_states"):
        m(sample, 1.0, torch.zeros(1, 5, 41, device=DEV), 0)
    with pytest.raises(ValueError, match="float32"):
        m(sample.double(), 1.0, text, 0)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        m(sample.cpu(), 1.0, text, 0)
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()
    lib, h = _lib.load(), m._context(torch.device(DEV))
    out = torch.full((4 * 4 * 6 + 1,), -7.0, device=DEV)
    for elems in (4 * 4 * 6 - 1, 4 * 4 * 6 + 1):
        assert lib.nesr_unet_forward_f32(h, ctypes.c_void_p(sample.data_ptr()), 1, 7, 4, 6, 1.0, 0, ctypes.c_void_p(text.data_ptr()), 5,
                                         ctypes.c_void_p(out.data_ptr()), elems, None) == _lib.ERR_ARG
        assert "out_elems" in lib.nesr_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())      # refused before any launch
