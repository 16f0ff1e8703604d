"""GPU: conv_last of the f32 (f16-pair) form in its narrow geometry (one 16-channel MFMA column block per workgroup,
conv3x3_f16x2_kernel<DMAW, 1>) is BIT-EQUAL to the general geometry, in both output modes: planar f32 NCHW (forward) and
clamped + quantised u8 HWC with flip / round_mode (forward_u8), 3 output channels.

conv_last runs only inside a forward, at the network's output size.  Shapes of conv_last here: 1024x1024 (x2 model on a
512x512 frame, the c2 shape), 148x212 (x4 model on a 37x53 frame: the trunk, and with it every tile row and column count, is
odd) and 100x140 (x2 model on 50x70: partial tiles in both directions), plus a batch of 3."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(2, 512, 512, 1), (4, 37, 53, 1), (2, 50, 70, 1), (2, 26, 38, 3)]


def _net(scale, cuda_device):
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    net = RRDBNet(3, 3, scale=scale, num_block=1)
    net.load_state_dict(synthetic_state_dict(seed=7, num_in_ch=3, scale=scale, num_block=1))
    return net.to(cuda_device)


@pytest.mark.parametrize("scale,h,w,n", CASES)
def test_narrow_conv_last_is_bit_equal_planar_f32(cuda_device, scale, h, w, n):
    net = _net(scale, cuda_device)
    x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(h + w)).to(cuda_device)
    with torch.no_grad():
        y_default = net(x).clone()
        net.set_conv_last("general")
        y_general = net(x).clone()
        net.set_conv_last("narrow")
        y_narrow = net(x).clone()
    net.check_status()
    assert y_general.shape == (n, 3, h * scale, w * scale)
    assert torch.isfinite(y_general).all() and y_general.abs().max().item() > 0
    assert torch.equal(y_narrow, y_general)
    assert torch.equal(y_default, y_narrow)        # narrow is the default


@pytest.mark.parametrize("scale,h,w,n", CASES[:3])
@pytest.mark.parametrize("flip,round_nearest", [(True, True), (False, False), (True, False)])
def test_narrow_conv_last_is_bit_equal_u8(cuda_device, scale, h, w, n, flip, round_nearest):
    net = _net(scale, cuda_device)
    img = torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(h * w), dtype=torch.uint8).to(cuda_device)
    with torch.no_grad():
        net.forward_u8(img, flip_rgb=flip, round_nearest=round_nearest)      # creates the context
        net.set_conv_last("general")
        y_general = net.forward_u8(img, flip_rgb=flip, round_nearest=round_nearest).clone()
        net.set_conv_last("narrow")
        y_narrow = net.forward_u8(img, flip_rgb=flip, round_nearest=round_nearest).clone()
    net.check_status()
    assert y_general.shape == (h * scale, w * scale, 3) and y_general.dtype == torch.uint8
    assert int(y_general.max()) > int(y_general.min())       # a real image, not a constant
    assert torch.equal(y_narrow, y_general)


def test_narrow_conv_last_writes_nan_after_a_range_failure(cuda_device):
    """The poisoned image (sticky range word) is the same in both geometries: NaN everywhere, NESR_ERR_RANGE at the check."""
    from neural_enhanced_super_resolution_amd._lib import NesrRangeError
    net = _net(2, cuda_device)
    x = torch.rand(1, 3, 24, 40).to(cuda_device)
    with torch.no_grad():
        net(x)
        net.check_status()
        bad = x.clone()
        bad[0, 1, 5, 7] = float("inf")
        for mode in ("general", "narrow"):
            net.set_conv_last(mode)
            got = []
            with pytest.raises(NesrRangeError):
                got.append(net(bad))
                net.check_status()
            if got:      # the forward itself did not raise: its image must be poisoned, not saturated
                assert torch.isnan(got[0]).all(), mode
