"""The contexts of a model on the device (ContextPool through RRDBNet / SRVGGNetCompact): a replica, a re-created replica and a
context on another device run with the switches the model was given, whenever it was given them.

RRDBNet(scale=2, one block, "f32") on [1, 3, 16, 64]: the trunk image is 8 x 32, exactly one tile of the fused dense-block
kernel, the smallest shape that still takes it."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sd():
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    return synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=1)


def _net(device):
    from neural_enhanced_super_resolution_amd import RRDBNet
    net = RRDBNet(3, 3, scale=2, num_block=1, compute_dtype="f32")
    net.load_state_dict(_sd(), strict=True)
    return net.eval().to(device)


@pytest.fixture(scope="module")
def x(cuda_device):
    g = torch.Generator().manual_seed(7)
    return torch.rand((1, 3, 16, 64), generator=g).to(cuda_device)


def _switched(net, slot, device=None):
    assert net.upconv_state(slot=slot, device=device) == "3x3"
    assert net.fused_state(slot=slot, device=device)[0] is False


def test_switches_set_after_slot_0_exists(cuda_device, x):
    net = _net(cuda_device)
    net(x)
    net.set_upconv("3x3")
    net.set_fused(False)
    y0 = net(x, slot=0)
    y1 = net(x, slot=1)
    net.check_status()
    assert torch.equal(y0, y1)
    _switched(net, 0)
    _switched(net, 1)
    if torch.cuda.device_count() >= 2:
        y_other = net(x.to("cuda:1"))
        net(x.to("cuda:1"), slot=1)
        net.check_status()
        _switched(net, 0, device="cuda:1")
        _switched(net, 1, device="cuda:1")
        assert torch.equal(y_other.to(cuda_device), y0)


def test_switches_set_before_any_forward(cuda_device, x):
    net = _net(cuda_device)
    net.set_upconv("3x3")
    net.set_fused(False)
    assert net.upconv_state() is None and net.upconv_state(slot=1) is None
    y0 = net(x, slot=0)
    y1 = net(x, slot=1)
    net.check_status()
    assert torch.equal(y0, y1)
    _switched(net, 0)
    _switched(net, 1)


def test_reupload_recreates_the_replica_with_its_switches(cuda_device, x):
    net = _net(cuda_device)
    net.set_upconv("3x3")
    net.set_fused(False)
    y0 = net(x, slot=0)
    y1 = net(x, slot=1)
    h0, h1 = net._handle(0, 0), net._handle(0, 1)
    net.load_state_dict(_sd(), strict=True)
    z0 = net(x, slot=0)
    assert net._handle(0, 0) is h0 and net._handle(0, 1) is None      # slot 0 uploaded in place, the replica gone until asked for
    z1 = net(x, slot=1)
    net.check_status()
    assert net._handle(0, 1) is not None and net._handle(0, 1) is not h1
    _switched(net, 0)
    _switched(net, 1)
    assert torch.equal(z0, y0) and torch.equal(z1, y1) and torch.equal(z0, z1)


def test_compact_replica(cuda_device):
    from neural_enhanced_super_resolution_amd import SRVGGNetCompact
    from neural_enhanced_super_resolution_amd.synth import synthetic_compact_state_dict
    net = SRVGGNetCompact(num_conv=2, upscale=2)
    net.load_state_dict(synthetic_compact_state_dict(seed=0, num_conv=2, upscale=2), strict=True)
    net.eval().to(cuda_device)
    g = torch.Generator().manual_seed(8)
    xc = torch.rand((1, 3, 8, 32), generator=g).to(cuda_device)
    y0 = net(xc, slot=0)
    y1 = net(xc, slot=1)
    net.check_range(1)
    net.check_status()
    assert y0.shape == (1, 3, 16, 64) and torch.equal(y0, y1)
