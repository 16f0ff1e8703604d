"""GPU: conv3x3(nearest_x2(x)) of the f16-pair form as four 2x2-tap convs on the low-res input (upconv2x2_f16x2.hip), through
the single-layer entry nesr_conv3x3_up and through a whole RRDBNet.

Not covered here because not built: a bf16 / f16 form of the kernel (those compute forms keep the 3x3 path, and so do their
ragged tile batches -- nesr_forward_ragged exists for bf16 / f16 only).  conv_last: tests/test_gpu_conv_last_narrow.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SPLIT_TOL = 2e-5   # relative to max(1, |ref|max): the tolerance of the upsampled f32-split case of the per-layer parity tests


def _case(cin, cout, h, w, seed, n=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wgt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x, wgt, b


def _ref(x, wgt, b, lrelu):
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wgt, b, padding=1)
    return F.leaky_relu(y, 0.2) if lrelu else y


# low-res sizes; the kernel's tile is 4 rows x 32 columns of low-res pixels
SIZES = [(13, 21), (1, 1), (4, 32), (5, 32), (4, 33), (5, 33), (3, 70), (256, 256), (512, 512)]


@pytest.mark.parametrize("h,w", SIZES)
def test_upconv_2x2_matches_torch(cuda_device, h, w):
    from neural_enhanced_super_resolution_amd import conv3x3
    x, wgt, b = _case(64, 64, h, w, seed=h * 1000 + w)
    ref = _ref(x, wgt, b, True)
    got = conv3x3(x.to(cuda_device), wgt, b, lrelu=True, upsample=True, dtype="f32-split", upconv="2x2").cpu()
    assert got.shape == ref.shape
    err = (got - ref).abs().max().item()
    print(f"upconv 2x2 {h}x{w}: max abs err {err:.3e} (|ref|max {ref.abs().max().item():.3f})")
    assert err < SPLIT_TOL * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("cin,cout,n,h,w,lrelu", [(64, 64, 3, 13, 21, True), (64, 32, 2, 9, 35, False), (16, 64, 3, 6, 40, True),
                                                  (48, 3, 2, 7, 9, False)])
def test_upconv_2x2_batches_and_channel_counts(cuda_device, cin, cout, n, h, w, lrelu):
    from neural_enhanced_super_resolution_amd import conv3x3
    x, wgt, b = _case(cin, cout, h, w, seed=cin + cout + n, n=n)
    ref = _ref(x, wgt, b, lrelu)
    got = conv3x3(x.to(cuda_device), wgt, b, lrelu=lrelu, upsample=True, dtype="f32-split", upconv="2x2").cpu()
    err = (got - ref).abs().max().item()
    print(f"upconv 2x2 n={n} {cin}->{cout} {h}x{w}: max abs err {err:.3e}")
    assert err < SPLIT_TOL * max(1.0, ref.abs().max().item())


def test_upconv_default_is_2x2_and_3x3_stays_reachable(cuda_device):
    """The 3x3 form is still there and differs from the 2x2 form only in rounding; the default entry takes the 2x2 form."""
    import os
    from neural_enhanced_super_resolution_amd import conv3x3, last_conv_kernel
    x, wgt, b = _case(64, 64, 13, 21, seed=5)
    ref = _ref(x, wgt, b, True)
    xd = x.to(cuda_device)
    y3 = conv3x3(xd, wgt, b, lrelu=True, upsample=True, dtype="f32-split", upconv="3x3").cpu()
    assert last_conv_kernel() == "f16-pair"
    y2 = conv3x3(xd, wgt, b, lrelu=True, upsample=True, dtype="f32-split", upconv="2x2").cpu()
    assert last_conv_kernel() == "upconv2x2"
    yd = conv3x3(xd, wgt, b, lrelu=True, upsample=True, dtype="f32-split").cpu()
    tol = SPLIT_TOL * max(1.0, ref.abs().max().item())
    assert (y3 - ref).abs().max().item() < tol and (y2 - ref).abs().max().item() < tol
    assert torch.equal(yd, y3 if os.environ.get("NESR_UPCONV") == "3x3" else y2)
    # forms without a folded kernel ignore the switch
    for dt in ("bf16", "f32-direct"):
        a = conv3x3(xd, wgt, b, upsample=True, dtype=dt, upconv="2x2").cpu()
        c = conv3x3(xd, wgt, b, upsample=True, dtype=dt, upconv="3x3").cpu()
        assert last_conv_kernel() == "generic"
        assert torch.equal(a, c)


def test_upconv_2x2_one_hot_small_integers_bit_equal_to_3x3(cuda_device):
    """Small integers: every product and every sum is exact in every plane of the pair, folded or not, so the two forms and
    torch agree bit for bit; catches swapped parities, taps, rows / columns and channel permutations."""
    from neural_enhanced_super_resolution_amd import conv3x3
    cin, cout = 32, 64
    for (h, w) in [(6, 7), (5, 37)]:
        x = ((torch.arange(cin * h * w, dtype=torch.float32).reshape(1, cin, h, w) * 7) % 61).contiguous()
        for tap in range(9):
            wt = torch.zeros(cout, cin, 3, 3)
            for o in range(cout):
                wt[o, (o * 5 + tap) % cin, tap // 3, tap % 3] = 1.0
            b = torch.arange(cout, dtype=torch.float32)
            ref = _ref(x, wt, b, False)
            y2 = conv3x3(x.to(cuda_device), wt, b, upsample=True, dtype="f32-split", upconv="2x2").cpu()
            y3 = conv3x3(x.to(cuda_device), wt, b, upsample=True, dtype="f32-split", upconv="3x3").cpu()
            assert torch.equal(y2, y3), f"tap {tap} {h}x{w}"
            assert torch.equal(y2, ref), f"tap {tap} {h}x{w}"
    # all nine taps at once, small integer weights: the folded sums are exact
    g = torch.Generator().manual_seed(2)
    wt = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).to(torch.float32)
    x = torch.randint(-4, 5, (2, cin, 9, 34), generator=g).to(torch.float32)
    b = torch.arange(cout, dtype=torch.float32)
    y2 = conv3x3(x.to(cuda_device), wt, b, upsample=True, dtype="f32-split", upconv="2x2").cpu()
    y3 = conv3x3(x.to(cuda_device), wt, b, upsample=True, dtype="f32-split", upconv="3x3").cpu()
    assert torch.equal(y2, y3) and torch.equal(y2, _ref(x, wt, b, False))


def test_upconv_2x2_raises_the_range_flag(cuda_device):
    from neural_enhanced_super_resolution_amd import conv3x3
    from neural_enhanced_super_resolution_amd._lib import NesrRangeError
    x, wgt, b = _case(64, 64, 9, 11, seed=1)
    big = x.clone()
    big[0, 3, 4, 5] = 3.0e38       # finite in f32, does not fit the pair; the pack kernel and the conv both flag it
    with pytest.raises(NesrRangeError):
        conv3x3(big.to(cuda_device), wgt, b, upsample=True, dtype="f32-split", upconv="2x2")
    # an OUTPUT beyond the range: inputs and weights fit, the sum does not
    xs = torch.full((1, 64, 5, 6), 60000.0)
    ws = torch.full((64, 64, 3, 3), 1.0)
    with pytest.raises(NesrRangeError):
        conv3x3(xs.to(cuda_device), ws, torch.zeros(64), upsample=True, dtype="f32-split", upconv="2x2")
    # folded taps that do not fit are refused like single taps that do not fit
    wb = torch.full((64, 64, 3, 3), 30000.0)
    with pytest.raises(NesrRangeError):
        conv3x3(x.to(cuda_device), wb, b, upsample=True, dtype="f32-split", upconv="2x2")


@pytest.mark.parametrize("scale,hw", [(2, (48, 64)), (2, (38, 54)), (4, (21, 33))])
def test_model_2x2_against_3x3_and_oracle(cuda_device, scale, hw):
    """Whole network: the setter switches the form, both forms meet the oracle, and they differ by rounding only."""
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    from oracle.rrdbnet_ref import RRDBNetRef
    nb = 2
    sd = synthetic_state_dict(seed=4, num_in_ch=3, scale=scale, num_block=nb)
    net = RRDBNet(3, 3, scale=scale, num_block=nb)
    net.load_state_dict(sd)
    net = net.to(cuda_device)
    ref_net = RRDBNetRef(3, 3, scale=scale, num_block=nb)
    ref_net.load_state_dict(sd)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, hw[0], hw[1], generator=g)
    with torch.no_grad():
        ref = ref_net(x)
        y2 = net(x.to(cuda_device)).cpu()
        assert net.upconv_state() == "2x2"
        net.set_upconv("3x3")
        assert net.upconv_state() == "3x3"
        y3 = net(x.to(cuda_device)).cpu()
        net.set_upconv("2x2")
        y2b = net(x.to(cuda_device)).cpu()
    assert torch.equal(y2, y2b)
    e2, e3, d = (y2 - ref).abs().max().item(), (y3 - ref).abs().max().item(), (y2 - y3).abs().max().item()
    print(f"x{scale} {hw}: 2x2 vs oracle {e2:.3e}, 3x3 vs oracle {e3:.3e}, 2x2 vs 3x3 {d:.3e}")
    assert e2 < 5e-5 and e3 < 5e-5      # the bound of the C2 oracle test
    # the setter reaches the launches of a forward: the folded sums round differently from nine separate products, so the two
    # forms cannot agree in every bit of ~1e5 outputs, and they differ by a few ulps of the O(1) output at most
    assert 0.0 < d <= 1e-5
    assert np.isfinite(y2.numpy()).all()
