"""GPU: the f16 compute form (RRDBNet(compute_dtype="f16"), NESR_DTYPE_F16): the bf16 kernels instantiated on
v_mfma_f32_{32x32x16,16x16x32}_f16 with f16 storage, f32 accumulation and epilogue -- upstream's half=True numerics.

  one layer     conv3x3(dtype="f16") on operands already rounded with torch's .half() against the float64 conv of the same
                operands, rounded once to f16 (the hook's output passes through f16 storage): within one f16 ulp everywhere
                and bitwise equal to it almost everywhere -- which pins the MFMA type (a bf16 leak is 8x off) and the
                rounding of the stores (round toward zero would miss on about half the values)
  whole network x2plus / x4plus against the f32 oracle: f16 must be far closer than bf16 on the same input
  strip kernel  the LDS-resident dense block in f16 against the per-layer f16 path on the edge shapes of test_gpu_strip.py
  range         f16 carries |x| <= 65504: weights beyond are refused, activations beyond give NaN + NesrRangeError
  wrapper       RealESRGANer(half=True) with an f16 model on a 2160p frame: the serial tile loop, bit for bit"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# Whole-network floors, measured on MI355X with seeded synthetic weights and torch.rand inputs ("The f16 compute form"):
# {(scale, num_block): (f16 PSNR dB, f16 max abs)} as measured; the asserted floor is 2 dB below the PSNR, the ceiling 2x the max abs.
F16_NET = {
    (2, 2): (98.27, 5.81e-5),      # bf16 on the same input: 80.23 dB, 4.46e-4
    (2, 23): (65.11, 3.35e-3),     #                          47.11 dB, 2.58e-2
    (4, 2): (96.92, 8.85e-5),      #                          77.57 dB, 7.45e-4
    (4, 23): (61.87, 4.91e-3),     #                          44.04 dB, 3.89e-2
}


def _psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10 * math.log10(1.0 / max(mse, 1e-30))


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _model(sd, scale, num_block, dtype="f16", strip=None, size_independent=False):
    """An RRDBNet whose device context is created now (NESR_STRIP is read then)."""
    from neural_enhanced_super_resolution_amd import RRDBNet

    def make():
        net = RRDBNet(3, 3, scale=scale, num_block=num_block, compute_dtype=dtype)
        net.load_state_dict(sd)
        net.eval().to("cuda:0")
        net.size_independent = size_independent
        u = {2: 2, 1: 4}.get(scale, 1)
        net(torch.zeros(1, 3, 4 * u, 4 * u, device="cuda:0"))
        net.check_status()
        return net
    return _with_env({"NESR_STRIP": strip}, make) if strip is not None else make()


def _oracle(sd, scale, num_block):
    from oracle.rrdbnet_ref import RRDBNetRef
    ref = RRDBNetRef(3, 3, scale=scale, num_block=num_block)
    ref.load_state_dict(sd, strict=True)
    return ref


# ------------------------------------------------------------------------------------------------------------ one layer
def _ulp16(v):
    """Spacing of f16 at |v| (v float64, already an f16 value); the subnormal spacing below 2^-14."""
    a = v.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


@pytest.mark.parametrize("cin,cout,hw", [(3, 32, (19, 37)), (12, 32, (19, 37)), (64, 64, (19, 37)), (160, 64, (19, 37)),
                                         (64, 32, (264, 264)), (160, 64, (264, 264))])       # 264 x 264: the large-tile kernel
@pytest.mark.parametrize("lrelu,up", [(False, False), (True, False), (True, True)])
def test_one_layer_rounding_pin(cuda_device, cin, cout, hw, lrelu, up):
    from neural_enhanced_super_resolution_amd import conv3x3
    if up and hw[0] > 100:
        hw = (hw[0] // 2, hw[1] // 2)      # the output is 2x: still the large-tile kernel
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn(2, cin, hw[0], hw[1], generator=g).half().float()
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / math.sqrt(9 * cin))).half().float()
    b = torch.randn(cout, generator=g) * 0.1
    y = conv3x3(x.to(cuda_device), w, b, lrelu=lrelu, upsample=up, dtype="f16").cpu().double()
    xd = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up else x.double()
    ref = F.conv2d(xd, w.double(), b.double(), padding=1)
    mag = F.conv2d(xd.abs(), w.double().abs(), b.double().abs(), padding=1)      # sum of |products|: what f32 accumulation errs against
    if lrelu:
        ref = F.leaky_relu(ref, 0.2)
    ref16 = ref.half().double()                       # the f64 value rounded once to f16, ties to even
    k = 9 * cin
    # Near zero, where the f32 sums of K products cancel, one f16 ulp is smaller than what f32 accumulation may be off by: there
    # the bound is absolute, K * 2^-24 of the sum of |products| (plus the f16 rounding of the store)
    ulp = _ulp16(ref16)
    e_acc = k * 2.0 ** -24 * mag
    diff = (y - ref16).abs()
    within = (diff <= ulp) | ((ulp < e_acc) & ((y - ref).abs() <= e_acc + ulp))
    assert within.all(), f"{int((~within).sum())} values more than one f16 ulp off, worst {float(diff.max()):.3e}"
    miss = float((diff > 0).double().mean())
    print(f"cin {cin} cout {cout} {tuple(hw)} lrelu {lrelu} up {up}: not bitwise the rounded f64 value: {miss:.2e}")
    # a correctly rounded store misses only where the f32 sum and the f64 value straddle a rounding boundary (a few % of the
    # values, most of them near zero); a store that rounds toward zero misses about half of them, a bf16 operand nearly all
    assert miss < 0.05, miss
    assert torch.isfinite(y).all()


def test_one_layer_f16_is_not_bf16(cuda_device):
    """The same layer through the bf16 hook is off by far more than one f16 ulp: the pin above can tell the two apart."""
    from neural_enhanced_super_resolution_amd import conv3x3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 64, 19, 37, generator=g).half().float()
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24.0).half().float()
    b = torch.zeros(64)
    ref16 = F.conv2d(x.double(), w.double(), b.double(), padding=1).half().double()
    e16 = (conv3x3(x.to(cuda_device), w, b, dtype="f16").cpu().double() - ref16).abs()
    ebf = (conv3x3(x.to(cuda_device), w, b, dtype="bf16").cpu().double() - ref16).abs()
    assert float(ebf.max()) > 4 * float(e16.max()), (float(ebf.max()), float(e16.max()))
    assert float((ebf > _ulp16(ref16)).double().mean()) > 0.3


# ------------------------------------------------------------------------------------------------------------ whole network
_NET_CACHE = {}


def _whole(scale, num_block):
    key = (scale, num_block)
    if key not in _NET_CACHE:
        from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
        sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=scale, num_block=num_block)
        x = torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(scale * 100 + num_block))
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        with torch.no_grad():
            want = _oracle(sd, scale, num_block)(x)
        out = {}
        for dt in ("f16", "bf16"):
            net = _model(sd, scale, num_block, dtype=dt)
            out[dt] = net(x.to("cuda:0")).cpu()
            net.check_status()
            del net
        _NET_CACHE[key] = (want, out)
    return _NET_CACHE[key]


@pytest.mark.parametrize("scale,num_block", [(2, 2), (2, 23), (4, 2), (4, 23)])
def test_whole_network_f16_against_f32_oracle(cuda_device, scale, num_block):
    want, out = _whole(scale, num_block)
    e16 = (out["f16"] - want).abs().max().item()
    ebf = (out["bf16"] - want).abs().max().item()
    p16, pbf = _psnr(out["f16"], want), _psnr(out["bf16"], want)
    print(f"x{scale}plus num_block {num_block} 512x512: f16 PSNR {p16:.2f} dB max abs {e16:.3e} | bf16 PSNR {pbf:.2f} dB max abs {ebf:.3e}")
    assert torch.isfinite(out["f16"]).all()
    assert e16 <= ebf / 4, (e16, ebf)
    assert p16 >= pbf + 12.0, (p16, pbf)
    floor_psnr, meas_max = F16_NET[(scale, num_block)]
    assert p16 >= floor_psnr - 2.0, p16
    assert e16 <= 2 * meas_max, e16


# ------------------------------------------------------------------------------------------------------------ strip kernel
NB = 2
SHAPES_X2 = [(2, 2), (8, 30), (22, 32), (24, 34), (26, 64), (46, 66), (48, 96), (50, 98), (200, 20), (20, 200), (130, 198)]
SHAPES_X4 = [(1, 1), (5, 15), (11, 16), (12, 17), (13, 33), (23, 47), (24, 48), (25, 49), (100, 9), (9, 100)]


def _ragged(net, imgs):
    sizes = [tuple(im.shape[-2:]) for im in imgs]
    H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
    x = torch.full((len(imgs), 3, H, W), 3.0, device="cuda:0")          # what lies outside an image must not matter
    for j, im in enumerate(imgs):
        x[j, :, :sizes[j][0], :sizes[j][1]] = im[0].to("cuda:0")
    out = net.forward_ragged(x, sizes)
    net.check_status()
    s = net.out_scale()
    return [out[j:j + 1, :, :h * s, :w * s].cpu() for j, (h, w) in enumerate(sizes)]


@pytest.mark.parametrize("scale", [2, 4])
def test_strip_kernel_f16_against_per_layer_f16_on_edge_shapes(cuda_device, scale):
    """NB = 2 RRDBs: six strip launches per forward, every third one with the second residual."""
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=scale, num_block=NB)
    strip = _model(sd, scale, NB, strip="1", size_independent=True)
    layer = _model(sd, scale, NB, strip="0", size_independent=True)
    ref = _oracle(sd, scale, NB)
    shapes = SHAPES_X2 if scale == 2 else SHAPES_X4
    g = torch.Generator().manual_seed(11)
    imgs = [torch.rand(1, 3, h, w, generator=g) for h, w in shapes]
    for net in (strip, layer):
        net.set_kernel_timing("cuda:0", True)
        net.kernel_time()
    got, per = _ragged(strip, imgs), _ragged(layer, imgs)
    assert strip.kernel_time()[1] == 3 * NB, "the ragged batch did not run the LDS-resident kernel"
    assert layer.kernel_time()[1] == 15 * NB
    again = _ragged(strip, imgs)
    worst = 0.0
    for j, im in enumerate(imgs):
        with torch.no_grad():
            want = ref(im)
        assert got[j].shape == want.shape
        assert torch.equal(got[j], again[j]), f"{shapes[j]}: not repeatable"
        d = (got[j] - per[j]).abs().max().item()
        worst = max(worst, d)
        assert d < 1e-3 * max(1.0, want.abs().max().item()), (shapes[j], d)      # f16 resolution of an O(1) output
        if im.numel() >= 3 * 64:
            ps, pl = _psnr(got[j], want), _psnr(per[j], want)
            assert abs(ps - pl) < 0.5, (shapes[j], ps, pl)
        assert torch.isfinite(got[j]).all()
    print(f"x{scale}: strip vs per-layer f16, worst max abs {worst:.3e}")


def test_strip_f16_image_alone_equals_image_in_full_ragged_batch(cuda_device):
    """RAGGED_MAX = 64 images, several per workgroup: an image alone is bitwise itself inside the batch."""
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=1)
    net = _model(sd, 2, 1, strip="1", size_independent=True)
    g = torch.Generator().manual_seed(9)
    shapes = [(2 * (3 + (7 * i) % 40), 2 * (5 + (11 * i) % 90)) for i in range(64)]
    imgs = [torch.rand(1, 3, h, w, generator=g) for h, w in shapes]
    net.set_kernel_timing(cuda_device, True)
    net.kernel_time()
    full = _ragged(net, imgs)
    assert net.kernel_time()[1] == 3
    for j in (0, 13, 31, 63):
        alone = _ragged(net, [imgs[j]])
        assert torch.equal(alone[0], full[j]), shapes[j]
    eq = net(torch.cat([imgs[1], imgs[1].flip(-1)], 0).to(cuda_device)).cpu()
    net.check_status()
    rg = _ragged(net, [imgs[1], imgs[1].flip(-1)])
    assert torch.equal(eq[0:1], rg[0]) and torch.equal(eq[1:2], rg[1])


# ------------------------------------------------------------------------------------------------------------ range
def _scaled_trunk(sd, gain):
    """conv_first x gain, conv_last / gain: the activations between are `gain` times larger, the image stays O(1)."""
    sd = {k: v.clone() for k, v in sd.items()}
    sd["conv_first.weight"] *= gain
    sd["conv_first.bias"] *= gain
    sd["conv_last.weight"] /= gain
    return sd


def test_weights_beyond_f16_are_refused(cuda_device):
    from neural_enhanced_super_resolution_amd import RRDBNet, conv3x3
    from neural_enhanced_super_resolution_amd._lib import NesrRangeError
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=1)
    sd["body.0.rdb2.conv3.weight"][1, 2, 0, 1] = 7.0e4
    net = RRDBNet(3, 3, scale=2, num_block=1, compute_dtype="f16")
    net.load_state_dict(sd)
    net.eval().to(cuda_device)
    with pytest.raises(NesrRangeError, match="65504"):
        net(torch.rand(1, 3, 16, 16, device=cuda_device))
    w = torch.zeros(32, 16, 3, 3)
    w[3, 4, 1, 1] = -6.6e4
    with pytest.raises(NesrRangeError):
        conv3x3(torch.rand(1, 16, 8, 8, device=cuda_device), w, torch.zeros(32), dtype="f16")
    # the same weights are fine for bf16 (f32's range)
    ok = RRDBNet(3, 3, scale=2, num_block=1, compute_dtype="bf16")
    ok.load_state_dict(sd)
    ok.eval().to(cuda_device)(torch.rand(1, 3, 16, 16, device=cuda_device))
    ok.check_status()


@pytest.mark.parametrize("strip", ["0", "1"])
def test_activation_overflow_gives_nan_and_range_error(cuda_device, strip):
    """Activations beyond 65504 (conv_first weights x3e5 stay below it, its outputs do not): NaN output and NesrRangeError, on the
    per-layer path and on the strip path; the next valid frame on the same context is clean."""
    from neural_enhanced_super_resolution_amd._lib import NesrRangeError
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = _scaled_trunk(synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=2), 3e5)
    net = _model(sd, 2, 2, strip=strip, size_independent=True)
    net.set_kernel_timing(cuda_device, True)
    net.kernel_time()
    x = torch.rand(1, 3, 48, 64, generator=torch.Generator().manual_seed(1)).to(cuda_device)
    got = net(x).cpu()
    assert net.kernel_time()[1] == (3 if strip == "1" else 15) * 2, "not the path under test"
    assert torch.isnan(got).all(), "an out-of-range forward must not return a plausible image"
    with pytest.raises(NesrRangeError, match="f16 form"):
        net.check_range()
    net.check_range()                                      # reported once
    ok = net(x * 1e-9).cpu()
    net.check_range()
    assert torch.isfinite(ok).all()
    # ragged batches and the 8-bit path report it as well
    with pytest.raises(NesrRangeError):
        _ragged(net, [x[:, :, :40, :60].cpu(), x.cpu()])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 1e5])
def test_bad_input_is_loud_in_f16(cuda_device, bad):
    from neural_enhanced_super_resolution_amd._lib import NesrRangeError
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    net = _model(synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=1), 2, 1)
    x = torch.rand(1, 3, 48, 64, generator=torch.Generator().manual_seed(1))
    x[0, 1, 7, 9] = bad
    got = net(x.to(cuda_device)).cpu()
    assert torch.isnan(got).all()
    with pytest.raises(NesrRangeError):
        net.check_status()


def test_banded_f16_same_operands(cuda_device):
    """banded.py's generic protocol (whole-block phase 0, as for bf16) on f16 contexts: the band rows carry f16 feature maps."""
    from neural_enhanced_super_resolution_amd import banded
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=9, num_in_ch=3, scale=2, num_block=2)
    nets = [_model(sd, 2, 2) for _ in range(3)]
    x = torch.rand(1, 3, 96, 80, generator=torch.Generator().manual_seed(4)).to(cuda_device)
    want = nets[-1](x)
    u = nets[0].unshuffle
    bands = banded.band_split(x.shape[2] // u, 2)
    tops, bots = [0, banded.APRON], [banded.APRON, 0]
    for r in range(2):
        lo, hi = bands[r]
        nets[r].band_begin(x[:, :, (lo - tops[r]) * u:(hi + bots[r]) * u].contiguous())

    def exchange(buffer, k):
        up = nets[1].band_rows(buffer, tops[1], k)
        down = nets[0].band_rows(buffer, bands[0][1] - bands[0][0] - k, k)
        nets[0].band_set_rows(buffer, bands[0][1] - bands[0][0], up)
        nets[1].band_set_rows(buffer, tops[1] - k, down)

    for i in range(nets[0].num_rdb):
        exchange(i % 3, banded.APRON)
        for net in nets[:2]:
            net.band_rdb(i)
    exchange(0, banded.APRON)
    exchange(3, banded.APRON)
    outs = []
    for r in range(2):
        y = nets[r].band_tail()
        outs.append(y[:, :, 4 * tops[r]: y.shape[2] - 4 * bots[r]])
    got = torch.cat(outs, 2)
    for n in nets:
        n.check_status()
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 4e-3        # the kernel may differ with the image size: f16 resolution, not bits


# ------------------------------------------------------------------------------------------------------------ wrapper
@pytest.fixture(scope="module")
def c3_half():
    """RealESRGANer(half=True, tile=512, tile_pad=10) on a 2160p u8 frame: the f16 model, the default (bf16) model, and f32."""
    from neural_enhanced_super_resolution_amd import RRDBNet, RealESRGANer
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2)
    frame = synthetic_frame(2160, 3840, seed=0)
    out = {}
    ups = {}
    for name, dt, half in (("f16", "f16", True), ("bf16", "f32", True), ("f32", "f32", False)):
        up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, compute_dtype=dt), tile=512, tile_pad=10,
                          pre_pad=0, half=half, device="cuda:0")
        out[name], _ = up.enhance(frame)
        ups[name] = up
    assert ups["f16"].model.compute_dtype == "f16" and ups["bf16"].model.compute_dtype == "bf16"
    return frame, ups, out


def test_wrapper_f16_equals_hand_pasted_serial_tiles(c3_half, cuda_device):
    from neural_enhanced_super_resolution_amd.realesrganer import normalize_u8_on_device
    frame, ups, out = c3_half
    up = ups["f16"]
    x = torch.from_numpy(frame).to(cuda_device)
    img = normalize_u8_on_device(x.permute(2, 0, 1).flip(0)).unsqueeze(0).half()
    canvas = img.new_zeros((1, 3, 4320, 7680))
    for (py0, py1, px0, px1), (oy0, oy1, ox0, ox1), (cy0, cy1, cx0, cx1) in up.tile_grid(2160, 3840):
        t = up.model(img[:, :, py0:py1, px0:px1])
        canvas[:, :, oy0:oy1, ox0:ox1] = t[:, :, cy0:cy1, cx0:cx1]
    up.model.check_status()
    q = (canvas[0].float().clamp_(0, 1).flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8).cpu().numpy()
    assert np.array_equal(q, out["f16"])


def test_wrapper_f16_is_closer_to_f32_than_bf16(c3_half):
    frame, ups, out = c3_half
    ref = out["f32"].astype(np.int16)
    m16 = float(np.abs(out["f16"].astype(np.int16) - ref).mean())
    mbf = float(np.abs(out["bf16"].astype(np.int16) - ref).mean())
    print(f"2160p x2plus tile 512/10, u8 mean abs vs the f32 path: f16 {m16:.4f}, bf16 {mbf:.4f}")
    assert m16 < mbf, (m16, mbf)
    assert out["f16"].shape == (4320, 7680, 3) and out["f16"].std() > 10
