"""GPU: gray, BGRA and 16-bit frames through enhance() on the device (RealESRGANer._enhance_frame_on_device, frame_io.py,
csrc/frame_io.hip).  The route performs the float32 operations of enhance_float and enhance's quantiser in their order on the same
network output, so equality with the host route (realesrganer.DEVICE_FRAMES = False) is required bit for bit, not within a
tolerance; against the oracle's fixtures the bounds are those of tests/test_gpu_golden.py::test_wrapper_cases_vs_golden."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import make_golden as G  # noqa: E402

KINDS = ("gray8", "bgra8", "bgr16", "gray16", "bgra16", "dark16", "bgra8_plain")


def _frame(kind, h, w, seed):
    """(frame, alpha_upsampler).  16-bit samples are 8-bit noise times an odd factor: not all multiples of 257."""
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    bgr = synthetic_frame(h, w, seed=seed)
    a = synthetic_frame(h, w, seed=seed + 100, channels=0)
    wide = lambda x: x.astype(np.uint16) * 251       # noqa: E731  (255 * 251 = 64005)
    if kind == "gray8":
        return np.ascontiguousarray(bgr[:, :, 1]), "realesrgan"
    if kind in ("bgra8", "bgra8_plain"):
        return np.concatenate([bgr, a[:, :, None]], 2), "realesrgan" if kind == "bgra8" else "plain"
    if kind == "bgr16":
        return wide(bgr), "realesrgan"
    if kind == "gray16":
        return wide(np.ascontiguousarray(bgr[:, :, 1])), "realesrgan"
    if kind == "bgra16":
        return wide(np.concatenate([bgr, a[:, :, None]], 2)), "realesrgan"
    if kind == "dark16":
        d = bgr.astype(np.uint16)
        d[0, 0, 0] = 256                              # the largest maximum enhance() still takes for 8-bit range
        return d, "realesrgan"
    raise ValueError(kind)


def _wrapper(net, device, **kw):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, SRVGGNetCompact
    from neural_enhanced_super_resolution_amd.synth import synthetic_compact_state_dict, synthetic_state_dict
    if net == "compact":
        cfg = dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=2, upscale=4, act_type="prelu")
        return RealESRGANer(scale=4, model_path={"params": synthetic_compact_state_dict(seed=5, **cfg)}, model=SRVGGNetCompact(**cfg), half=False,
                            device=device, **kw)
    scale = 4 if net == "x4" else 2
    sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=scale, num_block=2)
    return RealESRGANer(scale=scale, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=scale, num_block=2), half=net == "x2_half",
                        device=device, **kw)


def _both_routes(up, R, monkeypatch, img, **kw):
    monkeypatch.setattr(R, "DEVICE_FRAMES", True)
    assert up._device_frame_ok(img)
    a, ma = up.enhance(img, **kw)
    monkeypatch.setattr(R, "DEVICE_FRAMES", False)
    assert not up._device_frame_ok(img)
    b, mb = up.enhance(img, **kw)
    monkeypatch.setattr(R, "DEVICE_FRAMES", True)
    return a, ma, b, mb


@pytest.mark.parametrize("net", ["x2", "x2_half", "x4", "compact"])
@pytest.mark.parametrize("tile,pre_pad", [(0, 0), (0, 10), (32, 0), (32, 10)])
def test_device_route_equals_host_route_bitwise(cuda_device, monkeypatch, net, tile, pre_pad):
    from neural_enhanced_super_resolution_amd import realesrganer as R
    up = _wrapper(net, cuda_device, tile=tile, tile_pad=10, pre_pad=pre_pad)
    for hw in ((40, 52), (39, 51)):
        for i, kind in enumerate(KINDS):
            img, alpha = _frame(kind, hw[0], hw[1], seed=hw[0] + i)
            a, ma, b, mb = _both_routes(up, R, monkeypatch, img, alpha_upsampler=alpha)
            want_dtype = np.uint8 if kind in ("gray8", "bgra8", "bgra8_plain", "dark16") else np.uint16
            assert ma == mb and a.dtype == b.dtype == want_dtype and a.shape == b.shape, (kind, hw)
            assert a.shape[:2] == (hw[0] * up.scale, hw[1] * up.scale)
            assert np.array_equal(a, b), (kind, hw, int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max()))
            assert a.std() > 0, kind


@pytest.mark.parametrize("kind", ["bgra8", "gray16", "bgra8_plain"])
def test_outscale_equals_host_route_bitwise(cuda_device, monkeypatch, kind):
    from neural_enhanced_super_resolution_amd import realesrganer as R
    up = _wrapper("x2", cuda_device, tile=0, tile_pad=10, pre_pad=0)
    img, alpha = _frame(kind, 24, 28, seed=12)
    a, ma, b, mb = _both_routes(up, R, monkeypatch, img, outscale=1.5, alpha_upsampler=alpha)
    assert ma == mb and a.dtype == b.dtype == img.dtype and a.shape == b.shape and a.shape[:2] == (36, 42)
    assert np.array_equal(a, b), kind


def test_wrapper_cases_of_the_oracle(cuda_device, golden_dir, monkeypatch):
    """The gray, bgra and u16 fixtures of tests/golden/wrapper.npz through the device route, with that test's bounds."""
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, realesrganer as R
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    monkeypatch.setattr(R, "DEVICE_FRAMES", True)
    g = np.load(os.path.join(golden_dir, "wrapper.npz"))
    crop = np.load(os.path.join(golden_dir, "test_jpeg_crop_64x96_bgr.npy"))
    sd2 = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=2)
    seen = []
    for name, kw, kind in G.wrapper_cases():
        if kind not in ("gray", "bgra", "u16"):
            continue
        seen.append(kind)
        up = RealESRGANer(scale=2, model_path={"params_ema": sd2}, model=RRDBNet(3, 3, scale=2, num_block=2), half=False, device=cuda_device, **kw)
        img = G.wrapper_input(kind, crop)
        assert up._device_frame_ok(img)
        q, mode = up.enhance(img)
        want = g[f"{name}_q"]
        assert mode == str(g[f"{name}_mode"]) and q.shape == want.shape and q.dtype == want.dtype
        lsb = 257 if q.dtype == np.uint16 else 1
        diff = np.abs(q.astype(np.int64) - want.astype(np.int64))
        print(f"{name}: max diff {diff.max()}, differing share {(diff > 0).mean():.2e}")
        assert diff.max() <= lsb, (name, diff.max())
        assert (diff > 0).mean() < (1e-2 if q.dtype == np.uint16 else 1e-3), (name, (diff > 0).mean())
        if f"{name}_f" in g.files:
            f, _, _ = up.enhance_float(img)
            assert np.abs(f - g[f"{name}_f"]).max() < 1e-3, name
    assert sorted(seen) == ["bgra", "gray", "u16"]


@pytest.mark.parametrize("bits,max_range", [(8, 255), (16, 65535), (16, 255)])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_pack_kernel_equals_chain(cuda_device, bits, max_range, channels):
    from neural_enhanced_super_resolution_amd import frame_io
    rng = np.random.default_rng(bits + channels)
    for h, w in ((16, 24), (17, 23), (3, 1), (40, 52)):
        shape = (h, w + 8) if channels == 1 else (h, w + 8, channels)
        a = rng.integers(0, 65536 if max_range == 65535 else (256 if bits == 8 else 257), size=shape).astype(np.uint8 if bits == 8 else np.uint16)
        whole = frame_io.frame_to_tensor(a, cuda_device)
        for frame in (whole[:, :w].contiguous(), whole[:, 2:2 + w], whole[:, 4:4 + w]):      # dense, and two pitched views
            for form in ("network", "linear"):
                for half in (False, True):
                    x, xa = frame_io.pack_frame(frame, max_range, alpha=form, through_fp16=half, use_hip=True)
                    y, ya = frame_io.pack_frame(frame, max_range, alpha=form, through_fp16=half, use_hip=False)
                    assert x.shape == y.shape == (1, 3, h, w) and torch.equal(x.view(torch.int32), y.view(torch.int32))
                    if channels == 4:
                        assert xa.shape == ya.shape and torch.equal(xa.view(torch.int32), ya.view(torch.int32))
                    else:
                        assert xa is None and ya is None


@pytest.mark.parametrize("max_range", [255, 65535])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_unpack_kernel_equals_chain(cuda_device, max_range, channels):
    from neural_enhanced_super_resolution_amd import frame_io
    from tests.test_frame_io_host import _network_output
    for ho, wo in ((32, 48), (33, 47), (2, 3)):
        big = torch.from_numpy(_network_output(ho + 4, wo + 8, max_range, seed=ho)).to(cuda_device)
        big_a = torch.from_numpy(_network_output(ho + 4, wo + 8, max_range, seed=ho + 1)).to(cuda_device)
        plane = torch.rand((ho + 4, wo + 8), generator=torch.Generator().manual_seed(ho)).to(cuda_device)
        # post_process's views: the top-left crop of a larger output; and the dense tensor itself
        for out, a3, a1 in ((big[:, :, :ho, :wo], big_a[:, :, :ho, :wo], plane[:ho, :wo]),
                            (big[:, :, :ho, :wo].contiguous(), big_a[:, :, :ho, :wo].contiguous(), plane[:ho, :wo].contiguous())):
            for alpha in ([a3, a1] if channels == 4 else [None]):
                for half in (False, True):
                    q = frame_io.unpack_frame(out, channels, max_range, alpha=alpha, through_fp16=half, use_hip=True)
                    r = frame_io.unpack_frame(out, channels, max_range, alpha=alpha, through_fp16=half, use_hip=False)
                    assert q.dtype == r.dtype == (torch.uint8 if max_range == 255 else torch.int16) and q.shape == r.shape
                    assert torch.equal(q, r), (ho, wo, half, int((q.int() - r.int()).abs().max()))


def test_one_copy_home_and_no_float_canvas(cuda_device, monkeypatch):
    from neural_enhanced_super_resolution_amd import realesrganer as R
    from tests.test_gpu_resize import _count_frame_copies
    monkeypatch.setattr(R, "DEVICE_FRAMES", True)
    floats = []
    orig_cpu, orig_to = torch.Tensor.cpu, torch.Tensor.to

    def cpu(self, *a, **k):
        if self.is_cuda and self.dtype == torch.float32:
            floats.append(self.numel())
        return orig_cpu(self, *a, **k)

    def to(self, *a, **k):
        r = orig_to(self, *a, **k)
        if self.is_cuda and not r.is_cuda and self.dtype == torch.float32:
            floats.append(self.numel())
        return r
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    monkeypatch.setattr(torch.Tensor, "to", to)
    for tile, pre_pad in ((0, 0), (32, 10)):
        up = _wrapper("x2", cuda_device, tile=tile, tile_pad=10, pre_pad=pre_pad)
        up.enhance(_frame("gray8", 40, 52, seed=0)[0])       # the first call creates the contexts: the model's parameters cross to the host there
        for i, kind in enumerate(KINDS):
            img, alpha = _frame(kind, 40, 52, seed=i)
            for outscale in (None, 1.5):
                copies = _count_frame_copies(monkeypatch, R)
                del floats[:]
                q, _ = up.enhance(img, outscale=outscale, alpha_upsampler=alpha)
                assert copies == [q.shape], (kind, outscale, copies)              # exactly one, of the finished frame
                assert all(n <= 80 * 104 for n in floats), (kind, floats)           # nothing float32 beyond an alpha plane's size


@pytest.mark.parametrize("inflight", [1, 3])
def test_enhance_many_mixed_kinds(cuda_device, monkeypatch, inflight):
    from neural_enhanced_super_resolution_amd import realesrganer as R
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    monkeypatch.setattr(R, "DEVICE_FRAMES", True)
    up = _wrapper("x2", cuda_device, tile=0, tile_pad=10, pre_pad=0)
    imgs = [synthetic_frame(40, 52, seed=1), _frame("gray8", 40, 52, 2)[0], _frame("bgra16", 40, 52, 3)[0], _frame("bgr16", 40, 52, 4)[0],
            _frame("dark16", 24, 28, 5)[0], synthetic_frame(24, 28, seed=6), _frame("bgra8", 24, 28, 7)[0]]
    assert all(up._fused_u8_ok(i) or up._frame_inflight_ok(i) for i in imgs)
    want = [up.enhance(i) for i in imgs]
    got = up.enhance_many(imgs, inflight=inflight)
    assert len(got) == len(want)
    for (a, ma), (b, mb) in zip(got, want):
        assert ma == mb and a.dtype == b.dtype and np.array_equal(a, b)


def test_range_error_still_raises_for_a_gray_frame(cuda_device, monkeypatch):
    """The weights of tests/test_gpu_range.py::test_activation_overflow_is_loud (conv_first's outputs pass 65504, which the default
    f32 form cannot carry): enhance() of a gray frame raises out of the device route, as out of the host route."""
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, realesrganer as R
    from neural_enhanced_super_resolution_amd._lib import NesrRangeError
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    from tests.test_gpu_range import _scaled_trunk
    sd = _scaled_trunk(synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=2), 3e5)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=2), tile=0, pre_pad=0, half=False, device=cuda_device)
    gray, _ = _frame("gray16", 32, 48, seed=1)
    for on in (True, False):
        monkeypatch.setattr(R, "DEVICE_FRAMES", on)
        with pytest.raises(NesrRangeError):
            up.enhance(gray)
    monkeypatch.setattr(R, "DEVICE_FRAMES", True)
    with pytest.raises(NesrRangeError):
        up.enhance(_frame("bgra8", 33, 47, seed=2)[0])      # padded, two evaluations
