"""CPU: gray, BGRA and 16-bit frames (include/nesr_hip.h: nesr_pack_frame, nesr_unpack_frame, nesr_frame_scratch_bytes,
nesr_enhance_frame; frame_io.py; RealESRGANer._enhance_frame_on_device) -- the entries declared, bound and exported, every argument
error that can be seen without a context refused before a device is touched (no GPU here: the library loads without one), the torch
chains bit for bit the numpy lines of enhance_float and enhance's quantiser, and which frames take the device route.

A context cannot be created without a device, so the refusals that read one (a network that is not 3 in / 3 out, sides that the
unshuffle factor does not divide, scratch too small) are in tests/test_gpu_frame_host.py."""
import ctypes

import numpy as np
import pytest
import torch

ENTRIES = ("nesr_pack_frame", "nesr_unpack_frame", "nesr_frame_scratch_bytes", "nesr_enhance_frame")
ERR_ARG = -1
NETWORK, LINEAR = 0, 1
FAKE = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails its argument check first
FAKE2 = ctypes.c_void_p(0x2000)
FAKE3 = ctypes.c_void_p(0x3000)
ODD = ctypes.c_void_p(0x1001)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


def test_entries_declared_bound_and_exported(lib):
    from neural_enhanced_super_resolution_amd import _lib
    from tests.test_cabi import header_symbols
    syms = header_symbols()
    for s in ENTRIES:
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s)
    assert (_lib.ALPHA_NETWORK, _lib.ALPHA_LINEAR) == (NETWORK, LINEAR)


def _refused(lib, rc, text):
    assert rc == ERR_ARG
    assert text in lib.nesr_last_error().decode(), lib.nesr_last_error().decode()


def test_argument_errors_without_a_device(lib):
    H, W = 8, 12

    def pack(src=FAKE, h=H, w=W, c=3, bits=8, pitch=None, mr=255, img=FAKE2, mode=NETWORK, alpha=None):
        pitch = w * c * (bits // 8 if bits in (8, 16) else 1) if pitch is None else pitch
        return lib.nesr_pack_frame(0, src, h, w, c, bits, pitch, mr, 0, img, mode, alpha, None)

    def unpack(img=FAKE, h=H, w=W, plane=H * W, row=W, mode=NETWORK, alpha=None, ap=H * W, ar=W, c=3, bits=8, mr=255, dst=FAKE2, pitch=None):
        pitch = w * c * (bits // 8 if bits in (8, 16) else 1) if pitch is None else pitch
        return lib.nesr_unpack_frame(0, img, h, w, plane, row, 0, mode, alpha, ap, ar, c, bits, mr, dst, pitch, None)

    def enhance(ctx=FAKE, src=FAKE2, h=H, w=W, c=3, bits=8, mr=255, mode=NETWORK, scratch=FAKE3, nbytes=1 << 30, dst=ctypes.c_void_p(0x4000)):
        return lib.nesr_enhance_frame(ctx, src, h, w, c, bits, mr, mode, 0, scratch, nbytes, dst, None)

    for fn in (pack, unpack, enhance):
        for c in (0, 2, 5, -1):
            _refused(lib, fn(c=c, **({"alpha": FAKE3} if fn is unpack else {})), "channels")
        for bits in (0, 4, 12, 32):
            _refused(lib, fn(bits=bits), "bits")
        for mr in (0, 256, 1023, 65536, -255):
            _refused(lib, fn(bits=16, mr=mr), "max_range")
        _refused(lib, fn(bits=8, mr=65535), "needs 16 bits")
        for mode in (-1, 2):
            _refused(lib, fn(c=4, mode=mode, **({"alpha": FAKE3} if fn is unpack else {})), "alpha_mode")
        for h, w in ((0, W), (H, 0), (-3, W)):
            _refused(lib, fn(h=h, w=w), "sizes")
    _refused(lib, pack(src=None), "null")
    _refused(lib, pack(img=None), "null")
    _refused(lib, pack(pitch=W * 3 - 1), "pitch")
    _refused(lib, pack(bits=16, mr=65535, src=ODD), "even")
    _refused(lib, pack(bits=16, mr=65535, pitch=W * 6 + 1), "even")
    _refused(lib, unpack(img=None), "null")
    _refused(lib, unpack(dst=None), "null")
    _refused(lib, unpack(c=4, alpha=None), "null")
    _refused(lib, unpack(pitch=W * 3 - 1), "pitch")
    _refused(lib, unpack(bits=16, mr=65535, dst=ODD), "even")
    _refused(lib, unpack(row=W - 1), "image pitch")
    _refused(lib, unpack(plane=H * W - 1), "image pitch")
    _refused(lib, unpack(c=4, alpha=FAKE3, ar=W - 1), "alpha pitch")
    _refused(lib, unpack(c=4, alpha=FAKE3, ap=H * W - 1), "alpha pitch")
    assert lib.nesr_last_error() and unpack(c=4, alpha=FAKE3, mode=LINEAR, ap=0, ar=W - 1) == ERR_ARG
    for kw in (dict(ctx=None), dict(src=None), dict(scratch=None), dict(dst=None)):
        _refused(lib, enhance(**kw), "null")
    assert lib.nesr_frame_scratch_bytes(None, H, W, 3, NETWORK) == 0


# ------------------------------------------------------------------------------------------------ the torch chains on the CPU
def _frame(h, w, channels, bits, seed, dark=False):
    rng = np.random.default_rng(seed)
    hi = 257 if dark else (1 << bits)
    shape = (h, w) if channels == 1 else (h, w, channels)
    a = rng.integers(0, hi, size=shape).astype(np.uint8 if bits == 8 else np.uint16)
    a.flat[0] = hi - 1                                  # the top of the range is there
    a.flat[1] = 0
    return a


def _host_preparation(img, max_range, alpha_form):
    """enhance_float's lines up to pre_process, and pre_process's transpose (realesrganer.py)."""
    x = img.astype(np.float32) / max_range
    alpha = None
    if x.ndim == 2:
        x = np.repeat(x[:, :, None], 3, axis=2)
    elif x.shape[2] == 4:
        alpha = x[:, :, 3]
        x = x[:, :, 0:3][:, :, ::-1]
        if alpha_form == "network":
            alpha = np.transpose(np.repeat(alpha[:, :, None], 3, axis=2), (2, 0, 1))[None]
    else:
        x = x[:, :, ::-1]
    return np.ascontiguousarray(np.transpose(x, (2, 0, 1)))[None], alpha


@pytest.mark.parametrize("bits,max_range", [(8, 255), (16, 65535), (16, 255)])
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("hw", [(8, 12), (7, 13), (1, 5), (33, 31)])
def test_pack_chain_equals_enhance_floats_host_preparation(bits, max_range, channels, hw):
    from neural_enhanced_super_resolution_amd import frame_io
    img = _frame(hw[0], hw[1], channels, bits, seed=hw[0] * 7 + channels, dark=(bits, max_range) == (16, 255))
    for form in ("network", "linear"):
        got, got_a = frame_io.pack_frame(frame_io.frame_to_tensor(img), max_range, alpha=form, use_hip=False)
        want, want_a = _host_preparation(img, max_range, form)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
        if channels == 4:
            assert np.array_equal(got_a.numpy().view(np.uint32), np.ascontiguousarray(want_a).view(np.uint32))
        else:
            assert got_a is None
    # half=True: `self.img.half()` in pre_process, then the network's .float()
    got, got_a = frame_io.pack_frame(frame_io.frame_to_tensor(img), max_range, alpha="linear", through_fp16=True, use_hip=False)
    want, want_a = _host_preparation(img, max_range, "linear")
    assert np.array_equal(got.numpy(), torch.from_numpy(want).half().float().numpy())
    if channels == 4:
        assert np.array_equal(got_a.numpy(), want_a)             # the plain alpha plane never passes the network


def _network_output(ho, wo, max_range, seed):
    """Random float32 "network outputs" in [-0.25, 1.25] with exact rounding ties, the ends of the range and -0.0 among them."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.25, 1.25, size=(1, 3, ho, wo)).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    ks = rng.integers(0, max_range, size=n // 4)
    flat[: n // 4] = ((ks.astype(np.float64) + 0.5) / max_range).astype(np.float32)       # (k + 0.5) / max_range: ties where representable
    flat[n // 4: n // 4 + 3] = (0.0, 1.0, -0.0)
    flat[n // 4 + 3: n // 4 + 6] = np.float32(0.5) / np.float32(255), np.float32(2.5) / np.float32(255), np.float32(32767.5) / np.float32(65535)
    rng.shuffle(flat)
    return flat.reshape(1, 3, ho, wo)


def _numpy_finish(out, channels, max_range, alpha=None):
    """enhance_float from the clamp on, and enhance's quantiser (realesrganer.py), with the oracle's BGR2GRAY."""
    from oracle.realesrganer_ref import bgr2gray_f32

    def bgr(t):
        t = torch.from_numpy(t).squeeze().float().clamp_(0, 1).numpy()
        return np.transpose(t[[2, 1, 0], :, :], (1, 2, 0))

    img = bgr(out)
    if channels == 1:
        img = bgr2gray_f32(img)
    if channels == 4:
        a = bgr2gray_f32(bgr(alpha)) if alpha.ndim == 4 else alpha      # the plain plane is in [0, 1] already: the clamp is the identity
        img = np.concatenate([img, a[:, :, None]], axis=2)
    if max_range == 65535:
        return (img * 65535.0).round().astype(np.uint16)
    return (img * 255.0).round().astype(np.uint8)


@pytest.mark.parametrize("max_range", [255, 65535])
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("hw", [(16, 24), (9, 11)])
def test_unpack_chain_equals_the_numpy_chain(max_range, channels, hw):
    from neural_enhanced_super_resolution_amd import frame_io
    out = _network_output(hw[0], hw[1], max_range, seed=hw[0] + channels)
    alphas = [None]
    if channels == 4:
        plane = np.random.default_rng(5).uniform(0, 1, size=hw).astype(np.float32)
        plane.flat[:3] = (0.0, 1.0, np.float32(0.5) / np.float32(255))
        alphas = [_network_output(hw[0], hw[1], max_range, seed=99), plane]
    for alpha in alphas:
        got = frame_io.unpack_frame(torch.from_numpy(out), channels, max_range, alpha=None if alpha is None else torch.from_numpy(alpha), use_hip=False)
        want = _numpy_finish(out, channels, max_range, alpha)
        got = frame_io.frame_to_numpy(got)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want)
    # a cropped view, as post_process hands it over
    big = _network_output(hw[0] + 4, hw[1] + 6, max_range, seed=3)
    if channels != 4:
        view = torch.from_numpy(big)[:, :, : hw[0], : hw[1]]
        got = frame_io.frame_to_numpy(frame_io.unpack_frame(view, channels, max_range, use_hip=False))
        assert np.array_equal(got, _numpy_finish(np.ascontiguousarray(big[:, :, : hw[0], : hw[1]]), channels, max_range))


def test_unpack_chain_through_fp16():
    from neural_enhanced_super_resolution_amd import frame_io
    out = _network_output(10, 14, 255, seed=8)
    got = frame_io.unpack_frame(torch.from_numpy(out), 1, 255, through_fp16=True, use_hip=False).numpy()
    want = _numpy_finish(torch.from_numpy(out).half().float().numpy(), 1, 255)
    assert np.array_equal(got, want)


def test_forced_hip_route_refuses_cpu_tensors():
    from neural_enhanced_super_resolution_amd import frame_io
    with pytest.raises(ValueError, match="HIP kernel takes"):
        frame_io.pack_frame(torch.zeros((4, 4), dtype=torch.uint8), 255, use_hip=True)
    with pytest.raises(ValueError, match="HIP kernel takes"):
        frame_io.unpack_frame(torch.zeros((1, 3, 4, 4)), 3, 255, use_hip=True)
    with pytest.raises(ValueError, match="max_range"):
        frame_io.pack_frame(torch.zeros((4, 4), dtype=torch.uint8), 65535, use_hip=False)
    with pytest.raises(ValueError, match="a frame is"):
        frame_io.pack_frame(torch.zeros((4, 4, 2), dtype=torch.uint8), 255, use_hip=False)


# ------------------------------------------------------------------------------------------------ which frames take which route
KINDS = {
    "gray8": lambda: _frame(8, 12, 1, 8, 1),
    "bgra8": lambda: _frame(8, 12, 4, 8, 2),
    "bgr16": lambda: _frame(8, 12, 3, 16, 3),
    "gray16": lambda: _frame(8, 12, 1, 16, 4),
    "bgra16": lambda: _frame(8, 12, 4, 16, 5),
    "dark16": lambda: _frame(8, 12, 3, 16, 6, dark=True),
}


def _stub_wrapper(model):
    """A RealESRGANer around a HIP model that claims the ROCm device, without one: only the routing is exercised."""
    from neural_enhanced_super_resolution_amd import RealESRGANer
    up = RealESRGANer.__new__(RealESRGANer)
    up.scale, up.tile_size, up.tile_pad, up.pre_pad, up.half, up.devices = 2, 0, 10, 0, False, None
    up.device = torch.device("cuda", 0)
    up.model = model
    return up


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_routing_predicate(kind, monkeypatch):
    from neural_enhanced_super_resolution_amd import RRDBNet, SRVGGNetCompact, realesrganer as R
    img = KINDS[kind]()
    calls = []
    monkeypatch.setattr(R.RealESRGANer, "_enhance_frame_on_device",
                        lambda self, img, resize_to=None, alpha_upsampler="realesrgan": calls.append(("device", resize_to, alpha_upsampler)) or (img, "X"))

    def old(self, img, alpha_upsampler="realesrgan"):
        calls.append(("host", alpha_upsampler))
        return np.zeros(img.shape, np.float32), "X", 255
    monkeypatch.setattr(R.RealESRGANer, "enhance_float", old)
    up = _stub_wrapper(RRDBNet(3, 3, scale=2, num_block=1))
    assert up._device_frame_ok(img)
    up.enhance(img)
    up.enhance(img, outscale=1.5, alpha_upsampler="bicubic")
    assert calls == [("device", None, "realesrgan"), ("device", (12, 18), "bicubic")]
    mode = "L" if img.ndim == 2 else ("RGBA" if img.shape[2] == 4 else "RGB")
    assert up._frame_kind(img) == (255 if kind in ("gray8", "bgra8", "dark16") else 65535, mode)
    del calls[:]
    monkeypatch.setattr(R, "DEVICE_FRAMES", False)
    assert not up._device_frame_ok(img)
    up.enhance(img)
    assert calls == [("host", "realesrgan")]
    monkeypatch.setattr(R, "DEVICE_FRAMES", True)
    # not a HIP model, not the ROCm device, or a network the route does not cover: the parent's route
    assert _stub_wrapper(SRVGGNetCompact(3, 3, upscale=2, num_conv=2))._device_frame_ok(img)
    assert not _stub_wrapper(torch.nn.Identity())._device_frame_ok(img)
    assert not _stub_wrapper(RRDBNet(3, 3, scale=4, num_block=1))._device_frame_ok(img)      # the model's x4 under a x2 wrapper
    assert not _stub_wrapper(RRDBNet(12, 3, scale=4, num_block=1))._device_frame_ok(img)
    cpu = _stub_wrapper(RRDBNet(3, 3, scale=2, num_block=1))
    cpu.device = torch.device("cpu")
    assert not cpu._device_frame_ok(img)
    assert not up._device_frame_ok(img.astype(np.float32))


def test_frames_in_flight_predicate():
    from neural_enhanced_super_resolution_amd import RRDBNet
    up = _stub_wrapper(RRDBNet(3, 3, scale=2, num_block=1))
    assert all(up._frame_inflight_ok(make()) for make in KINDS.values())
    assert not up._frame_inflight_ok(_frame(8, 12, 3, 8, 1))          # 8-bit BGR has the fused route
    assert not up._frame_inflight_ok(_frame(7, 12, 1, 8, 1))          # needs the mod-pad
    up.pre_pad = 10
    assert not up._frame_inflight_ok(_frame(8, 12, 1, 8, 1))
    up.pre_pad, up.tile_size = 0, 8
    assert not up._frame_inflight_ok(_frame(8, 12, 1, 8, 1))          # needs tiling
    assert up._frame_inflight_ok(_frame(8, 8, 1, 8, 1))
