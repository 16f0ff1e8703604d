"""GPU: the resize kernels (csrc/resize.hip) against the torch chain (use_hip=False) and the numpy oracle, on whole tensors and on
row-strided views, inside the NESR tiler and behind RealESRGANer.enhance(outscale=...)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (h, w, out_h, out_w): enlarging, shrinking, mixed, odd sizes, fewer samples than taps, one pixel, one row, equal sizes
SMALL = [(24, 31, 36, 47), (40, 52, 23, 17), (33, 20, 70, 9), (5, 17, 17, 5), (17, 5, 5, 17), (1, 1, 7, 3), (1, 40, 1, 91), (1, 23, 6, 11),
         (19, 27, 19, 27), (9, 300, 4, 700), (70, 3, 150, 2)]


def _rand_u8(shape, seed, device):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(device)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_u8_equals_chain_and_oracle(cuda_device, C):
    from neural_enhanced_super_resolution_amd import imgproc as P
    from oracle import cv2_ref as O
    for n, (h, w, oh, ow) in enumerate(SMALL):
        img = _rand_u8((h, w, C), 100 * C + n, cuda_device)
        got = P.lanczos4_resize(img, oh, ow, use_hip=True)
        chain = P.lanczos4_resize(img, oh, ow, use_hip=False)
        assert got.shape == (oh, ow, C) and got.dtype == torch.uint8
        assert torch.equal(got, chain), (h, w, oh, ow)
        assert torch.equal(P.lanczos4_resize(img, oh, ow), got)                    # the default route is the kernel
        assert np.array_equal(got.cpu().numpy(), O.resize_lanczos4(img.cpu().numpy(), oh, ow)), (h, w, oh, ow)
        if (h, w) == (oh, ow):
            assert torch.equal(got, img)                                           # equal sizes copy


def test_u8_constant_and_extreme_images(cuda_device):
    """A constant image stays constant where the chain keeps it; a 0 / 255 pattern aligned with the taps' signs drives the sums
    to their extremes (beyond int32 before the saturation)."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    for v in (0, 1, 127, 255):
        img = torch.full((21, 34, 3), v, dtype=torch.uint8, device=cuda_device)
        for oh, ow in ((50, 77), (10, 13)):
            got = P.lanczos4_resize(img, oh, ow, use_hip=True)
            assert torch.equal(got, P.lanczos4_resize(img, oh, ow, use_hip=False))
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
    for img in ((((yy + xx) % 2) * 255), (((yy // 2 + xx // 2) % 2) * 255), ((yy % 2) * 255)):
        img = img.to(torch.uint8)[:, :, None].repeat(1, 1, 3).to(cuda_device)
        for oh, ow in ((128, 128), (127, 129), (96, 50)):
            assert torch.equal(P.lanczos4_resize(img, oh, ow, use_hip=True), P.lanczos4_resize(img, oh, ow, use_hip=False))


def test_u8_large_tiler_region(cuda_device):
    """2176 x 2176 -> 1024 x 1024 (a tile region of the forced-tiling route): thousands of workgroups, more than are co-resident."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _rand_u8((2176, 2176, 3), 7, cuda_device)
    got = P.lanczos4_resize(img, 1024, 1024, use_hip=True)
    assert torch.equal(got, P.lanczos4_resize(img, 1024, 1024, use_hip=False))


def test_u8_partial_last_tiles(cuda_device):
    """Sizes that leave the last tile row and column partial, whatever power-of-two tile the host picks (64 k + 1 and 64 k - 1)."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _rand_u8((150, 170, 3), 8, cuda_device)
    for oh, ow in ((257, 321), (191, 127), (65, 513)):
        assert torch.equal(P.lanczos4_resize(img, oh, ow, use_hip=True), P.lanczos4_resize(img, oh, ow, use_hip=False)), (oh, ow)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_u16_equals_oracle_and_chain_within_one(cuda_device, C):
    from neural_enhanced_super_resolution_amd import imgproc as P
    from oracle import cv2_ref as O
    for n, (h, w, oh, ow) in enumerate(SMALL):
        g = torch.Generator().manual_seed(300 * C + n)
        held = torch.randint(0, 65536, (h, w, C), dtype=torch.int32, generator=g)
        held[0, 0, :] = 65535
        want = O.resize_lanczos4(held.numpy().astype(np.uint16), oh, ow).astype(np.int64)
        got = P.lanczos4_resize(held.to(cuda_device), oh, ow, use_hip=True)
        assert got.dtype == torch.int32 and got.shape == (oh, ow, C)
        assert np.array_equal(got.cpu().numpy(), want), (h, w, oh, ow)             # bit for bit the oracle
        chain = P.lanczos4_resize(held.to(cuda_device), oh, ow, use_hip=False)
        assert (got - chain).abs().max().item() <= 1                               # torch's sum order (tests/test_imgproc.py)
        if hasattr(torch, "uint16"):                                               # a real uint16 tensor: the same bytes
            real = torch.from_numpy(held.numpy().astype(np.uint16)).to(cuda_device)
            r = P.lanczos4_resize(real, oh, ow)
            assert r.dtype == torch.uint16 and np.array_equal(r.cpu().numpy().astype(np.int64), want)


@pytest.mark.parametrize("C", [0, 1, 2, 3, 4])
def test_f32_linear_equals_oracle_and_chain(cuda_device, C):
    from neural_enhanced_super_resolution_amd import imgproc as P
    from oracle import cv2_ref as O
    for n, (h, w, oh, ow) in enumerate(SMALL + [(54, 96, 216, 384)]):
        g = torch.Generator().manual_seed(500 + n)
        img = torch.rand((h, w) if C == 0 else (h, w, C), generator=g)
        got = P.linear_resize_f32(img.to(cuda_device), oh, ow, use_hip=True)
        chain = P.linear_resize_f32(img.to(cuda_device), oh, ow, use_hip=False)
        assert got.shape == chain.shape and torch.equal(got, chain), (h, w, oh, ow)          # bit for bit: separate multiply and add
        planes = [img.numpy()] if C == 0 else [img[:, :, c].numpy() for c in range(C)]
        for c, p in enumerate(planes):
            mine = got.cpu().numpy() if C == 0 else got[:, :, c].cpu().numpy()
            assert np.array_equal(mine, O.resize_linear_f32(np.ascontiguousarray(p), oh, ow))


@pytest.mark.parametrize("C", [1, 3, 4])
def test_strided_views_crop_resize_paste(cuda_device, C):
    """frame[y0:y1, x0:x1] -> canvas[a:b, c:d] in one launch equals slice -> contiguous -> resize -> assign, and no canvas byte
    outside the rectangle changes (odd offsets and widths: every alignment of a row's first and last byte)."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    frame = _rand_u8((90, 131, C), 40 + C, cuda_device)
    pattern = (torch.arange(120 * 157 * C, device=cuda_device) * 37 % 251).to(torch.uint8).reshape(120, 157, C)
    for (y0, y1, x0, x1), (a, b, c, d) in (((3, 80, 5, 126), (7, 100, 1, 150)), ((10, 21, 17, 60), (0, 35, 50, 157)), ((0, 90, 0, 131), (1, 118, 2, 61)),
                                           ((40, 41, 9, 10), (60, 67, 33, 36)), ((2, 71, 1, 99), (5, 74, 6, 104))):
        canvas = pattern.clone()
        src = frame[y0:y1, x0:x1]
        assert src.shape[0] == 1 or (x0, x1) == (0, 131) or not src.is_contiguous()       # a row-strided view, not a copy
        r = P.lanczos4_resize(src, b - a, d - c, use_hip=True, out=canvas[a:b, c:d])
        assert r.data_ptr() == canvas[a:b, c:d].data_ptr()
        want = pattern.clone()
        want[a:b, c:d] = P.lanczos4_resize(src.contiguous(), b - a, d - c, use_hip=False)
        assert torch.equal(canvas, want), ((y0, y1, x0, x1), (a, b, c, d))
    # uint16 and float32 sources as views
    g = torch.Generator().manual_seed(9)
    held = torch.randint(0, 65536, (50, 61, C), dtype=torch.int32, generator=g).to(cuda_device)
    v = held[3:40, 7:58]
    assert torch.equal(P.lanczos4_resize(v, 55, 31, use_hip=True), P.lanczos4_resize(v.contiguous(), 55, 31, use_hip=True))
    f = torch.rand((50, 61, C), generator=g).to(cuda_device)
    assert torch.equal(P.linear_resize_f32(f[3:40, 7:58], 55, 31, use_hip=True), P.linear_resize_f32(f[3:40, 7:58].contiguous(), 55, 31, use_hip=False))


def test_process_with_tiling_hip_equals_chain(cuda_device):
    """A 3 x 3 tile grid with a stub processor (nearest x4 of the tile into a x2 canvas, so every region is resized)."""
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    img = _rand_u8((88, 100, 3), 21, cuda_device)
    calls = []

    def proc(t):
        calls.append(tuple(t.shape))
        return t.repeat_interleave(4, 0).repeat_interleave(4, 1)

    hip = A.process_with_tiling(proc, img, 36, 6, 2, cuda_device, as_numpy=False)
    assert len(calls) == 9
    chain = A.process_with_tiling(proc, img, 36, 6, 2, cuda_device, as_numpy=False, use_hip=False)
    assert hip.shape == (176, 200, 3) and torch.equal(hip, chain)
    forced = A.process_with_tiling(proc, img, 36, 6, 2, cuda_device, as_numpy=False, use_hip=True)
    assert torch.equal(forced, chain)


def test_process_with_tiling_real_network(cuda_device):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, nesr_adapter as A
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=6, num_in_ch=12, scale=4, num_block=1)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(12, 3, num_block=1), tile=0, tile_pad=0, pre_pad=0,
                      half=False, device=cuda_device)
    img = torch.from_numpy(synthetic_frame(40, 44, seed=5)[:, :, ::-1].copy()).to(cuda_device)

    def one(t):
        return A.apply_esrgan_3channel(up, t, as_numpy=False)

    hip = A.process_with_tiling(one, img, 24, 4, 2.0, cuda_device, as_numpy=False)
    chain = A.process_with_tiling(one, img, 24, 4, 2.0, cuda_device, as_numpy=False, use_hip=False)
    assert hip.shape == (80, 88, 3) and torch.equal(hip, chain)


def _count_frame_copies(monkeypatch, R):
    copies = []
    orig = R.RealESRGANer._frame_to_host

    def counted(t, host=None):
        copies.append(tuple(t.shape))
        return orig(t, host)

    monkeypatch.setattr(R.RealESRGANer, "_frame_to_host", staticmethod(counted))
    return copies


@pytest.mark.parametrize("route", ["fused", "tiled"])
def test_enhance_outscale_u8_routes(cuda_device, monkeypatch, route):
    """enhance(outscale=s) on the two device-resident 8-bit routes: bit for bit the result with the HIP resize switched off
    (realesrganer.HIP_RESIZE = False: frame to the host, torch chain), and the frame crosses to the host once, already resized
    (counted at RealESRGANer._frame_to_host, the routes' own copy helper)."""
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, realesrganer as R
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=2)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=2), tile=0 if route == "fused" else 32,
                      tile_pad=4, pre_pad=0, half=False, device=cuda_device)
    img = synthetic_frame(40, 52, seed=4)
    assert up._fused_u8_ok(img) == (route == "fused") and up._u8_on_device_ok(img)
    for s in (1.5, 3.5):
        copies = _count_frame_copies(monkeypatch, R)
        monkeypatch.setattr(R, "HIP_RESIZE", True)
        a, mode = up.enhance(img, outscale=s)
        assert copies == [(int(40 * s), int(52 * s), 3)]                            # one copy, of the resized frame
        monkeypatch.setattr(R, "HIP_RESIZE", False)
        b, _ = up.enhance(img, outscale=s)
        assert a.shape == (int(40 * s), int(52 * s), 3) and a.dtype == np.uint8 and mode == "RGB"
        assert np.array_equal(a, b), s


@pytest.mark.parametrize("kind", ["u16", "bgra", "bgra_plain_alpha", "gray"])
def test_enhance_outscale_float_route(cuda_device, monkeypatch, kind):
    """16-bit, BGRA and gray images keep the float route: equal, bit for bit, to the HIP resize switched off.  8-bit frames and the
    plain alpha plane get the kernels through imgproc.  A 16-bit frame keeps the torch chain inside enhance(): the uint16 kernel
    is bit for bit oracle/cv2_ref.py (k ascending: test_u16_equals_oracle_and_chain_within_one) and the chain sums in torch's
    order, so the kernel there measured max |hip - chain| = 1 on 13 of 4536 samples at outscale 1.5 -- enhance()'s present
    16-bit values would have moved."""
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, realesrganer as R
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=2)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=2), tile=0, pre_pad=0, half=False,
                      device=cuda_device)
    img = synthetic_frame(24, 28, seed=12)
    alpha = "realesrgan"
    if kind == "u16":
        img = img.astype(np.uint16) * 257
    elif kind == "gray":
        img = np.ascontiguousarray(img[:, :, 1])
    else:
        img = np.concatenate([img, synthetic_frame(24, 28, seed=13)[:, :, :1]], 2)
        alpha = "bicubic" if kind == "bgra_plain_alpha" else alpha
    for s in (1.5, 3.5):
        monkeypatch.setattr(R, "HIP_RESIZE", True)
        a, mode = up.enhance(img, outscale=s, alpha_upsampler=alpha)
        monkeypatch.setattr(R, "HIP_RESIZE", False)
        b, _ = up.enhance(img, outscale=s, alpha_upsampler=alpha)
        assert a.shape == b.shape and a.shape[:2] == (int(24 * s), int(28 * s)) and a.dtype == img.dtype
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        print(f"{kind} outscale {s}: max |hip - chain| = {d.max()}, differing = {(d > 0).sum()} of {d.size}")
        assert np.array_equal(a, b), (kind, s)


def test_memory_of_one_resize(cuda_device):
    """2160 x 3840 x 3 -> 3240 x 5760: the kernel allocates the destination and its tables; the chain's first intermediate alone is
    3 x 2160 x 5760 x 64 B = 2.4 GB (that half shows the test measures what it claims)."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _rand_u8((2160, 3840, 3), 5, cuda_device)
    P.lanczos4_resize(img[:8, :8], 12, 12, use_hip=True)                           # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = P.lanczos4_resize(img, 3240, 5760, use_hip=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"HIP resize: peak rises by {rise} bytes; destination {out.numel()}")
    assert rise <= out.numel() + (1 << 20)
    del out
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = P.lanczos4_resize(img, 3240, 5760, use_hip=False)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"torch chain: peak rises by {rise} bytes")
    assert rise > (1 << 30)


def test_repeated_calls_allocate_nothing_and_any_stream(cuda_device):
    """The same sizes again: the allocator's device total stays put (tables are cached), and a side stream gives the same bytes."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _rand_u8((300, 400, 3), 6, cuda_device)
    out = torch.empty((450, 333, 3), dtype=torch.uint8, device=cuda_device)
    first = P.lanczos4_resize(img, 450, 333, use_hip=True).clone()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        P.lanczos4_resize(img, 450, 333, use_hip=True, out=out)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = P.lanczos4_resize(img, 450, 333, use_hip=True)
    st.synchronize()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (4 << 20)       # nothing but what torch's allocator took for `side`
    assert torch.equal(out, first) and torch.equal(side, first)
