"""GPU: the PNG decoder's kernels (csrc/png_decode.hip through imgproc.decode_png) against the specification
(tests/png_decode_ref.py; tests/test_png_decode_spec.py holds it to zlib and shows that the grid visits every rule).  Every criterion
is bit equality with the frame, or the specification's status bit."""
import numpy as np
import pytest
import torch

from tests import png_cases, png_decode_cases as cases, png_decode_ref as ref

pytestmark = pytest.mark.gpu
CASES = png_cases.cases()
FOREIGN = cases.foreign()
OTHERS = cases.handmade() + [cases.far_match()]


def _want(frame, order):
    if order == "bgr" and frame.ndim == 3:
        frame = np.concatenate([frame[:, :, 2::-1], frame[:, :, 3:]], axis=2)
    return np.ascontiguousarray(frame)


def _equal(got, frame, order):
    want = _want(frame, order)
    assert got.dtype == (torch.int16 if frame.dtype == np.uint16 else torch.uint8) and tuple(got.shape) == want.shape
    return np.array_equal(got.cpu().numpy().view(frame.dtype), want)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_own_files_decode_to_the_frame(cuda_device, case):
    from neural_enhanced_super_resolution_amd import imgproc
    _, kind, h, w, c, depth = case
    img, order = png_cases.image(kind, h, w, c, depth)
    frame = png_cases.file_order(img, order)
    data = png_cases.spec(kind, h, w, c, depth)[0]
    info, segs = ref.parse(data)
    for o in ("rgb", "bgr"):
        assert _equal(imgproc.decode_png(data, order=o, device=cuda_device), frame, o), o
        if len(segs) == 1:                                   # inflate=None took the hybrid route: the device inflater on the same file
            assert _equal(imgproc.decode_png(data, order=o, device=cuda_device, inflate="device"), frame, o), o
    # a strided window of a larger canvas; nothing outside it is written
    dtype = torch.int16 if depth == 16 else torch.uint8
    canvas = torch.full((h + 7, w + 11) + ((c,) if c > 1 else ()), 101, dtype=dtype, device=cuda_device)
    before = canvas.clone()
    window = canvas[3:3 + h, 5:5 + w]
    for inflate in ("device", "host"):
        got = imgproc.decode_png(data, device=cuda_device, inflate=inflate, out=window)
        assert got.data_ptr() == window.data_ptr() and _equal(window, frame, "rgb"), inflate
        mask = torch.ones_like(canvas, dtype=torch.bool)
        mask[3:3 + h, 5:5 + w] = False
        assert torch.equal(canvas[mask], before[mask]), inflate
        window.fill_(101)


@pytest.mark.parametrize("case", FOREIGN + OTHERS, ids=[c[0] for c in FOREIGN + OTHERS])
def test_foreign_files_both_routes(cuda_device, case):
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    cid, data, frame = case
    info, segs = ref.parse(data)
    status = ref.inflate_plan(data, info, segs)[1] if info["contiguous"] else None
    order = "bgr" if len(data) % 2 else "rgb"
    assert _equal(imgproc.decode_png(data, order=order, device=cuda_device, inflate="host"), frame, order)
    assert _equal(imgproc.decode_png(data, order=order, device=cuda_device), frame, order)         # Z_SYNC_FLUSH: falls back
    if status == 0:
        assert _equal(imgproc.decode_png(data, order=order, device=cuda_device, inflate="device"), frame, order)
    else:                                                      # a plan that is not contiguous, or a dependent segment
        assert status in (None, ref.DEPENDENT)
        with pytest.raises(_lib.NesrUnsupportedError):
            imgproc.decode_png(data, order=order, device=cuda_device, inflate="device")


LONG = [cases.many_segments, cases.many_pieces]


@pytest.mark.parametrize("build", LONG, ids=[b.__name__ for b in LONG])
def test_long_files_take_a_second_turn_of_the_scan_and_of_the_adler_fold(cuda_device, build):
    """More than 1024 segments (pngd_scan carries across a step) and more than 256 Adler pieces (two per lane of pngd_adler_check),
    all-device route; the path is asserted from the host parser so that a changed constant cannot leave it untested"""
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    cid, data, frame = build()
    info, _ = _lib.png_parse(data)
    npieces = -(-info.stream_bytes // cases.kernel_constant("png_decode_kernels.h", "ADLER_PIECE"))
    assert info.contiguous and (info.n_segments > cases.SCAN_LANES if build is cases.many_segments else npieces > 256)
    assert _equal(imgproc.decode_png(data, device=cuda_device, inflate="device"), frame, "rgb")


SYNC = [c for c in FOREIGN if "sync" in c[0]]


@pytest.mark.parametrize("case", SYNC, ids=[c[0] for c in SYNC])
def test_sync_flush_falls_back_when_the_default_route_tries_the_device(cuda_device, monkeypatch, case):
    """inflate=None sends only large files to the device inflater (imgproc._png_default_on_device); with the size rule lifted these
    small ones go there too, end in DEPENDENT wherever a segment reaches back, and the host inflates instead"""
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    cid, data, frame = case
    info, segs = ref.parse(data)
    monkeypatch.setattr(imgproc, "PNG_DEVICE_MIN_RATIO", 0)
    want = bool(info["contiguous"]) and len(segs) >= 2
    assert imgproc._png_default_on_device(*_lib.png_parse(data), len(data)) == want
    assert _equal(imgproc.decode_png(data, order="bgr", device=cuda_device), frame, "bgr")


def test_the_grid_reaches_the_device_inflater_with_every_kind_of_plan():
    plans = [ref.parse(c[1]) for c in FOREIGN]
    assert sum(1 for i, s in plans if i["contiguous"] and len(s) >= 2) >= 10 and any(not i["contiguous"] for i, _ in plans)
    assert sum(1 for c in FOREIGN if "sync" in c[0]) >= 7


CORRUPT = cases.corrupt()


@pytest.mark.parametrize("case", CORRUPT, ids=[c[0] for c in CORRUPT])
def test_corrupt_input_ends_in_its_status_bit(cuda_device, case):
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    cid, data, bit = case
    with pytest.raises(_lib.NesrBadFileError) as e:
        imgproc.decode_png(data, device=cuda_device, inflate="device")
    assert e.value.status == bit
    good = FOREIGN[30]
    assert _equal(imgproc.decode_png(good[1], device=cuda_device, inflate="device"), good[2], "rgb")


def test_round_trip_on_the_device(cuda_device):
    from neural_enhanced_super_resolution_amd import frame_io, imgproc
    for kind, (h, w), (c, depth) in [("impulses", (70, 320), (3, 8)), ("runs", (33, 130), (4, 16)), ("gradient", (300, 257), (1, 16))]:
        img = png_cases.content(kind, h, w, c, depth)
        frame = frame_io.frame_to_tensor(np.ascontiguousarray(img), cuda_device)
        data = imgproc.encode_png(frame, order="bgr")
        back = imgproc.decode_png(data, order="bgr", device=cuda_device)
        assert back.dtype == frame.dtype and torch.equal(back, frame)


def test_long_groups_cross_bands(cuda_device):
    """More rows than one band of the unfilter's wavefront in one group (every row Paeth, Average or Up), wider than a band is tall"""
    from neural_enhanced_super_resolution_amd import imgproc
    import zlib
    for c, depth in [(3, 8), (4, 16)]:
        frame = png_cases.content("impulses", 600, 37, c, depth)
        raw_types = 2 + np.arange(600) % 3                    # rows 1 .. 599 depend on the row above: one group of 600 rows
        full = np.stack([cases.filtered_cycle(frame, first=t) for t in range(5)])       # [5][H][row]: row y of full[t] has type (t + y) % 5
        pick = (raw_types - np.arange(600)) % 5
        filt = full[pick, np.arange(600)]
        assert np.array_equal(filt[:, 0], raw_types)
        data = cases.make_file(600, 37, c, depth, [zlib.compress(filt.tobytes(), 6)])
        assert np.array_equal(ref.decode(data), frame)
        assert _equal(imgproc.decode_png(data, device=cuda_device), frame, "rgb")


# ------------------------------------------------------------------------------------------------ wrappers
def _wrapper(device, **kw):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=1)
    return RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=1), half=False, device=device, tile=0,
                        tile_pad=10, pre_pad=0, **kw)


def _frames(h, w, seed):
    """B G R (A) / gray frames at 8 and 16 bit, and a 16-bit frame so dark (max <= 256) that enhance() takes it for 8-bit range"""
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    bgr = synthetic_frame(h, w, seed=seed)
    bgra = np.concatenate([bgr, synthetic_frame(h, w, seed=seed + 100, channels=0)[:, :, None]], 2)
    gray = np.ascontiguousarray(bgr[:, :, 1])
    wide = lambda x: x.astype(np.uint16) * 251       # noqa: E731
    return {"bgr8": bgr, "gray8": gray, "bgra8": bgra, "gray16": wide(gray), "bgr16": wide(bgr), "bgra16": wide(bgra), "dark16": bgr.astype(np.uint16)}


def _png_of(img):
    """A foreign one-stream PNG file of a B G R (A) / gray frame (forced filter cycle, zlib level 6)"""
    import zlib
    rgb = png_cases.file_order(img, "bgr")
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    return cases.make_file(h, w, c, 8 * img.dtype.itemsize, [zlib.compress(cases.filtered_cycle(rgb).tobytes(), 6)])


def test_enhance_image_file_is_enhance_of_the_decoded_frame(cuda_device, golden_dir):
    import os
    from tests import png_ref
    up = _wrapper(cuda_device)
    for name, img in _frames(24, 20, seed=41).items():
        for data in (_png_of(img), png_ref.encode_png(img, "bgr")):         # one stream (hybrid) and our own segments (all-device)
            assert np.array_equal(png_cases.file_order(ref.decode(data), "bgr"), img), name
            want, mode = up.enhance(img)
            got, gmode = up.enhance_image_file(data)
            assert gmode == mode and got.dtype == want.dtype and np.array_equal(got, want), name
            assert want.dtype == (np.uint8 if name == "dark16" else img.dtype)
        file_bytes, fmode = up.enhance_image_file_to(data)
        assert (file_bytes, fmode) == up.enhance_png(img), name
    with open(os.path.join(golden_dir, "jpeg", "impulses_37x53x3_q95.jpg"), "rb") as f:
        jpeg = f.read()
    frame, mode = up.enhance_image_file(jpeg)
    assert mode == "RGB" and np.array_equal(frame, up.enhance_file(jpeg)[0])
    assert up.enhance_image_file_to(jpeg) == up.enhance_file_jpeg(jpeg)
    assert up.enhance_image_file_to(jpeg, fmt="png") == up.enhance_file_png(jpeg)
    bgr8 = _frames(24, 20, seed=41)["bgr8"]
    assert up.enhance_image_file_to(_png_of(bgr8), fmt="jpeg", quality=80) == up.enhance_jpeg(bgr8, quality=80)
    for name in ("bgra8", "gray16"):
        with pytest.raises(ValueError):
            up.enhance_image_file_to(_png_of(_frames(24, 20, seed=41)[name]), fmt="jpeg")
    with pytest.raises(ValueError):
        up.enhance_image_file(b"GIF89a" + bytes(32))
    with pytest.raises(ValueError, match="enhance_file"):
        up.enhance_file(_png_of(bgr8))                                     # enhance_file* stay JPEG-only


def test_enhance_iterations_takes_png_bytes(cuda_device):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, imgproc
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=6, num_in_ch=12, scale=4, num_block=1)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(12, 3, num_block=1), tile=0, tile_pad=0, pre_pad=0, half=False,
                      device=cuda_device)
    cfg = {"iterations": 1, "upscale_factor": 2.0}
    frames = _frames(12, 20, seed=43)
    for name in ("bgr8", "gray8", "bgra8"):
        data = _png_of(frames[name])
        t = imgproc.decode_png(data, order="rgb", device=cuda_device)
        t = t[:, :, None].expand(-1, -1, 3).contiguous() if t.dim() == 2 else t[:, :, :3].contiguous()
        assert np.array_equal(A.enhance_iterations(up, data, cfg, "cuda"), A.enhance_iterations(up, t, cfg, "cuda")), name
    with pytest.raises(ValueError, match="16-bit"):
        A.enhance_iterations(up, _png_of(frames["bgr16"]), cfg, "cuda")
