"""GPU: the PNG encoder's kernels (csrc/png.hip through imgproc.encode_png and nesr_png_encode) against the specification
(tests/png_ref.py; tests/test_png_spec.py shows that standard decoders return the frame from its bytes and that the grid of
tests/png_cases.py takes every path of the coder).  On the grid every criterion is byte equality; beyond the specification's reach
(frames it would take too long to encode in numpy) the criteria are the contract itself: the file decodes to the frame bit for bit,
and it is not larger than the file of cv2's settings."""
import ctypes
import io

import numpy as np
import pytest
import torch

from tests import png_cases, png_ref

pytestmark = pytest.mark.gpu
CASES = png_cases.cases()


def _first_difference(got, want):
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return f"{len(got)} bytes against {len(want)}, first difference at byte {at}"


def _on_device(img, device):
    from neural_enhanced_super_resolution_amd import frame_io
    return frame_io.frame_to_tensor(np.ascontiguousarray(img), device)      # uint8, or int16 carrying the uint16 pattern


# ------------------------------------------------------------------------------------------------ bytes
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_bytes_equal_the_specification(cuda_device, case):
    from neural_enhanced_super_resolution_amd import imgproc
    _, kind, h, w, c, depth = case
    img, order = png_cases.image(kind, h, w, c, depth)
    other = "bgr" if order == "rgb" else "rgb"
    want = png_cases.spec(kind, h, w, c, depth)[0]
    frame = _on_device(img, cuda_device)
    got = imgproc.encode_png(frame, order=order)
    assert got == want, _first_difference(got, want)
    assert imgproc.encode_png(frame, order=order) == got, "the same call twice"
    # a window of a larger frame: rows 3 .. 3 + h, columns 5 .. 5 + w of a frame filled with another value
    big = torch.full((h + 7, w + 11) + ((c,) if c > 1 else ()), 101, dtype=frame.dtype, device=cuda_device)
    big[3:3 + h, 5:5 + w] = frame
    window = big[3:3 + h, 5:5 + w]
    assert not window.is_contiguous() or h == 1
    assert imgproc.encode_png(window, order=order) == want, "row-strided window"
    if c >= 3:          # the other channel order on the flipped frame is the same picture
        flipped = torch.cat([frame[:, :, :3].flip(2), frame[:, :, 3:]], dim=2)
        assert imgproc.encode_png(flipped, order=other) == want, other
    else:
        assert imgproc.encode_png(frame[:, :, None], order=other) == want, "[H, W, 1], and the order does not matter"
    if depth == 16 and hasattr(torch, "uint16"):
        assert imgproc.encode_png(frame.view(torch.uint16), order=order) == want, "torch.uint16"


def _synthetic_photo(h, w, c, depth, seed):
    """Photo-like: smooth waves plus fine noise; a band of full noise (stored blocks) and a flat band (long runs)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    top = 65535 if depth == 16 else 255
    planes = []
    for k in range(c):
        p = 0.5 + 0.25 * np.sin(x / (37.0 + 11 * k) + y / 53.0) + 0.2 * np.cos(y / (29.0 + 7 * k) - x / 71.0)
        planes.append(p + rng.normal(0, 0.01, (h, w)).astype(np.float32))
    img = (np.clip(np.stack(planes, -1), 0, 1) * top).astype(np.uint16 if depth == 16 else np.uint8)
    img[h // 3:h // 3 + h // 8] = rng.randint(0, top + 1, (h // 8, w, c)).astype(img.dtype)
    img[2 * h // 3:2 * h // 3 + h // 8] = top // 3
    return img[:, :, 0] if c == 1 else img


@pytest.mark.parametrize("shape", [(1080, 1920, 3, 8), (2160, 3840, 1, 16)], ids=["1080p-rgb8", "2160p-gray16"])
def test_beyond_the_specifications_reach(cuda_device, shape):
    """1080 x 1920 RGB: 190 chunks.  2160 x 3840 gray 16 bit: 507 chunks.  The chunk-size scan (csrc/png.hip png_scan64) takes 1024
    entries per step, so neither crosses a step; the smallest frames that do have more than 1024 x 32768 filtered bytes, and
    test_scan_carries_across_a_step below encodes one of them."""
    from neural_enhanced_super_resolution_amd import imgproc
    h, w, c, depth = shape
    img = _synthetic_photo(h, w, c, depth, seed=h)
    data = imgproc.encode_png(_on_device(img, cuda_device))
    assert png_ref.refilter_matches(data, img), "the stdlib decoder (zlib, every CRC, the layout) does not return the frame"
    types = png_ref.decode_png(data, full=False)[0][:, 0]
    assert len(set(types.tolist())) >= 2                            # the adaptive filter chose among the types
    host = imgproc.encode_png(img)
    print(f"{shape}: device route {len(data)} bytes, cv2's settings {len(host)} bytes, raw {img.nbytes}")
    assert len(data) <= len(host)
    try:
        from PIL import Image
        got = np.asarray(Image.open(io.BytesIO(data)))
        assert np.array_equal(got.astype(img.dtype), img), "Pillow"
    except ImportError:
        pass


def test_scan_carries_across_a_step(cuda_device):
    """gray 8 bit 4097 x 8191: 4097 x 8192 filtered bytes = 1025 chunks, one more than a step of the chunk-size scan."""
    from neural_enhanced_super_resolution_amd import imgproc
    h, w = 4097, 8191
    img = np.full((h, w), 9, np.uint8)
    img[::64, ::5] = (np.arange(len(range(0, w, 5))) % 251).astype(np.uint8)[None, :]       # some literals among the runs
    img[4096, 4000:] = 200                                                         # and the last chunk differs
    data = imgproc.encode_png(_on_device(img, cuda_device))
    assert len(png_ref.read_chunks(data)) == 4 + 1025
    assert png_ref.refilter_matches(data, img)
    assert len(data) <= len(imgproc.encode_png(img))


# ------------------------------------------------------------------------------------------------ capacity
def _encode_raw(frame, depth, cap, guard=256):
    """nesr_png_encode into a buffer of cap + guard bytes filled with 0xA5 -> (length word, status word, the buffer)."""
    from neural_enhanced_super_resolution_amd import _lib
    from neural_enhanced_super_resolution_amd._contexts import device_call
    h, w, c = frame.shape
    need = _lib.load().nesr_png_scratch_bytes(h, w, c, depth)
    scratch = torch.empty(need, dtype=torch.uint8, device=frame.device)
    out = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device=frame.device)
    words = torch.full((2,), -1, dtype=torch.int64, device=frame.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    device_call("nesr_png_encode", frame.device, p(frame), w * c * depth // 8, h, w, c, depth, _lib.ORDER_RGB, p(scratch), need, p(out), cap, p(words))
    length, status = (int(v) for v in words.cpu())
    return length, status, out.cpu().numpy()


@pytest.mark.parametrize("case", [("noise", 37, 53, 3, 8), ("runs", 70, 320, 3, 8), ("gradient", 33, 130, 4, 16), ("noise", 1, 1, 1, 8)],
                         ids=["37x53-noise", "70x320-runs", "33x130x4x16-gradient", "1x1"])
def test_capacity(cuda_device, case):
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    kind, h, w, c, depth = case
    img = png_cases.content(kind, h, w, c, depth)
    want = png_cases.spec(kind, h, w, c, depth)[0]
    frame = _on_device(img.reshape(h, w, c), cuda_device)
    # it fits exactly: the whole file, nothing behind it
    length, status, buf = _encode_raw(frame, depth, len(want))
    assert (length, status) == (len(want), 0) and buf[:length].tobytes() == want and (buf[length:] == 0xA5).all()
    # the bound always fits
    length, status, buf = _encode_raw(frame, depth, png_ref.bound(h, w, c, depth))
    assert (length, status) == (len(want), 0) and buf[:length].tobytes() == want and (buf[length:] == 0xA5).all()
    # one byte short (inside IEND), inside the Adler IDAT, inside a chunk (at each alignment of its end), inside the head, one byte
    caps = [len(want) - 1, len(want) - 2, len(want) - 13, len(want) - 20, len(want) - 29, len(want) - 30, len(want) - 31, len(want) - 32,
            60, 49, 48, 47, 46, 20, 1]
    for cap in caps:
        if not 0 < cap < len(want):
            continue
        length, status, buf = _encode_raw(frame, depth, cap)
        assert (length, status) == (len(want), 1), cap
        assert buf[:cap].tobytes() == want[:cap], cap
        assert (buf[cap:] == 0xA5).all(), cap
    with pytest.raises(_lib.NesrNoFitError) as e:
        imgproc._png_encode_hip(frame, depth, False, len(want) - 1)
    assert e.value.needed == len(want)


# ------------------------------------------------------------------------------------------------ wrappers
def _wrapper(device, **kw):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=2)
    return RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=2), half=False, device=device, **kw)


def _frames(h, w, seed):
    """gray, BGR and BGRA at 8 and 16 bit (16-bit samples: 8-bit noise times an odd factor, not all multiples of 257)"""
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    bgr = synthetic_frame(h, w, seed=seed)
    bgra = np.concatenate([bgr, synthetic_frame(h, w, seed=seed + 100, channels=0)[:, :, None]], 2)
    gray = np.ascontiguousarray(bgr[:, :, 1])
    wide = lambda x: x.astype(np.uint16) * 251       # noqa: E731
    return {"gray8": gray, "bgr8": bgr, "bgra8": bgra, "gray16": wide(gray), "bgr16": wide(bgr), "bgra16": wide(bgra)}


def _assert_file_is(data, frame):
    """`data` decodes to `frame` (B G R (A) or gray, as enhance() returns it) bit for bit"""
    assert png_ref.refilter_matches(data, frame, "bgr")
    filt, (h, w, c, depth) = png_ref.decode_png(data, full=False)
    assert (h, w) == frame.shape[:2] and c == (1 if frame.ndim == 2 else frame.shape[2]) and depth == 8 * frame.dtype.itemsize


@pytest.mark.parametrize("tile", [0, 32])
def test_enhance_png_is_the_file_of_enhance(cuda_device, tile):
    up = _wrapper(cuda_device, tile=tile, tile_pad=10, pre_pad=0)
    for name, img in _frames(40, 56, seed=31).items():
        for kw in ({}, {"outscale": 1.5}):
            before, mode = up.enhance(img, **kw)
            data, pmode = up.enhance_png(img, **kw)
            after, _ = up.enhance(img, **kw)
            assert pmode == mode == {1: "L", 3: "RGB", 4: "RGBA"}[1 if img.ndim == 2 else img.shape[2]], name
            assert before.shape[:2] == ((60, 84) if kw else (80, 112)) and before.dtype == img.dtype and before.std() > 0, name
            assert np.array_equal(before, after), name
            _assert_file_is(data, before)
            assert data == png_ref.encode_png(before, "bgr"), (name, kw)       # and the specification's bytes for that frame


def test_only_the_file_comes_home(cuda_device, monkeypatch):
    from neural_enhanced_super_resolution_amd import realesrganer as R
    up = _wrapper(cuda_device, tile=0, tile_pad=10, pre_pad=0)
    frames = _frames(40, 56, seed=32)
    copies = []
    real = R.RealESRGANer._frame_to_host
    monkeypatch.setattr(R.RealESRGANer, "_frame_to_host", staticmethod(lambda t, host=None: copies.append(tuple(t.shape)) or real(t, host)))
    for name in ("bgr8", "bgra16", "gray16"):
        del copies[:]
        out, _ = up.enhance(frames[name])
        assert len(copies) == 1, name
        del copies[:]
        data, _ = up.enhance_png(frames[name])
        assert copies == [], "enhance_png brings the file home, not the frame"
        _assert_file_is(data, out)


def test_enhance_png_refusals(cuda_device):
    up = _wrapper(cuda_device, tile=0, tile_pad=10, pre_pad=0)
    bgr = _frames(16, 16, seed=33)["bgr8"]
    for bad in (bgr[:, :, :2], np.concatenate([bgr, bgr[:, :, :2]], 2), bgr[None], [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match="enhance_png"):
            up.enhance_png(bad)
    assert up.model.calls == 0


def test_enhance_file_png(cuda_device, golden_dir):
    import glob
    import os
    up = _wrapper(cuda_device, tile=0, tile_pad=10, pre_pad=0)
    path = sorted(glob.glob(os.path.join(golden_dir, "jpeg", "impulses_37x53x3_q95.jpg")))[0]
    with open(path, "rb") as f:
        jpeg = f.read()
    frame, mode = up.enhance_file(jpeg)
    data, pmode = up.enhance_file_png(jpeg)
    assert mode == pmode == "RGB" and frame.shape == (74, 106, 3)
    _assert_file_is(data, frame)
    from neural_enhanced_super_resolution_amd import imgproc
    decoded = imgproc.decode_jpeg_u8(jpeg, order="bgr", device=cuda_device).cpu().numpy()
    assert data == up.enhance_png(decoded)[0] == up.enhance_file_png(path)[0]
    with pytest.raises(ValueError, match="enhance_file_png"):
        up.enhance_file_png(data)                                                # a PNG file is not decoded on the device


def test_enhance_iterations_png_and_intermediates(cuda_device):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=6, num_in_ch=12, scale=4, num_block=2)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(12, 3, num_block=2), tile=0, tile_pad=0, pre_pad=0, half=False,
                      device=cuda_device)
    img = synthetic_frame(12, 20, seed=8)[:, :, ::-1].copy()
    cfg = {"iterations": 2, "upscale_factor": 2.0}      # untiled 12-channel route: the network's x4 per iteration
    t0, t1 = [], []
    frame = A.enhance_iterations(up, img, cfg, "cuda", trace=t0)
    assert frame.shape == (192, 320, 3)
    data = A.enhance_iterations(up, img, cfg, "cuda", trace=t1, png=True)
    assert isinstance(data, bytes) and t0 == t1
    assert png_ref.refilter_matches(data, frame, "rgb") and data == png_ref.encode_png(frame, "rgb")
    # intermediates: one file per iteration when the configuration asks, each that iteration's frame = the next iteration's input
    files = []
    again = A.enhance_iterations(up, img, dict(cfg, intermediate_saves=True), "cuda", intermediates=files)
    assert np.array_equal(again, frame) and len(files) == 2
    first = A.enhance_iterations(up, img, dict(cfg, iterations=1), "cuda")
    assert first.shape == (48, 80, 3)
    assert png_ref.refilter_matches(files[0], first, "rgb") and png_ref.refilter_matches(files[1], frame, "rgb")
    assert np.array_equal(A.enhance_iterations(up, first, dict(cfg, iterations=1), "cuda"), frame)
    none = []
    A.enhance_iterations(up, img, cfg, "cuda", intermediates=none)                 # not configured: nothing is saved
    A.enhance_iterations(up, img, dict(cfg, intermediate_saves=False), "cuda", intermediates=none)
    assert none == []
    both = []
    assert A.enhance_iterations(up, img, dict(cfg, intermediate_saves=True), "cuda", png=True, intermediates=both) == data and both == files
    with pytest.raises(ValueError):
        A.enhance_iterations(up, img, cfg, "cuda", png=True, encode="jpeg")
    with pytest.raises(ValueError):
        A.enhance_iterations(up, img, cfg, "cuda", encode="png")
    # the no-model configuration ends in the same encode
    plain = A.enhance_iterations(None, img, {"iterations": 1, "upscale_factor": 2.0}, device=cuda_device)
    assert A.enhance_iterations(None, img, {"iterations": 1, "upscale_factor": 2.0}, device=cuda_device, png=True) == png_ref.encode_png(plain, "rgb")
