"""GPU: the JPEG encoder's kernels (csrc/jpeg.hip through imgproc.encode_jpeg_u8 and nesr_jpeg_encode_u8) against the specification
(tests/jpeg_ref.py, pinned to libjpeg-turbo in tests/test_jpeg_spec.py).  Every criterion is byte equality.  The grid is
tests/jpeg_cases.py's: the smallest frames, each dummy-block and padding rule, and three shapes that cross the kernels' strip,
workgroup and scan-chunk boundaries at least twice (named there); tests/test_jpeg_spec.py proves from the specification's
counters that the grid takes every path of the entropy coder."""
import ctypes

import numpy as np
import pytest
import torch

from tests import jpeg_cases, jpeg_ref

pytestmark = pytest.mark.gpu
CASES = jpeg_cases.cases()


def _first_difference(got, want):
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return f"{len(got)} bytes against {len(want)}, first difference at byte {at}"


# ------------------------------------------------------------------------------------------------ 5: kernel bytes
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_bytes_equal_the_specification(cuda_device, case):
    from neural_enhanced_super_resolution_amd import imgproc
    _, kind, h, w, c = case
    img, order = jpeg_cases.image(kind, h, w, c)
    other = "bgr" if order == "rgb" else "rgb"
    frame = torch.from_numpy(img).to(cuda_device)
    # a window of a larger frame: rows 3 .. 3 + h, columns 5 .. 5 + w of a frame filled with another value
    big = torch.full((h + 7, w + 11) + ((3,) if c == 3 else ()), 201, dtype=torch.uint8, device=cuda_device)
    big[3:3 + h, 5:5 + w] = frame
    window = big[3:3 + h, 5:5 + w]
    assert not window.is_contiguous() or h == 1
    for q in jpeg_cases.QUALITIES:
        want = jpeg_cases.spec(kind, h, w, c, q)[0]
        got = imgproc.encode_jpeg_u8(frame, q, order=order)
        assert got == want, (q, _first_difference(got, want))
        assert imgproc.encode_jpeg_u8(frame, q, order=order) == got, "the same call twice"
        assert imgproc.encode_jpeg_u8(window, q, order=order) == want, (q, "row-strided window")
        if c == 3:      # the other channel order on the flipped frame is the same picture
            assert imgproc.encode_jpeg_u8(frame.flip(2), q, order=other) == want, (q, other)
            assert imgproc.encode_jpeg_u8(window.flip(2), q, order=other) == want, (q, other, "flipped copy of the window")
        else:
            assert imgproc.encode_jpeg_u8(frame[:, :, None], q) == want, (q, "[H, W, 1]")


def test_host_route_and_refusals(cuda_device):
    from neural_enhanced_super_resolution_amd import imgproc
    frame = torch.from_numpy(jpeg_cases.content("impulses", 37, 53, 3)).to(cuda_device)
    want = jpeg_cases.spec("impulses", 37, 53, 3, 95)[0]
    assert imgproc.encode_jpeg_u8(frame) == want
    try:
        import PIL  # noqa: F401
        assert imgproc.encode_jpeg_u8(frame, use_hip=False) == want                 # Pillow on a copy of the frame
    except ImportError:
        with pytest.raises(RuntimeError, match="Pillow"):
            imgproc.encode_jpeg_u8(frame, use_hip=False)
    with pytest.raises(ValueError):
        imgproc.encode_jpeg_u8(frame.to(torch.int32))
    with pytest.raises(ValueError):
        imgproc.encode_jpeg_u8(frame.cpu(), use_hip=True)


def test_scan_tiles_and_sizes_beyond_the_specifications_reach(cuda_device):
    """4752 x 4752 noise: 529 254 blocks = 2068 chunks of the bit-offset scan and over 4000 chunks of the stuffing scan, so both
    single-workgroup scans (1024 entries per step, csrc/jpeg.hip jpeg_scan64) carry across two step boundaries -- a path no frame
    the numpy specification encodes in a test's time can reach.  The reference here is Pillow's libjpeg-turbo itself, which
    tests/test_jpeg_spec.py shows the specification equals."""
    pytest.importorskip("PIL")
    from neural_enhanced_super_resolution_amd import imgproc
    from tests.make_jpeg_golden import pillow_bytes
    g = torch.Generator(device="cpu").manual_seed(11)
    img = torch.randint(0, 256, (4752, 4752, 3), dtype=torch.uint8, generator=g)
    want = pillow_bytes(img.numpy(), 95)
    assert len(want) - 623 > 2048 * 4096
    got = imgproc.encode_jpeg_u8(img.to(cuda_device), 95)
    assert got == want, _first_difference(got, want)


# ------------------------------------------------------------------------------------------------ 6: capacity
def _encode_raw(frame, quality, cap, guard=256):
    """nesr_jpeg_encode_u8 into a buffer of cap + guard bytes filled with 0xA5 -> (length word, status word, the buffer)."""
    from neural_enhanced_super_resolution_amd import _lib
    from neural_enhanced_super_resolution_amd._contexts import device_call
    h, w, c = frame.shape
    need = _lib.load().nesr_jpeg_scratch_bytes(h, w, c)
    scratch = torch.empty(need, dtype=torch.uint8, device=frame.device)
    out = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device=frame.device)
    words = torch.full((2,), -1, dtype=torch.int64, device=frame.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    device_call("nesr_jpeg_encode_u8", frame.device, p(frame), w * c, h, w, c, _lib.ORDER_RGB, quality, p(scratch), need, p(out), cap, p(words))
    length, status = (int(v) for v in words.cpu())
    return length, status, out.cpu().numpy()


@pytest.mark.parametrize("shape", [(37, 53, 3), (200, 333, 3), (9, 17, 1)])
def test_capacity(cuda_device, shape, monkeypatch):
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    h, w, c = shape
    img = jpeg_cases.content("noise", h, w, c)
    want = jpeg_cases.spec("noise", h, w, c, 100)[0]
    frame = torch.from_numpy(img.reshape(h, w, c)).to(cuda_device)
    # it fits exactly: the whole file, nothing behind it
    length, status, buf = _encode_raw(frame, 100, len(want))
    assert (length, status) == (len(want), 0) and buf[:length].tobytes() == want and (buf[length:] == 0xA5).all()
    # one byte short, and far too short (inside the header; inside the scan): the full size, "did not fit", the first out_cap bytes, an untouched guard
    for cap in (len(want) - 1, len(want) - 2, 100, min(700, len(want) - 3), 1):
        length, status, buf = _encode_raw(frame, 100, cap)
        assert (length, status) == (len(want), 1), cap
        assert buf[:cap].tobytes() == want[:cap], cap
        assert (buf[cap:] == 0xA5).all(), cap
    # the wrapper: a first buffer that is too small (noise at quality 100 needs more than H W C / 2 + 4096 at 200 x 333), one more run
    runs = []
    real = imgproc._jpeg_encode_hip
    monkeypatch.setattr(imgproc, "_jpeg_encode_hip", lambda f, q, bgr, cap: runs.append(cap) or real(f, q, bgr, cap))
    assert imgproc.encode_jpeg_u8(frame, 100) == want
    first = h * w * c // 2 + 4096
    assert runs == ([first] if len(want) <= first else [first, len(want)])
    if shape == (200, 333, 3):
        assert len(runs) == 2
    with pytest.raises(_lib.NesrNoFitError) as e:
        real(frame, 100, False, len(want) - 1)
    assert e.value.needed == len(want)


# ------------------------------------------------------------------------------------------------ 7: wrappers
def _wrapper(device, **kw):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=2)
    return RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=2), half=False, device=device, **kw)


@pytest.mark.parametrize("tile,pre_pad", [(0, 0), (32, 10)])
def test_enhance_jpeg_is_the_file_of_enhance(cuda_device, tile, pre_pad):
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    up = _wrapper(cuda_device, tile=tile, tile_pad=10, pre_pad=pre_pad)
    bgr = synthetic_frame(40, 56, seed=21)
    for img in (bgr, np.ascontiguousarray(bgr[:, :, 1])):
        for kw in ({}, {"outscale": 1.5}):
            before, mode = up.enhance(img, **kw)
            data, jmode = up.enhance_jpeg(img, **kw)
            after, _ = up.enhance(img, **kw)
            assert jmode == mode == ("RGB" if img.ndim == 3 else "L")
            assert before.shape[:2] == ((60, 84) if kw else (80, 112)) and before.std() > 0
            assert np.array_equal(before, after)
            assert data == jpeg_ref.encode_jpeg(before, 95, order="bgr"), (img.shape, kw)
        assert up.enhance_jpeg(img, quality=30)[0] == jpeg_ref.encode_jpeg(up.enhance(img)[0], 30, order="bgr")


def test_enhance_leaves_the_frame_it_left_before(cuda_device, monkeypatch):
    """enhance() with the routes called as the parent called them (no `keep` argument reaches them) and one copy home."""
    from neural_enhanced_super_resolution_amd import realesrganer as R
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    up = _wrapper(cuda_device, tile=0, tile_pad=10, pre_pad=0)
    img = synthetic_frame(40, 56, seed=22)
    copies = []
    real = R.RealESRGANer._frame_to_host
    monkeypatch.setattr(R.RealESRGANer, "_frame_to_host", staticmethod(lambda t, host=None: copies.append(tuple(t.shape)) or real(t, host)))
    out, _ = up.enhance(img)
    assert copies == [(80, 112, 3)]
    want = up.model.forward_u8(torch.from_numpy(img).to(cuda_device), flip_rgb=True, round_nearest=True).cpu().numpy()
    assert np.array_equal(out, want)
    del copies[:]
    data, _ = up.enhance_jpeg(img)
    assert copies == [], "enhance_jpeg brings the file home, not the frame"
    assert data == jpeg_ref.encode_jpeg(out, 95, order="bgr")


def test_enhance_jpeg_refuses_alpha_and_16_bit(cuda_device):
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    up = _wrapper(cuda_device, tile=0, tile_pad=10, pre_pad=0)
    bgr = synthetic_frame(16, 16, seed=23)
    for bad in (np.concatenate([bgr, bgr[:, :, :1]], 2), bgr.astype(np.uint16) * 251, bgr[:, :, 0].astype(np.uint16) * 251):
        with pytest.raises(ValueError, match="enhance_jpeg"):
            up.enhance_jpeg(bad)
    assert up.model.calls == 0


def test_enhance_iterations_encode(cuda_device):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=6, num_in_ch=12, scale=4, num_block=2)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(12, 3, num_block=2), tile=0, tile_pad=0, pre_pad=0, half=False,
                      device=cuda_device)
    img = synthetic_frame(12, 20, seed=8)[:, :, ::-1].copy()
    cfg = {"iterations": 2, "upscale_factor": 2.0}      # untiled 12-channel route: the network's x4 per iteration
    t0, t1, t2 = [], [], []
    frame = A.enhance_iterations(up, img, cfg, "cuda", trace=t0)
    assert isinstance(frame, np.ndarray) and frame.shape == (192, 320, 3) and frame.std() > 0
    data = A.enhance_iterations(up, img, cfg, "cuda", trace=t1, encode="jpeg")
    assert isinstance(data, bytes) and data == jpeg_ref.encode_jpeg(frame, 95, order="rgb")
    assert A.enhance_iterations(up, img, cfg, "cuda", trace=t2, encode=("jpeg", 30)) == jpeg_ref.encode_jpeg(frame, 30, order="rgb")
    assert t0 == t1 == t2 and len(t0) == 2
    assert np.array_equal(A.enhance_iterations(up, img, cfg, "cuda"), frame)
    assert np.array_equal(A.enhance_iterations(up, img, cfg, "cuda", encode=None), frame)
    with pytest.raises(ValueError):
        A.enhance_iterations(up, img, cfg, "cuda", encode="png")
    # the filtered loop and the no-model configuration end in the same encode
    plain = A.enhance_iterations(None, img, {"iterations": 1, "upscale_factor": 2.0}, device=cuda_device)
    assert A.enhance_iterations(None, img, {"iterations": 1, "upscale_factor": 2.0}, device=cuda_device, encode="jpeg") == \
        jpeg_ref.encode_jpeg(plain, 95, order="rgb")
