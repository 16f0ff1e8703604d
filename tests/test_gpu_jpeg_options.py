"""GPU: the JPEG encoder's options (4:4:4 / 4:2:2, optimised Huffman tables, restart intervals: csrc/jpeg.hip through
imgproc.encode_jpeg_u8 and nesr_jpeg_encode_ex_u8) against the specification (tests/jpeg_options_ref.py, pinned to libjpeg-turbo in
tests/test_jpeg_options_spec.py).  Every criterion on a file is byte equality."""
import ctypes
import hashlib
import json

import numpy as np
import pytest
import torch

from tests import jpeg_cases, jpeg_decode_ref
from tests import jpeg_options_cases as cases
from tests import jpeg_options_ref as ref

pytestmark = pytest.mark.gpu
IMAGES = [(k, h, w) for (h, w) in cases.SHAPES for k in cases.CONTENTS]


def _first_difference(got, want):
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return f"{len(got)} bytes against {len(want)}, first difference at byte {at}"


def _dht(data):
    """The DHT segments of a file up to SOS: [(tc_th, BITS, HUFFVAL)] in file order."""
    out, at = [], 2
    while data[at + 1] != 0xDA:
        length = int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] == 0xC4:
            seg = data[at + 4:at + 2 + length]
            while seg:
                n = sum(seg[1:17])
                out.append((seg[0], list(seg[1:17]), list(seg[17:17 + n])))
                seg = seg[17 + n:]
        at += 2 + length
    return out


def _explain(got, want, tables):
    """Why two optimised files differ: the first table whose BITS / HUFFVAL is not the specification's, else the first byte."""
    try:
        for (tc_th, bits, vals), (wbits, wvals) in zip(_dht(got), tables):
            if (bits, vals) != (wbits, wvals):
                return f"table {tc_th:#04x}: BITS {bits} HUFFVAL {vals[:16]}... against BITS {wbits} HUFFVAL {wvals[:16]}..."
    except (IndexError, ValueError):
        pass
    return _first_difference(got, want)


# ------------------------------------------------------------------------------------------------ 1: the grid
@pytest.mark.parametrize("image", IMAGES, ids=[f"{k}_{h}x{w}" for k, h, w in IMAGES])
def test_kernel_bytes_equal_the_specification(cuda_device, image):
    from neural_enhanced_super_resolution_amd import imgproc
    kind, h, w = image
    for layout in cases.LAYOUTS:
        img = cases.image(kind, h, w, layout)
        frame = torch.from_numpy(img).to(cuda_device)
        big = torch.full((h + 7, w + 11) + ((3,) if img.ndim == 3 else ()), 201, dtype=torch.uint8, device=cuda_device)
        big[3:3 + h, 5:5 + w] = frame
        window = big[3:3 + h, 5:5 + w]
        flipped = window.flip(2) if img.ndim == 3 else None
        for f in cases.files():
            if f[:4] != (kind, h, w, layout):
                continue
            _, _, _, _, q, opt, ri = f
            want, st = cases.spec(*f)
            kw = dict(sampling="4:2:2" if layout == "gray" else layout, optimize=opt, restart_interval=ri)      # gray ignores sampling
            got = imgproc.encode_jpeg_u8(frame, q, **kw)
            assert got == want, (cases.file_id(f), _explain(got, want, st["tables"]))
            assert imgproc.encode_jpeg_u8(window, q, **kw) == want, (cases.file_id(f), "row-strided window")
            if flipped is not None:
                assert imgproc.encode_jpeg_u8(flipped, q, order="bgr", **kw) == want, (cases.file_id(f), "bgr")


# ------------------------------------------------------------------------------------------------ 2: the kernels' own constants
def _noise(h, w, c, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3) if c == 3 else (h, w)).astype(np.uint8)


# 256 blocks per workgroup of the length / emit / histogram / interval passes, 1024 entries per step of the scans, 64 lanes,
# 4096 unstuffed bytes per chunk of the stuffing pass (csrc/jpeg.hip, csrc/jpeg_kernels.h)
BOUNDARY = {
    "444_ri5": dict(img=lambda: _noise(96, 1024, 3, 1), sampling="4:4:4", optimize=False, ri=5),
    "gray_ri1": dict(img=lambda: _noise(24, 1600, 1, 2), sampling="4:2:0", optimize=True, ri=1),
    "gray_ri1_scan_steps": dict(img=lambda: _noise(40, 4200, 1, 3), sampling="4:2:0", optimize=False, ri=1),
    "422_ri_row": dict(img=lambda: _noise(96, 1024, 3, 4), sampling="4:2:2", optimize=True, ri=64),
    "constant_optimised": dict(img=lambda: np.full((96, 1024, 3), 77, np.uint8), sampling="4:2:0", optimize=True, ri=0),
    "ff_interval_start_ends_a_chunk": dict(img=cases.ff_interval_start_image, sampling="4:2:0", optimize=False, ri=1, quality=100),
    "ri_beyond_the_frame": dict(img=lambda: _noise(37, 53, 3, 5), sampling="4:2:0", optimize=False, ri=65535),
}


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_files_that_cross_the_kernels_constants(cuda_device, name):
    from neural_enhanced_super_resolution_amd import imgproc
    case = BOUNDARY[name]
    img = case["img"]()
    quality = case.get("quality", 95)
    want, st = ref.encode_jpeg_stats(img, quality, "rgb", case["sampling"], case["optimize"], case["ri"])
    nint, blocks = st["intervals"], st["blocks"]
    if name == "444_ri5":
        # 1536 MCUs of 3 blocks: 308 intervals of 15 blocks over 18 workgroups of 256 blocks, and 256 is no multiple of 15
        assert (blocks, nint) == (4608, 308) and nint > 4 * 64 and 256 % 15 != 0 and st["markers_wrapped"] > 0
        assert len(want) - st["header_bytes"] > 2 * 4096
    elif name == "gray_ri1":
        assert (blocks, nint) == (600, 600) and st["markers_wrapped"] >= 590
    elif name == "gray_ri1_scan_steps":
        assert nint == 2625 and nint > 2 * 1024, "the interval scan carries across two of its 1024-entry steps"
    elif name == "422_ri_row":
        assert (blocks, nint) == (12 * 64 * 4, 12) and 256 % (64 * 4) == 0      # an interval is exactly one workgroup: boundaries coincide
    elif name == "constant_optimised":
        # One-symbol tables give 1-bit codes, so a block (DC + EOB) is 2 bits and cannot be less: 16 blocks share each 32-bit
        # stream word, every one of them through atomicOr.  (A hundred blocks per word is out of any Huffman code's reach.)
        assert st["single_symbol_tables"] == 3 and blocks == 6 * 64 * 6
        assert 0 <= (len(want) - st["header_bytes"] - 2) * 8 - 2 * blocks < 32, "2 bits per block but for the first DC differences"
    elif name == "ff_interval_start_ends_a_chunk":
        # FF Dn FF 00 for one stream byte behind 4095 one-byte intervals: the chunk grows beyond three times its size
        grown = cases.chunk_outputs(want, st["header_bytes"])
        assert nint == 8192 and max(grown.values()) == 3 * 4095 + 4 > 3 * 4096, grown
    else:
        assert nint == 1 and st["markers"] == 0 and b"\xff\xdd\x00\x04\xff\xff" in want[:st["header_bytes"]]
    got = imgproc.encode_jpeg_u8(torch.from_numpy(img).to(cuda_device), quality, sampling=case["sampling"], optimize=case["optimize"], restart_interval=case["ri"])
    assert got == want, _explain(got, want, st["tables"])


# ------------------------------------------------------------------------------------------------ 3: the 16-bit length limit
@pytest.mark.parametrize("quality,sampling", cases.LENGTH_LIMIT)
def test_length_limit_frames(cuda_device, quality, sampling):
    from neural_enhanced_super_resolution_amd import imgproc
    with open(cases.length_limit_digest_path()) as fh:
        digest = json.load(fh)[f"q{quality}_{sampling}"]
    want, st = cases.length_limit_spec(quality, sampling)
    assert st["limit_moves"] > 0
    got = imgproc.encode_jpeg_u8(torch.from_numpy(cases.length_limit_image()).to(cuda_device), quality, sampling=sampling, optimize=True)
    for (tc_th, bits, vals), (wbits, wvals) in zip(_dht(got), st["tables"]):
        assert (bits, vals) == (wbits, wvals), f"table {tc_th:#04x}: BITS {bits} against {wbits}; HUFFVAL {vals} against {wvals}"
    assert len(_dht(got)) == 4
    assert (len(got), hashlib.sha256(got).hexdigest()) == (digest["length"], digest["sha256"]), _first_difference(got, want)


# ------------------------------------------------------------------------------------------------ 4: the C entries
def _opts(quality=95, sampling="4:2:0", optimize=False, ri=0):
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.JpegOpts(quality, _lib.JPEG_SAMPLING[sampling], int(optimize), ri)


def _encode_raw(frame, opts, cap, guard=256, order=0):
    """nesr_jpeg_encode_ex_u8 with 0xA5 guards behind out_cap and on both sides of the scratch -> (length, status, out, guards intact)."""
    from neural_enhanced_super_resolution_amd import _lib
    from neural_enhanced_super_resolution_amd._contexts import device_call
    h, w, c = frame.shape
    need = _lib.load().nesr_jpeg_scratch_bytes_ex(h, w, c, ctypes.byref(opts))
    assert need > 0 and need % 256 == 0
    scratch = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=frame.device)
    out = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device=frame.device)
    words = torch.full((2,), -1, dtype=torch.int64, device=frame.device)
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)      # noqa: E731
    assert (scratch.data_ptr() + guard) % 16 == 0
    device_call("nesr_jpeg_encode_ex_u8", frame.device, p(frame), w * c, h, w, c, order, ctypes.byref(opts), p(scratch, guard), need, p(out), cap, p(words))
    length, status = (int(v) for v in words.cpu())
    s = scratch.cpu().numpy()
    return length, status, out.cpu().numpy(), bool((s[:guard] == 0xA5).all() and (s[guard + need:] == 0xA5).all())


def test_default_options_are_the_existing_entry(cuda_device):
    from neural_enhanced_super_resolution_amd import _lib
    from neural_enhanced_super_resolution_amd._contexts import device_call
    lib = _lib.load()
    for kind, h, w, c, q in jpeg_cases.GOLDEN_FILES:
        img, order = jpeg_cases.image(kind, h, w, c)
        order = _lib.ORDER_BGR if order == "bgr" else _lib.ORDER_RGB
        frame = torch.from_numpy(np.ascontiguousarray(img).reshape(h, w, c)).to(cuda_device)
        opts = _opts(q)
        assert lib.nesr_jpeg_scratch_bytes_ex(h, w, c, ctypes.byref(opts)) == lib.nesr_jpeg_scratch_bytes(h, w, c)
        length, status, buf, intact = _encode_raw(frame, opts, 16384, order=order)
        need = lib.nesr_jpeg_scratch_bytes(h, w, c)
        scratch = torch.empty(need, dtype=torch.uint8, device=cuda_device)
        out = torch.full((16384,), 0xA5, dtype=torch.uint8, device=cuda_device)
        words = torch.full((2,), -1, dtype=torch.int64, device=cuda_device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
        device_call("nesr_jpeg_encode_u8", cuda_device, p(frame), w * c, h, w, c, order, q, p(scratch), need, p(out), 16384, p(words))
        assert [int(v) for v in words.cpu()] == [length, 0] and status == 0 and intact
        assert out.cpu().numpy()[:length].tobytes() == buf[:length].tobytes()
        with open(jpeg_cases.golden_path(kind, h, w, c, q), "rb") as fh:
            assert buf[:length].tobytes() == fh.read()


def test_header_and_argument_checks(cuda_device):
    from neural_enhanced_super_resolution_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int(-1)
    for sampling, c in (("4:4:4", 3), ("4:2:2", 3), ("4:2:0", 3), ("4:2:2", 1)):
        for ri in (0, 7):
            opts = _opts(30, sampling, False, ri)
            assert lib.nesr_jpeg_header_ex(37, 53, c, ctypes.byref(opts), None, 0, ctypes.byref(n)) == 0
            buf = (ctypes.c_uint8 * n.value)()
            assert lib.nesr_jpeg_header_ex(37, 53, c, ctypes.byref(opts), buf, n.value, ctypes.byref(n)) == 0
            img = np.zeros((37, 53, 3) if c == 3 else (37, 53), np.uint8)
            want, st = ref.encode_jpeg_stats(img, 30, "rgb", sampling, False, ri)
            assert bytes(buf) == want[:st["header_bytes"]], (sampling, c, ri)
    assert lib.nesr_jpeg_header_ex(37, 53, 3, ctypes.byref(_opts(optimize=True)), None, 0, ctypes.byref(n)) == _lib.ERR_ARG
    bad = [_lib.JpegOpts(95, 3, 0, 0), _lib.JpegOpts(95, -1, 0, 0), _lib.JpegOpts(95, 0, 0, -1), _lib.JpegOpts(95, 0, 0, 65536), _lib.JpegOpts(0, 0, 0, 0)]
    t = torch.zeros(4096, dtype=torch.uint8, device=cuda_device)
    p = ctypes.c_void_p(t.data_ptr())
    for o in bad:
        assert lib.nesr_jpeg_header_ex(8, 8, 3, ctypes.byref(o), None, 0, ctypes.byref(n)) == _lib.ERR_ARG
        assert lib.nesr_jpeg_encode_ex_u8(0, p, 24, 8, 8, 3, 0, ctypes.byref(o), p, 1 << 30, p, 4096, p, None) == _lib.ERR_ARG
    for o in bad[:4]:
        assert lib.nesr_jpeg_scratch_bytes_ex(8, 8, 3, ctypes.byref(o)) == 0
    assert lib.nesr_jpeg_scratch_bytes_ex(8, 8, 3, None) == 0
    assert lib.nesr_jpeg_encode_ex_u8(0, p, 24, 8, 8, 3, 0, None, p, 1 << 30, p, 4096, p, None) == _lib.ERR_ARG
    assert lib.nesr_jpeg_scratch_bytes_ex(8, 8, 3, ctypes.byref(_opts(ri=65535))) > 0


@pytest.mark.parametrize("options", [dict(sampling="4:4:4", optimize=True, ri=0), dict(sampling="4:2:2", optimize=False, ri=2),
                                     dict(sampling="4:2:0", optimize=True, ri=3)], ids=["optimised", "restart", "both"])
def test_capacity(cuda_device, options, monkeypatch):
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    h, w = 200, 333
    img = jpeg_cases.content("noise", h, w, 3)
    want, st = ref.encode_jpeg_stats(img, 100, "rgb", options["sampling"], options["optimize"], options["ri"])
    frame = torch.from_numpy(img).to(cuda_device)
    opts = _opts(100, **options)
    length, status, buf, intact = _encode_raw(frame, opts, len(want))
    assert (length, status, intact) == (len(want), 0, True) and buf[:length].tobytes() == want and (buf[length:] == 0xA5).all()
    # short by one byte, inside the scan, inside the DHTs the device writes, inside the host's part of the header, one byte
    for cap in (len(want) - 1, len(want) - 2, st["header_bytes"] + 5000, st["header_bytes"] - 3, 300, 100, 1):
        length, status, buf, intact = _encode_raw(frame, opts, cap)
        assert (length, status, intact) == (len(want), 1, True), cap
        assert buf[:cap].tobytes() == want[:cap], cap
        assert (buf[cap:] == 0xA5).all(), cap
    # the wrapper: 4:4:4 and 4:2:2 noise at quality 100 need more than H W C / 2 + 4096, so one more run at the size the device reported
    runs = []
    real = imgproc._jpeg_encode_hip
    monkeypatch.setattr(imgproc, "_jpeg_encode_hip", lambda f, q, bgr, cap, *o: runs.append(cap) or real(f, q, bgr, cap, *o))
    assert imgproc.encode_jpeg_u8(frame, 100, sampling=options["sampling"], optimize=options["optimize"], restart_interval=options["ri"]) == want
    first = h * w * 3 // 2 + 4096
    assert runs == ([first] if len(want) <= first else [first, len(want)])
    if options["sampling"] != "4:2:0":
        assert len(runs) == 2
    with pytest.raises(_lib.NesrNoFitError) as e:
        real(frame, 100, False, len(want) - 1, (options["sampling"], options["optimize"], options["ri"]))
    assert e.value.needed == len(want)


# ------------------------------------------------------------------------------------------------ 5: host route, round trip, wrappers
def test_host_route_and_refusals(cuda_device):
    from neural_enhanced_super_resolution_amd import imgproc
    img = jpeg_cases.content("impulses", 37, 53, 3)
    frame = torch.from_numpy(img).to(cuda_device)
    kw = dict(sampling="4:2:2", optimize=True, restart_interval=3)
    want = ref.encode_jpeg(img, 95, "rgb", "4:2:2", True, 3)
    assert imgproc.encode_jpeg_u8(frame, **kw) == want
    try:
        import PIL  # noqa: F401
        assert imgproc.encode_jpeg_u8(frame, use_hip=False, **kw) == want
        assert imgproc.encode_jpeg_u8(frame[:, :, 1], use_hip=False, **kw) == ref.encode_jpeg(img[:, :, 1], 95, "rgb", "4:2:2", True, 3)
    except ImportError:
        with pytest.raises(RuntimeError, match="Pillow"):
            imgproc.encode_jpeg_u8(frame, use_hip=False, **kw)
    for bad in (dict(sampling="4:4:0"), dict(sampling="4:1:1"), dict(restart_interval=-1), dict(restart_interval=65536)):
        with pytest.raises(ValueError):
            imgproc.encode_jpeg_u8(frame, **bad)


@pytest.mark.parametrize("layout", cases.LAYOUTS)
def test_round_trip_on_the_device(cuda_device, layout):
    """Our own file with a restart interval through the decoder's interval-per-lane route: no synchronisation round."""
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    img = cases.image("impulses", 37, 53, layout)
    sampling = "4:2:0" if layout == "gray" else layout
    want = ref.encode_jpeg(img, 95, "rgb", sampling, True, 2)
    data = imgproc.encode_jpeg_u8(torch.from_numpy(img).to(cuda_device), 95, sampling=sampling, optimize=True, restart_interval=2)
    assert data == want
    frame = imgproc.decode_jpeg_u8(data, device=cuda_device, use_hip=True)
    rounds, launches = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().nesr_jpeg_decode_last_launches(ctypes.byref(rounds), ctypes.byref(launches)) == 0
    assert rounds.value == 0 and launches.value > 0
    assert np.array_equal(frame.cpu().numpy(), jpeg_decode_ref.decode_jpeg(want))


def test_wrappers_pass_the_options(cuda_device):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, imgproc
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=2)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=2), half=False, device=cuda_device, tile=0, tile_pad=10,
                      pre_pad=0)
    img = synthetic_frame(32, 48, seed=21)
    kw = dict(sampling="4:4:4", optimize=True, restart_interval=8)
    out, mode = up.enhance(img)
    want = ref.encode_jpeg(out, 95, "bgr", "4:4:4", True, 8)
    data, jmode = up.enhance_jpeg(img, **kw)
    assert jmode == mode and data == want
    assert data == imgproc.encode_jpeg_u8(torch.from_numpy(out).to(cuda_device), 95, order="bgr", **kw)
    assert data != up.enhance_jpeg(img)[0]
    # the file routes: a JPEG file in, the same options out
    src = imgproc.encode_jpeg_u8(torch.from_numpy(img).to(cuda_device), 95, order="bgr")
    decoded, _ = up.enhance_file(src)
    want_file = ref.encode_jpeg(decoded, 95, "bgr", "4:4:4", True, 8)
    assert up.enhance_file_jpeg(src, **kw)[0] == want_file
    assert up.enhance_image_file_to(src, **kw)[0] == want_file
    # enhance_iterations with the three-tuple
    sd12 = synthetic_state_dict(seed=6, num_in_ch=12, scale=4, num_block=2)
    up12 = RealESRGANer(scale=2, model_path={"params_ema": sd12}, model=RRDBNet(12, 3, num_block=2), tile=0, tile_pad=0, pre_pad=0, half=False,
                        device=cuda_device)
    rgb = synthetic_frame(12, 20, seed=8)[:, :, ::-1].copy()
    cfg = {"iterations": 1, "upscale_factor": 2.0}
    frame = A.enhance_iterations(up12, rgb, cfg, "cuda")
    assert A.enhance_iterations(up12, rgb, cfg, "cuda", encode=("jpeg", 30, kw)) == ref.encode_jpeg(frame, 30, "rgb", "4:4:4", True, 8)
    assert A.enhance_iterations(up12, rgb, cfg, "cuda", encode=("jpeg", 30)) == ref.encode_jpeg(frame, 30, "rgb")
    with pytest.raises(ValueError):
        A.enhance_iterations(up12, rgb, cfg, "cuda", encode=("jpeg", 30, kw, 1))
