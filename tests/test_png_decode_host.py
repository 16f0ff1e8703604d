"""CPU, with the library built: nesr_png_parse against the specification's parse (tests/png_decode_ref.py), the codes of the files it
refuses, the table that is too small, and imgproc.decode_png's host route (stdlib zlib + numpy) frame for frame."""
import ctypes

import numpy as np
import pytest
import torch

from tests import png_cases, png_decode_cases as cases, png_decode_ref as ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib


def _files():
    out = [(f"golden-{kind}-{h}x{w}x{c}x{d}", open(png_cases.golden_path(kind, h, w, c, d), "rb").read(),
            png_cases.file_order(*png_cases.image(kind, h, w, c, d))) for kind, h, w, c, d in png_cases.GOLDEN_FILES]
    out += [(cid, png_cases.spec(kind, h, w, c, d)[0], png_cases.file_order(*png_cases.image(kind, h, w, c, d))) for cid, kind, h, w, c, d in png_cases.cases()]
    return out + list(cases.foreign()) + list(cases.handmade()) + [cases.far_match()]


def test_parse_equals_the_specification(lib):
    for cid, data, _ in _files() + [(c[0], c[1], None) for c in cases.bad() + cases.corrupt()]:
        want, wsegs = ref.parse(data)
        info, segs = lib.png_parse(data)
        got = {k: int(getattr(info, k)) for k in want}
        assert got == want, cid
        assert [(int(s.offset), int(s.bytes), int(s.first), int(s.last)) for s in segs[:info.n_segments]] == [tuple(int(v) for v in s) for s in wsegs], cid


def test_refused_files_get_their_codes(lib):
    for cid, data in cases.unsupported_files():
        with pytest.raises(lib.NesrUnsupportedError):
            lib.png_parse(data)
    for cid, data in cases.badfile_files():
        with pytest.raises(lib.NesrBadFileError):
            lib.png_parse(data)
    info = lib.PngInfo()
    assert lib.load().nesr_png_parse(None, 0, ctypes.byref(info), None, 0) == lib.ERR_ARG


def test_a_table_too_small_still_reports_n_segments(lib):
    data = dict((c[0], c[1]) for c in cases.foreign())["70x320x3x8-gradient-full"]
    want, wsegs = ref.parse(data)
    info = lib.PngInfo()
    segs = (lib.PngSegment * 3)()
    assert lib.load().nesr_png_parse(data, len(data), ctypes.byref(info), segs, 3) == lib.ERR_NOFIT
    assert info.n_segments == len(wsegs) == 9 and (info.H, info.W, info.C, info.depth) == (70, 320, 3, 8)
    assert [(s.offset, s.bytes) for s in segs] == [s[:2] for s in wsegs[:3]]
    assert lib.load().nesr_png_parse(data, len(data), ctypes.byref(info), None, 0) == lib.ERR_NOFIT and info.n_segments == 9


def test_parse_reads_nothing_past_n(lib):
    """Every prefix of a file, from a buffer that ends where the prefix ends, is refused (or, whole, accepted) without a fault"""
    data = png_cases.spec("runs", 33, 130, 4, 16)[0]
    for n in list(range(0, 120)) + [len(data) - 13, len(data) - 1]:
        buf = (ctypes.c_uint8 * max(n, 1)).from_buffer_copy(data[:n] or b"\0")
        info = lib.PngInfo()
        assert lib.load().nesr_png_parse(buf, n, ctypes.byref(info), None, 0) == lib.ERR_BADFILE


def test_decode_png_host_route_returns_every_frame(lib):
    from neural_enhanced_super_resolution_amd import imgproc
    for k, (cid, data, frame) in enumerate(_files()):
        order = "bgr" if k % 2 else "rgb"
        got = imgproc.decode_png(data, order=order, device="cpu", use_hip=False)
        want = frame
        if order == "bgr" and frame.ndim == 3:
            want = np.concatenate([frame[:, :, 2::-1], frame[:, :, 3:]], axis=2)
        assert got.dtype == (torch.int16 if frame.dtype == np.uint16 else torch.uint8), cid
        assert tuple(got.shape) == want.shape and np.array_equal(got.numpy().view(frame.dtype), want), cid


def test_decode_png_host_route_refuses_bad_files(lib):
    from neural_enhanced_super_resolution_amd import imgproc
    for cid, data, bit in cases.corrupt():
        with pytest.raises(lib.NesrBadFileError):
            imgproc.decode_png(data, device="cpu", use_hip=False)
    with pytest.raises(lib.NesrBadFileError):
        imgproc.decode_png(cases.badfile_files()[0][1], device="cpu", use_hip=False)
    with pytest.raises(lib.NesrUnsupportedError):
        imgproc.decode_png(cases.unsupported_files()[0][1], device="cpu", use_hip=False)
