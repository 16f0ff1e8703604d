"""CPU: the specification of the JPEG encoder (tests/jpeg_ref.py) byte for byte against Pillow's libjpeg-turbo and against committed
files; the host-side entries of the C ABI (nesr_jpeg_header, nesr_jpeg_scratch_bytes, nesr_jpeg_encode_u8's argument checks); and
the proof, from the specification's counters, that the grid takes every path of the entropy coder and of the dummy-block rule."""
import ctypes
import os

import numpy as np
import pytest

from tests import jpeg_cases, jpeg_ref

CASES = jpeg_cases.cases()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ 1: against Pillow
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_specification_equals_pillow(case):
    pytest.importorskip("PIL")                      # only for a machine without Pillow
    from tests.make_jpeg_golden import pillow_bytes
    _, kind, h, w, c = case
    img, order = jpeg_cases.image(kind, h, w, c)
    for q in jpeg_cases.QUALITIES:
        assert jpeg_cases.spec(kind, h, w, c, q)[0] == pillow_bytes(img, q, order), f"quality {q}"


def test_specification_equals_pillow_beyond_the_grid():
    """Qualities at the ends of the scaling rule and both sides of 50; the channel order; the 623 / 328 header bytes."""
    pytest.importorskip("PIL")
    from tests.make_jpeg_golden import pillow_bytes
    img = jpeg_cases.content("impulses", 37, 53, 3)
    for q in (2, 5, 49, 50, 51, 75, 99):
        assert jpeg_ref.encode_jpeg(img, q) == pillow_bytes(img, q)
        assert jpeg_ref.encode_jpeg(img[:, :, ::-1], q, order="bgr") == pillow_bytes(img, q)
        assert jpeg_ref.encode_jpeg(img[:, :, 1], q) == pillow_bytes(img[:, :, 1], q)
    assert len(jpeg_ref.header(37, 53, 3, 95)) == 623 and len(jpeg_ref.header(37, 53, 1, 95)) == 328


# ------------------------------------------------------------------------------------------------ 2: against committed files
@pytest.mark.parametrize("entry", jpeg_cases.GOLDEN_FILES, ids=[os.path.basename(jpeg_cases.golden_path(*e)) for e in jpeg_cases.GOLDEN_FILES])
def test_specification_equals_committed_file(entry):
    kind, h, w, c, q = entry
    with open(jpeg_cases.golden_path(*entry), "rb") as f:
        want = f.read()
    assert 300 < len(want) < 16384
    assert jpeg_cases.spec(kind, h, w, c, q)[0] == want


# ------------------------------------------------------------------------------------------------ 3: header and argument checks
def _header(lib, h, w, c, q):
    n = ctypes.c_int(-1)
    assert lib.nesr_jpeg_header(h, w, c, q, None, 0, ctypes.byref(n)) == 0          # the size alone
    buf = (ctypes.c_uint8 * n.value)()
    assert lib.nesr_jpeg_header(h, w, c, q, buf, n.value, ctypes.byref(n)) == 0
    return bytes(buf)


def test_header_equals_the_specification(lib):
    shapes = jpeg_cases.SHAPES + [(64, 96, 3), (65535, 65535, 3), (4320, 7680, 3)]
    for h, w, c in shapes:
        for q in jpeg_cases.QUALITIES + [50, 75]:
            assert _header(lib, h, w, c, q) == jpeg_ref.header(h, w, c, q), (h, w, c, q)
    n = ctypes.c_int(0)
    for bad in ((0, 8, 3, 95), (8, 0, 3, 95), (8, 8, 2, 95), (8, 8, 4, 95), (8, 8, 3, 0), (8, 8, 3, 101), (65536, 8, 3, 95)):
        assert lib.nesr_jpeg_header(*bad, None, 0, ctypes.byref(n)) == -1, bad
    assert lib.nesr_jpeg_header(8, 8, 3, 95, None, 0, None) == -1


def test_scratch_bytes_is_monotone(lib):
    for c in (1, 3):
        sizes = [1, 7, 8, 9, 16, 17, 100, 1000, 4320, 16384]
        grid = [[lib.nesr_jpeg_scratch_bytes(h, w, c) for w in sizes] for h in sizes]
        assert grid[0][0] > 0
        for i in range(len(sizes)):
            for j in range(len(sizes)):
                assert i == 0 or grid[i][j] >= grid[i - 1][j]
                assert j == 0 or grid[i][j] >= grid[i][j - 1]
        assert grid[-1][-1] > grid[0][0]
    assert lib.nesr_jpeg_scratch_bytes(64, 64, 3) > lib.nesr_jpeg_scratch_bytes(64, 64, 1)
    for bad in ((0, 8, 3), (8, 0, 3), (8, 8, 2), (8, 8, 4), (65536, 8, 1)):
        assert lib.nesr_jpeg_scratch_bytes(*bad) == 0


def test_encode_rejects_bad_arguments_without_touching_a_device(lib):
    """Every pointer below is a made-up address: a check that let one through would fail with NESR_ERR_HIP (no device here) or fault."""
    p = ctypes.c_void_p(0x10000)
    h, w, c = 24, 40, 3
    need = lib.nesr_jpeg_scratch_bytes(h, w, c)

    def call(src=p, stride=w * c, h=h, w=w, c=c, order=0, quality=95, scratch=p, scratch_bytes=need, out=p, cap=4096, out_len=p):
        return lib.nesr_jpeg_encode_u8(0, src, stride, h, w, c, order, quality, scratch, scratch_bytes, out, cap, out_len, None)

    for kw in ({"src": None}, {"scratch": None}, {"out": None}, {"out_len": None}, {"h": 0}, {"w": 0}, {"h": -3}, {"c": 2}, {"c": 4}, {"c": 0},
               {"quality": 0}, {"quality": 101}, {"stride": w * c - 1}, {"scratch_bytes": need - 1}, {"scratch_bytes": 0}, {"order": 2},
               {"h": 65536}, {"scratch": ctypes.c_void_p(0x10004)}):
        assert call(**kw) == -1, kw
        assert lib.nesr_last_error()
    assert call(c=1, stride=w - 1, scratch_bytes=lib.nesr_jpeg_scratch_bytes(h, w, 1)) == -1


# ------------------------------------------------------------------------------------------------ 4: the grid takes every path
def _stats():
    return {(case[0], q): jpeg_cases.spec(*case[1:], q)[1] for case in CASES for q in jpeg_cases.QUALITIES}


def test_grid_takes_every_path():
    stats = _stats()
    assert any(s["zrl"] > 0 for s in stats.values())
    assert any(s["stuffed"] > 0 for s in stats.values())
    for c in (1, 3):      # saturated content at quality 100 reaches the largest categories, gray and colour
        top = [s for (name, q), s in stats.items() if name.endswith("-saturated") and f"x{c}-" in name and q == 100]
        assert any(s["max_ac_cat"] == 10 for s in top) and any(s["max_dc_cat"] == 11 for s in top)
    assert max(s["max_ac_cat"] for s in stats.values()) == 10 and max(s["max_dc_cat"] for s in stats.values()) == 11
    assert any(s["dummy_right"] > 0 and s["dummy_bottom"] == 0 for s in stats.values())
    assert any(s["dummy_bottom"] > 0 and s["dummy_right"] == 0 for s in stats.values())
    assert any(s["dummy_both_in_one_mcu"] > 0 for s in stats.values())
    assert any(s["all_eob"] for s in stats.values())
    assert stats[("17x9x3-noise", 95)]["dummy_bottom"] == 2 and stats[("17x9x3-noise", 95)]["dummy_right"] == 0
    assert stats[("9x17x3-noise", 95)]["dummy_right"] == 2 and stats[("9x17x3-noise", 95)]["dummy_bottom"] == 0
    assert stats[("24x16x3-noise", 95)]["dummy_bottom"] == 2          # H = 8 mod 16
    assert stats[("1x1x3-noise", 95)]["dummy_both_in_one_mcu"] == 1 and stats[("1x1x3-noise", 95)]["dummy_blocks"] == 3


def test_the_boundary_shapes_cross_the_kernels_boundaries():
    """What tests/jpeg_cases.py says of its last three shapes, from the specification's counts (csrc/jpeg_kernels.h: 256 blocks per
    workgroup and scan chunk, 4096 unstuffed bytes per stuffing chunk)."""
    data, s = jpeg_cases.spec("noise", 16, 4112, 3, 95)
    assert s["blocks"] == 257 * 6 and s["blocks"] > 2 * 256
    assert len(data) - s["stuffed"] - 623 - 2 > 2 * 4096
    assert jpeg_cases.spec("noise", 520, 24, 3, 95)[1]["blocks"] == 396
    assert jpeg_cases.spec("noise", 24, 1600, 1, 95)[1]["blocks"] == 600


def test_the_chroma_row_rule_matters_on_the_grid():
    """H = 8 mod 16: padding the source rows all the way down (the rule of the columns) gives other bytes, so the 24 x 16 and 8 x 16
    cases would catch a kernel that used it."""
    img = jpeg_cases.content("noise", 24, 16, 3)
    padded = np.pad(img, ((0, 8), (0, 0), (0, 0)), mode="edge")
    body = jpeg_ref.encode_jpeg(padded, 95)[623:]
    assert jpeg_ref.encode_jpeg(img, 95)[623:] != body


def test_encode_jpeg_u8_host_route():
    """A CPU tensor or an ndarray goes to Pillow; use_hip=True on them is an error, never a third route."""
    pytest.importorskip("PIL")
    import torch
    from neural_enhanced_super_resolution_amd import imgproc
    img = jpeg_cases.content("impulses", 37, 53, 3)
    want = jpeg_cases.spec("impulses", 37, 53, 3, 95)[0]
    assert imgproc.encode_jpeg_u8(img) == want
    assert imgproc.encode_jpeg_u8(torch.from_numpy(img)) == want
    assert imgproc.encode_jpeg_u8(torch.from_numpy(img[:, :, ::-1].copy()), order="bgr", use_hip=False) == want
    gray = jpeg_cases.content("noise", 37, 53, 1)
    assert imgproc.encode_jpeg_u8(gray, quality=30) == jpeg_cases.spec("noise", 37, 53, 1, 30)[0]
    with pytest.raises(ValueError):
        imgproc.encode_jpeg_u8(torch.from_numpy(img), use_hip=True)
    for bad in (img.astype(np.uint16), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            imgproc.encode_jpeg_u8(bad)
    with pytest.raises(ValueError):
        imgproc.encode_jpeg_u8(img, quality=0)
    with pytest.raises(ValueError):
        imgproc.encode_jpeg_u8(img, order="gbr")
