"""CPU: the specification of the PNG encoder (tests/png_ref.py).  Lossless is the contract: a standard decoder returns the frame bit
for bit -- a stdlib decoder here (zlib.decompress of the concatenated IDATs, unfiltering, every CRC, the layout) and Pillow.  The
counters prove the grid of tests/png_cases.py reaches every path of the coder; committed files pin the bytes against edits; and the
size conditions compare with cv2's settings (the host route of imgproc.encode_png) and with zlib's own Z_RLE."""
import io
import os
import zlib

import numpy as np
import pytest

from tests import png_cases, png_ref

CASES = png_cases.cases()
IDS = [c[0] for c in CASES]


# ------------------------------------------------------------------------------------------------ 1: decoding
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_specification_decodes_to_the_frame(case):
    _, kind, h, w, c, depth = case
    img, order = png_cases.image(kind, h, w, c, depth)
    data, stats = png_cases.spec(kind, h, w, c, depth)
    want = png_cases.file_order(img, order)
    assert len(data) <= png_ref.bound(h, w, c, depth)
    assert data[:png_ref.HEAD_BYTES] == png_ref.head(h, w, c, depth) and len(data) - png_ref.HEAD_BYTES - png_ref.TAIL_BYTES > 0
    chunks = png_ref.read_chunks(data)
    assert len(chunks) == 4 + stats["chunks"]                      # IHDR, IDAT[78 01], one per deflate chunk, IDAT[Adler-32], IEND
    if h * w * c * depth // 8 <= 8192:                              # the byte-serial decoder: every small frame
        got = png_ref.decode_png(data)
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert png_ref.refilter_matches(data, img, order)               # the same statement for every frame (png_ref.refilter_matches)
    # every chunk alone is a deflate stream that ends byte-aligned: no match reaches before its first byte
    out = b""
    for _, payload in chunks[2:-2]:
        d = zlib.decompressobj(-15)
        out += d.decompress(payload)
        assert d.unused_data == b"" and payload[-4:] == b"\x00\x00\xff\xff"
    assert out == stats["filtered"].tobytes()


PILLOW_CASES = [c for c in CASES if c[5] == 8 or c[4] == 1]        # Pillow reads 16-bit colour PNG files at 8 bits


@pytest.mark.parametrize("case", PILLOW_CASES, ids=[c[0] for c in PILLOW_CASES])
def test_pillow_decodes_to_the_frame(case):
    Image = pytest.importorskip("PIL.Image")
    _, kind, h, w, c, depth = case
    img, order = png_cases.image(kind, h, w, c, depth)
    got = np.asarray(Image.open(io.BytesIO(png_cases.spec(kind, h, w, c, depth)[0])))
    assert np.array_equal(got.astype(img.dtype), png_cases.file_order(img, order))


def test_order_and_shapes():
    img = png_cases.content("impulses", 37, 53, 4, 16)
    flipped = np.concatenate([img[:, :, 2::-1], img[:, :, 3:]], axis=2)
    assert png_ref.encode_png(flipped, "bgr") == png_ref.encode_png(img, "rgb")
    gray = png_cases.content("noise", 37, 53, 1, 8)
    assert png_ref.encode_png(gray[:, :, None]) == png_ref.encode_png(gray) == png_ref.encode_png(gray, "bgr")
    with pytest.raises(ValueError):
        png_ref.encode_png(np.zeros((4, 4, 2), np.uint8))


# ------------------------------------------------------------------------------------------------ 2: path coverage
def test_the_grid_reaches_every_path():
    total = {}
    for _, kind, h, w, c, depth in CASES:
        for k, v in png_cases.spec(kind, h, w, c, depth)[1].items():
            if k != "filtered":
                total[k] = total.get(k, 0) + int(v)
    for key in ("btype0", "btype1", "btype2",                       # stored, fixed, dynamic
                "filter0", "filter1", "filter2", "filter3", "filter4",
                "rem0", "rem1", "rem2", "rem_match",                # (R - 1) % 258 = 0, 1, 2 (literals) and >= 3 (a match)
                "split258",                                         # at least one match of 258
                "cut_runs",                                         # a run cut by a chunk boundary
                "repair15",                                         # an unrestricted literal/length code deeper than 15
                "match_chunks",                                     # the single distance code
                "nomatch_chunks"):                                  # no distance code
        assert total.get(key, 0) > 0, (key, total)
    # the 7-bit repair of the code-length code is reached too (if an edit of the grid loses it, tests/test_png_host.py still covers
    # the rule: Fibonacci counts on 19 symbols)
    assert total.get("repair7", 0) > 0, total


# ------------------------------------------------------------------------------------------------ 3: committed files
@pytest.mark.parametrize("entry", png_cases.GOLDEN_FILES, ids=[os.path.basename(png_cases.golden_path(*e)) for e in png_cases.GOLDEN_FILES])
def test_specification_equals_committed_file(entry):
    with open(png_cases.golden_path(*entry), "rb") as f:
        want = f.read()
    assert 75 < len(want) < 65536
    assert png_cases.spec(*entry)[0] == want


# ------------------------------------------------------------------------------------------------ 4: size
def _host_route(img, order):
    from neural_enhanced_super_resolution_amd import imgproc
    return imgproc.encode_png(img, order=order, use_hip=False)


def _deflate_bytes(data):
    """bytes of the zlib stream of a PNG file: the IDAT payloads"""
    return sum(len(p) for k, p in png_ref.read_chunks(data) if k == b"IDAT")


def test_not_larger_than_cv2_settings_on_the_photograph():
    """The host route is cv2's settings (Sub on every row, level 1, Z_RLE, one IDAT).  The crop, and the crop tiled to 256 x 384."""
    crop = png_cases.crop_bgr()
    for img in (crop, np.tile(crop, (4, 4, 1))):
        ours, theirs = png_ref.encode_png(img, "bgr"), _host_route(img, "bgr")
        print(f"{img.shape}: specification {len(ours)} bytes, cv2's settings {len(theirs)} bytes")
        assert png_ref.refilter_matches(theirs, img, "bgr", layout=False) and png_ref.refilter_matches(ours, img, "bgr")
        assert len(ours) <= len(theirs)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chunking_and_code_construction_cost(case):
    """Against zlib's one-stream Z_RLE deflate of the specification's own filtered bytes: at most 1 % plus 48 bytes per chunk (chunk
    framing and one tree header per chunk) more.  File against file: the specification's whole file, and the smallest PNG file that
    holds zlib's stream -- signature, IHDR, one IDAT, IEND: 57 bytes around it.  Measured worst case over the grid: DESIGN.md
    section 15."""
    _, kind, h, w, c, depth = case
    data, stats = png_cases.spec(kind, h, w, c, depth)
    deflate = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    one = len(deflate.compress(stats["filtered"].tobytes()) + deflate.flush())
    over = len(data) - (one + 57)
    print(f"{case[0]}: {len(data)} bytes against {one} + 57 in one Z_RLE stream, {stats['chunks']} chunks: {over:+d} bytes, "
          f"{over / stats['chunks']:+.1f} per chunk, {100.0 * over / one:+.2f} %")
    assert len(data) <= (one + 57) + 0.01 * one + 48 * stats["chunks"]
