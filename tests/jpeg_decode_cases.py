"""The files the JPEG decoder's tests share (tests/test_jpeg_decode_spec.py on the CPU, tests/test_gpu_jpeg_decode.py on the
device): Pillow writes them on the fly from the seeded images of tests/jpeg_cases.py; a committed subset with its expected pixels
lies under tests/golden/jpeg_decode (tests/make_jpeg_decode_golden.py), so the fixture checks need no Pillow."""
from __future__ import annotations

import functools
import io
import os
import re

import numpy as np

from tests import jpeg_cases, jpeg_decode_ref

GOLDEN = os.path.join(jpeg_cases.GOLDEN, "jpeg_decode")
REFERENCE_ASSET = os.path.join(GOLDEN, "reference_test.jpeg")       # the reference's images/test.jpeg: 512 x 512, 4:2:0, DRI = 32

# The kernels' own constants (csrc/jpeg_decode_kernels.h); test_jpeg_decode_spec.py proves that the boundary files cross each twice.
SUBSEQ_BITS = 1024            # bits of the unstuffed stream per lane of the self-synchronising decode
SUBSEQ_PER_GROUP = 256        # lanes (subsequences) per workgroup of that decode
RECON_BLOCKS = 32             # blocks per workgroup of the reconstruction (dequantise, IDCT)
UNSTUFF_CHUNK = 4096          # bytes of the scan per workgroup of the scan preparation


def kernel_constant(header, name):
    """`constexpr int NAME = value;` as csrc/<header> states it today: what a test's claim that a file reaches a path is measured by"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neural_enhanced_super_resolution_amd", "csrc", header)
    with open(path) as f:
        return int(re.search(rf"constexpr int {name} = (\d+);", f.read()).group(1))


SCAN_LANES = 1024             # values per step of the single-workgroup scans (csrc/codec_device.h: group_scan_1024)

SHAPES = [(1, 1), (8, 8), (7, 25), (17, 33), (24, 16), (8, 16), (40, 56), (37, 53), (64, 96)]
CONTENTS = ["noise", "impulses", "constant", jpeg_cases.CROP]
LAYOUTS = [(3, 0), (3, 1), (3, 2), (1, 0)]                           # (channels, Pillow's subsampling: 0 4:4:4, 1 4:2:2, 2 4:2:0)
QUALITIES = [30, 95, 100]
OPTIONS = [{}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 2}, {"restart_marker_blocks": 5}, {"restart_marker_rows": 1}]


def _opt_id(opt):
    return "-".join(f"{k.replace('restart_marker_', 'r')}{v if v is not True else ''}" for k, v in opt.items()) or "plain"


def _grid():
    """(id, kind, h, w, c, subsampling, quality, options).  Every shape meets every layout and content; quality and option rotate so
    that each value meets each shape, layout and content.  Then noise at 100 and impulses at 30 (the saturating blocks) with every
    option and layout, and the boundary files."""
    out = []
    for si, (h, w) in enumerate(SHAPES):
        for li, (c, sub) in enumerate(LAYOUTS):
            for ki, kind in enumerate(CONTENTS):
                out.append((kind, h, w, c, sub, QUALITIES[(si + li + ki) % 3], OPTIONS[(2 * si + li + 3 * ki) % 6]))
    for c, sub in LAYOUTS:
        for opt in OPTIONS:
            out.append(("noise", 40, 56, c, sub, 100, opt))
            out.append(("impulses", 37, 53, c, sub, 30, opt))
    out += BOUNDARY
    return [(f"{k}-{h}x{w}x{c}-s{s}-q{q}-{_opt_id(o)}", k, h, w, c, s, q, o) for (k, h, w, c, s, q, o) in out]


# The smallest files that cross the kernels' constants at least twice (the counters in test_jpeg_decode_spec.py prove it):
#   noise 96 x 1024 x 3, 4:2:0, q95, no DRI   a stream of over 100 KB: more than two workgroups of subsequences (32 KB each), tens of
#                                             unstuff chunks, 2304 blocks = 72 reconstruction workgroups
#   constant 96 x 1024 x 3, 4:2:0, no DRI     6 bits per block: over a hundred blocks inside one subsequence
#   noise 24 x 1600 gray, one restart per row  200 blocks per interval, restart markers in several unstuff chunks
#   noise 96 x 1024 x 3, 4:4:4, DRI = 5       more intervals than one workgroup holds lanes
BOUNDARY = [("noise", 96, 1024, 3, 2, 95, {}), ("constant", 96, 1024, 3, 2, 95, {}), ("noise", 24, 1600, 1, 0, 95, {"restart_marker_rows": 1}),
            ("noise", 96, 1024, 3, 0, 95, {"restart_marker_blocks": 5})]


def cases():
    return _grid()


def _pillow_gray(img, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality)
    data = buf.getvalue()
    return data, np.asarray(Image.open(io.BytesIO(data)))


# Two files beyond the grid, each the smallest that makes one of the decoder's single-workgroup scans take a second step of 1024 values
# (test_jpeg_decode_spec.py asserts it from the header).  -> (id, bytes, Pillow's pixels: the specification is pinned to them and is
# too slow at these sizes)
@functools.lru_cache(maxsize=None)
def long_scan():
    """Gray noise 2200 x 2048 at quality 95: a scan of over 1024 unstuff chunks (jd_scan_chunks carries)"""
    img = np.random.RandomState(2200).randint(0, 256, (2200, 2048)).astype(np.uint8)
    return ("noise-2200x2048x1-q95-plain",) + _pillow_gray(img, 95)


@functools.lru_cache(maxsize=None)
def many_mcus():
    """Gray 4104 x 4104 of 16 x 16 squares: 513 x 513 MCUs, over 1024 groups of the DC prefix sum (jd_dc_scan carries)"""
    y, x = np.ogrid[:4104, :4104]
    return ("squares-4104x4104x1-q50-plain",) + _pillow_gray(((y // 16 + x // 16) % 256).astype(np.uint8), 50)


def image_rgb(kind, h, w, c):
    """The case's image: [h, w, 3] RGB or [h, w] gray."""
    if kind == jpeg_cases.CROP:
        img = jpeg_cases.crop_bgr()[:h, :w, ::-1]
        return np.ascontiguousarray(img if c == 3 else img[:, :, 1])
    return jpeg_cases.content(kind, h, w, c)


def write_file(kind, h, w, c, sub, quality, opt):
    """Pillow's file for a case."""
    from PIL import Image
    buf = io.BytesIO()
    kw = dict(opt)
    if c == 3:
        kw["subsampling"] = sub
    Image.fromarray(image_rgb(kind, h, w, c)).save(buf, format="JPEG", quality=quality, **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def _file(key):
    kind, h, w, c, sub, quality, opt = key
    return write_file(kind, h, w, c, sub, quality, dict(opt))


def file_bytes(kind, h, w, c, sub, quality, opt):
    return _file((kind, h, w, c, sub, quality, tuple(sorted(opt.items()))))


@functools.lru_cache(maxsize=None)
def _spec(data):
    return jpeg_decode_ref.decode_jpeg_stats(data, "rgb")


def spec(data):
    """(pixels in RGB order or gray, counters) of the specification for a file; computed once per process and shared.  Treat the array as
    read-only."""
    return _spec(bytes(data))


def spec_pixels(data, order="rgb"):
    px = spec(data)[0]
    return px if px.ndim == 2 or order == "rgb" else px[:, :, ::-1]


# the committed files of tests/golden/jpeg_decode: <name>.jpg and <name>.npy (RGB or gray pixels)
GOLDEN_FILES = [("noise", 1, 1, 3, 2, 95, {}), ("noise", 7, 25, 3, 2, 100, {"restart_marker_blocks": 1}), ("impulses", 17, 33, 3, 1, 30, {"optimize": True}),
                ("impulses", 37, 53, 3, 2, 30, {"restart_marker_blocks": 2}), ("constant", 24, 16, 3, 0, 95, {}), ("noise", 40, 56, 3, 0, 100, {"restart_marker_rows": 1}),
                (jpeg_cases.CROP, 64, 96, 3, 2, 95, {}), ("noise", 37, 53, 1, 0, 95, {"restart_marker_blocks": 5}), ("impulses", 8, 16, 3, 2, 95, {"optimize": True}),
                (jpeg_cases.CROP, 64, 96, 1, 0, 95, {})]


def golden_name(kind, h, w, c, sub, quality, opt):
    return os.path.join(GOLDEN, f"{kind}_{h}x{w}x{c}_s{sub}_q{quality}_{_opt_id(opt)}")


# ------------------------------------------------------------------------------------------------ headers outside the supported list
def segments(data):
    """(marker, offset of the FF, segment length) of the marker segments up to and including SOS."""
    pos = 2
    while pos + 4 <= len(data):
        m = data[pos + 1]
        n = (data[pos + 2] << 8) | data[pos + 3]
        yield m, pos, n
        if m == 0xDA:
            return
        pos += 2 + n


def _patched(data, marker, offset, value):
    """`data` with one byte of the first `marker` segment replaced (offset counted from the segment's length field)."""
    at = next(p for m, p, _ in segments(data) if m == marker) + 2 + offset
    return data[:at] + bytes([value]) + data[at + 1:]


def odd_headers():
    """[(name, bytes, "unsupported" | "bad")]: valid files outside the supported list, and malformed ones.  Needs Pillow."""
    from PIL import Image
    rgb = image_rgb("impulses", 37, 53, 3)
    base = file_bytes("impulses", 37, 53, 3, 2, 95, {})

    def save(img, **kw):
        buf = io.BytesIO()
        img.save(buf, format="JPEG", quality=90, **kw)
        return buf.getvalue()

    sos = next(p for m, p, _ in segments(base) if m == 0xDA)
    dqt = next(p for m, p, _ in segments(base) if m == 0xDB)
    return [
        ("progressive", save(Image.fromarray(rgb), progressive=True), "unsupported"),
        ("four-components", save(Image.fromarray(np.dstack([rgb, rgb[:, :, 0]]), "CMYK")), "unsupported"),
        ("twelve-bit", _patched(base, 0xC0, 2, 12), "unsupported"),
        ("sixteen-bit-dqt", _patched(base, 0xDB, 2, 0x10), "unsupported"),
        ("sampling-4-1-1", _patched(base, 0xC0, 9, 0x41), "unsupported"),
        ("arithmetic", base[:next(p for m, p, _ in segments(base) if m == 0xC0) + 1] + b"\xc9" + base[next(p for m, p, _ in segments(base) if m == 0xC0) + 2:], "unsupported"),
        ("truncated-header", base[:100], "bad"),
        ("missing-sos", base[:sos], "bad"),
        ("sos-cut-short", base[:sos + 6], "bad"),
        ("length-past-the-end", base[:dqt + 2] + b"\xff\xff" + base[dqt + 4:], "bad"),
        ("no-soi", b"\x00\x00" + base[2:], "bad"),
        ("eoi-before-sos", base[:2] + b"\xff\xd9" + base[2:], "bad"),
        ("empty", b"", "bad"),
        ("missing-huffman-table", _patched(base, 0xDA, 4, 0x33), "bad"),
        ("empty-scan", base[:parse_offset(base)], "bad"),
    ]


def parse_offset(data):
    return jpeg_decode_ref.parse(data)["scan_offset"]
