"""The grid the JPEG option tests share (tests/test_jpeg_options_spec.py on the CPU, tests/test_gpu_jpeg_options.py on the device):
images of tests/jpeg_cases.py's seeded contents, and the specification's bytes for a file of the grid, computed once per process."""
from __future__ import annotations

import functools
import os

import numpy as np

from tests import jpeg_cases, jpeg_options_ref

# ten shapes from 1 x 1 to 64 x 96; ceil(W / 8) = 1 2 2 2 3 7 4 1 12 is of both parities (an odd count leaves a 4:2:2 dummy block)
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 9), (9, 17), (24, 16), (37, 53), (7, 25), (25, 7), (64, 96)]
CONTENTS = jpeg_cases.CONTENTS
LAYOUTS = ["gray", "4:4:4", "4:2:2", "4:2:0"]
QUALITIES = jpeg_cases.QUALITIES
OPTIMIZE = [False, True]
INTERVALS = [0, 1, 3]
GOLDEN = os.path.join(jpeg_cases.GOLDEN, "jpeg_options")


def image(kind, h, w, layout):
    return jpeg_cases.content(kind, h, w, 1 if layout == "gray" else 3)


def files():
    """(kind, h, w, layout, quality, optimize, restart interval) of the 3840 files of the grid."""
    return [(k, h, w, lay, q, o, ri) for (h, w) in SHAPES for k in CONTENTS for lay in LAYOUTS for q in QUALITIES for o in OPTIMIZE for ri in INTERVALS]


def file_id(f):
    k, h, w, lay, q, o, ri = f
    return f"{k}_{h}x{w}_{lay.replace(':', '')}_q{q}_{'opt' if o else 'std'}_ri{ri}"


_CACHES = {}


@functools.lru_cache(maxsize=None)
def spec(kind, h, w, layout, quality, optimize, ri, wrong=None):
    """(bytes, counters) of the specification for a file of the grid; the blocks of an image are shared among its files."""
    img = image(kind, h, w, layout)
    cache = _CACHES.setdefault((kind, h, w, layout), {})
    return jpeg_options_ref.encode_jpeg_stats(img, quality, "rgb", "4:2:0" if layout == "gray" else layout, optimize, ri, wrong=wrong, _blocks_cache=cache)


def length_limit_image():
    """512 x 512: a flat frame with geometrically fewer and fewer random pixels, so the symbol counts fall off fast enough for
    Huffman code lengths beyond 16 bits."""
    rng = np.random.default_rng(5)
    img = np.full((512, 512, 3), 128, np.uint8)
    for i in range(40):
        n = max(1, 4096 >> i) if i < 14 else 1
        ys, xs = rng.integers(0, 512, n), rng.integers(0, 512, n)
        img[ys, xs] = rng.integers(0, 256, (n, 3))
    return img


def chunk_outputs(data, header_bytes, chunk=4096):
    """Bytes of the file per chunk of the unstuffed scan (the stuffing pass's unit): a stream byte, the 00 behind an FF, and the
    FF Dn in front of the byte an interval starts with all count for that byte's chunk."""
    scan, out, at, i, marker = data[header_bytes:-2], {}, 0, 0, 0
    while i < len(scan):
        if scan[i] == 0xFF and scan[i + 1] != 0:
            marker, i = 2, i + 2
            continue
        n = 2 if scan[i] == 0xFF else 1
        out[at // chunk] = out.get(at // chunk, 0) + n + marker
        marker, at, i = 0, at + 1, i + n
    return out


def ff_interval_start_image():
    """Gray 16 x 32768 (two block rows of 4096), flat but for a black last block: 8191 one-byte intervals at Ri = 1, then an interval
    that starts with FF (the DC code of category 11) on the last byte of the second stuffing chunk."""
    img = np.full((16, 32768), 128, np.uint8)
    img[8:, 32760:] = 0
    return img


LENGTH_LIMIT = [(100, "4:2:0"), (95, "4:4:4")]             # (quality, sampling), both optimised


@functools.lru_cache(maxsize=None)
def length_limit_spec(quality, sampling):
    return jpeg_options_ref.encode_jpeg_stats(length_limit_image(), quality, "rgb", sampling, True, 0)


def length_limit_digest_path():
    return os.path.join(GOLDEN, "length_limit.json")


# the committed files of tests/golden/jpeg_options (tests/make_jpeg_options_golden.py writes them with Pillow)
GOLDEN_FILES = [("noise", 17, 9, "4:4:4", 95, False, 0), ("noise", 9, 17, "4:2:2", 95, False, 0), ("impulses", 37, 53, "4:2:2", 30, True, 3),
                ("saturated", 24, 16, "4:4:4", 100, True, 1), ("constant", 7, 25, "4:2:2", 95, True, 1), ("noise", 37, 53, "gray", 95, True, 3),
                ("impulses", 25, 7, "4:2:0", 95, True, 0), ("noise", 16, 16, "4:2:0", 1, False, 1), ("saturated", 9, 17, "gray", 100, False, 1),
                ("impulses", 64, 96, "4:4:4", 95, True, 3)]


def golden_path(f):
    return os.path.join(GOLDEN, file_id(f) + ".jpg")
