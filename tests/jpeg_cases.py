"""The shape, content and quality grid the JPEG tests share (tests/test_jpeg_spec.py on the CPU, tests/test_gpu_jpeg.py on the
device), seeded and numpy only, and the specification's bytes for a case, computed once per process."""
from __future__ import annotations

import functools
import os

import numpy as np

from tests import jpeg_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CROP = "crop"                      # tests/golden/test_jpeg_crop_64x96_bgr.npy, a photograph's crop in BGR order

# (H, W, channels).  Colour: the smallest frames, dummy Y blocks at the bottom (17 x 9) and at the right (9 x 17), H = 8 mod 16 (the
# chroma rows' own padding rule), W = 8 mod 16, odd sizes, more than one MCU row and column.  The last three cross the kernels' own
# boundaries at least twice (csrc/jpeg.hip):
#   16 x 4112 colour  257 MCUs in one row: 17 strips of the transform (16 MCUs each), 1542 blocks = 7 workgroups of the length and
#                     emit passes = 7 chunks of the bit-offset scan (256 blocks each); its noise stream spans over 20 chunks of
#                     the byte-stuffing scan (4096 bytes each)
#   520 x 24 colour   33 MCU rows of 2: 396 blocks, a workgroup boundary inside an MCU row
#   24 x 1600 gray    3 block rows of 200: 3 strips of the gray transform (96 blocks each) per row, 600 blocks = 3 workgroups
SHAPES = [(1, 1, 3), (8, 8, 3), (16, 16, 3), (17, 9, 3), (9, 17, 3), (24, 16, 3), (8, 16, 3), (16, 24, 3), (37, 53, 3), (7, 25, 3), (25, 7, 3),
          (200, 333, 3), (16, 4112, 3), (520, 24, 3), (1, 1, 1), (9, 17, 1), (37, 53, 1), (24, 1600, 1)]
CONTENTS = ["noise", "constant", "saturated", "impulses"]
QUALITIES = [1, 30, 95, 100]


def content(kind, h, w, c):
    """The seeded image of a case: HWC for c = 3, HW for c = 1."""
    rng = np.random.RandomState((h * 7919 + w * 31 + c + {"noise": 0, "constant": 1, "saturated": 2, "impulses": 3}[kind] * 1000003) % (2 ** 31))
    shape = (h, w, 3) if c == 3 else (h, w)
    if kind == "noise":
        return rng.randint(0, 256, shape).astype(np.uint8)
    if kind == "constant":
        return np.full(shape, 77, np.uint8)
    if kind == "saturated":      # 0 / 255 only: 8 x 8 blocks in turn black, white (the largest DC steps) and random per sample (the largest AC)
        img = (rng.randint(0, 2, shape) * 255).astype(np.uint8)
        turn = (np.arange(h)[:, None] // 8 + np.arange(w)[None, :] // 8) % 3
        img[turn == 0] = 0
        img[turn == 1] = 255
        return img
    ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 2) % 256         # a gradient with isolated impulses
    img = ramp if c == 1 else np.stack([ramp, ramp[::-1], 255 - ramp], -1)
    img = img.astype(np.uint8)
    img[rng.randint(0, 24, shape) == 0] = 255
    return img


def crop_bgr():
    return np.load(os.path.join(GOLDEN, "test_jpeg_crop_64x96_bgr.npy"))


def cases():
    """(id, kind, h, w, c) of every image of the grid; the crop is its own content."""
    out = [(f"{h}x{w}x{c}-{kind}", kind, h, w, c) for (h, w, c) in SHAPES for kind in CONTENTS]
    return out + [("64x96x3-crop", CROP, 64, 96, 3)]


def image(kind, h, w, c):
    """The case's image and its channel order."""
    if kind == CROP:
        return crop_bgr(), "bgr"
    return content(kind, h, w, c), "rgb"


@functools.lru_cache(maxsize=None)
def spec(kind, h, w, c, quality):
    """(bytes, counters) of the specification for a case; computed once and shared."""
    img, order = image(kind, h, w, c)
    return jpeg_ref.encode_jpeg_stats(img, quality, order)


# the committed files of tests/golden/jpeg (tests/make_jpeg_golden.py writes them with Pillow): (kind, h, w, c, quality)
GOLDEN_FILES = [("noise", 1, 1, 3, 100), ("noise", 17, 9, 3, 95), ("saturated", 9, 17, 3, 100), ("impulses", 24, 16, 3, 30), ("noise", 8, 16, 3, 1),
                ("impulses", 37, 53, 3, 95), ("constant", 7, 25, 3, 95), (CROP, 64, 96, 3, 95), ("noise", 37, 53, 1, 95), ("saturated", 9, 17, 1, 100)]


def golden_path(kind, h, w, c, quality):
    return os.path.join(GOLDEN, "jpeg", f"{kind}_{h}x{w}x{c}_q{quality}.jpg")
