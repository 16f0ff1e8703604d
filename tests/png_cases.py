"""The grid the PNG tests share (tests/test_png_spec.py on the CPU, tests/test_gpu_png.py on the device), seeded and numpy only, and
the specification's bytes for a case, computed once per process.

Shapes, the smallest at which each rule can go wrong (S = 32768 filtered bytes per deflate chunk, a filtered row is 1 + W bpp bytes):
  (1,1) (1,2) (3,1) (2,3)   tiny frames: no left neighbour, no row above, a stream shorter than any table
  (37,53)                   a plain mid-sized frame, all six kinds, every content
  (32,1023) gray 8          N = S exactly: one full chunk and no empty one behind it
  (64,1023) gray 8          N = 2 S
  (33,1023) gray 8          one chunk and a remainder of one row
  (70,320)                  RGB 8: 3 chunks, boundaries in the middle of rows; all six kinds (up to 6 chunks)
  (2,20000) RGB 8           a row that crosses two chunk boundaries
  (33,130) RGBA 16          bpp 8, 2 chunks
Contents: noise, constant, runs (run lengths from 1-4, 258-262 and 516-520 at the level of the file's bytes, so that every remainder
rule of the tokeniser is hit and runs are cut by chunk boundaries), gradient, two (two-valued), impulses, the committed photograph's
crop, and deep (byte counts in Fibonacci proportion, shuffled, so that the unrestricted Huffman code of a chunk is deeper than 15;
at (33,1023) gray 8, where its block is exactly the first chunk)."""
from __future__ import annotations

import functools
import os

import numpy as np

from tests import png_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = [(1, 8), (3, 8), (4, 8), (1, 16), (3, 16), (4, 16)]
CONTENTS = ["noise", "constant", "runs", "gradient", "two", "impulses", "deep"]


def _from_file_bytes(stream, h, w, c, depth):
    """file bytes [h * w * bpp] -> the frame (RGB(A) order, native uint16 for 16 bit)"""
    raw = np.ascontiguousarray(stream.astype(np.uint8).reshape(h, -1))
    img = raw.view(">u2").astype(np.uint16) if depth == 16 else raw
    return img.reshape(h, w, c)[:, :, 0] if c == 1 else img.reshape(h, w, c)


def content(kind, h, w, c, depth):
    """The seeded frame of a case: [h, w] for c = 1, else [h, w, c]; uint8 or uint16."""
    rng = np.random.RandomState((h * 7919 + w * 31 + c * 7 + depth + CONTENTS.index(kind) * 1000003) % (2 ** 31))
    n = h * w * c * depth // 8
    dtype = np.uint16 if depth == 16 else np.uint8
    top = 65535 if depth == 16 else 255
    shape = (h, w) if c == 1 else (h, w, c)
    if kind == "noise":
        return rng.randint(0, top + 1, shape).astype(dtype)
    if kind == "constant":
        return np.full(shape, 0x4D4D if depth == 16 else 77, dtype)
    if kind == "runs":
        lengths = np.concatenate([np.arange(1, 5), np.arange(258, 263), np.arange(516, 521)])
        out = np.empty(0, np.uint8)
        while len(out) < n:
            k = rng.choice(lengths, 64, p=np.r_[np.full(4, 0.2), np.full(10, 0.02)])
            out = np.concatenate([out, np.repeat(rng.randint(0, 256, 64).astype(np.uint8), k)])
        return _from_file_bytes(out[:n], h, w, c, depth)
    if kind == "gradient":
        ramp = np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 2
        if depth == 16:
            ramp = ramp * 257 + 40
        img = ramp if c == 1 else np.stack([ramp, ramp[::-1] * 2, top - ramp, ramp // 3][:c], -1)
        return (img % (top + 1)).astype(dtype)
    if kind == "two":
        return (rng.randint(0, 2, shape) * top).astype(dtype)
    if kind == "impulses":
        ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 2) % 256
        img = ramp if c == 1 else np.stack([ramp, ramp[::-1], 255 - ramp, ramp // 2][:c], -1)
        img = (img * (257 if depth == 16 else 1)).astype(dtype)
        img[rng.randint(0, 24, shape) == 0] = top
        return img
    if kind == "deep":
        # One block of 32 x 1023 bytes: 16 values with the counts 1597, 987, ..., 3, 2, 1 (Fibonacci) and 43 more that share the rest,
        # about 664 each.  With the end-of-block symbol's count of 1 the chain 1, 1, 2, 3, ... is a chain up to 377 (a node of weight
        # 986, its deepest leaf 13 below it), and that node sits about log2(32768 / 986) = 5 levels deep among the rest: an unrestricted
        # depth near 18.  No value is frequent enough for runs of four, so there is no match to disturb the counts.  Values are 0, +1,
        # -1, +2, ...: spread around zero, so filter type 0 wins the rows and the file's bytes are these.  At (33, 1023) gray 8 the
        # block is exactly the first chunk's 32 rows.
        fib = [1, 2]
        while len(fib) < 16:
            fib.append(fib[-1] + fib[-2])
        size = 32 * 1023
        rest = size - sum(fib)
        counts = fib[::-1] + [rest // 43 + (1 if i < rest % 43 else 0) for i in range(43)]
        values = np.array([(i + 1) // 2 if i % 2 else 256 - i // 2 for i in range(59)], np.int64) % 256
        block = np.repeat(values.astype(np.uint8), counts)
        out = np.concatenate([rng.permutation(block) for _ in range(n // size + 1)])
        return _from_file_bytes(out[:n], h, w, c, depth)
    raise ValueError(kind)


def crop_bgr():
    return np.load(os.path.join(GOLDEN, "test_jpeg_crop_64x96_bgr.npy"))


def _grid():
    out = []
    for shape in [(1, 1), (1, 2), (3, 1), (2, 3)]:
        out += [("noise", shape, k) for k in KINDS] + [("constant", shape, (3, 8))]
    out += [(kind, (37, 53), k) for k in KINDS for kind in CONTENTS[:6]]
    out += [(kind, (32, 1023), (1, 8)) for kind in ("noise", "constant", "runs")]
    out += [(kind, (64, 1023), (1, 8)) for kind in ("noise", "runs")]
    out += [(kind, (33, 1023), (1, 8)) for kind in ("runs", "two", "deep")]
    out += [(kind, (70, 320), (3, 8)) for kind in ("noise", "constant", "runs", "gradient", "impulses")]
    out += [("runs", (70, 320), k) for k in KINDS if k != (3, 8)]
    out += [(kind, (2, 20000), (3, 8)) for kind in ("runs", "noise", "constant")]
    out += [(kind, (33, 130), (4, 16)) for kind in ("noise", "runs", "gradient")]
    return out


def cases():
    """(id, content, h, w, c, depth) of every frame of the grid; the crop is its own content, in BGR order."""
    out = [(f"{h}x{w}x{c}x{d}-{kind}", kind, h, w, c, d) for kind, (h, w), (c, d) in _grid()]
    return out + [("64x96x3x8-crop", "crop", 64, 96, 3, 8)]


def image(kind, h, w, c, depth):
    """The case's frame and its channel order."""
    if kind == "crop":
        return crop_bgr(), "bgr"
    return content(kind, h, w, c, depth), "rgb"


def file_order(img, order):
    """The frame a decoder returns for (img, order): channels R G B (A)."""
    if order == "bgr" and img.ndim == 3 and img.shape[2] >= 3:
        return np.concatenate([img[:, :, 2::-1], img[:, :, 3:]], axis=2)
    return img


@functools.lru_cache(maxsize=None)
def spec(kind, h, w, c, depth):
    """(bytes, counters) of the specification for a case; computed once and shared."""
    img, order = image(kind, h, w, c, depth)
    return png_ref.encode_png_stats(img, order)


# the committed files of tests/golden/png (tests/make_png_golden.py writes them): (content, h, w, c, depth)
GOLDEN_FILES = [("noise", 1, 1, 1, 8), ("noise", 2, 3, 4, 16), ("constant", 37, 53, 3, 8), ("runs", 37, 53, 1, 8), ("gradient", 37, 53, 3, 16),
                ("two", 37, 53, 4, 8), ("impulses", 37, 53, 1, 16), ("crop", 64, 96, 3, 8), ("deep", 33, 1023, 1, 8), ("runs", 33, 130, 4, 16)]


def golden_path(kind, h, w, c, depth):
    return os.path.join(GOLDEN, "png", f"{kind}_{h}x{w}x{c}x{depth}.png")
