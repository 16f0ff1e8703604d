"""The inputs the PNG decoder's tests share (tests/test_png_decode_spec.py and tests/test_png_decode_host.py on the CPU,
tests/test_gpu_png_decode.py on the device): numpy + stdlib, seeded, built once per process.

  foreign()   files a standard encoder writes: stdlib zlib at several levels and strategies, with Z_FULL_FLUSH / Z_SYNC_FLUSH cuts or
              none, re-cut into small IDATs, with a zero-length IDAT, with ancillary chunks; filter types forced to cycle 0..4 from
              row 0 on, so that Up / Average / Paeth meet the zero row above and the missing left pixel
  handmade()  deflate streams assembled bit by bit (png_ref.Bits) for what zlib never writes or writes rarely
  bad()       one broken input per rule -> the specification's status bit

Every file is (id, bytes, frame in R G B (A) order)."""
from __future__ import annotations

import functools
import struct
import zlib

import numpy as np

from tests import png_cases, png_decode_ref as ref, png_ref
from tests.jpeg_decode_cases import SCAN_LANES, kernel_constant  # noqa: F401

KINDS = png_cases.KINDS
STRATEGIES = [("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
              ("fixed", 6, zlib.Z_FIXED), ("huff", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE)]
CONTENTS = ["runs", "gradient", "two", "impulses"]


def filtered_cycle(frame, first=0):
    """frame (R G B (A) order) -> the filtered stream [H, 1 + W bpp] with filter type (first + y) % 5 on row y"""
    raw, bpp, _, _ = png_ref.file_rows(frame, "rgb")
    h, n = raw.shape
    x = raw.astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255
    types = (first + np.arange(h)) % 5
    out = np.empty((h, n + 1), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(h)]
    return out


def deflate_parts(stream, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None, every=None):
    """-> the zlib stream as a list of parts; with `flush` ("full" / "sync") a part ends after every `every` bytes of input"""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if flush is None:
        return [co.compress(stream) + co.flush()]
    mode = zlib.Z_FULL_FLUSH if flush == "full" else zlib.Z_SYNC_FLUSH
    parts = []
    for at in range(0, len(stream), every):
        parts.append(co.compress(stream[at:at + every]) + co.flush(mode))
    parts.append(co.flush())
    return parts


def make_file(h, w, c, depth, parts, before=(), after=()):
    """A PNG file whose IDATs are `parts`; `before` / `after`: ancillary (kind, payload) chunks around the IDATs"""
    ihdr = struct.pack(">IIBBBBB", w, h, depth, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0)
    out = [png_ref.SIGNATURE, png_ref.chunk(b"IHDR", ihdr)]
    out += [png_ref.chunk(k, p) for k, p in before]
    out += [png_ref.chunk(b"IDAT", p) for p in parts]
    out += [png_ref.chunk(k, p) for k, p in after]
    return b"".join(out + [png_ref.chunk(b"IEND", b"")])


def recut(parts, size):
    z = b"".join(parts)
    return [z[i:i + size] for i in range(0, len(z), size)]


def _frame(kind, h, w, c, depth):
    """png_cases.content, the crop (R G B), and `period8`: rows that repeat with a period of 8 bytes, so that matches reach across every
    flush point"""
    if kind == "crop":
        return np.ascontiguousarray(png_cases.crop_bgr()[:, :, ::-1])
    if kind == "period8":
        rng = np.random.RandomState(8)
        row = np.tile(rng.randint(0, 256, 8).astype(np.uint8), (w * c + 7) // 8)[:w * c]
        return np.tile(row.reshape(1, w, c), (h, 1, 1))
    return png_cases.content(kind, h, w, c, depth)


@functools.lru_cache(maxsize=None)
def foreign():
    out = []

    def add(cid, kind, h, w, c, depth, **kw):
        cut, before, after, empty = kw.pop("cut", None), kw.pop("before", ()), kw.pop("after", ()), kw.pop("empty", False)
        frame = _frame(kind, h, w, c, depth)
        filt = filtered_cycle(frame, first=kw.pop("first", 0))
        parts = deflate_parts(filt.tobytes(), **kw)
        if cut:
            parts = recut(parts, cut)
        if empty:
            parts = parts[:len(parts) // 2] + [b""] + parts[len(parts) // 2:]
        out.append((f"{h}x{w}x{c}x{depth}-{kind}-{cid}", make_file(h, w, c, depth, parts, before, after), frame))

    k = 0
    for shape in [(1, 1), (1, 2), (3, 1), (2, 3)]:
        for c, d in KINDS:
            name, level, strat = STRATEGIES[k % 7]
            add(name, "gradient" if k % 2 else "two", *shape, c, d, level=level, strategy=strat)
            k += 1
    for c, d in KINDS:
        for i, (name, level, strat) in enumerate(STRATEGIES):
            add(name, CONTENTS[(i + c) % 4], 37, 53, c, d, level=level, strategy=strat, first=i % 5)
        row = 1 + 53 * c * d // 8
        add("full", "runs", 37, 53, c, d, flush="full", every=5 * row + 3)
        add("sync", "impulses", 37, 53, c, d, flush="sync", every=5 * row + 3)
    for i, (name, level, strat) in enumerate(STRATEGIES):
        add(name, CONTENTS[i % 4], 70, 320, 3, 8, level=level, strategy=strat)
    add("full", "gradient", 70, 320, 3, 8, flush="full", every=9000)
    add("sync8", "period8", 70, 320, 3, 8, flush="sync", every=9000)
    add("full8", "period8", 70, 320, 3, 8, flush="full", every=9000)
    add("cut100", "impulses", 70, 320, 3, 8, cut=100)
    add("empty", "runs", 70, 320, 3, 8, cut=4000, empty=True)
    add("ancillary", "gradient", 70, 320, 3, 8, before=((b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"Comment\0x")), after=((b"tIME", bytes(7)),))
    add("l6", "crop", 64, 96, 3, 8, level=6)
    add("full", "crop", 64, 96, 3, 8, flush="full", every=3000)
    return out


@functools.lru_cache(maxsize=None)
def far_match():
    """A gray frame whose rows repeat with a period of 31 x 1024 bytes of the filtered stream: zlib at level 9 finds matches at a
    distance of 31744 -> (id, bytes, frame).  32 rows of 991 noise bytes (filter type 0) are the period; 3 periods."""
    rng = np.random.RandomState(31)
    block = rng.randint(0, 256, (32, 991)).astype(np.uint8)
    frame = np.tile(block, (3, 1))
    filt = np.zeros((96, 992), np.uint8)
    filt[:, 1:] = frame
    return "96x991x1x8-period31744", make_file(96, 991, 1, 8, deflate_parts(filt.tobytes(), level=9)), frame


# Two files beyond the grid, each the smallest that makes one loop of the all-device route take a second turn
# (test_png_decode_spec.py asserts it from the parsed plan) -> (id, bytes, frame)
@functools.lru_cache(maxsize=None)
def many_segments():
    """Gray noise 64 x 1040 with a Z_FULL_FLUSH every 64 bytes: over 1024 contiguous segments (pngd_scan carries across a step)"""
    frame = np.random.RandomState(1040).randint(0, 256, (64, 1040)).astype(np.uint8)
    parts = deflate_parts(filtered_cycle(frame).tobytes(), flush="full", every=64)
    return "64x1040x1x8-noise-full64", make_file(64, 1040, 1, 8, parts), frame


@functools.lru_cache(maxsize=None)
def many_pieces():
    """Gray 2049 x 4100 of 8 x 8 squares, level 1 with a Z_FULL_FLUSH every 32768 bytes: a filtered stream of 257 Adler pieces, two per
    lane of pngd_adler_check.  Every row has filter type 0; the frame itself is what the lossless file holds."""
    y, x = np.ogrid[:2049, :4100]
    frame = ((y // 8 + x // 8 + 41) % 256).astype(np.uint8)
    filt = np.zeros((2049, 4101), np.uint8)
    filt[:, 1:] = frame
    return "2049x4100x1x8-squares-full32768", make_file(2049, 4100, 1, 8, deflate_parts(filt.tobytes(), level=1, flush="full", every=32768)), frame


# ------------------------------------------------------------------------------------------------ hand-made streams
FIXED_CODES = png_ref.canonical_codes(png_ref.FIXED_LENGTHS)


def _rev(v, n):
    return int(format(v, f"0{n}b")[::-1], 2) if n else 0


class Stream:
    """A deflate stream written token by token"""

    def __init__(self):
        self.bits = png_ref.Bits()
        self.n = 0

    def put(self, v, n):
        if n:
            self.bits.put(v, n)
            self.n += n

    def align(self):
        self.put(0, (-self.n) % 8)

    def stored(self, data, final=0, nlen=None):
        self.put(final, 3)
        self.align()
        self.put(len(data), 16)
        self.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        for v in data:
            self.put(int(v), 8)

    def fixed(self, tokens, final=0):
        """tokens: int literal / 256 | (length symbol, extra value, distance symbol, extra value)"""
        self.put(final | 2, 3)
        self.body(tokens, FIXED_CODES, png_ref.FIXED_LENGTHS, [_rev(s, 5) for s in range(32)], [5] * 32)

    def body(self, tokens, lcodes, llens, dcodes, dlens):
        for t in tokens:
            if isinstance(t, tuple):
                ls, lv, ds, dv = t
                self.put(lcodes[ls], llens[ls])
                self.put(lv, png_ref.symbol_extra_bits(ls) if ls <= 285 else 0)
                self.put(dcodes[ds], dlens[ds])
                self.put(dv, ref.DIST_EXTRA[ds] if ds < 30 else 0)
            else:
                self.put(lcodes[t], llens[t])

    def dynamic(self, lit, dist, cl, rle, tokens, final=0, hlit=None, hdist=None):
        """lit / dist / cl: code lengths (cl: 19 entries); rle: [(code-length symbol, extra value)] as written"""
        self.put(final | 4, 3)
        self.put((len(lit) if hlit is None else hlit) - 257, 5)
        self.put((len(dist) if hdist is None else hdist) - 1, 5)
        hclen = max([i for i in range(19) if cl[png_ref.CL_ORDER[i]]] + [3]) + 1
        self.put(hclen - 4, 4)
        for i in range(hclen):
            self.put(cl[png_ref.CL_ORDER[i]], 3)
        clc = png_ref.canonical_codes(cl)
        for s, v in rle:
            self.put(clc[s], cl[s])
            self.put(v, {16: 2, 17: 3, 18: 7}.get(s, 0))
        self.body(tokens, png_ref.canonical_codes(lit), lit, png_ref.canonical_codes(dist), dist)

    def to_bytes(self):
        self.align()
        return self.bits.to_bytes()


def zwrap(d, stream):
    """deflate bytes -> zlib stream with the Adler-32 of `stream`"""
    return b"\x78\x01" + d + struct.pack(">I", zlib.adler32(bytes(stream)) & 0xFFFFFFFF)


def _gray_row(d, expect):
    """A 1 x (N - 1) gray frame whose filtered stream is `expect` (its first byte the filter type 0) -> (bytes, frame)"""
    expect = np.asarray(expect, np.uint8)
    assert expect[0] == 0
    return make_file(1, len(expect) - 1, 1, 8, [zwrap(d, expect)]), expect[None, 1:].copy()


# the dynamic header of `cross16`: four 2-bit literal/length codes (0, 1, 256, 257) and four 2-bit distance codes; the lengths of
# symbol 257 and of the four distance codes are ONE run of code 16 that starts in the literal/length code and ends in the distance code
_X_LIT = [2, 2] + [0] * 254 + [2, 2]
_X_DIST = [2, 2, 2, 2]
_X_CL = [0, 0, 1] + [0] * 13 + [2, 0, 2]
_X_RLE = [(2, 0), (2, 0), (18, 127), (18, 105), (2, 0), (16, 2)]
_W_CL = [3, 3, 2] + [0] * 13 + [3, 3, 2]                # a code-length code that also has 0, 1 and 17


@functools.lru_cache(maxsize=None)
def handmade():
    out = []

    def add(cid, s, expect):
        data, frame = _gray_row(s.to_bytes(), expect)
        out.append((f"hand-{cid}", data, frame))

    s = Stream()
    s.fixed([0, 7, (257, 0, 0, 0), 256], final=1)
    add("len3-dist1", s, [0, 7, 7, 7, 7])
    s = Stream()
    s.fixed([0, 9, (285, 0, 0, 0), 256], final=1)
    add("len258-sym285", s, [0] + [9] * 259)
    s = Stream()
    s.fixed([0, 9, (284, 31, 0, 0), 256], final=1)
    add("len258-sym284", s, [0] + [9] * 259)
    rng = np.random.RandomState(5)
    far = np.concatenate([[0], rng.randint(0, 256, 32767)]).astype(np.uint8)
    s = Stream()
    s.stored(far)
    s.fixed([(285, 0, 29, 8191), 256], final=1)
    add("dist32768", s, np.concatenate([far, far[:258]]))
    s = Stream()
    s.fixed([0, 1, 2, (264, 0, 1, 0), 256], final=1)
    add("overlap", s, [0, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2])
    s = Stream()
    s.stored([0, 5, 6])
    s.stored([])
    s.stored([])
    s.stored([7], final=1)
    add("stored-len0", s, [0, 5, 6, 7])
    alt = np.concatenate([[0], np.tile([5, 9], 150)]).astype(np.uint8)
    stats = {}
    d = png_ref.deflate_chunk(alt, True, stats)
    assert stats.get("btype2") == 1 and stats.get("nomatch_chunks") == 1
    out.append(("hand-nodist",) + _gray_row(d, alt))
    s = Stream()
    s.dynamic(_X_LIT, _X_DIST, _X_CL, _X_RLE, [0, 1, (257, 0, 0, 0), 256], final=1)
    add("cross16", s, [0, 1, 1, 1, 1])
    return out


# ------------------------------------------------------------------------------------------------ broken inputs
def _dyn(lit=_X_LIT, dist=_X_DIST, cl=_X_CL, rle=_X_RLE, tokens=(0, 1, 256), **kw):
    s = Stream()
    s.dynamic(list(lit), list(dist), list(cl), list(rle), list(tokens), final=1, **kw)
    return s.to_bytes()


def _fixed(tokens):
    s = Stream()
    s.fixed(tokens, final=1)
    return s.to_bytes()


@functools.lru_cache(maxsize=None)
def bad():
    """[(id, file bytes, status bit)]: one input per rule of the inflate list, each a 1 x 4 gray file (N = 5) unless the rule needs more"""
    out = []

    def add(cid, d, status, expect=(0, 1, 1, 1, 1), n=None):
        z = zwrap(d, bytes(expect))
        out.append((f"bad-{cid}", make_file(1, (n or 5) - 1, 1, 8, [z]), status))

    good = _fixed([0, 1, (257, 0, 0, 0), 256])
    add("truncated", good[:-1], ref.TRUNC)
    add("lit286", _fixed([0, 1, 286, 256]), ref.BADCODE)
    add("dist30", _fixed([0, 1, (257, 0, 30, 0), 256]), ref.BADCODE)
    s = Stream()
    s.stored([0, 1, 1, 1, 1], final=1, nlen=0x1234)
    add("nlen", s.to_bytes(), ref.BADSTORED)
    add("btype3", bytes([0x07, 0, 0, 0]), ref.BADHEADER)
    add("hlit30", _dyn(hlit=287), ref.BADHEADER)
    add("hdist30", _dyn(hdist=31), ref.BADHEADER)
    add("rep16-first", _dyn(rle=[(16, 0)] + _X_RLE), ref.BADHEADER)
    add("overrun", _dyn(rle=_X_RLE[:-1] + [(16, 3)]), ref.BADHEADER)
    zeros = [(18, 127), (18, 105)]                      # 254 zero lengths: symbols 2 .. 255
    dist4 = [(2, 0)] * 4
    add("no256", _dyn(cl=_W_CL, rle=[(2, 0), (2, 0)] + zeros + [(0, 0), (2, 0)] + dist4), ref.BADHEADER)
    add("oversubscribed", _dyn(cl=_W_CL, rle=[(1, 0), (1, 0)] + zeros + [(1, 0), (1, 0)] + dist4), ref.BADHEADER)
    add("incomplete", _dyn(cl=_W_CL, rle=[(2, 0), (0, 0)] + zeros + [(2, 0), (0, 0)] + dist4), ref.BADHEADER)
    add("cl-incomplete", _dyn(cl=[0, 0, 2] + [0] * 13 + [2, 0, 2]), ref.BADHEADER)
    nodist = _dyn(dist=[0], cl=_W_CL, rle=[(2, 0), (2, 0)] + zeros + [(2, 0), (2, 0), (0, 0)], tokens=[0, 1, (257, 0, 0, 0), 256])
    add("match-without-distance-code", nodist + bytes(3), ref.BADCODE)
    s = Stream()
    s.fixed([0, 1, (257, 0, 2, 0), 256], final=1)
    add("distance-before-start", s.to_bytes(), ref.DEPENDENT)
    add("trailing", good + b"\0", ref.BADEND)
    return out


@functools.lru_cache(maxsize=None)
def corrupt():
    """The six corrupt files of the device test -> [(id, bytes, status bit)].  The first three are two-segment files (a Z_FULL_FLUSH cut)
    whose last segment is broken, so that the measuring pass meets a good and a bad segment in one launch."""
    frame = png_cases.content("gradient", 37, 53, 3, 8)
    filt = filtered_cycle(frame).tobytes()
    head = zlib.compressobj(6, zlib.DEFLATED, 15, 8)
    first = head.compress(filt[:3000]) + head.flush(zlib.Z_FULL_FLUSH)
    rest = head.compress(filt[3000:]) + head.flush()                   # the last segment and the Adler-32
    tail, adler = rest[:-4], rest[-4:]

    def two(last_seg, check=adler):
        return make_file(37, 53, 3, 8, [first, last_seg + check])

    lit286 = Stream()
    lit286.fixed([1, 286, 256], final=1)
    nlen = Stream()
    nlen.stored(filt[3000:3010], final=1, nlen=0x1234)
    short = zlib.compressobj(6, zlib.DEFLATED, 15, 8)
    short_z = short.compress(filt[:-7]) + short.flush()
    five = bytearray(filt)
    five[160] = 5                                                       # the type byte of row 1
    out = [("truncated", two(tail[:-2]), ref.TRUNC),
           ("code", two(lit286.to_bytes()), ref.BADCODE),
           ("nlen", two(nlen.to_bytes()), ref.BADSTORED),
           ("adler", two(tail, bytes([adler[0] ^ 1]) + adler[1:]), ref.ADLER),
           ("total", make_file(37, 53, 3, 8, [short_z]), ref.TOTAL),
           ("filter5", make_file(37, 53, 3, 8, [zlib.compress(bytes(five), 6)]), ref.FILTER)]
    return out


# ------------------------------------------------------------------------------------------------ files the parser classifies
def _raw_file(ihdr, parts, pre=(), post=()):
    out = [png_ref.SIGNATURE, png_ref.chunk(b"IHDR", ihdr)] + [png_ref.chunk(k, p) for k, p in pre]
    out += [png_ref.chunk(b"IDAT", p) for p in parts] + [png_ref.chunk(k, p) for k, p in post]
    return b"".join(out + [png_ref.chunk(b"IEND", b"")])


@functools.lru_cache(maxsize=None)
def unsupported_files():
    """[(id, bytes)]: valid PNG headers outside the supported list"""
    z = [zlib.compress(bytes(64))]
    ihdr = lambda w, h, depth, ctype, lace=0: struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, lace)      # noqa: E731
    return [("palette", _raw_file(ihdr(4, 4, 8, 3), z, pre=((b"PLTE", bytes(6)),))), ("gray-alpha", _raw_file(ihdr(4, 4, 8, 4), z)),
            ("gray-alpha16", _raw_file(ihdr(4, 4, 16, 4), z)), ("depth1", _raw_file(ihdr(4, 4, 1, 0), z)), ("depth2", _raw_file(ihdr(4, 4, 2, 0), z)),
            ("depth4", _raw_file(ihdr(4, 4, 4, 0), z)), ("adam7", _raw_file(ihdr(4, 4, 8, 2, 1), z)), ("wide", _raw_file(ihdr(65536, 1, 8, 0), z))]


@functools.lru_cache(maxsize=None)
def badfile_files():
    """[(id, bytes)]: malformed structure, or a zlib header the decoder refuses"""
    ihdr = struct.pack(">IIBBBBB", 4, 1, 8, 0, 0, 0, 0)
    stream = bytes(5)
    z = zlib.compress(stream)
    good = _raw_file(ihdr, [z])
    d, adler = z[2:-4], z[-4:]
    crc = bytearray(good)
    crc[29] ^= 1
    longer = bytearray(good)
    longer[33:37] = struct.pack(">I", 1000)                                   # the IDAT's length field
    return [("signature", b"\x89PNX" + good[4:]), ("empty", b""), ("short", good[:20]), ("ihdr-crc", bytes(crc)),
            ("ihdr-second", png_ref.SIGNATURE + png_ref.chunk(b"gAMA", bytes(4)) + good[8:]),
            ("two-ihdr", _raw_file(ihdr, [z], pre=((b"IHDR", ihdr),))), ("no-idat", _raw_file(ihdr, [])),
            ("idat-apart", png_ref.SIGNATURE + png_ref.chunk(b"IHDR", ihdr) + png_ref.chunk(b"IDAT", z[:5]) + png_ref.chunk(b"tEXt", b"a\0b") +
             png_ref.chunk(b"IDAT", z[5:]) + png_ref.chunk(b"IEND", b"")),
            ("no-iend", good[:-12]), ("after-iend", good + b"\0"), ("length", bytes(longer)), ("critical", _raw_file(ihdr, [z], pre=((b"ABCD", b""),))),
            ("zero-width", _raw_file(struct.pack(">IIBBBBB", 0, 1, 8, 0, 0, 0, 0), [z])), ("depth3", _raw_file(struct.pack(">IIBBBBB", 4, 1, 3, 0, 0, 0, 0), [z])),
            ("filter-method", _raw_file(struct.pack(">IIBBBBB", 4, 1, 8, 0, 0, 1, 0), [z])), ("cm", _raw_file(ihdr, [b"\x79\x01"[:1] + b"\x9b" + d + adler])),
            ("fdict", _raw_file(ihdr, [b"\x78\x20" + d + adler])), ("fcheck", _raw_file(ihdr, [b"\x78\x02" + d + adler])),
            ("window", _raw_file(ihdr, [b"\x88\x1c" + d + adler])), ("tiny-z", _raw_file(ihdr, [b"\x78\x01", b"\0\0\0\1"]))]
