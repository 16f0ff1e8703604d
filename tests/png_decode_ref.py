"""The specification of the device PNG decoder (csrc/png_decode.hip, csrc/png_decode_api.cpp): pure numpy + stdlib.

parse(data) -> (info, segments)      the chunk walk and the segment plan (nesr_png_parse restates it in C++)
inflate_segment(b, first, last)      a plain inflate with the kernel's exact rules -> (bytes, status, counters)
inflate_plan(data, info, segments)   every segment inflated alone -> (filtered stream, status, counters)
unfilter(filtered, bpp)              the five row filters undone -> raw rows
decode(data)                         the frame ([H, W] or [H, W, C], uint8 / uint16, R G B (A) order), zlib for the entropy stage

File.  Signature; chunks walked with their lengths checked against the file's; IHDR first (13 bytes, CRC checked); IDATs consecutive and
at least one; ancillary chunks and PLTE skipped; IEND last with nothing behind it.  The CRCs of the other chunks are NOT checked: the
Adler-32 of the inflated stream covers the data instead.  Supported: depth 8 or 16, colour type 0, 2 or 6, no interlace, at most
65535 x 65535.  UNSUPPORTED: palette, gray+alpha, depth 1 / 2 / 4, Adam7, larger frames.  BADFILE: anything malformed, and a zlib header
with CM != 8, a window above 32 KiB, FDICT set or a bad check value.

Segment plan.  Z is the concatenation of the IDAT payloads, D = Z[2:-4] the deflate stream.  A cut is an IDAT boundary strictly inside
D whose preceding four bytes of D are 00 00 FF FF (the empty stored block of a flush).  A segment is the D-bytes between consecutive cuts:
(file offset of its first byte, byte length, first, last).  The plan is contiguous when no segment spans an IDAT boundary: only then
are a segment's bytes file[offset : offset + bytes], and only such plans go to the device inflater.

Inflate (RFC 1951), per segment.  Bits are read LSB first, Huffman codes are packed MSB first.  A non-last segment ends where a block
without BFINAL ends exactly at the segment's last byte; a block with BFINAL there is BADEND.  The last segment ends with its BFINAL
block, whose pad bits are ignored; bytes behind it are BADEND.  Input that runs out is TRUNC.  A distance larger than the bytes the
segment itself has produced is DEPENDENT: a status, not a bad file (Z_SYNC_FLUSH writes such files; the whole stream then inflates on
the host).  The whole stream: the sizes must add up to N = H (1 + W bpp) (TOTAL), the Adler-32 must match (ADLER), a filter type above
4 is FILTER."""
import struct
import zlib

import numpy as np

from tests import png_ref

UNSUPPORTED, BADFILE = "unsupported", "badfile"
TRUNC, BADCODE, BADSTORED, BADHEADER, DEPENDENT, BADEND, TOTAL, ADLER, FILTER = 1, 2, 4, 8, 16, 32, 64, 128, 256

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class PngError(ValueError):
    def __init__(self, code, msg):
        super().__init__(f"{code}: {msg}")
        self.code = code


def _bad(msg):
    raise PngError(BADFILE, msg)


def parse(data):
    """-> (info, segments).  info: H, W, C, depth, contiguous, n_segments, stream_bytes, adler.  segments: [(offset, bytes, first, last)]"""
    data = bytes(data)
    n = len(data)
    if n < 8 or data[:8] != png_ref.SIGNATURE:
        _bad("no PNG signature")
    at, idats, state, hdr = 8, [], 0, None            # state 0: before the IDATs, 1: inside them, 2: behind them
    while True:
        if at + 12 > n:
            _bad("the file ends before IEND")
        length, kind = struct.unpack(">I4s", data[at:at + 8])
        if length > 0x7FFFFFFF or at + 12 + length > n:
            _bad("a chunk length past the end")
        if hdr is None:
            if kind != b"IHDR" or length != 13:
                _bad("the first chunk is not IHDR")
            if struct.unpack(">I", data[at + 21:at + 25])[0] != zlib.crc32(data[at + 4:at + 21]) & 0xFFFFFFFF:
                _bad("IHDR's CRC")
            w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", data[at + 8:at + 21])
            legal = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
            if w == 0 or h == 0 or w > 0x7FFFFFFF or h > 0x7FFFFFFF or comp or flt or lace > 1 or depth not in legal.get(ctype, ()):
                _bad("IHDR's fields")
            if lace or ctype not in (0, 2, 6) or depth < 8 or w > 65535 or h > 65535:
                raise PngError(UNSUPPORTED, f"colour type {ctype}, depth {depth}, interlace {lace}, {w} x {h}")
            hdr = (h, w, {0: 1, 2: 3, 6: 4}[ctype], depth)
        elif kind == b"IHDR":
            _bad("two IHDR chunks")
        elif kind == b"IDAT":
            if state == 2:
                _bad("IDAT chunks that are not consecutive")
            state = 1
            idats.append((at + 8, length))
        elif kind == b"IEND":
            if length != 0 or at + 12 != n:
                _bad("IEND is not the end of the file")
            break
        else:
            if not (kind[0] & 0x20) and kind != b"PLTE":
                _bad("an unknown critical chunk")
            state = 2 if state else 0
        at += 12 + length
    zlen = sum(length for _, length in idats)
    if zlen < 7:
        _bad("no deflate stream in the IDATs")

    def zbyte(pos):
        for off, length in idats:
            if pos < length:
                return data[off + pos]
            pos -= length
        raise IndexError

    z0, z1 = zbyte(0), zbyte(1)
    if (z0 & 15) != 8 or (z0 >> 4) > 7 or (z1 & 0x20) or (z0 * 256 + z1) % 31:
        _bad("the zlib header")
    adler = 0
    for k in range(4):
        adler = adler << 8 | zbyte(zlen - 4 + k)
    h, w, c, depth = hdr
    # the pieces of D, the IDAT payloads clipped to Z[2 : zlen - 4): (file offset, D position, length, starts at an IDAT boundary)
    pieces, zpos = [], 0
    for off, length in idats:
        lo, hi = max(zpos, 2), min(zpos + length, zlen - 4)
        if hi > lo:
            pieces.append((off + lo - zpos, lo - 2, hi - lo, lo == zpos))
        zpos += length
    segments, seg_off, seg_at, tail, contiguous = [], pieces[0][0], 0, b"", True
    spans = False
    for off, dpos, length, boundary in pieces:
        if dpos > 0:
            if boundary and tail == b"\x00\x00\xff\xff":
                segments.append((seg_off, dpos - seg_at, seg_at == 0, False))
                contiguous &= not spans
                seg_off, seg_at, spans = off, dpos, False
            elif dpos > seg_at:
                spans = True
        tail = (tail + data[off + max(0, length - 4):off + length])[-4:]
    dlen = zlen - 6
    segments.append((seg_off, dlen - seg_at, seg_at == 0, True))
    contiguous &= not spans
    info = {"H": h, "W": w, "C": c, "depth": depth, "contiguous": int(contiguous), "n_segments": len(segments),
            "stream_bytes": h * (1 + w * c * depth // 8), "adler": adler}
    return info, segments


def deflate_bytes(data):
    """D = Z[2:-4] of a file parse() accepts"""
    z = b"".join(p for k, p in _chunks(data) if k == b"IDAT")
    return z[2:-4]


def _chunks(data):
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        out.append((kind, data[at + 8:at + 8 + n]))
        at += 12 + n
    return out


# ------------------------------------------------------------------------------------------------ inflate
class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Reader:
    def __init__(self, b):
        self.b, self.pos, self.total = b, 0, 8 * len(b)

    def take(self, n):
        """n bits, LSB first; past the end: TRUNC"""
        if self.pos + n > self.total:
            self.pos = self.total + 1
            raise _Stop(TRUNC)
        v = 0
        for k in range(n):
            p = self.pos + k
            v |= ((self.b[p >> 3] >> (p & 7)) & 1) << k
        self.pos += n
        return v


def _build(lengths):
    """code lengths -> (count per length, symbols sorted by (length, symbol), left): left > 0 incomplete, < 0 over-subscribed"""
    count = [0] * 16
    for v in lengths:
        count[v] += 1
    left = 1
    for d in range(1, 16):
        left = (left << 1) - count[d]
        if left < 0:
            return count, [], left
    syms = [s for d in range(1, 16) for s, v in enumerate(lengths) if v == d]
    return count, syms, left


def _decode(r, table):
    """one symbol: the code read bit by bit, MSB first (puff's loop); a code that is in no table: BADCODE"""
    count, syms, _ = table
    code = first = index = 0
    for d in range(1, 16):
        code |= r.take(1)
        if code - count[d] < first:
            return syms[index + code - first]
        index += count[d]
        first = (first + count[d]) << 1
        code <<= 1
    raise _Stop(BADCODE)


FIXED_LIT = _build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = _build([5] * 32)


def inflate_segment(b, first=True, last=True, limit=None):
    """-> (bytes, status, counters).  `limit`: stop with TOTAL when more than that many bytes come out (the kernel's capacity guard)."""
    b = bytes(b)
    r, out = _Reader(b), bytearray()
    seen = {"btype0": 0, "btype1": 0, "btype2": 0, "rep16": 0, "rep17": 0, "rep18": 0, "len258": 0, "far": 0, "overlap": 0, "stored0": 0,
            "nodist": 0, "onedist": 0, "cross16": 0, "maxdist": 0}
    status = 0
    try:
        while True:
            if r.pos == r.total and not last and r.pos > 0:
                break
            final = r.take(1)
            btype = r.take(2)
            if btype == 3:
                raise _Stop(BADHEADER)
            seen[f"btype{btype}"] += 1
            if btype == 0:
                r.pos = (r.pos + 7) & ~7
                ln, nl = r.take(16), r.take(16)
                if ln != (~nl & 0xFFFF):
                    raise _Stop(BADSTORED)
                if r.pos + 8 * ln > r.total:
                    r.pos = r.total + 1
                    raise _Stop(TRUNC)
                seen["stored0"] += ln == 0
                out += b[r.pos >> 3:(r.pos >> 3) + ln]
                r.pos += 8 * ln
            else:
                if btype == 1:
                    lit, dist = FIXED_LIT, FIXED_DIST
                else:
                    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
                    if hlit > 286 or hdist > 30:
                        raise _Stop(BADHEADER)
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[png_ref.CL_ORDER[i]] = r.take(3)
                    clt = _build(cl)
                    if clt[2] != 0:                        # the code-length code must be complete
                        raise _Stop(BADHEADER)
                    lens = []
                    while len(lens) < hlit + hdist:
                        s = _decode(r, clt)
                        if s < 16:
                            lens.append(s)
                            continue
                        if s == 16:
                            if not lens:
                                raise _Stop(BADHEADER)
                            v, rep = lens[-1], 3 + r.take(2)
                        elif s == 17:
                            v, rep = 0, 3 + r.take(3)
                        else:
                            v, rep = 0, 11 + r.take(7)
                        seen[f"rep{s}"] += 1
                        if len(lens) + rep > hlit + hdist:
                            raise _Stop(BADHEADER)
                        seen["cross16"] += s == 16 and len(lens) < hlit < len(lens) + rep
                        lens += [v] * rep
                    if lens[256] == 0:
                        raise _Stop(BADHEADER)
                    lit = _build(lens[:hlit])
                    nlit = hlit - lens[:hlit].count(0)
                    if lit[2] != 0 and not (nlit == 1 and lit[0][1] == 1):
                        raise _Stop(BADHEADER)           # incomplete or over-subscribed (one single 1-bit code is zlib's exception)
                    dist = _build(lens[hlit:])
                    ndist = hdist - lens[hlit:].count(0)
                    if dist[2] < 0 or (dist[2] > 0 and ndist > 0 and not (ndist == 1 and dist[0][1] == 1)):
                        raise _Stop(BADHEADER)
                    seen["nodist"] += ndist == 0
                    seen["onedist"] += ndist == 1
                while True:
                    s = _decode(r, lit)
                    if s < 256:
                        out.append(s)
                    elif s == 256:
                        break
                    else:
                        if s > 285:
                            raise _Stop(BADCODE)
                        ln = LEN_BASE[s - 257] + r.take(LEN_EXTRA[s - 257])
                        d = _decode(r, dist)                # no distance codes: every code is in no table, BADCODE
                        if d > 29:
                            raise _Stop(BADCODE)
                        d = DIST_BASE[d] + r.take(DIST_EXTRA[d])
                        if d > len(out):
                            raise _Stop(DEPENDENT)
                        seen["len258"] += ln == 258
                        seen["far"] += d >= 31744
                        seen["overlap"] += d < ln
                        seen["maxdist"] = max(seen["maxdist"], d)
                        for _ in range(ln):
                            out.append(out[-d])
                    if limit is not None and len(out) > limit:
                        raise _Stop(TOTAL)
            if limit is not None and len(out) > limit:
                raise _Stop(TOTAL)
            if final:
                if not last or (r.pos + 7) >> 3 != len(b):
                    raise _Stop(BADEND)
                break
    except _Stop as e:
        status = e.status
    return bytes(out), status, seen


def inflate_plan(data, info, segments):
    """Every segment of a contiguous plan inflated alone, as the device does -> (filtered stream or None, status bits, counters)"""
    assert info["contiguous"]
    n, parts, status, seen = info["stream_bytes"], [], 0, {"segments": len(segments), "dependent": 0}
    for off, nbytes, first, last in segments:
        out, st, cnt = inflate_segment(data[off:off + nbytes], first, last, limit=n)
        status |= st
        seen["dependent"] += st == DEPENDENT
        for k, v in cnt.items():
            seen[k] = max(seen.get(k, 0), v) if k == "maxdist" else seen.get(k, 0) + v
        parts.append(out)
    stream = b"".join(parts)
    if not status and len(stream) != n:
        status |= TOTAL
    if not status and zlib.adler32(stream) & 0xFFFFFFFF != info["adler"]:
        status |= ADLER
    if not status and filter_types(stream, info).max() > 4:
        status |= FILTER
    return (stream if not status else None), status, seen


def filter_types(stream, info):
    return np.frombuffer(stream, np.uint8).reshape(info["H"], -1)[:, 0]


# ------------------------------------------------------------------------------------------------ unfilter
def unfilter(filtered, bpp):
    """filtered uint8 [H, 1 + n] -> raw uint8 [H, n].  Types 0 and 2 are whole-row operations, Sub is a running sum per byte lane;
    Average and Paeth walk the row pixel by pixel (vectorised over the bpp bytes of a pixel)."""
    filtered = np.asarray(filtered, np.uint8)
    h, n = filtered.shape[0], filtered.shape[1] - 1
    raw = np.zeros((h + 1, n + bpp), np.int64)          # a zero row above and a zero pixel to the left
    for y in range(h):
        t, line, cur, up = int(filtered[y, 0]), filtered[y, 1:].astype(np.int64), raw[y + 1], raw[y]
        if t > 4:
            raise PngError(BADFILE, f"filter type {t}")
        if t == 0:
            cur[bpp:] = line
        elif t == 1:
            pad = (-n) % bpp
            lanes = np.concatenate([line, np.zeros(pad, np.int64)]).reshape(-1, bpp)
            cur[bpp:] = (np.cumsum(lanes, axis=0) & 255).reshape(-1)[:n]
        elif t == 2:
            cur[bpp:] = (line + up[bpp:]) & 255
        else:
            for i in range(0, n, bpp):
                a, b, c, x = cur[i:i + bpp], up[i + bpp:i + 2 * bpp], up[i:i + bpp], line[i:i + bpp]
                if t == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
                    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
                cur[i + bpp:i + 2 * bpp] = (x + pred) & 255
    return np.ascontiguousarray(raw[1:, bpp:].astype(np.uint8))


def frame_from_raw(raw, info, order="rgb"):
    h, w, c, depth = info["H"], info["W"], info["C"], info["depth"]
    img = raw.view(">u2").astype(np.uint16) if depth == 16 else raw
    img = img.reshape(h, w, c)
    if order == "bgr" and c >= 3:
        img = np.concatenate([img[:, :, 2::-1], img[:, :, 3:]], axis=2)
    return np.ascontiguousarray(img[:, :, 0] if c == 1 else img)


def decode(data, order="rgb"):
    """The frame of a supported file; zlib inflates (PngError BADFILE on zlib.error, a wrong size or a filter type above 4)."""
    info, _ = parse(data)
    try:
        stream = zlib.decompress(b"".join(p for k, p in _chunks(bytes(data)) if k == b"IDAT"))
    except zlib.error as e:
        raise PngError(BADFILE, str(e)) from e
    if len(stream) != info["stream_bytes"]:
        raise PngError(BADFILE, "the stream's size is not H (1 + W bpp)")
    filt = np.frombuffer(stream, np.uint8).reshape(info["H"], -1)
    return frame_from_raw(unfilter(filt, info["C"] * info["depth"] // 8), info, order)
