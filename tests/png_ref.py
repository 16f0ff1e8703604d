"""The specification of the device PNG encoder (csrc/png.hip): pure numpy + stdlib.  encode_png(frame, order) -> the file's bytes,
encode_png_stats(frame, order) -> (bytes, counters).  The kernels reproduce these bytes; tests/test_png_spec.py shows that standard
decoders return the frame from them bit for bit and pins them with golden files.

File: signature, IHDR, IDAT[78 01], one IDAT per deflate chunk, IDAT[Adler-32], IEND.  No ancillary chunk.

Samples: channel order R G B (A) in the file whatever `order` the frame has; 16-bit samples big-endian; bpp = channels x bytes per
sample.

Filter, per row: the five PNG types, each computed from RAW neighbours (the row above the first is zeros); the winner has the
smallest sum of min(v, 256 - v) over the row's filtered bytes, ties to the lowest type.

Deflate: the filtered stream (N = H (1 + W bpp) bytes) is cut into chunks of S = 32768 bytes, each coded alone.
  tokens   distance 1 only.  A maximal run of R equal bytes inside the chunk: the first byte a literal, then (R - 1) // 258 matches
           of 258, then one match of (R - 1) % 258 if that is >= 3, else that many literals.
  block    one per chunk, BFINAL 0; BTYPE the cheapest of stored (40 + 8 n bits), fixed and dynamic by exact bit count, ties to the
           lower BTYPE.  Chunks start byte-aligned.
  sync     after the block an empty stored block: 3 header bits (BFINAL 1 in the last chunk only), padding to the byte, 00 00 FF FF.
  dynamic  code_lengths() below for the literal/length code (286 symbols, 15 bits; symbol 256 always counts once) and the code-length
           code (19 symbols, 7 bits).  The distance code is one symbol: length 1 when the chunk has a match, else 0; HDIST = 0.
           HLIT and HCLEN trimmed.  The lengths of both codes form ONE sequence, run-coded greedily (rle_lengths()).

code_lengths(counts, limit): symbols with a count, sorted ascending by (count, symbol).  Fewer than two: that symbol (or symbol 0)
and the lowest other symbol get length 1.  Else Huffman's algorithm with two queues (sorted leaves; internal nodes in creation
order), taking a leaf before an internal node of equal weight; leaf depths above `limit` are clamped to it and give a histogram of
lengths bl[1 .. limit]; while sum(bl[d] << (limit - d)) exceeds 1 << limit: bl[limit] -= 1, the largest d < limit with bl[d] > 0
gives bl[d] -= 1 and bl[d + 1] += 2 (the repair rule); lengths are then dealt out in sorted order, the longest to the first (rarest)
symbols.  Codes are canonical (RFC 1951 3.2.2)."""
import struct
import zlib

import numpy as np

S = 32768
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEAD_BYTES, TAIL_BYTES = 47, 28


def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def head(h, w, c, depth):
    """The 47 fixed bytes: signature, IHDR, IDAT[78 01]"""
    ctype = {1: 0, 3: 2, 4: 6}[c]
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) + chunk(b"IDAT", b"\x78\x01")


def bound(h, w, c, depth):
    """The exact worst case: every chunk stored (5 bytes of block header, 5 of sync, 12 of IDAT framing)"""
    n = h * (1 + w * c * depth // 8)
    return HEAD_BYTES + TAIL_BYTES + n + 22 * ((n + S - 1) // S)


def file_rows(frame, order="rgb"):
    """frame ([H, W], [H, W, 1|3|4]; uint8 or uint16) -> (uint8 [H, W * bpp] in the file's byte order, bpp, C, depth)"""
    frame = np.asarray(frame)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    h, w, c = frame.shape
    if c not in (1, 3, 4) or frame.dtype not in (np.uint8, np.uint16) or order not in ("rgb", "bgr"):
        raise ValueError("png_ref: uint8 / uint16 frames of 1, 3 or 4 channels in 'rgb' or 'bgr' order")
    if order == "bgr" and c >= 3:
        frame = np.concatenate([frame[:, :, 2::-1], frame[:, :, 3:]], axis=2)
    depth = 8 * frame.dtype.itemsize
    raw = np.ascontiguousarray(frame.astype(">u2") if depth == 16 else frame).view(np.uint8).reshape(h, -1)
    return raw, c * depth // 8, c, depth


def filter_rows(raw, bpp):
    """-> (filtered stream uint8 [H, 1 + W bpp], types [H])"""
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
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255          # [5, H, n]
    cost = np.minimum(cand, 256 - cand).sum(axis=2)                                   # [5, H]
    types = np.argmin(cost, axis=0)                                                   # the first minimum: the lowest type
    out = np.empty((h, n + 1), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(h)]
    return out, types


# ------------------------------------------------------------------------------------------------ Huffman codes
def code_lengths(counts, limit, stats=None):
    n = len(counts)
    lengths = [0] * n
    used = sorted((int(c), s) for s, c in enumerate(counts) if c > 0)
    m = len(used)
    if m < 2:
        s = used[0][1] if m else 0
        lengths[s] = 1
        lengths[1 if s == 0 else 0] = 1
        return lengths
    w = [c for c, _ in used]
    iw, pl, pi = [0] * (m - 1), [0] * m, [0] * (m - 1)
    li = ii = 0
    for k in range(m - 1):
        tot = 0
        for _ in range(2):
            if li < m and (ii >= k or w[li] <= iw[ii]):
                tot += w[li]
                pl[li] = k
                li += 1
            else:
                tot += iw[ii]
                pi[ii] = k
                ii += 1
        iw[k] = tot
    di = [0] * (m - 1)
    for k in range(m - 3, -1, -1):
        di[k] = di[pi[k]] + 1
    bl = [0] * (limit + 1)
    deep = False
    for i in range(m):
        d = di[pl[i]] + 1
        deep |= d > limit
        bl[min(d, limit)] += 1
    total = sum(bl[d] << (limit - d) for d in range(1, limit + 1))
    if deep and stats is not None:
        stats[f"repair{limit}"] = stats.get(f"repair{limit}", 0) + 1
    while total > (1 << limit):
        bl[limit] -= 1
        for d in range(limit - 1, 0, -1):
            if bl[d]:
                bl[d] -= 1
                bl[d + 1] += 2
                break
        total -= 1
    j = m
    for d in range(1, limit + 1):
        for _ in range(bl[d]):
            j -= 1
            lengths[used[j][1]] = d
    return lengths


def canonical_codes(lengths):
    """-> codes, bit-reversed (ready to be written LSB first)"""
    maxlen = max(lengths) if len(lengths) else 0
    bl = [0] * (maxlen + 2)
    for v in lengths:
        if v:
            bl[v] += 1
    nxt, code = [0] * (maxlen + 2), 0
    for d in range(1, maxlen + 1):
        code = (code + bl[d - 1]) << 1
        nxt[d] = code
    out = [0] * len(lengths)
    for s, v in enumerate(lengths):
        if v:
            out[s] = int(format(nxt[v], f"0{v}b")[::-1], 2)
            nxt[v] += 1
    return out


def rle_lengths(seq):
    """Greedy 16 / 17 / 18 coding -> [(symbol, extra value, extra bits)]"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        r = 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            t = min(r, 138)
            out.append((18, t - 11, 7) if t >= 11 else (17, t - 3, 3))
            i += t
        elif v != 0 and i > 0 and seq[i - 1] == v and r >= 3:
            t = min(r, 6)
            out.append((16, t - 3, 2))
            i += t
        else:
            out.append((v, 0, 0))
            i += 1
    return out


FIXED_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def length_symbol(length):
    """match length 3 .. 258 -> (symbol, extra value, extra bits); vectorised"""
    v = np.asarray(length, np.int64) - 3
    nb = np.zeros_like(v)
    big = v >= 8
    nb[big] = np.floor(np.log2(np.maximum(v[big], 1))).astype(np.int64) - 2
    sym = np.where(big, 257 + 4 * nb + 4 + ((v >> nb) & 3), 257 + v)
    ev = np.where(big, v & ((1 << nb) - 1), 0)
    last = v == 255
    return np.where(last, 285, sym), np.where(last, 0, ev), np.where(last, 0, nb)


def symbol_extra_bits(sym):
    return 0 if sym < 265 or sym == 285 else (sym - 261) // 4


class Bits:
    def __init__(self):
        self.vals, self.lens = [], []

    def put(self, value, nbits):
        self.vals.append(np.atleast_1d(np.asarray(value, np.uint64)))
        self.lens.append(np.atleast_1d(np.asarray(nbits, np.int64)))

    def nbits(self):
        return int(sum(int(x.sum()) for x in self.lens))

    def to_bytes(self):
        v, n = np.concatenate(self.vals), np.concatenate(self.lens)
        bits = ((v[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
        keep = np.arange(32)[None, :] < n[:, None]
        return np.packbits(bits[keep], bitorder="little").tobytes()


def tokens(b):
    """chunk bytes -> (positions of token starts, literal/length symbol, extra value, extra bits, is-match) and counters"""
    n = len(b)
    start = np.ones(n, bool)
    start[1:] = b[1:] != b[:-1]
    s = np.flatnonzero(start)
    run = np.diff(np.append(s, n))
    p = np.arange(n) - np.repeat(s, run)
    rr = np.repeat(run, run) - 1
    full, rem = rr // 258, rr % 258
    q = p - 1
    k, off = q // 258, q % 258
    lit = (p == 0) | ((k == full) & (rem < 3))
    mat = (p >= 1) & (off == 0) & ((k < full) | (rem >= 3))
    mlen = np.where(k < full, 258, rem)
    pos = np.flatnonzero(lit | mat)
    is_m = mat[pos]
    sym, ev, eb = length_symbol(np.where(is_m, mlen[pos], 3))
    sym = np.where(is_m, sym, b[pos].astype(np.int64))
    ev, eb = np.where(is_m, ev, 0), np.where(is_m, eb, 0)
    r1 = run - 1
    seen = {"rem0": int(((r1 % 258 == 0) & (r1 > 0)).sum()), "rem1": int((r1 % 258 == 1).sum()), "rem2": int((r1 % 258 == 2).sum()),
            "rem_match": int((r1 % 258 >= 3).sum()), "split258": int((r1 >= 258).sum())}
    return sym, ev, eb, is_m, seen


def deflate_chunk(b, last, stats):
    n = len(b)
    sym, ev, eb, is_m, seen = tokens(b)
    for k, v in seen.items():
        stats[k] = stats.get(k, 0) + v
    hist = np.bincount(sym, minlength=286).astype(np.int64)
    hist[256] = 1
    nmatch = int(is_m.sum())
    stats["match_chunks" if nmatch else "nomatch_chunks"] = stats.get("match_chunks" if nmatch else "nomatch_chunks", 0) + 1
    extra = sum(int(hist[s_]) * symbol_extra_bits(s_) for s_ in range(257, 286))
    ll = code_lengths(hist, 15, stats)
    dl = 1 if nmatch else 0
    hlit = max(i for i in range(286) if ll[i]) + 1
    hlit = max(hlit, 257)
    rle = rle_lengths(ll[:hlit] + [dl])
    clhist = [0] * 19
    for s_, _, _ in rle:
        clhist[s_] += 1
    cl = code_lengths(clhist, 7, stats)
    hclen = max(i for i in range(19) if cl[CL_ORDER[i]]) + 1
    hclen = max(hclen, 4)
    stored_bits = 40 + 8 * n
    fixed_bits = 3 + sum(int(hist[s_]) * FIXED_LENGTHS[s_] for s_ in range(286)) + extra + 5 * nmatch
    dyn_bits = (3 + 14 + 3 * hclen + sum(cl[s_] + x for s_, _, x in rle) + sum(int(hist[s_]) * ll[s_] for s_ in range(286)) + extra + dl * nmatch)
    btype = min((stored_bits, 0), (fixed_bits, 1), (dyn_bits, 2))[1]
    stats[f"btype{btype}"] = stats.get(f"btype{btype}", 0) + 1
    bits = Bits()
    if btype == 0:
        body = b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + b.tobytes()
    else:
        bits.put(btype << 1, 3)
        if btype == 2:
            bits.put(hlit - 257, 5)
            bits.put(0, 5)
            bits.put(hclen - 4, 4)
            for i in range(hclen):
                bits.put(cl[CL_ORDER[i]], 3)
            clc = canonical_codes(cl)
            for s_, v, x in rle:
                bits.put(clc[s_], cl[s_])
                if x:
                    bits.put(v, x)
            lens, dist_bits = np.array(ll + [0, 0]), dl
        else:
            lens, dist_bits = np.array(FIXED_LENGTHS), 5
        codes = np.array(canonical_codes(list(lens)), np.uint64)
        ls = lens[sym]
        value = codes[sym] | (ev.astype(np.uint64) << ls.astype(np.uint64))
        bits.put(value, ls + eb + np.where(is_m, dist_bits, 0))
        bits.put(codes[256], lens[256])
        assert bits.nbits() == (fixed_bits if btype == 1 else dyn_bits)
        bits.put(1 if last else 0, 3)
        return bits.to_bytes() + b"\x00\x00\xff\xff"
    return body + (b"\x01" if last else b"\x00") + b"\x00\x00\xff\xff"


def encode_png_stats(frame, order="rgb"):
    raw, bpp, c, depth = file_rows(frame, order)
    h, w = raw.shape[0], raw.shape[1] // bpp
    filt, types = filter_rows(raw, bpp)
    stream = filt.reshape(-1)
    stats = {f"filter{t}": int((types == t).sum()) for t in range(5)}
    nchunks = (len(stream) + S - 1) // S
    stats["chunks"] = nchunks
    stats["cut_runs"] = int(sum(stream[k * S] == stream[k * S - 1] for k in range(1, nchunks)))
    out = [head(h, w, c, depth)]
    for k in range(nchunks):
        out.append(chunk(b"IDAT", deflate_chunk(stream[k * S:(k + 1) * S], k == nchunks - 1, stats)))
    out.append(chunk(b"IDAT", struct.pack(">I", zlib.adler32(stream.tobytes()) & 0xFFFFFFFF)))
    out.append(chunk(b"IEND", b""))
    stats["filtered"] = stream
    return b"".join(out), stats


def encode_png(frame, order="rgb"):
    return encode_png_stats(frame, order)[0]


# ------------------------------------------------------------------------------------------------ a decoder for the tests
def read_chunks(data):
    """-> [(kind, payload)]; checks the signature, every CRC and that nothing follows IEND"""
    assert data[:8] == SIGNATURE
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        payload = data[at + 8:at + 8 + n]
        assert len(payload) == n
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + payload) & 0xFFFFFFFF, (kind, at)
        out.append((kind, payload))
        at += 12 + n
    assert at == len(data) and out[-1] == (b"IEND", b"")
    return out


def decode_png(data, full=True, layout=True):
    """A stdlib decoder: zlib.decompress of the concatenated IDATs, then unfiltering -> the frame ([H, W] or [H, W, C], uint8 / uint16,
    RGB(A) order).  Also checks the layout: IHDR, the 2-byte IDAT, data IDATs, the 4-byte IDAT, IEND, nothing else.
    full=False skips the byte-serial unfiltering and returns (filtered [H, 1 + W bpp], (H, W, C, depth)) for refilter_matches().
    layout=False: any PNG file of IHDR, IDATs and IEND (the host route of imgproc.encode_png writes one IDAT)."""
    chunks = read_chunks(data)
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}
    if layout:
        assert len(kinds) >= 5 and chunks[1][1] == b"\x78\x01" and len(chunks[-2][1]) == 4
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (comp, flt, lace) == (0, 0, 0) and depth in (8, 16) and ctype in (0, 2, 6)
    c = {0: 1, 2: 3, 6: 4}[ctype]
    bpp = c * depth // 8
    stream = zlib.decompress(b"".join(p for k, p in chunks if k == b"IDAT"))
    assert len(stream) == h * (1 + w * bpp)
    filt = np.frombuffer(stream, np.uint8).reshape(h, 1 + w * bpp)
    if not full:
        return filt, (h, w, c, depth)
    n = w * bpp
    rows = np.zeros((h + 1, n + bpp), np.int64)         # a zero row above and bpp zero bytes to the left
    for y in range(h):
        t, line, cur, up = int(filt[y, 0]), filt[y, 1:].astype(np.int64), rows[y + 1], rows[y]
        assert t <= 4
        if t == 0:
            cur[bpp:] = line
        elif t == 2:
            cur[bpp:] = (line + up[bpp:]) & 255
        else:
            for i in range(n):
                a, b, cc = int(cur[i]), int(up[i + bpp]), int(up[i])
                if t == 1:
                    pred = a
                elif t == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - cc
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else cc)
                cur[i + bpp] = (int(line[i]) + pred) & 255
    raw = np.ascontiguousarray(rows[1:, bpp:].astype(np.uint8))
    img = raw.view(">u2").astype(np.uint16) if depth == 16 else raw
    img = img.reshape(h, w, c)
    return img[:, :, 0] if c == 1 else img


def refilter_matches(data, frame, order="rgb", layout=True):
    """Decoding check for frames too large for decode_png's byte loop: the file's filtered stream must equal `frame`'s raw bytes
    filtered with the file's own filter type per row.  A PNG filter is a bijection given the raw bytes before it, so (by induction
    over the bytes) this holds exactly when unfiltering the file returns `frame`."""
    filt, (h, w, c, depth) = decode_png(data, full=False, layout=layout)
    raw, bpp, c2, depth2 = file_rows(frame, order)
    if (h, w * bpp, c, depth) != (raw.shape[0], raw.shape[1], c2, depth2):
        return False
    types = filt[:, 0]
    if types.max() > 4:
        return False
    x = raw.astype(np.int16)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    t = types[:, None]
    pred = np.where(t == 0, 0, np.where(t == 1, a, np.where(t == 2, b, np.where(t == 3, (a + b) >> 1, paeth))))
    return bool(np.array_equal(((x - pred) & 255).astype(np.uint8), filt[:, 1:]))
