"""Specification of the baseline JPEG encoder (numpy only): libjpeg's compressor as cv2.imwrite and PIL.Image.save run it by
default -- 4:2:0 for colour, Annex K quantisation tables scaled by quality, Annex K Huffman tables, islow integer FDCT, no restart
markers, JFIF 1.01 header.  The integer pipeline is reproducible, so tests/test_jpeg_spec.py pins this file byte for byte against
Pillow's bundled libjpeg-turbo and against committed files, and the GPU tests pin csrc/jpeg.hip against this file.

encode_jpeg(img, quality, order) -> bytes;  encode_jpeg_stats(...) -> (bytes, counters), the counters proving which paths an input
takes (ZRL symbols, stuffed bytes, largest DC / AC category, dummy blocks by kind, all-EOB).
"""
from __future__ import annotations

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])

LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                     99, 99] + [99] * 32)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def quant_tables(quality):
    """(luma, chroma) in natural order: jpeg_quality_scaling + jpeg_add_quant_table with force_baseline."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {quality} outside 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (LUMA_Q, CHROMA_Q))


def huff_codes(bits, vals):
    """symbol -> (code, length), canonical assignment from BITS / HUFFVAL."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def header(h, w, channels, quality):
    """SOI .. SOS as libjpeg writes them (623 bytes for colour, 328 for gray)."""
    ql, qc = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((ql, qc)[:2 if channels == 3 else 1]):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in q[ZIGZAG])
    out += b"\xff\xc0" + (8 + 3 * channels).to_bytes(2, "big") + b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([channels])
    if channels == 3:
        out += b"\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    else:
        out += b"\x01\x11\x00"
    tabs = [(0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS)]
    if channels == 3:
        tabs += [(0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)]
    for tc_th, bits, vals in tabs:
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc_th]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda" + (6 + 2 * channels).to_bytes(2, "big") + bytes([channels])
    out += b"\x01\x00\x02\x11\x03\x11" if channels == 3 else b"\x01\x00"
    return bytes(out + b"\x00\x3f\x00")


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_islow(blocks):
    """jfdctint.c on [..., 8, 8] int64 samples (already level-shifted)."""
    F = [2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172]
    c0298, c0390, c0541, c0765, c0899, c1175, c1501, c1847, c1961, c2053, c2562, c3072 = F

    def one_pass(d, first):
        t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
        t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
        t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
        t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o = [None] * 8
        if first:
            o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
        else:
            o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
        n = 11 if first else 15
        z1 = (t12 + t13) * c0541
        o[2] = _descale(z1 + t13 * c0765, n)
        o[6] = _descale(z1 - t12 * c1847, n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * c1175
        t4, t5, t6, t7 = t4 * c0298, t5 * c2053, t6 * c3072, t7 * c1501
        z1, z2, z3, z4 = -z1 * c0899, -z2 * c2562, -z3 * c1961 + z5, -z4 * c0390 + z5
        o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
        return np.stack(o, -1)

    rows = one_pass(blocks.astype(np.int64), True)                       # along each row
    return np.swapaxes(one_pass(np.swapaxes(rows, -1, -2), False), -1, -2)  # along each column


def _blocks(plane, q):
    """[H8, W8] samples -> quantised zigzag coefficients [H8/8, W8/8, 64]."""
    h, w = plane.shape
    b = plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2).astype(np.int64) - 128
    c = fdct_islow(b).reshape(h // 8, w // 8, 64)
    qq = q[None, None, :]
    mag = (np.abs(c) + 4 * qq) // (8 * qq)
    return (np.sign(c) * mag)[..., ZIGZAG]


def _pad(plane, h, w):
    return np.pad(plane, ((0, h - plane.shape[0]), (0, w - plane.shape[1])), mode="edge")


def _ceil(a, b):
    return -(-a // b)


def scan_blocks(img, quality=95, order="rgb"):
    """The blocks of the one scan in coding order: (coefs [N, 64] int64 zigzag, comp [N] 0 Y | 1 Cb | 2 Cr, counters)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3) or min(img.shape[:2]) < 1:
        raise ValueError(f"an HW or HWx3 uint8 image, got {img.dtype} {img.shape}")
    if order not in ("rgb", "bgr"):
        raise ValueError(f"order {order!r}")
    ql, qc = quant_tables(quality)
    h, w = img.shape[:2]
    stats = {"dummy_right": 0, "dummy_bottom": 0, "dummy_both_in_one_mcu": 0}
    if img.ndim == 2:
        y = _blocks(_pad(img.astype(np.int64), _ceil(h, 8) * 8, _ceil(w, 8) * 8), ql)
        coefs = y.reshape(-1, 64)
        stats["dummy_blocks"] = 0
        return coefs, np.zeros(len(coefs), np.int64), stats
    x = img.astype(np.int64)
    r, g, b = (x[..., 0], x[..., 1], x[..., 2]) if order == "rgb" else (x[..., 2], x[..., 1], x[..., 0])
    yy = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    mh, mw = _ceil(h, 16), _ceil(w, 16)
    yb = _blocks(_pad(yy, mh * 16, mw * 16), ql)

    def down(p):
        p = _pad(p, h + (h & 1), mw * 16)                 # source columns to the MCU width, source rows to even
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        bias = 1 + (np.arange(s.shape[1]) & 1)             # 1, 2, 1, 2 ... restarting every row
        return _pad((s + bias[None, :]) >> 2, mh * 8, mw * 8)   # then DOWNSAMPLED rows to the MCU height

    cbb, crb = _blocks(down(cb), qc), _blocks(down(cr), qc)
    bh, bw = _ceil(h, 8), _ceil(w, 8)                      # real Y blocks
    coefs, comp = [], []
    for my in range(mh):
        for mx in range(mw):
            kinds = set()
            prev = None
            for k, (by, bx) in enumerate(((2 * my, 2 * mx), (2 * my, 2 * mx + 1), (2 * my + 1, 2 * mx), (2 * my + 1, 2 * mx + 1))):
                if by < bh and bx < bw:
                    blk = yb[by, bx]
                else:                                      # dummy: the DC of the block coded just before it, no AC
                    blk = np.zeros(64, np.int64)
                    blk[0] = prev[0]
                    kind = "dummy_bottom" if by >= bh else "dummy_right"
                    stats[kind] += 1
                    kinds.add(kind)
                    if by >= bh and bx >= bw:
                        kinds.add("dummy_right")
                coefs.append(blk)
                comp.append(0)
                prev = blk
            stats["dummy_both_in_one_mcu"] += len(kinds) == 2
            coefs += [cbb[my, mx], crb[my, mx]]
            comp += [1, 2]
    stats["dummy_blocks"] = stats["dummy_right"] + stats["dummy_bottom"]
    return np.stack(coefs), np.array(comp), stats


def encode_jpeg_stats(img, quality=95, order="rgb"):
    img = np.asarray(img)
    coefs, comp, stats = scan_blocks(img, quality, order)
    channels = 1 if img.ndim == 2 else 3
    dc_tabs = [huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS)]
    ac_tabs = [huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS)]
    acc, nbits = 0, 0
    chunks = []
    pred = [0, 0, 0]
    zrl = max_dc = max_ac = 0
    all_eob = True

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | code
        nbits += length

    for blk, c in zip(coefs.tolist(), comp.tolist()):
        t = 0 if c == 0 else 1
        d = blk[0] - pred[c]
        pred[c] = blk[0]
        cat = abs(d).bit_length()
        max_dc = max(max_dc, cat)
        put(*dc_tabs[t][cat])
        if cat:
            put((d if d >= 0 else d - 1) & ((1 << cat) - 1), cat)
        run = 0
        for v in blk[1:]:
            if v == 0:
                run += 1
                continue
            all_eob = False
            while run > 15:
                put(*ac_tabs[t][0xF0])
                zrl += 1
                run -= 16
            size = abs(v).bit_length()
            max_ac = max(max_ac, size)
            put(*ac_tabs[t][(run << 4) | size])
            put((v if v >= 0 else v - 1) & ((1 << size) - 1), size)
            run = 0
        if run:
            put(*ac_tabs[t][0x00])
        if nbits >= 4096:                                   # flush whole bytes, keep the tail
            keep = nbits & 7
            chunks.append((acc >> keep).to_bytes((nbits - keep) // 8, "big"))
            acc &= (1 << keep) - 1
            nbits = keep
    if nbits & 7:
        fill = 8 - (nbits & 7)
        put((1 << fill) - 1, fill)
    chunks.append(acc.to_bytes(nbits // 8, "big"))
    raw = b"".join(chunks)
    stats.update(zrl=zrl, stuffed=raw.count(b"\xff"), max_dc_cat=max_dc, max_ac_cat=max_ac, all_eob=all_eob, blocks=len(coefs))
    data = header(img.shape[0], img.shape[1], channels, quality) + raw.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    return data, stats


def encode_jpeg(img, quality=95, order="rgb"):
    """HWC 3-channel ("rgb" or "bgr") or HW gray uint8 -> the bytes of the baseline JPEG file."""
    return encode_jpeg_stats(img, quality, order)[0]
