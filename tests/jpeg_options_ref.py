"""Specification of the JPEG encoder's options (numpy and stdlib, on top of tests/jpeg_ref.py): libjpeg's compressor with a chroma
layout of 4:4:4, 4:2:2 or 4:2:0, Huffman tables optimised for the frame (jpeg_gen_optimal_table) and a restart interval in MCUs --
cv2.imwrite's IMWRITE_JPEG_SAMPLING_FACTOR, IMWRITE_JPEG_OPTIMIZE and IMWRITE_JPEG_RST_INTERVAL, Pillow's subsampling, optimize and
restart_marker_blocks.  tests/test_jpeg_options_spec.py pins this file byte for byte against Pillow's libjpeg-turbo and against
committed files; the GPU tests pin csrc/jpeg.hip against this file.

encode_jpeg_stats(img, quality, order, sampling, optimize, restart_interval) -> (bytes, counters).  The counters prove which rules
an input reaches: h2v1 dummy blocks, moves of the 16-bit length limit, stuffed pad bytes, restart markers and how many wrapped past
RST7, intervals that end on a byte, tables with a single used symbol, and the BITS / HUFFVAL of every table.

`wrong` names one deliberate mistake (WRONG lists them); the spec test shows that each is told apart from Pillow by some file.
"""
from __future__ import annotations

import numpy as np

from tests import jpeg_ref
from tests.jpeg_ref import ZIGZAG, _blocks, _ceil, _pad, quant_tables

SAMPLINGS = ("4:4:4", "4:2:2", "4:2:0")
WRONG = ("h2v1_bias_constant", "ties_to_smaller_symbol", "no_reserved_symbol", "no_length_limit", "predictors_not_reset", "n_not_wrapped",
         "pad_byte_not_stuffed", "dri_before_dht", "dummy_dc_zero")
STANDARD = [(jpeg_ref.DC_LUMA_BITS, jpeg_ref.DC_VALS), (jpeg_ref.AC_LUMA_BITS, jpeg_ref.AC_LUMA_VALS),
            (jpeg_ref.DC_CHROMA_BITS, jpeg_ref.DC_VALS), (jpeg_ref.AC_CHROMA_BITS, jpeg_ref.AC_CHROMA_VALS)]      # index: table * 2 + is_ac


def scan_blocks(img, quality=95, order="rgb", sampling="4:2:0", wrong=None):
    """jpeg_ref.scan_blocks for the three layouts: (coefs [N, 64] zigzag, comp [N], blocks per MCU, counters)."""
    img = np.asarray(img)
    if sampling not in SAMPLINGS:
        raise ValueError(f"sampling {sampling!r}: one of {SAMPLINGS} (4:4:0 and 4:1:1 are not encoded)")
    if img.ndim == 2 or sampling == "4:2:0":
        coefs, comp, stats = jpeg_ref.scan_blocks(img, quality, order)
        coefs = np.array(coefs)
        if wrong == "dummy_dc_zero" and img.ndim == 3:
            coefs[_dummy_mask_420(img.shape[0], img.shape[1])] = 0
        stats["dummy_h2v1"] = 0
        return coefs, comp, (1 if img.ndim == 2 else 6), stats
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or min(img.shape[:2]) < 1:
        raise ValueError(f"an HW or HWx3 uint8 image, got {img.dtype} {img.shape}")
    if order not in ("rgb", "bgr"):
        raise ValueError(f"order {order!r}")
    ql, qc = quant_tables(quality)
    h, w = img.shape[:2]
    x = img.astype(np.int64)
    r, g, b = (x[..., 0], x[..., 1], x[..., 2]) if order == "rgb" else (x[..., 2], x[..., 1], x[..., 0])
    yy = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    stats = {"dummy_right": 0, "dummy_bottom": 0, "dummy_both_in_one_mcu": 0, "dummy_blocks": 0, "dummy_h2v1": 0}
    mh = _ceil(h, 8)
    if sampling == "4:4:4":
        mw = _ceil(w, 8)
        planes = [_blocks(_pad(p, mh * 8, mw * 8), q) for p, q in ((yy, ql), (cb, qc), (cr, qc))]
        coefs = np.stack(planes, 2).reshape(-1, 64)                        # Y Cb Cr per MCU, MCUs in raster order
        return coefs, np.tile([0, 1, 2], mh * mw), 3, stats
    mw = _ceil(w, 16)

    def down(p):
        p = _pad(p, h, mw * 16)                                            # source columns to the MCU width, no source row
        bias = np.arange(mw * 8) & 1                                       # 0, 1, 0, 1 ... restarting every row
        if wrong == "h2v1_bias_constant":
            bias = bias * 0 + 1
        return _pad((p[:, 0::2] + p[:, 1::2] + bias[None, :]) >> 1, mh * 8, mw * 8)

    yb = _blocks(_pad(yy, mh * 8, mw * 16), ql)
    cbb, crb = _blocks(down(cb), qc), _blocks(down(cr), qc)
    bw = _ceil(w, 8)
    coefs, comp = [], []
    for my in range(mh):
        for mx in range(mw):
            first = yb[my, 2 * mx]
            second = yb[my, 2 * mx + 1]
            if 2 * mx + 1 >= bw:                                           # dummy: the DC of the block coded just before it, no AC
                second = np.zeros(64, np.int64)
                second[0] = 0 if wrong == "dummy_dc_zero" else first[0]
                stats["dummy_h2v1"] += 1
            coefs += [first, second, cbb[my, mx], crb[my, mx]]
            comp += [0, 0, 1, 2]
    stats["dummy_right"] = stats["dummy_blocks"] = stats["dummy_h2v1"]
    return np.stack(coefs), np.array(comp), 4, stats


def _dummy_mask_420(h, w):
    mh, mw, bh, bw = _ceil(h, 16), _ceil(w, 16), _ceil(h, 8), _ceil(w, 8)
    mask = []
    for my in range(mh):
        for mx in range(mw):
            mask += [not (by < bh and bx < bw) for by, bx in ((2 * my, 2 * mx), (2 * my, 2 * mx + 1), (2 * my + 1, 2 * mx), (2 * my + 1, 2 * mx + 1))]
            mask += [False, False]
    return np.array(mask)


def ac_symbols(blk):
    """The AC symbols of one zigzag block in coding order: [(symbol, extra bits, their count)]."""
    out, run = [], 0
    last = 0
    for k in np.flatnonzero(blk[1:]).tolist():
        v = int(blk[k + 1])
        run = k - last
        last = k + 1
        while run > 15:
            out.append((0xF0, 0, 0))
            run -= 16
        size = abs(v).bit_length()
        out.append(((run << 4) | size, (v if v >= 0 else v - 1) & ((1 << size) - 1), size))
    if last < 63:
        out.append((0x00, 0, 0))
    return out


def gen_optimal_table(freq, wrong=None):
    """jpeg_gen_optimal_table (jchuff.c) on 256 counts -> (BITS[16], HUFFVAL, moves of the length limit, deepest unlimited length)."""
    freq = [int(v) for v in freq] + [0 if wrong == "no_reserved_symbol" else 1]      # the reserved symbol 256: no code of all 1-bits
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        v = 1000000000
        for i in range(257):                                       # the least frequent; among equals the LARGER symbol
            if freq[i] and (freq[i] <= v if wrong != "ties_to_smaller_symbol" else freq[i] < v):
                v, c1 = freq[i], i
        v = 1000000000
        for i in range(257):
            if freq[i] and i != c1 and (freq[i] <= v if wrong != "ties_to_smaller_symbol" else freq[i] < v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 34
    for s in codesize:
        if s:
            bits[s] += 1
    deepest = max(codesize)
    moves = 0
    if wrong != "no_length_limit":
        for i in range(32, 16, -1):
            while bits[i] > 0:
                j = i - 2
                while bits[j] == 0:
                    j -= 1
                bits[i] -= 2
                bits[i - 1] += 1
                bits[j + 1] += 2
                bits[j] -= 1
                moves += 1
    if wrong != "no_reserved_symbol":
        i = 32
        while i > 0 and bits[i] == 0:
            i -= 1
        if i > 0:
            bits[i] -= 1                                           # the reserved symbol had the longest code
    vals = [j for i in range(1, 33) for j in range(256) if codesize[j] == i]
    return bits[1:33], vals, moves, deepest


def _codes(bits, vals):
    table, code, k = {}, 0, 0
    for length in range(1, len(bits) + 1):
        for _ in range(bits[length - 1]):
            if k < len(vals):
                table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def header(h, w, channels, quality, sampling, tables, restart_interval, wrong=None):
    """SOI .. SOS: jpeg_ref.header with the layout's SOF0 bytes, the given DHTs [(BITS, HUFFVAL)] and DRI after them."""
    ql, qc = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((ql, qc)[:2 if channels == 3 else 1]):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in q[ZIGZAG])
    out += b"\xff\xc0" + (8 + 3 * channels).to_bytes(2, "big") + b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([channels])
    if channels == 3:
        out += bytes([1, {"4:4:4": 0x11, "4:2:2": 0x21, "4:2:0": 0x22}[sampling], 0, 2, 0x11, 1, 3, 0x11, 1])
    else:
        out += b"\x01\x11\x00"
    dri = b"\xff\xdd\x00\x04" + restart_interval.to_bytes(2, "big") if restart_interval else b""
    if wrong == "dri_before_dht":
        out += dri
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), tables):
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc_th]) + bytes(min(b, 255) for b in bits[:16]) + bytes(vals)
    if wrong != "dri_before_dht":
        out += dri
    out += b"\xff\xda" + (6 + 2 * channels).to_bytes(2, "big") + bytes([channels])
    out += b"\x01\x00\x02\x11\x03\x11" if channels == 3 else b"\x01\x00"
    return bytes(out + b"\x00\x3f\x00")


def encode_jpeg_stats(img, quality=95, order="rgb", sampling="4:2:0", optimize=False, restart_interval=0, *, wrong=None, _blocks_cache=None):
    img = np.asarray(img)
    ri = int(restart_interval)
    if not 0 <= ri <= 65535:
        raise ValueError(f"restart_interval {restart_interval} outside 0..65535")
    if wrong is not None and wrong not in WRONG:
        raise ValueError(wrong)
    key = (quality, order, sampling, wrong if wrong in ("h2v1_bias_constant", "dummy_dc_zero") else None)
    if _blocks_cache is not None and key in _blocks_cache:
        coefs, comp, per, stats, acs = _blocks_cache[key]
        stats = dict(stats)
    else:
        coefs, comp, per, stats = scan_blocks(img, quality, order, sampling, wrong)
        acs = [ac_symbols(b) for b in coefs]
        if _blocks_cache is not None:
            _blocks_cache[key] = (coefs, comp, per, dict(stats), acs)
    channels = 1 if img.ndim == 2 else 3
    ntab = 2 if channels == 3 else 1
    dcs = coefs[:, 0].tolist()
    comp = comp.tolist()
    nmcu = len(dcs) // per
    step = ri if ri else nmcu
    # the DC symbol of every block: predictors are 0 at each interval's start
    dc_syms = []
    pred = [0, 0, 0]
    for n, (v, c) in enumerate(zip(dcs, comp)):
        if n % (step * per) == 0 and wrong != "predictors_not_reset":
            pred = [0, 0, 0]
        d = v - pred[c]
        pred[c] = v
        cat = abs(d).bit_length()
        dc_syms.append((cat, (d if d >= 0 else d - 1) & ((1 << cat) - 1), cat))
    if optimize:
        freq = [[0] * 256 for _ in range(4)]
        for n, c in enumerate(comp):
            t = 0 if c == 0 else 1
            freq[2 * t][dc_syms[n][0]] += 1
            for s, _, _ in acs[n]:
                freq[2 * t + 1][s] += 1
        built = [gen_optimal_table(f, wrong) for f in freq[:2 * ntab]]
        tables = [(b, v) for b, v, _, _ in built]
        stats.update(limit_moves=sum(m for _, _, m, _ in built), deepest=[d for _, _, _, d in built],
                     single_symbol_tables=sum(len(v) == 1 for _, v, _, _ in built))
    else:
        tables = STANDARD[:2 * ntab]
        stats.update(limit_moves=0, deepest=[], single_symbol_tables=0)
    codes = [_codes(b, v) for b, v in tables]
    out = bytearray()
    stuffed_pads = aligned = markers = wrapped = stuffed = 0
    nint = _ceil(nmcu, step)
    for i in range(nint):
        acc = nbits = 0
        done = bytearray()
        for n in range(i * step * per, min((i + 1) * step, nmcu) * per):
            t = 0 if comp[n] == 0 else 1
            for tab, syms in ((codes[2 * t], (dc_syms[n],)), (codes[2 * t + 1], acs[n])):
                for s, extra, ne in syms:
                    code, length = tab.get(s, (0, 0)) if wrong == "no_reserved_symbol" else tab[s]
                    acc = (((acc << length) | code) << ne) | extra
                    nbits += length + ne
            if nbits >= 4096:                               # flush whole bytes, keep the tail
                keep = nbits & 7
                done += (acc >> keep).to_bytes((nbits - keep) // 8, "big")
                acc &= (1 << keep) - 1
                nbits = keep
        aligned += nbits % 8 == 0
        fill = -nbits % 8
        acc = (acc << fill) | ((1 << fill) - 1)
        raw = bytes(done) + acc.to_bytes((nbits + fill) // 8, "big")
        stuffed += raw.count(b"\xff")
        if fill and raw[-1:] == b"\xff":
            stuffed_pads += 1
            if wrong == "pad_byte_not_stuffed":
                raw = raw[:-1].replace(b"\xff", b"\xff\x00") + b"\xff"
                out += raw
                raw = None
        if raw is not None:
            out += raw.replace(b"\xff", b"\xff\x00")
        if i + 1 < nint:
            wrapped += i > 7
            markers += 1
            out += bytes([0xFF, 0xD0 + (i & 7 if wrong != "n_not_wrapped" else min(i, 15))])
    stats.update(stuffed=stuffed, stuffed_pad_bytes=stuffed_pads, intervals=nint, intervals_byte_aligned=aligned, markers=markers,
                 markers_wrapped=wrapped, blocks=len(dcs), tables=[(list(b[:16]), list(v)) for b, v in tables])
    head = header(img.shape[0], img.shape[1], channels, quality, sampling, tables, ri, wrong)
    stats["header_bytes"] = len(head)
    return head + bytes(out) + b"\xff\xd9", stats


def encode_jpeg(img, quality=95, order="rgb", sampling="4:2:0", optimize=False, restart_interval=0):
    return encode_jpeg_stats(img, quality, order, sampling, optimize, restart_interval)[0]
