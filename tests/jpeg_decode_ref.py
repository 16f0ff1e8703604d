"""The specification of the baseline JPEG decoder (csrc/jpeg_decode.hip), numpy only: libjpeg-turbo's default decompressor
(JDCT_ISLOW, fancy upsampling on, no merged upsampling) restated in integers, as cv2.imread(path, IMREAD_UNCHANGED) and Pillow's
Image.open run it.  tests/test_jpeg_decode_spec.py pins it against Pillow pixel for pixel.

EXIF orientation is NOT applied: that is IMREAD_UNCHANGED's behaviour (and Pillow's).  cv2.imread's default flag would rotate a
file whose orientation is not 1; the reference's asset has orientation 1, so both readings agree on it.

Supported input (parse raises Unsupported for a valid file outside it, BadFile for a malformed one):
  SOF0 or SOF1 Huffman, 8 bits, one interleaved scan over all components, 1 component or 3 (YCbCr), sampling 1x1 gray, 4:4:4,
  4:2:2 (h2v1), 4:2:0 (h2v2), 8-bit DQT, any DHT, any DRI; APPn and COM are skipped.

decode_jpeg(data, order) -> [H, W, 3] (order "rgb" or "bgr") or [H, W] for a gray file.
decode_jpeg_stats(data, order) -> (pixels, counters); the counters prove which paths an input takes.
"""
from __future__ import annotations

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Unsupported(ValueError):
    """A valid JPEG file outside the supported list."""


class BadFile(ValueError):
    """Malformed marker segments, or a scan that cannot be decoded."""


# ------------------------------------------------------------------------------------------------------------------ header
def parse(data):
    """Walks the marker segments up to and including SOS.  -> dict: H, W, C, hs, vs (the luma sampling factors; 1, 1 for gray),
    restart_interval, scan_offset, scan_bytes, q[comp] (natural order), dc[comp] / ac[comp] = (bits[16], vals)."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise BadFile("no SOI")
    pos = 2
    qt, huff = {}, {}
    frame = None
    ri = 0
    adobe = None
    while True:
        if pos + 2 > n:
            raise BadFile("the header ends before SOS")
        if data[pos] != 0xFF:
            raise BadFile(f"no marker at byte {pos}")
        while pos + 1 < n and data[pos + 1] == 0xFF:                   # fill bytes
            pos += 1
        if pos + 2 > n:
            raise BadFile("the header ends before SOS")
        m = data[pos + 1]
        pos += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise BadFile("EOI before SOS")
        if pos + 2 > n:
            raise BadFile("a segment length past the end")
        seg_len = (data[pos] << 8) | data[pos + 1]
        if seg_len < 2 or pos + seg_len > n:
            raise BadFile("a segment length past the end")
        seg = data[pos + 2:pos + seg_len]
        if m in (0xC0, 0xC1):
            if frame is not None:
                raise BadFile("two frame headers")
            if len(seg) < 6:
                raise BadFile("short SOF")
            prec, H, W, C = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if len(seg) < 6 + 3 * C:
                raise BadFile("short SOF")
            if prec != 8:
                raise Unsupported(f"{prec}-bit precision")
            if C not in (1, 3):
                raise Unsupported(f"{C} components")
            if H == 0 or W == 0:
                raise BadFile("an empty frame")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(C)]
            frame = (H, W, C, comps)
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Unsupported(f"SOF{m - 0xC0}: progressive, lossless, hierarchical or arithmetic coding")
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    raise BadFile("short DHT")
                tc, th = seg[at] >> 4, seg[at] & 15
                bits = list(seg[at + 1:at + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or at + 17 + cnt > len(seg):
                    raise BadFile("bad DHT")
                code = 0
                for length in range(1, 17):                            # the codes of a length must fit that length
                    code += bits[length - 1]
                    if code > (1 << length):
                        raise BadFile("bad DHT")
                    code <<= 1
                huff[(tc, th)] = (bits, list(seg[at + 17:at + 17 + cnt]))
                at += 17 + cnt
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    if pq == 1:
                        raise Unsupported("16-bit DQT")
                    raise BadFile("bad DQT")
                if tq > 3 or at + 65 > len(seg):
                    raise BadFile("bad DQT")
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = seg[at + 1 + k]
                qt[tq] = t
                at += 65
        elif m == 0xDD:
            if len(seg) < 2:
                raise BadFile("short DRI")
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise BadFile("SOS before SOF")
            H, W, C, comps = frame
            if len(seg) < 1 or len(seg) < 4 + 2 * seg[0]:
                raise BadFile("short SOS")
            ns = seg[0]
            if ns != C:
                raise Unsupported("more than one scan")
            sel = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            if [s[0] for s in sel] != [c[0] for c in comps]:
                raise Unsupported("the scan's components are not the frame's in order")
            if seg[1 + 2 * ns] != 0 or seg[2 + 2 * ns] != 63 or seg[3 + 2 * ns] != 0:
                raise Unsupported("a spectral selection or successive approximation")
            if C == 3:
                if adobe == 0:
                    raise Unsupported("Adobe transform 0 (RGB)")
                if [c[0] for c in comps] == [ord("R"), ord("G"), ord("B")] and adobe is None:
                    raise Unsupported("RGB component ids")
                if comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1) or comps[0][1:3] not in ((1, 1), (2, 1), (2, 2)):
                    raise Unsupported("sampling factors other than 4:4:4, 4:2:2, 4:2:0")
                hs, vs = comps[0][1], comps[0][2]
            else:
                hs = vs = 1                                            # a single component's scan is not interleaved: one block per MCU
            out = dict(H=H, W=W, C=C, hs=hs, vs=vs, restart_interval=ri, q=[], dc=[], ac=[])
            for (cid, _, _, tq), (_, td, ta) in zip(comps, sel):
                if tq not in qt or (0, td) not in huff or (1, ta) not in huff:
                    raise BadFile("a table the scan names is missing")
                out["q"].append(qt[tq])
                out["dc"].append(huff[(0, td)])
                out["ac"].append(huff[(1, ta)])
            out["scan_offset"] = pos + seg_len
            end = n - 2 if n - 2 >= pos + seg_len and data[n - 2] == 0xFF and data[n - 1] == 0xD9 else n
            out["scan_bytes"] = end - out["scan_offset"]
            if out["scan_bytes"] < 1:
                raise BadFile("an empty scan")
            return out
        pos += seg_len


# ------------------------------------------------------------------------------------------------------------------ entropy
def _lut16(bits, vals):
    """16-bit window -> (length << 8) | symbol, 0 where no code matches."""
    lut = np.zeros(65536, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            if k < len(vals):
                lo = code << (16 - length)
                lut[lo:lo + (1 << (16 - length))] = (length << 8) | vals[k]
            k += 1
            code += 1
        code <<= 1
    return lut.tolist()


def unstuff(scan):
    """The scan's bytes -> (unstuffed stream, byte offsets at which a restart interval begins (the first is 0), RSTn numbers,
    FF 00 pairs).  A byte is dropped when it is the 00 of FF 00 or either byte of FF Dn."""
    b = np.frombuffer(scan, np.uint8)
    n = len(b)
    prev = np.concatenate([[0], b[:-1]]) if n else b
    nxt = np.concatenate([b[1:], [0]]) if n else b
    zero = (b == 0) & (prev == 0xFF)
    rst_hi = (b == 0xFF) & (nxt >= 0xD0) & (nxt <= 0xD7)
    rst_lo = (b >= 0xD0) & (b <= 0xD7) & (prev == 0xFF)
    keep = ~(zero | rst_hi | rst_lo)
    kept_before = np.cumsum(keep) - keep
    starts = [0] + kept_before[rst_hi].tolist()
    numbers = (nxt[rst_hi] - 0xD0).tolist()
    return b[keep].tobytes(), starts, numbers, int(zero.sum())


class _Bits:
    def __init__(self, data, start, end):
        self.d = data + b"\0\0\0\0\0"
        self.p = start * 8
        self.end = end * 8

    def peek16(self):
        i = self.p >> 3
        d = self.d
        return (((d[i] << 16) | (d[i + 1] << 8) | d[i + 2]) >> (8 - (self.p & 7))) & 0xFFFF


def _decode_scan(hdr, scan, stats):
    """-> coef[nblocks, 64] int32, natural order, dequantised, blocks in scan order."""
    H, W, C, hs, vs = hdr["H"], hdr["W"], hdr["C"], hdr["hs"], hdr["vs"]
    mcus_x, mcus_y = -(-W // (8 * hs)), -(-H // (8 * vs))
    per = hs * vs + 2 if C == 3 else 1
    comp_of = [0] * (hs * vs) + [1, 2] if C == 3 else [0]
    nmcu = mcus_x * mcus_y
    stream, starts, numbers, ff00 = unstuff(scan)
    ri = hdr["restart_interval"]
    nseg = -(-nmcu // ri) if ri else 1
    if len(starts) != nseg:
        raise BadFile(f"{len(starts) - 1} restart markers, {nseg - 1} expected")
    if any(v != (i & 7) for i, v in enumerate(numbers)):
        raise BadFile("a restart marker out of sequence")
    dc_lut = [_lut16(*t) for t in hdr["dc"]]
    ac_lut = [_lut16(*t) for t in hdr["ac"]]
    coef = np.zeros((nmcu * per, 64), np.int32)
    block_bits = np.zeros(nmcu * per, np.int64)
    zrl = eob = 0
    bounds = starts + [len(stream)]
    for s in range(nseg):
        br = _Bits(stream, bounds[s], bounds[s + 1])
        pred = [0, 0, 0]
        first = s * ri if ri else 0
        last = min(first + ri, nmcu) if ri else nmcu
        for blk in range(first * per, last * per):
            comp = comp_of[blk % per]
            block_bits[blk] = br.p
            e = dc_lut[comp][br.peek16()]
            if e == 0:
                raise BadFile("a code that is not in the table")
            br.p += e >> 8
            size = e & 255
            if size > 15:
                raise BadFile("a DC size above 15")
            diff = 0
            if size:
                v = br.peek16() >> (16 - size)
                br.p += size
                diff = v if v >= (1 << (size - 1)) else v - (1 << size) + 1
            pred[comp] += diff
            row = coef[blk]
            row[0] = pred[comp]
            k = 1
            lut = ac_lut[comp]
            while k < 64:
                e = lut[br.peek16()]
                if e == 0:
                    raise BadFile("a code that is not in the table")
                br.p += e >> 8
                run, size = (e >> 4) & 15, e & 15
                if size == 0:
                    if run == 15:
                        zrl += 1
                        k += 16
                        continue
                    eob += 1
                    break
                k += run
                if k > 63:
                    raise BadFile("a run past coefficient 63")
                v = br.peek16() >> (16 - size)
                br.p += size
                row[ZIGZAG[k]] = v if v >= (1 << (size - 1)) else v - (1 << size) + 1
                k += 1
            if br.p > br.end:
                raise BadFile("the stream ends early")
    q = np.array(hdr["q"], np.int32)
    comp_idx = np.array([comp_of[i % per] for i in range(nmcu * per)])
    coef *= q[comp_idx]
    stats.update(restart_intervals=nseg, zrl=zrl, eob=eob, ff00=ff00, scan_bytes=len(scan), unstuffed_bytes=len(stream),
                 blocks=nmcu * per, block_start_bits=block_bits)
    return coef


# ------------------------------------------------------------------------------------------------------------------ IDCT
def _idct_pass(d, shift):
    """jidctint.c: one 8-point pass along axis 0 of d[8, ...] (int64), descaled by `shift` bits."""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (d[0] + d[4]) << 13
    tmp1 = (d[0] - d[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = -z1 * 7373, -z2 * 20995
    z3, z4 = -z3 * 16069 + z5, -z4 * 3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([(tmp10 + t3 + r) >> shift, (tmp11 + t2 + r) >> shift, (tmp12 + t1 + r) >> shift, (tmp13 + t0 + r) >> shift,
                     (tmp13 - t0 + r) >> shift, (tmp12 - t1 + r) >> shift, (tmp11 - t2 + r) >> shift, (tmp10 - t3 + r) >> shift])


def idct_blocks(coef, stats=None):
    """coef[n, 64] dequantised, natural order -> samples[n, 8, 8] uint8.  Columns first (descale 11), then rows (descale 18), plus
    128, clamped to 0..255.  libjpeg's C code indexes its range table with the result & 1023, which wraps a value beyond +-512
    round; its SIMD code saturates instead.  `idct_beyond_wrap` counts the samples on which the two differ."""
    c = coef.astype(np.int64).reshape(-1, 8, 8)
    ws = _idct_pass(np.moveaxis(c, 1, 0), 11)                          # [r_out, n, col]
    ws = ws.astype(np.int32).astype(np.int64)
    out = _idct_pass(np.moveaxis(ws, 2, 0), 18)                        # [c_out, r, n]
    out = np.moveaxis(out, (0, 1, 2), (2, 1, 0))                       # [n, r, c]
    if stats is not None:
        stats["saturated"] = stats.get("saturated", 0) + int(((out < -128) | (out > 127)).sum())
        stats["idct_beyond_wrap"] = stats.get("idct_beyond_wrap", 0) + int(((out < -512) | (out > 511)).sum())
    return np.clip(out + 128, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ upsampling
def _h2v1(p, w_out):
    """jdsample.c h2v1_fancy_upsample on the rows of p[rows, cw] -> [rows, w_out]; plain replication when cw <= 2."""
    cw = p.shape[1]
    s = p.astype(np.int32)
    if cw <= 2:
        return np.repeat(p, 2, axis=1)[:, :w_out]
    prev = np.concatenate([s[:, :1], s[:, :-1]], 1)
    nxt = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    even = (3 * s + prev + 1) >> 2
    odd = (3 * s + nxt + 2) >> 2
    even[:, 0] = s[:, 0]
    odd[:, -1] = s[:, -1]
    out = np.empty((p.shape[0], 2 * cw), np.int32)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out[:, :w_out].astype(np.uint8)


def _h2v2(p, h_out, w_out):
    """jdsample.c h2v2_fancy_upsample on p[ch, cw] (the real samples only: ceil(H / 2) x ceil(W / 2)) -> [h_out, w_out]: the row above
    the first and below the last is that row itself, likewise the columns; plain replication when cw <= 2."""
    ch, cw = p.shape
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h_out, :w_out]
    s = p.astype(np.int32)
    above = np.concatenate([s[:1], s[:-1]], 0)
    below = np.concatenate([s[1:], s[-1:]], 0)
    col = np.empty((2 * ch, cw), np.int32)
    col[0::2], col[1::2] = 3 * s + above, 3 * s + below
    last = np.concatenate([col[:, :1], col[:, :-1]], 1)
    nxt = np.concatenate([col[:, 1:], col[:, -1:]], 1)
    out = np.empty((2 * ch, 2 * cw), np.int32)
    out[:, 0::2] = (3 * col + last + 8) >> 4
    out[:, 1::2] = (3 * col + nxt + 7) >> 4
    return out[:h_out, :w_out].astype(np.uint8)


def _planes(hdr, samples):
    """samples[nblocks, 8, 8] in scan order -> the component planes, padded to whole MCUs."""
    H, W, C, hs, vs = hdr["H"], hdr["W"], hdr["C"], hdr["hs"], hdr["vs"]
    mcus_x, mcus_y = -(-W // (8 * hs)), -(-H // (8 * vs))
    if C == 1:
        return [samples.reshape(mcus_y, mcus_x, 8, 8).transpose(0, 2, 1, 3).reshape(mcus_y * 8, mcus_x * 8)]
    per = hs * vs + 2
    m = samples.reshape(mcus_y, mcus_x, per, 8, 8)
    y = m[:, :, :hs * vs].reshape(mcus_y, mcus_x, vs, hs, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mcus_y * vs * 8, mcus_x * hs * 8)
    cb = m[:, :, hs * vs].transpose(0, 2, 1, 3).reshape(mcus_y * 8, mcus_x * 8)
    cr = m[:, :, hs * vs + 1].transpose(0, 2, 1, 3).reshape(mcus_y * 8, mcus_x * 8)
    return [y, cb, cr]


def decode_jpeg_stats(data, order="rgb"):
    if order not in ("rgb", "bgr"):
        raise ValueError(f"order must be 'rgb' or 'bgr', got {order!r}")
    data = bytes(data)
    hdr = parse(data)
    stats = {}
    coef = _decode_scan(hdr, data[hdr["scan_offset"]:hdr["scan_offset"] + hdr["scan_bytes"]], stats)
    planes = _planes(hdr, idct_blocks(coef, stats))
    H, W, hs, vs = hdr["H"], hdr["W"], hdr["hs"], hdr["vs"]
    stats["header"] = hdr
    if hdr["C"] == 1:
        return planes[0][:H, :W].copy(), stats
    y = planes[0][:H, :W].astype(np.int32)
    ch, cw = -(-H // vs), -(-W // hs)
    chroma = []
    for p in planes[1:]:
        p = p[:ch, :cw]
        chroma.append((_h2v2(p, H, W) if vs == 2 else _h2v1(p, W) if hs == 2 else p).astype(np.int32) - 128)
    cb, cr = chroma
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    out = np.stack([r, g, b] if order == "rgb" else [b, g, r], -1)
    return np.clip(out, 0, 255).astype(np.uint8), stats


def decode_jpeg(data, order="rgb"):
    return decode_jpeg_stats(data, order)[0]
