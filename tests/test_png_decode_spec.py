"""CPU: the specification of the PNG decoder (tests/png_decode_ref.py) against stdlib zlib and png_ref.decode_png -- on the encoder's
own files, on foreign files built with zlib, on hand-made deflate streams and on one broken input per rule -- and the counters that
prove the grid visits every rule."""
import zlib

import numpy as np
import pytest

from tests import png_cases, png_decode_cases as cases, png_decode_ref as ref, png_ref


def _z(data):
    return b"".join(p for k, p in ref._chunks(data) if k == b"IDAT")


def _check(data, frame, seen, serial=False):
    info, segs = ref.parse(data)
    assert info["n_segments"] == len(segs) and segs[0][2] and segs[-1][3]
    want = zlib.decompress(_z(data))
    joined = b""
    if info["contiguous"]:
        for off, nbytes, first, last in segs:                      # every segment alone equals zlib's raw inflate of the same bytes
            out, st, _ = ref.inflate_segment(data[off:off + nbytes], first, last)
            if st == 0:
                assert out == zlib.decompressobj(-15).decompress(data[off:off + nbytes])
        stream, status, cnt = ref.inflate_plan(data, info, segs)
        for k, v in cnt.items():
            seen[k] = max(seen.get(k, 0), v) if k == "maxdist" else seen.get(k, 0) + v
        if status == ref.DEPENDENT:
            seen["dependent_files"] = seen.get("dependent_files", 0) + 1
        else:
            assert status == 0 and stream == want
        joined = b"".join(data[o:o + n] for o, n, _, _ in segs)
        assert joined == ref.deflate_bytes(data)
    else:
        seen["noncontiguous"] = seen.get("noncontiguous", 0) + 1
    got = ref.decode(data)
    assert got.dtype == frame.dtype and np.array_equal(got, frame)
    if serial:
        assert np.array_equal(got, png_ref.decode_png(data, layout=False))


@pytest.fixture(scope="module")
def seen():
    """The whole grid, walked once: the counters of every rule"""
    out = {}
    for kind, h, w, c, d in png_cases.GOLDEN_FILES:
        img, order = png_cases.image(kind, h, w, c, d)
        _check(open(png_cases.golden_path(kind, h, w, c, d), "rb").read(), png_cases.file_order(img, order), out, serial=h * w <= 37 * 53)
    for _, kind, h, w, c, d in png_cases.cases():
        img, order = png_cases.image(kind, h, w, c, d)
        _check(png_cases.spec(kind, h, w, c, d)[0], png_cases.file_order(img, order), out)
    for cid, data, frame in cases.foreign():
        _check(data, frame, out, serial=frame.shape[0] * frame.shape[1] <= 37 * 53 and "ancillary" not in cid)
    for cid, data, frame in cases.handmade() + [cases.far_match()]:
        _check(data, frame, out, serial=frame.size <= 300)
    return out


def test_grid_equals_zlib_and_the_byte_serial_decoder(seen):
    assert seen["segments"] > 200


def test_counters_every_rule_is_visited(seen):
    assert seen["btype0"] and seen["btype1"] and seen["btype2"]
    assert seen["rep16"] and seen["rep17"] and seen["rep18"] and seen["cross16"]
    assert seen["len258"] and seen["overlap"] and seen["stored0"]
    assert seen["far"] and seen["maxdist"] == 32768
    assert seen["nodist"] and seen["onedist"]                   # the two incomplete distance codes zlib allows; our encoder writes both
    assert seen["dependent"] and seen["dependent_files"] >= 2 and seen["noncontiguous"] >= 1


def test_segment_plans():
    full = dict((c[0], c[1]) for c in cases.foreign())
    info, segs = ref.parse(full["70x320x3x8-gradient-full"])
    assert info["contiguous"] and len(segs) == 9 and [s[2] for s in segs] == [1] + [0] * 8 and [s[3] for s in segs] == [0] * 8 + [1]
    info, segs = ref.parse(full["70x320x3x8-impulses-cut100"])
    assert not info["contiguous"] and len(segs) == 1               # arbitrary IDAT cuts: one segment that spans them
    info, segs = ref.parse(full["70x320x3x8-period8-full8"])
    assert ref.inflate_plan(full["70x320x3x8-period8-full8"], info, segs)[1] == 0          # Z_FULL_FLUSH: every segment alone
    info, segs = ref.parse(full["70x320x3x8-period8-sync8"])
    assert ref.inflate_plan(full["70x320x3x8-period8-sync8"], info, segs)[1] == ref.DEPENDENT
    data, _ = png_cases.spec("runs", 70, 320, 3, 8)                 # our own file: one segment per chunk, each its own IDAT
    info, segs = ref.parse(data)
    assert info["contiguous"] and len(segs) == 3 and segs[0][0] == png_ref.HEAD_BYTES + 8


def test_the_long_files_reach_the_second_turn_of_the_device_loops():
    """What tests/png_decode_cases.py says of many_segments and many_pieces, from the parsed plan and the kernels' constants"""
    cid, data, frame = cases.many_segments()
    info, segs = ref.parse(data)
    assert info["contiguous"] and info["n_segments"] == len(segs) > cases.SCAN_LANES          # pngd_scan: a second step of 1024
    assert ref.inflate_plan(data, info, segs)[1] == 0 and np.array_equal(ref.decode(data), frame)
    cid, data, frame = cases.many_pieces()
    info, segs = ref.parse(data)
    npieces = -(-info["stream_bytes"] // cases.kernel_constant("png_decode_kernels.h", "ADLER_PIECE"))
    assert info["contiguous"] and len(segs) >= 2 and npieces > 256                              # pngd_adler_check: 256 lanes, two pieces each
    filt = np.frombuffer(zlib.decompress(_z(data)), np.uint8).reshape(frame.shape[0], frame.shape[1] + 1)
    assert not filt[:, 0].any() and np.array_equal(filt[:, 1:], frame)                          # filter type 0: the file holds the frame


@pytest.mark.parametrize("cid,data,bit", cases.bad() + cases.corrupt()[:3], ids=[c[0] for c in cases.bad() + cases.corrupt()[:3]])
def test_bad_input_gets_its_status_bit_and_a_zlib_error(cid, data, bit):
    info, segs = ref.parse(data)
    assert ref.inflate_plan(data, info, segs)[1] == bit
    with pytest.raises(zlib.error):
        zlib.decompress(_z(data))


@pytest.mark.parametrize("cid,data,bit", cases.corrupt()[3:], ids=[c[0] for c in cases.corrupt()[3:]])
def test_whole_stream_rules(cid, data, bit):
    info, segs = ref.parse(data)
    assert ref.inflate_plan(data, info, segs)[1] == bit
    with pytest.raises(ref.PngError):
        ref.decode(data)


def test_parser_classifies():
    for cid, data in cases.unsupported_files():
        with pytest.raises(ref.PngError) as e:
            ref.parse(data)
        assert e.value.code == ref.UNSUPPORTED, cid
    for cid, data in cases.badfile_files():
        with pytest.raises(ref.PngError) as e:
            ref.parse(data)
        assert e.value.code == ref.BADFILE, cid


def test_unfilter_equals_the_byte_serial_decoder():
    for c, d in png_cases.KINDS:
        frame = png_cases.content("impulses", 9, 11, c, d)
        filt = cases.filtered_cycle(frame, first=2)
        data = cases.make_file(9, 11, c, d, [zlib.compress(filt.tobytes())])
        assert np.array_equal(ref.decode(data), png_ref.decode_png(data, layout=False))
        assert np.array_equal(ref.decode(data), frame)
