"""CPU: the specification of the JPEG decoder (tests/jpeg_decode_ref.py) pixel for pixel against Pillow's libjpeg-turbo, against
committed files and against the reference's asset; the proof, from the specification's counters, that the grid takes every path and
that the boundary files cross the kernels' constants; the host-side parser (nesr_jpeg_parse) against the specification's header
fields and on files outside the supported list; nesr_jpeg_decode_u8's argument checks; decode_jpeg_u8's host route."""
import ctypes
import io
import os

import numpy as np
import pytest

from tests import jpeg_cases, jpeg_decode_cases as dc, jpeg_decode_ref as ref

CASES = dc.cases()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


def _file(case):
    return dc.file_bytes(*case[1:])


# ------------------------------------------------------------------------------------------------ 1: against Pillow
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_specification_equals_pillow(case):
    pytest.importorskip("PIL")                      # only for a machine without Pillow
    from PIL import Image
    data = _file(case)
    want = np.asarray(Image.open(io.BytesIO(data)))
    got = dc.spec(data)[0]
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want)
    if want.ndim == 3:
        assert np.array_equal(ref.decode_jpeg(data, "bgr"), want[:, :, ::-1])


# ------------------------------------------------------------------------------------------------ 2, 3: committed files
@pytest.mark.parametrize("entry", dc.GOLDEN_FILES, ids=[os.path.basename(dc.golden_name(*e)) for e in dc.GOLDEN_FILES])
def test_specification_equals_committed_pixels(entry):
    name = dc.golden_name(*entry)
    with open(name + ".jpg", "rb") as f:
        data = f.read()
    want = np.load(name + ".npy")
    assert 300 < len(data) < 16384 and want.shape[:2] == entry[1:3]
    assert np.array_equal(ref.decode_jpeg(data), want)


def test_specification_decodes_the_reference_asset():
    """images/test.jpeg of the reference: 512 x 512, 4:2:0, DRI = 32, one DQT segment with two tables, one DHT segment with four tables,
    EXIF and ICC segments, no JFIF segment.  Its pixels were recorded from the reference's own read."""
    with open(dc.REFERENCE_ASSET, "rb") as f:
        data = f.read()
    want = np.load(os.path.join(jpeg_cases.GOLDEN, "test_jpeg_full.npz"))["input_bgr"]
    got, s = ref.decode_jpeg_stats(data, "bgr")
    assert np.array_equal(got, want)
    hdr = s["header"]
    assert (hdr["H"], hdr["W"], hdr["C"], hdr["hs"], hdr["vs"], hdr["restart_interval"]) == (512, 512, 3, 2, 2, 32)
    assert s["restart_intervals"] == 32 and len(data) == 145083
    markers = [m for m, _, _ in dc.segments(data)]
    assert markers.count(0xDB) == 1 and markers.count(0xC4) == 1 and 0xE0 not in markers and 0xEE not in markers and 0xE1 in markers and 0xE2 in markers
    # its four tables are Annex K's, in one DHT segment; the decoder takes them from the file like any others
    from tests import jpeg_ref
    assert hdr["ac"][0] == (list(jpeg_ref.AC_LUMA_BITS), list(jpeg_ref.AC_LUMA_VALS)) and hdr["ac"][1] == (list(jpeg_ref.AC_CHROMA_BITS), list(jpeg_ref.AC_CHROMA_VALS))
    assert hdr["dc"][0][0] == list(jpeg_ref.DC_LUMA_BITS) and hdr["dc"][2][0] == list(jpeg_ref.DC_CHROMA_BITS)


# ------------------------------------------------------------------------------------------------ 4: paths and boundaries
def test_grid_takes_every_path():
    stats = {c[0]: dc.spec(_file(c))[1] for c in CASES}
    assert any(s["zrl"] > 0 for s in stats.values()) and any(s["eob"] > 0 for s in stats.values())
    assert any(s["ff00"] > 0 for s in stats.values())
    assert any(s["saturated"] > 0 for n, s in stats.items() if n.startswith("noise") and "-q100-" in n)
    assert any(s["saturated"] > 0 for n, s in stats.items() if n.startswith("impulses") and "-q30-" in n)
    for layout in ("x3-s0", "x3-s1", "x3-s2", "x1-s0"):
        mine = {n: s for n, s in stats.items() if layout in n}
        assert any(s["restart_intervals"] > 1 for s in mine.values()) and any(s["restart_intervals"] == 1 for s in mine.values())
        assert any(s["saturated"] > 0 for s in mine.values())
        for opt in ("plain", "optimize", "rblocks1", "rblocks2", "rblocks5", "rrows1"):
            assert any(n.endswith(opt) for n in mine), (layout, opt)
    # more than eight intervals: the restart numbers wrap
    assert any(s["restart_intervals"] > 8 for s in stats.values())
    # libjpeg's C code wraps an IDCT output beyond +-512 through its range table and its SIMD code saturates; no file of the grid
    # reaches that far, so the difference is not observable here and the kernels saturate
    assert all(s["idct_beyond_wrap"] == 0 for s in stats.values())
    # chroma planes of at most two columns take plain replication, wider ones the fancy upsampler
    widths = {(s["header"]["W"] + 1) // 2 for s in stats.values() if s["header"]["hs"] == 2}
    assert min(widths) <= 2 and max(widths) > 2


def test_the_boundary_files_cross_the_kernels_constants():
    """What tests/jpeg_decode_cases.py says of BOUNDARY, from the specification's counters (csrc/jpeg_decode_kernels.h)."""
    group_bits = dc.SUBSEQ_BITS * dc.SUBSEQ_PER_GROUP
    noise, flat, rows, many = (dc.spec(dc.file_bytes(*b))[1] for b in dc.BOUNDARY)
    # self-synchronising path, more than two workgroups of subsequences, and every workgroup boundary inside a block
    assert noise["restart_intervals"] == 1 and noise["unstuffed_bytes"] * 8 > 2 * group_bits
    starts = noise["block_start_bits"]
    for g in (1, 2, 3):
        assert g * group_bits not in starts and starts[-1] > g * group_bits
    assert noise["scan_bytes"] > 2 * dc.UNSTUFF_CHUNK and noise["ff00"] > 2
    assert noise["blocks"] > 2 * dc.RECON_BLOCKS and noise["blocks"] % dc.RECON_BLOCKS == 0
    # hundreds of blocks start inside one subsequence
    per_sub = np.bincount(flat["block_start_bits"] // dc.SUBSEQ_BITS)
    assert flat["restart_intervals"] == 1 and per_sub.max() > 100 and len(per_sub) > 2
    # one restart interval per block row of 200: markers in several unstuff chunks, 600 blocks = 18.75 reconstruction workgroups
    assert rows["restart_intervals"] == 3 and rows["scan_bytes"] > 2 * dc.UNSTUFF_CHUNK and rows["blocks"] == 600 and rows["blocks"] % dc.RECON_BLOCKS != 0
    # more restart intervals than one workgroup of the restart-interval decode holds, and than 8
    assert many["restart_intervals"] > 2 * 64


def test_the_long_files_reach_the_second_step_of_the_scans(lib):
    """What tests/jpeg_decode_cases.py says of long_scan and many_mcus, from the host parser's fields and the kernels' constants
    (the plan of csrc/jpeg_decode_api.cpp: nchunks = ceil(scan_bytes / UNSTUFF_CHUNK), dc_groups = ceil(MCUs / DC_GROUP))"""
    pytest.importorskip("PIL")
    from neural_enhanced_super_resolution_amd import _lib
    chunk, group = dc.kernel_constant("jpeg_decode_kernels.h", "UNSTUFF_CHUNK"), dc.kernel_constant("jpeg_decode_kernels.h", "DC_GROUP")
    info = _lib.jpeg_parse(dc.long_scan()[1])
    nchunks = -(-info.scan_bytes // chunk)
    assert info.restart_interval == 0 and nchunks > dc.SCAN_LANES                              # jd_scan_chunks carries
    info = _lib.jpeg_parse(dc.many_mcus()[1])
    dc_groups = -(-(info.mcus_x * info.mcus_y) // group)
    assert info.restart_interval == 0 and dc_groups > dc.SCAN_LANES                            # jd_dc_scan carries (no DRI: the DC prefix sum runs)


# ------------------------------------------------------------------------------------------------ 5: parser and argument checks
def _lookup_all(h):
    """Every 16-bit window through the device's table layout (csrc/jpeg_decode.hip: step) -> length << 8 | symbol, 0 when no code matches."""
    v = np.arange(65536, dtype=np.int64)
    look = np.array(h.look, np.int64)[v >> 7]
    out = look.copy()
    todo = look == 0
    maxcode, valoff, vals = np.array(h.maxcode, np.int64), np.array(h.valoff, np.int64), np.array(h.vals, np.int64)
    for length in range(10, 17):
        code = v >> (16 - length)
        hit = todo & (code <= maxcode[length])
        out[hit] = (length << 8) | vals[(code[hit] + valoff[length]) & 255]
        todo &= ~hit
    return out


def test_parser_equals_the_specification(lib):
    from neural_enhanced_super_resolution_amd import _lib
    files = [_file(c) for c in CASES]
    with open(dc.REFERENCE_ASSET, "rb") as f:
        files.append(f.read())
    for i, data in enumerate(files):
        info = _lib.jpeg_parse(data)
        hdr = ref.parse(data)
        assert (info.H, info.W, info.C, info.hs, info.vs, info.restart_interval, info.scan_offset, info.scan_bytes) == tuple(
            hdr[k] for k in ("H", "W", "C", "hs", "vs", "restart_interval", "scan_offset", "scan_bytes"))
        assert info.mcus_x == -(-info.W // (8 * info.hs)) and info.mcus_y == -(-info.H // (8 * info.vs))
        for c in range(info.C):
            assert list(info.q[c]) == hdr["q"][c]
            for mine, theirs in ((info.dc[c], hdr["dc"][c]), (info.ac[c], hdr["ac"][c])):
                lut = np.array(ref._lut16(*theirs), np.int64)
                assert np.array_equal(np.array(mine.look, np.int64), np.where((lut >> 8) <= 9, lut, 0)[::128])
                if i % 16 == 1 or i == len(files) - 1:        # every window, on the files with tables of their own and a few more
                    assert np.array_equal(_lookup_all(mine), lut)
        assert lib.nesr_jpeg_decode_scratch_bytes(ctypes.byref(info)) > info.H * info.W * info.C


def test_parser_classifies_odd_headers(lib):
    pytest.importorskip("PIL")
    from neural_enhanced_super_resolution_amd import _lib
    for name, data, want in dc.odd_headers():
        expected = {"unsupported": (_lib.NesrUnsupportedError, ref.Unsupported, -7), "bad": (_lib.NesrBadFileError, ref.BadFile, -8)}[want]
        with pytest.raises(expected[0]):
            _lib.jpeg_parse(data)
        with pytest.raises(expected[1]):
            ref.parse(data)
        info = _lib.JpegInfo()
        assert lib.nesr_jpeg_parse(data, len(data), ctypes.byref(info)) == expected[2], name
    assert lib.nesr_jpeg_parse(None, 10, ctypes.byref(_lib.JpegInfo())) == -1 and lib.nesr_jpeg_parse(b"\xff\xd8\xff\xd9", 4, None) == -1


def test_parser_survives_every_truncation(lib):
    """Every prefix of a header, and every single-byte change of its first 700 bytes, parses or is rejected: no other outcome."""
    from neural_enhanced_super_resolution_amd import _lib
    with open(dc.golden_name(*dc.GOLDEN_FILES[3]) + ".jpg", "rb") as f:
        data = f.read()
    info = _lib.JpegInfo()
    for n in range(len(data)):
        assert lib.nesr_jpeg_parse(data[:n], n, ctypes.byref(info)) in (0, -7, -8)
    rng = np.random.RandomState(5)
    for at in range(2, min(700, len(data))):
        changed = data[:at] + bytes([rng.randint(0, 256)]) + data[at + 1:]
        rc = lib.nesr_jpeg_parse(changed, len(changed), ctypes.byref(info))
        assert rc in (0, -7, -8)
        if rc == 0:
            assert 0 < info.scan_offset and info.scan_offset + info.scan_bytes <= len(changed)


def test_decode_rejects_bad_arguments_without_touching_a_device(lib):
    """Every pointer below is a made-up address: a check that let one through would fail with NESR_ERR_HIP (no device here) or fault."""
    from neural_enhanced_super_resolution_amd import _lib
    with open(dc.golden_name(*dc.GOLDEN_FILES[3]) + ".jpg", "rb") as f:
        data = f.read()
    info = _lib.jpeg_parse(data)
    p = ctypes.c_void_p(0x10000)
    need = lib.nesr_jpeg_decode_scratch_bytes(ctypes.byref(info))
    assert need > 0 and lib.nesr_jpeg_decode_scratch_bytes(None) == 0

    def call(file=p, n=len(data), info=info, dst=p, stride=info.W * 3, order=0, scratch=p, scratch_bytes=need, status=p):
        return lib.nesr_jpeg_decode_u8(0, file, n, ctypes.byref(info) if info is not None else None, dst, stride, order, scratch, scratch_bytes, status, None)

    for kw in ({"file": None}, {"info": None}, {"dst": None}, {"scratch": None}, {"status": None}, {"stride": info.W * 3 - 1}, {"scratch_bytes": need - 1},
               {"scratch_bytes": 0}, {"order": 2}, {"n": len(data) - 3}, {"scratch": ctypes.c_void_p(0x10004)}, {"status": ctypes.c_void_p(0x10002)}):
        assert call(**kw) == -1, kw
        assert lib.nesr_last_error()
    for field, value in (("H", 0), ("W", 70000), ("C", 2), ("hs", 3), ("vs", 4), ("restart_interval", -1), ("scan_bytes", 0), ("scan_offset", -1), ("mcus_x", 1000)):
        broken = _lib.jpeg_parse(data)
        setattr(broken, field, value)
        assert call(info=broken) == -1, field
        assert lib.nesr_jpeg_decode_scratch_bytes(ctypes.byref(broken)) == 0


# ------------------------------------------------------------------------------------------------ 6: host routes
def test_decode_jpeg_u8_host_route():
    pytest.importorskip("PIL")
    import torch
    from neural_enhanced_super_resolution_amd import imgproc
    for entry in (dc.GOLDEN_FILES[3], dc.GOLDEN_FILES[7], ("noise", 40, 56, 3, 1, 100, {"optimize": True})):
        data = dc.file_bytes(*entry)
        for order in ("rgb", "bgr"):
            got = imgproc.decode_jpeg_u8(data, order=order, use_hip=False, device="cpu")
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), dc.spec_pixels(data, order))
        assert np.array_equal(imgproc.decode_jpeg_u8(data, device="cpu").numpy(), dc.spec_pixels(data))
        with pytest.raises(ValueError):
            imgproc.decode_jpeg_u8(data, use_hip=True, device="cpu")
        with pytest.raises(ValueError):
            imgproc.decode_jpeg_u8(data, order="gbr", device="cpu")
