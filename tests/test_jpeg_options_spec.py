"""CPU: the specification of the JPEG encoder's options (tests/jpeg_options_ref.py: 4:4:4 / 4:2:2 / 4:2:0, optimised Huffman tables,
restart intervals) byte for byte against Pillow's libjpeg-turbo over the grid of tests/jpeg_options_cases.py, against committed
files and digests, the proof from its counters that the grid reaches every rule, and that each listed wrong encoder is told apart."""
import hashlib
import json

import pytest

from tests import jpeg_options_cases as cases
from tests import jpeg_options_ref as ref

IMAGES = [(k, h, w) for (h, w) in cases.SHAPES for k in cases.CONTENTS]


def _files_of(kind, h, w):
    return [f for f in cases.files() if f[:3] == (kind, h, w)]


# ------------------------------------------------------------------------------------------------ 1: against Pillow
@pytest.mark.parametrize("image", IMAGES, ids=[f"{k}_{h}x{w}" for k, h, w in IMAGES])
def test_specification_equals_pillow(image):
    pytest.importorskip("PIL")
    from tests.make_jpeg_options_golden import pillow_file
    files = _files_of(*image)
    assert len(files) == 96
    for f in files:
        assert cases.spec(*f)[0] == pillow_file(f), cases.file_id(f)


def test_default_options_are_the_unchanged_specification():
    from tests import jpeg_ref
    for kind, h, w in [("noise", 37, 53), ("impulses", 17, 9)]:
        for layout in ("gray", "4:2:0"):
            img = cases.image(kind, h, w, layout)
            assert cases.spec(kind, h, w, layout, 95, False, 0)[0] == jpeg_ref.encode_jpeg(img, 95)
    img = cases.image("noise", 9, 17, "gray")
    assert ref.encode_jpeg(img, sampling="4:4:4") == ref.encode_jpeg(img, sampling="4:2:2") == jpeg_ref.encode_jpeg(img), "gray ignores sampling"
    for bad in ("4:4:0", "4:1:1", "444", None):
        with pytest.raises(ValueError):
            ref.encode_jpeg(cases.image("noise", 8, 8, "4:4:4"), sampling=bad)
    for bad in (-1, 65536):
        with pytest.raises(ValueError):
            ref.encode_jpeg(img, restart_interval=bad)


# ------------------------------------------------------------------------------------------------ 2: against committed files
@pytest.mark.parametrize("f", cases.GOLDEN_FILES, ids=[cases.file_id(f) for f in cases.GOLDEN_FILES])
def test_specification_equals_committed_file(f):
    with open(cases.golden_path(f), "rb") as fh:
        want = fh.read()
    assert 150 < len(want) < 16384
    assert cases.spec(*f)[0] == want


@pytest.mark.parametrize("quality,sampling", cases.LENGTH_LIMIT)
def test_length_limit_frames(quality, sampling):
    """The two 512 x 512 frames whose unlimited AC code lengths pass 16 bits: the specification's own counter says the BITS
    adjustment loop moved codes, and the file is Pillow's (committed as length and sha256)."""
    data, st = cases.length_limit_spec(quality, sampling)
    assert st["limit_moves"] > 0 and max(st["deepest"]) > 16, st["deepest"]
    assert all(sum(b) == len(v) and len(b) == 16 for b, v in st["tables"])
    with open(cases.length_limit_digest_path()) as fh:
        want = json.load(fh)[f"q{quality}_{sampling}"]
    assert (len(data), hashlib.sha256(data).hexdigest()) == (want["length"], want["sha256"])
    try:
        from tests.make_jpeg_options_golden import pillow_bytes
    except ImportError:
        return
    assert data == pillow_bytes(cases.length_limit_image(), quality, "rgb", sampling, True, 0)


def test_interval_that_starts_with_ff_on_a_chunks_last_byte():
    """One stream byte that becomes four of the file (FF Dn FF 00) behind 4095 one-byte intervals: the 4096-byte chunk of the
    device's stuffing pass it ends grows beyond three times its size.  The file is Pillow's."""
    img = cases.ff_interval_start_image()
    data, st = ref.encode_jpeg_stats(img, 100, "rgb", "4:2:0", False, 1)
    grown = cases.chunk_outputs(data, st["header_bytes"])
    assert st["intervals"] == 8192 and grown == {0: 3 * 4096 - 2, 1: 3 * 4095 + 4, 2: 2}
    assert b"\xff\xd6\xff\x00" in data
    pytest.importorskip("PIL")
    from tests.make_jpeg_options_golden import pillow_bytes
    assert data == pillow_bytes(img, 100, "rgb", "4:2:0", False, 1)


# ------------------------------------------------------------------------------------------------ 3: the grid reaches every rule
def test_grid_reaches_every_rule():
    total = {k: 0 for k in ("dummy_h2v1", "stuffed_pad_bytes", "markers_wrapped", "intervals_byte_aligned", "single_symbol_tables")}
    gray_optimised = 0
    for f in cases.files():
        if f[0] == "saturated" and f[4] not in (95, 100):      # a quarter of the grid proves nothing new here
            continue
        st = cases.spec(*f)[1]
        for k in total:
            total[k] += st[k]
        gray_optimised += f[3] == "gray" and f[5]
        if f[3] == "4:2:2":
            assert (st["dummy_h2v1"] > 0) == (-(-f[2] // 8) % 2 == 1), cases.file_id(f)
        if f[0] == "constant" and f[5]:
            assert st["single_symbol_tables"] >= 1, cases.file_id(f)
    assert all(v > 0 for v in total.values()), total
    assert gray_optimised > 0
    assert sum(cases.length_limit_spec(*e)[1]["limit_moves"] for e in cases.LENGTH_LIMIT) > 0
    # the committed files alone reach them too (the check without Pillow)
    golden = [cases.spec(*f)[1] for f in cases.GOLDEN_FILES]
    for k in total:
        assert sum(st[k] for st in golden) > 0, k


# ------------------------------------------------------------------------------------------------ 4: wrong encoders are caught
# the file that tells each wrong encoder from libjpeg; all but the length limit's are committed files, so Pillow is not needed
CAUGHT_BY = {
    "h2v1_bias_constant": ("noise", 9, 17, "4:2:2", 95, False, 0),
    "ties_to_smaller_symbol": ("impulses", 25, 7, "4:2:0", 95, True, 0),
    "no_reserved_symbol": ("noise", 37, 53, "gray", 95, True, 3),
    "predictors_not_reset": ("saturated", 9, 17, "gray", 100, False, 1),
    "n_not_wrapped": ("noise", 37, 53, "gray", 95, True, 3),
    "pad_byte_not_stuffed": ("impulses", 64, 96, "4:4:4", 95, True, 3),
    "dri_before_dht": ("noise", 16, 16, "4:2:0", 1, False, 1),
    "dummy_dc_zero": ("noise", 9, 17, "4:2:2", 95, False, 0),
}


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_wrong_encoder_is_caught(wrong):
    if wrong == "no_length_limit":
        q, sampling = cases.LENGTH_LIMIT[1]
        with open(cases.length_limit_digest_path()) as fh:
            want = json.load(fh)[f"q{q}_{sampling}"]
        data = ref.encode_jpeg_stats(cases.length_limit_image(), q, "rgb", sampling, True, 0, wrong=wrong)[0]
        assert hashlib.sha256(data).hexdigest() != want["sha256"]
        return
    f = CAUGHT_BY[wrong]
    assert f in cases.GOLDEN_FILES
    with open(cases.golden_path(f), "rb") as fh:
        want = fh.read()
    assert cases.spec(*f)[0] == want
    assert cases.spec(*f, wrong=wrong)[0] != want, cases.file_id(f)
