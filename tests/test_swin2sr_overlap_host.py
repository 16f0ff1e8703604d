"""CPU: the plan of Swin2SR's overlapped tiles and its restatement (tests/swin2sr_overlap_ref.py).

  plans       nesr_swin2sr_overlap_plan (no device, no context), the package's _tiling.overlap_plan and the specification give the
              same counts, tile, padded size and rows on a sweep of (h, w, T, O) with windows of 4, 7, 8 and 12
  properties  every padded pixel is covered; the number of windows over a pixel is cnt_y cnt_x; the last window of an axis ends at
              n; an axis no longer than the effective tile has one window; all windows lie inside the padded frame
  refusals    tile < 1, an effective tile that is no multiple of the window, tile_overlap < 0 or >= the effective tile, a plan
              capacity too small, null counts, a bad scale or frame; Swin2SR.overlap_plan needs no device either
  table       the window counts and the largest per-pixel counts the rows are described by
  faults      each named mistake of the route, applied to the float32 restatement, puts wrong samples into every row named for it
  criterion   for every row the float32 composition has no wrong sample against the float64 one with tol = 8 x max |f32 - f64|,
              and at most MAX_THIN of the samples are thin
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import swin2sr_cases as C
from tests import swin2sr_overlap_ref as OR
from tests import swin2sr_ref as R

SIZES = (1, 3, 7, 8, 9, 16, 17, 24, 25, 40, 61)
ROWS = list(range(len(OR.OVERLAP_CASES)))


def sweep():
    """(h, w, T, O, ws): valid plans only (the refusals have their own test)."""
    out = []
    for ws in (4, 7, 8, 12):
        for h in SIZES:
            for w in (SIZES if h in (9, 24) else (5, 30)):
                hp, wp = -(-h // ws) * ws, -(-w // ws) * ws
                for T in (ws, 2 * ws, 3 * ws, 5 * ws, 1000):
                    t = min(T, hp, wp)
                    if t % ws:
                        continue
                    for O in sorted({0, 1, 2, t // 4, t // 2, t // 2 + 1, t - 2, t - 1}):
                        if 0 <= O < t:
                            out.append((h, w, T, O, ws))
    return out


SWEEP = sweep()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


def c_plan(lib, s, ws, h, w, T, O):
    vals = [ctypes.c_int(-1) for _ in range(5)]
    counts = tuple(ctypes.byref(v) for v in vals)
    assert lib.nesr_swin2sr_overlap_plan(s, ws, h, w, T, O, *counts, None, 0) == 0, lib.nesr_last_error()
    ty, tx, t, hp, wp = (v.value for v in vals)
    rows = np.full((ty * tx + 1, 4), -7, np.int32)                     # one row of guard
    ptr = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.nesr_swin2sr_overlap_plan(s, ws, h, w, T, O, *counts, ptr, rows.size - 4) == 0, lib.nesr_last_error()
    assert (rows[-1] == -7).all()
    return (ty, tx), t, (hp, wp), [tuple(int(v) for v in r) for r in rows[:-1]]


def test_the_sweep_holds_the_edge_cases():
    assert len(SWEEP) > 1000
    axes = set()
    for h, w, T, O, ws in SWEEP:
        for n in (h, w):
            npad = -(-n // ws) * ws
            axes.add((npad, min(T, -(-h // ws) * ws, -(-w // ws) * ws), O))
    assert any(n == t for n, t, O in axes) and any(n > t and O == 0 for n, t, O in axes) and any(O == t - 1 and n > t for n, t, O in axes)
    assert any(n > t and (n - t) % (t - O) for n, t, O in axes), "no last start off the stride"
    assert any(n > t and (n - t) % (t - O) == 0 for n, t, O in axes) and any(2 * O > t for n, t, O in axes)


def test_the_three_plans_agree(lib):
    from neural_enhanced_super_resolution_amd._tiling import overlap_plan
    for s in (2, 3):
        for h, w, T, O, ws in SWEEP:
            want = OR.plan(h, w, T, O, ws, s)
            assert c_plan(lib, s, ws, h, w, T, O) == want, (s, h, w, T, O, ws)
            assert overlap_plan(h, w, T, O, ws, s) == want, (s, h, w, T, O, ws)


def test_plan_properties():
    for h, w, T, O, ws in SWEEP:
        s = 2
        (ty, tx), t, (hp, wp), rows = OR.plan(h, w, T, O, ws, s)
        assert hp % ws == 0 and wp % ws == 0 and 0 <= hp - h < ws and 0 <= wp - w < ws and t == min(T, hp, wp) and len(rows) == ty * tx
        cover = np.zeros((hp, wp), np.int64)
        for wy, wx, oy, ox in rows:
            assert 0 <= wy and wy + t <= hp and 0 <= wx and wx + t <= wp, "a window leaves the padded frame"
            assert (oy, ox) == (wy * s, wx * s)
            cover[wy:wy + t, wx:wx + t] += 1
        assert (cover >= 1).all(), "a padded pixel no window covers"
        assert (cover == np.outer(OR.counts(hp, t, O), OR.counts(wp, t, O))).all(), "the count is not cnt_y cnt_x"
        assert rows[-1][0] + t == hp and rows[-1][1] + t == wp, "the last window does not end at the edge"
        assert rows == sorted(rows) and len(set(rows)) == len(rows), "not row-major, or a window twice"
        for n, k in ((hp, ty), (wp, tx)):
            assert k == len(OR.starts(n, t, O)) and (k == 1) == (n == t)      # t <= T: an axis no longer than the tile has one window
            assert max(OR.counts(n, t, O)) <= -(-t // (t - O)) + 1


def test_table_rows():
    for (name, (h, w), T, O, windows, most) in OR.OVERLAP_CASES:
        cfg = R.config(**C.by_name(name).cfg)
        (ty, tx), t, (hp, wp), rows = OR.plan(h, w, T, O, cfg["window_size"], cfg["upscale"])
        assert ty * tx == windows == len(rows), (name, ty, tx)
        assert max(OR.counts(hp, t, O)) * max(OR.counts(wp, t, O)) == most, name
    assert OR.plan(5, 40, 16, 4, 4, 4)[1] == 8                            # the tile clamped to the padded height
    for fault, rows in OR.FAULT_ROWS.items():                             # regular_count is named for the rows whose last start is off the stride
        if fault == "regular_count":
            for i, (name, (h, w), T, O, _, _) in enumerate(OR.OVERLAP_CASES):
                ws = R.config(**C.by_name(name).cfg)["window_size"]
                _, t, (hp, wp), _ = OR.plan(h, w, T, O, ws, 1)
                off = any(n > t and (n - t) % (t - O) for n in (hp, wp))
                assert off == (i in rows), (i, name)


def test_plan_refusals_need_no_device(lib):
    from neural_enhanced_super_resolution_amd import Swin2SR, _lib
    from neural_enhanced_super_resolution_amd._tiling import overlap_plan
    vals = [ctypes.c_int(-1) for _ in range(5)]
    counts = tuple(ctypes.byref(v) for v in vals)
    buf = np.full(4 * 35, -7, np.int32)
    ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    # (upscale, window_size, H, W, tile, tile_overlap)
    for args, word in (((2, 4, 21, 30, 0, 4), "tile must"), ((2, 4, 21, 30, -8, 4), "tile must"), ((2, 4, 21, 30, 6, 2), "multiple of window_size 4"),
                       ((2, 7, 15, 20, 10, 2), "multiple of window_size 7"),
                       ((2, 4, 21, 30, 8, -1), "tile_overlap must"), ((2, 4, 21, 30, 8, 8), "tile_overlap must"), ((2, 4, 5, 40, 16, 8), "tile_overlap must"),
                       ((2, 4, 0, 30, 8, 4), "H x W"), ((2, 4, 21, -3, 8, 4), "H x W"), ((0, 4, 21, 30, 8, 4), "upscale"), ((9, 4, 21, 30, 8, 4), "upscale"),
                       ((2, 0, 21, 30, 8, 4), "window_size")):
        assert lib.nesr_swin2sr_overlap_plan(*args, *counts, ptr, buf.size) == _lib.ERR_ARG, args
        assert word in lib.nesr_last_error().decode(), (args, lib.nesr_last_error())
    assert lib.nesr_swin2sr_overlap_plan(2, 4, 21, 30, 8, 4, *counts, ptr, 4 * 35 - 1) == _lib.ERR_ARG and "capacity" in lib.nesr_last_error().decode()
    assert (buf == -7).all() and tuple(v.value for v in vals) == (5, 7, 8, 24, 32)      # the counts are there, the plan untouched
    assert lib.nesr_swin2sr_overlap_plan(2, 4, 21, 30, 8, 4, None, *counts[1:], ptr, buf.size) == _lib.ERR_ARG
    m = Swin2SR(**C.by_name("small_shift").cfg)                          # the class's plan needs no device either
    p = m.overlap_plan(21, 30, 8, 4)
    assert p["tiles"] == (5, 7) and p["tile"] == 8 and p["padded"] == (24, 32)
    assert [tuple(r) for r in p["plan"].tolist()] == OR.plan(21, 30, 8, 4, 4, 2)[3]
    with pytest.raises(_lib.NesrHipError, match="multiple of window_size 4"):
        m.overlap_plan(21, 30, 6, 2)
    with pytest.raises(_lib.NesrHipError, match="tile_overlap must"):
        m.overlap_plan(21, 30, 8, 8)
    for bad in ((21, 30, 6, 2, 4, 2), (21, 30, 8, 8, 4, 2), (21, 30, 8, -1, 4, 2), (21, 30, 0, 0, 4, 2)):
        with pytest.raises(ValueError):
            overlap_plan(*bad)


@pytest.mark.parametrize("row", ROWS, ids=OR.row_id)
def test_float32_composition_meets_the_criterion(row):
    """The condition the GPU test's criterion rests on, for the reference alone."""
    frame, y64, y32, tol = OR.overlap_reference(row)
    excluded, wrong, n = R.u8_check(R.quantise(y32), y64, tol)
    print(f"{OR.row_id(row)}: tol {tol:.3e}, {excluded} of {n} samples thin ({100.0 * excluded / n:.2f} %), {wrong} wrong")
    assert wrong == 0 and excluded <= C.MAX_THIN * n


FAULT_CASES = [(f, r) for f in OR.FAULTS for r in OR.FAULT_ROWS[f]]


@pytest.mark.parametrize("fault,row", FAULT_CASES, ids=[f"{f}-{OR.row_id(r)}" for f, r in FAULT_CASES])
def test_each_named_fault_puts_wrong_samples_into_its_rows(fault, row):
    name, (h, w), T, O, _, _ = OR.OVERLAP_CASES[row]
    case = C.by_name(name)
    frame, y64, _, tol = OR.overlap_reference(row)
    bad = OR.overlap_float(case.sd, frame, T, O, torch.float32, fault=fault, **case.cfg)
    excluded, wrong, n = R.u8_check(R.quantise(bad), y64, tol)
    print(f"{fault} on {OR.row_id(row)}: {wrong} of {n} samples wrong ({100.0 * wrong / n:.1f} %)")
    assert wrong > 0
