"""CPU: the tile plan of Swin2SR's tiled upscale and its restatement (tests/swin2sr_tiled_ref.py).

  plan        on a sweep of (h, w, T, P) that holds n < T, n = T, n = T + 1, n < T + 2 P and P = 0: the cores partition the frame,
              every window lies inside it, all windows have one shape, every core pixel has min(P, its distance to the edge) pixels of
              context on each side, the crop lies inside the window's output
  C plan      nesr_swin2sr_tile_plan (no device, no context) and the package's Python planner give the same rows on the sweep
  refusals    tile < 1, tile_pad < 0, a plan capacity too small, null counts
  faults      each named mistake of the tiling, applied to the restatement, puts wrong samples into a case under swin2sr_ref.u8_check
  criterion   for every case the float32 composition has no wrong sample against the float64 one with tol = 8 x max |f32 - f64|,
              and at most MAX_THIN of the samples are thin
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import swin2sr_cases as C
from tests import swin2sr_ref as R
from tests import swin2sr_tiled_ref as TR

SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 40)
TILES = ((1, 0), (1, 2), (4, 0), (4, 2), (8, 0), (8, 3), (8, 4), (8, 16), (16, 4), (64, 16))
SWEEP = [(h, w, T, P) for (T, P) in TILES for h in SIZES for w in (SIZES if h in (8, 9, 23) else (9, 30))]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


def c_plan(lib, s, h, w, T, P):
    ty, tx, wh, ww = (ctypes.c_int(-1) for _ in range(4))
    counts = (ctypes.byref(ty), ctypes.byref(tx), ctypes.byref(wh), ctypes.byref(ww))
    assert lib.nesr_swin2sr_tile_plan(s, h, w, T, P, *counts, None, 0) == 0, lib.nesr_last_error()
    rows = np.full((ty.value * tx.value + 1, 8), -7, np.int32)          # one row of guard
    ptr = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.nesr_swin2sr_tile_plan(s, h, w, T, P, *counts, ptr, rows.size - 8) == 0, lib.nesr_last_error()
    assert (rows[-1] == -7).all()
    return (ty.value, tx.value), (wh.value, ww.value), [tuple(int(v) for v in r) for r in rows[:-1]]


def test_the_sweep_holds_the_edge_cases():
    per_axis = {(n, T, P) for h, w, T, P in SWEEP for n in (h, w)}
    assert any(n < T for n, T, P in per_axis) and any(n == T for n, T, P in per_axis) and any(n == T + 1 for n, T, P in per_axis)
    assert any(T < n < T + 2 * P for n, T, P in per_axis) and any(P == 0 and n > T for n, T, P in per_axis)
    assert any(n > T + 2 * P and n % T for n, T, P in per_axis)


@pytest.mark.parametrize("s", [1, 3])
def test_plan_properties(s):
    for h, w, T, P in SWEEP:
        (ty, tx), (sy, sx), rows = TR.plan(h, w, T, P, s)
        assert (ty, tx) == (-(-h // T), -(-w // T)) and len(rows) == ty * tx and (sy, sx) == (min(T + 2 * P, h), min(T + 2 * P, w))
        cover = np.zeros((h * s, w * s), np.int32)
        for wy, wx, cy, cx, ch, cw, oy, ox in rows:
            assert 0 <= wy and wy + sy <= h and 0 <= wx and wx + sx <= w, "a window leaves the frame"
            assert ch > 0 and cw > 0 and 0 <= cy and cy + ch <= sy * s and 0 <= cx and cx + cw <= sx * s, "the crop leaves the window's output"
            assert oy - cy == wy * s and ox - cx == wx * s, "the crop and its place do not name the same pixels"
            cover[oy:oy + ch, ox:ox + cw] += 1
            for n, w0, S, c0, c1 in ((h, wy, sy, oy // s, (oy + ch) // s), (w, wx, sx, ox // s, (ox + cw) // s)):
                assert oy % s == 0 and ox % s == 0 and ch % s == 0 and cw % s == 0
                for p in (c0, c1 - 1):                                 # the core's end pixels have the least context
                    assert p - w0 >= min(P, p) and (w0 + S - 1) - p >= min(P, n - 1 - p), (h, w, T, P, p, w0, S)
        assert (cover == 1).all(), "the cores do not partition the frame"


def test_c_plan_and_python_planner_agree_with_the_specification(lib):
    from neural_enhanced_super_resolution_amd._tiling import slid_window_plan
    for s in (2, 4):
        for h, w, T, P in SWEEP:
            want = TR.plan(h, w, T, P, s)
            assert c_plan(lib, s, h, w, T, P) == want, (s, h, w, T, P)
            assert slid_window_plan(h, w, T, P, s) == want, (s, h, w, T, P)


def test_table_rows():
    """The tile counts and window shapes the cases are described by."""
    shapes = {"small_shift": (16, 16), "window_12_frame": (14, 14), "published_width": (20, 24), "x3_range255": (8, 8), "odd_depth_x4": (5, 16),
              "clamp_and_bias": (16, 16), "one_window_high": (16, 9)}
    for name, (h, w), T, P, tiles in TR.TILED_CASES:
        (ty, tx), win, rows = TR.plan(h, w, T, P, C.by_name(name).cfg["upscale"])
        assert ty * tx == tiles == len(rows) and win == shapes[name], (name, ty, tx, win)


def test_plan_refusals_need_no_device(lib):
    from neural_enhanced_super_resolution_amd import Swin2SR, _lib
    ty, tx, wh, ww = (ctypes.c_int(-1) for _ in range(4))
    counts = (ctypes.byref(ty), ctypes.byref(tx), ctypes.byref(wh), ctypes.byref(ww))
    buf = np.full(8 * 12, -7, np.int32)
    ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for args, word in (((2, 21, 30, 0, 4), "tile must"), ((2, 21, 30, -8, 4), "tile must"), ((2, 21, 30, 8, -1), "tile_pad must"),
                       ((2, 0, 30, 8, 4), "H x W"), ((2, 21, -3, 8, 4), "H x W"), ((0, 21, 30, 8, 4), "upscale"), ((9, 21, 30, 8, 4), "upscale")):
        assert lib.nesr_swin2sr_tile_plan(*args, *counts, ptr, buf.size) == _lib.ERR_ARG, args
        assert word in lib.nesr_last_error().decode(), (args, lib.nesr_last_error())
    assert lib.nesr_swin2sr_tile_plan(2, 21, 30, 8, 4, *counts, ptr, 8 * 12 - 1) == _lib.ERR_ARG and "capacity" in lib.nesr_last_error().decode()
    assert (buf == -7).all() and (ty.value, tx.value, wh.value, ww.value) == (3, 4, 16, 16)      # the counts are there, the plan untouched
    assert lib.nesr_swin2sr_tile_plan(2, 21, 30, 8, 4, None, ctypes.byref(tx), ctypes.byref(wh), ctypes.byref(ww), ptr, buf.size) == _lib.ERR_ARG
    m = Swin2SR(**C.by_name("small_shift").cfg)                          # the class's plan needs no device either
    p = m.tile_plan(21, 30, 8, 4)
    assert p["tiles"] == (3, 4) and p["window"] == (16, 16) and [tuple(r) for r in p["plan"].tolist()] == TR.plan(21, 30, 8, 4, 2)[2]
    with pytest.raises(_lib.NesrHipError, match="tile must"):
        m.tile_plan(21, 30, 0, 4)
    with pytest.raises(_lib.NesrHipError, match="tile_pad must"):
        m.tile_plan(21, 30, 8, -2)


@pytest.mark.parametrize("name", [t[0] for t in TR.TILED_CASES])
def test_float32_composition_meets_the_criterion(name):
    """The condition the GPU test's criterion rests on, for the reference alone."""
    frame, y64, y32, tol = TR.tiled_reference(name)
    excluded, wrong, n = R.u8_check(R.quantise(y32), y64, tol)
    print(f"{name}: tol {tol:.3e}, {excluded} of {n} samples thin ({100.0 * excluded / n:.2f} %), {wrong} wrong")
    assert wrong == 0 and excluded <= C.MAX_THIN * n


FAULT_CASES = [(f, n) for f in TR.FAULTS for n in ("small_shift", "x3_range255")] + [("frame_symmetric_pad", "window_12_frame"), ("untiled", "odd_depth_x4"),
                                                                                      ("crop_off_by_row", "one_window_high")]


@pytest.mark.parametrize("fault,name", FAULT_CASES, ids=[f"{f}-{n}" for f, n in FAULT_CASES])
def test_each_named_fault_puts_wrong_samples_into_a_case(fault, name):
    _, (h, w), T, P, _ = TR.tiled_case(name)
    case = C.by_name(name)
    frame, y64, _, tol = TR.tiled_reference(name)
    bad = TR.tiled_float(case.sd, frame, T, P, torch.float32, fault=fault, **case.cfg)
    excluded, wrong, n = R.u8_check(R.quantise(bad), y64, tol)
    print(f"{fault} on {name}: {wrong} of {n} samples wrong ({100.0 * wrong / n:.1f} %)")
    assert wrong > 0
