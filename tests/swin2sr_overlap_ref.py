"""The specification of Swin2SR's overlapped tiles with averaged seams (nesr_swin2sr_upscale_overlapped_u8, Swin2SR.upscale(tile=,
tile_overlap=)), the tiling of the Swin2SR / SwinIR authors' test script (--tile, --tile_overlap): the plan in plain Python and the
result as a composition of tests/swin2sr_ref.swin2sr_forward, window by window.

For an [H, W, 3] u8 frame, window size ws, scale s, tile T and overlap O: x = frame / 255, padded ONCE by numpy's "symmetric" mode on
the right and bottom to Hp x Wp, the next multiples of ws (the frame's own extension; no processor padding to (n // 8 + 1) * 8,
here or per window).  t = min(T, Hp, Wp) must be a multiple of ws and 0 <= O < t.  Per axis of padded length n the starts are
list(range(0, n - t, t - O)) + [n - t]: the last tile slides back to end at the edge and is in general not on the stride.  Every
t x t window, in row-major order, goes through the network alone (its reflect padding is a no-op); its [3, t s, t s] output after
/ img_range + mean and before any clamp is added into E, and Wt counts the windows that covered a pixel.  out = E / Wt, cropped to
H s x W s; then the usual clamp, x 255, round half to even.  The count is separable, Wt(y, x) = cnt_y(y // s) cnt_x(x // s).

`fault` names one deliberate mistake of the route (FAULTS); tests/test_swin2sr_overlap_host.py shows that each puts wrong samples
into the OVERLAP_CASES rows named for it.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import swin2sr_cases as C
from tests import swin2sr_ref as R

# (case of swin2sr_cases, frame (h, w), tile, tile_overlap, windows, largest count): the frame is R.seeded_frame(h, w, 50 + h)
OVERLAP_CASES = (
    ("small_shift", (21, 30), 8, 4, 35, 4),        # window 4: 24 x 32 padded, 5 x 7 windows on the stride
    ("small_shift", (13, 18), 8, 5, 20, 9),        # stride 3, overlap above t / 2: nine evaluations a pixel, the last start off the stride
    ("x3_range255", (11, 13), 8, 2, 6, 4),         # 12 x 16, stride 6, last starts 4 and 8
    ("odd_depth_x4", (5, 40), 16, 4, 9, 2),        # 8 x 40: t = 8, the tile clamped to the padded height; one row of windows
    ("published_width", (20, 28), 16, 8, 6, 4),    # window 8, embed 180: 24 x 32, 2 x 3 windows
    ("window_7_odd", (15, 20), 14, 6, 4, 4),       # window 7: 21 x 21, stride 8, last start 7
    ("clamp_and_bias", (21, 30), 8, 4, 35, 4),     # outputs that leave [0, 1]
    ("one_window_high", (17, 9), 8, 3, 15, 6),     # 24 x 16, stride 5: starts 0 5 10 15 16 and 0 5 8
    ("window_12_frame", (19, 23), 12, 4, 9, 4),    # window 12: 24 x 24, stride 8, last start 12
)
FAULTS = ("processor_pad", "last_wins", "quantise_first", "regular_count", "clamp_first")
# the rows a fault can fail: regular_count needs a last start off the stride, clamp_first outputs outside [0, 1]
FAULT_ROWS = {"processor_pad": tuple(range(9)), "last_wins": tuple(range(9)), "quantise_first": tuple(range(9)),
              "regular_count": (1, 2, 5, 7, 8), "clamp_first": (6,)}


def starts(n, t, O):
    """The tile starts of one padded axis."""
    assert 1 <= t <= n and 0 <= O < t, (n, t, O)
    return list(range(0, n - t, t - O)) + [n - t]


def counts(n, t, O):
    """cnt[p]: the number of starts v with v <= p < v + t."""
    return [sum(1 for v in starts(n, t, O) if v <= p < v + t) for p in range(n)]


def plan(h, w, T, O, ws, s):
    """((tiles_y, tiles_x), t, (Hp, Wp), rows): a row (win_y, win_x, out_y, out_x) per window in row-major order; the origin in input
    pixels of the padded frame and in output pixels."""
    hp, wp = -(-h // ws) * ws, -(-w // ws) * ws
    t = min(T, hp, wp)
    if t % ws:
        raise ValueError(f"the effective tile {t} is no multiple of window_size {ws}")
    if not 0 <= O < t:
        raise ValueError(f"tile_overlap {O} is not in 0 .. {t - 1}")
    ys, xs = starts(hp, t, O), starts(wp, t, O)
    return (len(ys), len(xs)), t, (hp, wp), [(y, x, y * s, x * s) for y in ys for x in xs]


def padded_frame(frame, ws, dtype):
    """[1, 3, Hp, Wp]: frame / 255 (in float64, then `dtype`), symmetric-padded once to the window."""
    a = np.asarray(frame).astype(np.float64) / 255.0
    h, w = a.shape[:2]
    a = np.pad(a, ((0, -h % ws), (0, -w % ws), (0, 0)), mode="symmetric")
    return torch.from_numpy(a).permute(2, 0, 1).unsqueeze(0).to(dtype).contiguous()


def overlap_float(sd, frame, T, O, dtype=torch.float64, fault=None, **cfg):
    """The overlapped result before the clamp, [h s, w s, 3] in `dtype`: the network on every window, summed in plan order in
    `dtype`, divided by the count."""
    assert fault is None or fault in FAULTS, fault
    c = R.config(**cfg)
    ws, s = c["window_size"], c["upscale"]
    h, w = np.asarray(frame).shape[:2]
    x = padded_frame(frame, ws, dtype)
    _, t, (hp, wp), rows = plan(h, w, T, O, ws, s)
    E = torch.zeros((3, hp * s, wp * s), dtype=dtype)
    Wt = torch.zeros((hp * s, wp * s), dtype=dtype)
    for wy, wx, oy, ox in rows:
        win = x[:, :, wy:wy + t, wx:wx + t].contiguous()
        if fault == "processor_pad":            # the window padded to (t // 8 + 1) * 8 like a frame of the other route
            m = R.padded_size(t)
            win = torch.from_numpy(np.pad(win.numpy(), ((0, 0), (0, 0), (0, m - t), (0, m - t)), mode="symmetric")).contiguous()
        with torch.no_grad():
            y = R.swin2sr_forward(sd, win, **cfg)[0, :, :t * s, :t * s]
        if fault == "quantise_first":           # u8 levels before the mean
            y = (y.clamp(0, 1) * 255.0).round() / 255.0
        elif fault == "clamp_first":
            y = y.clamp(0, 1)
        if fault == "last_wins":                # a paste
            E[:, oy:oy + t * s, ox:ox + t * s] = y
            Wt[oy:oy + t * s, ox:ox + t * s] = 1
        else:
            E[:, oy:oy + t * s, ox:ox + t * s] += y
            Wt[oy:oy + t * s, ox:ox + t * s] += 1
    if fault == "regular_count":                # every start taken on the stride, the last one too
        reg = lambda n: [sum(1 for i in range(len(starts(n, t, O))) if i * (t - O) <= p < i * (t - O) + t) for p in range(n)]
        cy, cx = torch.tensor(reg(hp), dtype=dtype), torch.tensor(reg(wp), dtype=dtype)
        Wt = cy.repeat_interleave(s)[:, None] * cx.repeat_interleave(s)[None, :]      # zero past the last regular tile's end: inf there
    return (E / Wt)[:, :h * s, :w * s].permute(1, 2, 0).contiguous()


@functools.lru_cache(maxsize=None)
def overlap_reference(row):
    """(frame uint8 ndarray, float64 composition [h s, w s, 3], float32 composition, tol = 8 x max |f32 - f64|) of row `row` of
    OVERLAP_CASES, computed once."""
    name, (h, w), T, O, _, _ = OVERLAP_CASES[row]
    case = C.by_name(name)
    frame = R.seeded_frame(h, w, 50 + h)
    y64 = overlap_float(case.sd, frame, T, O, torch.float64, **case.cfg)
    y32 = overlap_float(case.sd, frame, T, O, torch.float32, **case.cfg)
    return frame, y64, y32, 8 * float((y32.double() - y64).abs().max())


def row_id(row):
    name, (h, w), T, O, _, _ = OVERLAP_CASES[row]
    return f"{name}-{h}x{w}-{T}-{O}"
