"""The specification of Swin2SR's tiled upscale (nesr_swin2sr_upscale_tiled_u8, Swin2SR.upscale(tile=, tile_pad=)): the tile plan
in plain Python and the tiled result as a composition of tests/swin2sr_ref.upscale_float, window by window.

The plan, per axis of length n with tile T >= 1 and tile_pad P >= 0: cores i = 0 .. ceil(n / T) - 1, [c0, c1) = [i T, min((i + 1) T,
n)); every window is S = min(T + 2 P, n) long and starts at w0 = clamp(c0 - P, 0, n - S).  A window at the edge slides inward
instead of shrinking, so all windows of a frame have one shape.  Each window is a frame of its own to `upscale_float` (/ 255, the
processor's symmetric padding to (S // 8 + 1) * 8, the model's reflect padding, the network, the crop to S s); rows
[(c0 - w0) s, (c1 - w0) s) and the matching columns of its output land at (c0y s, c0x s) of the result.

`fault` names one deliberate mistake of the tiling (FAULTS); tests/test_swin2sr_tiled_host.py shows that each puts wrong samples
into a case of TILED_CASES.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import swin2sr_cases as C
from tests import swin2sr_ref as R

# (case of swin2sr_cases, frame (h, w), tile, tile_pad, tiles): the frame is R.seeded_frame(h, w, 50 + h)
TILED_CASES = (
    ("small_shift", (21, 30), 8, 4, 12),          # windows 16 x 16, 24 x 24 to the model
    ("window_12_frame", (19, 23), 8, 3, 9),       # 14 x 14 -> 16 x 16 -> 24 x 24: both paddings in every window
    ("published_width", (20, 28), 16, 4, 4),      # 20 x 24 -> 24 x 32: the window's height clamped to the frame
    ("x3_range255", (11, 13), 4, 2, 12),          # 8 x 8 -> 16 x 16
    ("odd_depth_x4", (5, 40), 8, 4, 5),           # 5 x 16 -> 8 x 24: a frame shorter than the window's side
    ("clamp_and_bias", (21, 30), 8, 4, 12),
    ("one_window_high", (17, 9), 8, 4, 6),        # 16 x 9 -> 24 x 16
)
FAULTS = ("crop_without_w0", "shrunk_windows", "frame_symmetric_pad", "crop_off_by_row", "untiled")


def tiled_case(name):
    return next(t for t in TILED_CASES if t[0] == name)


def axis(n, T, P):
    """(S, [(w0, c0, c1)]) of one axis."""
    assert n >= 1 and T >= 1 and P >= 0, (n, T, P)
    S = min(T + 2 * P, n)
    out = []
    for i in range(-(-n // T)):
        c0, c1 = i * T, min((i + 1) * T, n)
        out.append((min(max(c0 - P, 0), n - S), c0, c1))
    return S, out


def plan(h, w, T, P, s):
    """((tiles_y, tiles_x), (win_h, win_w), rows): a row (win_y, win_x, crop_y, crop_x, crop_h, crop_w, out_y, out_x) per tile in
    row-major order; the window's origin in input pixels, the rest in output pixels."""
    sy, ys = axis(h, T, P)
    sx, xs = axis(w, T, P)
    rows = [(wy, wx, (y0 - wy) * s, (x0 - wx) * s, (y1 - y0) * s, (x1 - x0) * s, y0 * s, x0 * s) for wy, y0, y1 in ys for wx, x0, x1 in xs]
    return (len(ys), len(xs)), (sy, sx), rows


def _window_against_the_frame(sd, frame, wy, wx, sy, sx, dtype, **cfg):
    """The fault `frame_symmetric_pad`: the window's padding to (S // 8 + 1) * 8 is cut from the symmetric extension of the whole
    frame, so it holds the frame's pixels beyond the window where there are any."""
    s = R.config(**cfg)["upscale"]
    mh, mw = R.padded_size(sy), R.padded_size(sx)
    a = np.asarray(frame).astype(np.float64) / 255.0
    a = np.pad(a, ((0, mh), (0, mw), (0, 0)), mode="symmetric")[wy:wy + mh, wx:wx + mw]
    x = torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).unsqueeze(0).to(dtype).contiguous()
    with torch.no_grad():
        y = R.swin2sr_forward(sd, x, **cfg)
    return y[0, :, :sy * s, :sx * s].permute(1, 2, 0).contiguous()


def tiled_float(sd, frame, T, P, dtype=torch.float64, fault=None, **cfg):
    """The tiled result before the clamp, [h s, w s, 3] in `dtype`: upscale_float on every window, cropped and pasted."""
    assert fault is None or fault in FAULTS, fault
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    s = R.config(**cfg)["upscale"]
    if fault == "untiled":
        return R.upscale_float(sd, frame, dtype, **cfg)
    _, (sy, sx), rows = plan(h, w, T, P, s)
    out = torch.zeros((h * s, w * s, 3), dtype=dtype)
    done = {}
    for wy, wx, cy, cx, ch, cw, oy, ox in rows:
        wh, ww = sy, sx
        if fault == "shrunk_windows":          # [c0 - P, c1 + P) cut at the frame's edge instead of slid inward
            y0, x0 = oy // s, ox // s
            wy, wx = max(y0 - P, 0), max(x0 - P, 0)
            wh, ww = min(y0 + ch // s + P, h) - wy, min(x0 + cw // s + P, w) - wx
            cy, cx = (y0 - wy) * s, (x0 - wx) * s
        key = (wy, wx, wh, ww)
        if key not in done:
            if fault == "frame_symmetric_pad":
                done[key] = _window_against_the_frame(sd, frame, wy, wx, wh, ww, dtype, **cfg)
            else:
                done[key] = R.upscale_float(sd, np.ascontiguousarray(frame[wy:wy + wh, wx:wx + ww]), dtype, **cfg)
        y = done[key]
        if fault == "crop_without_w0":         # the core's offset in the frame used inside the window (wrapped where it leaves it)
            cy, cx = oy, ox
        elif fault == "crop_off_by_row":       # one output row too low, where the window has one
            cy = min(cy + 1, wh * s - ch)
        ry = (torch.arange(ch) + cy) % (wh * s)
        rx = (torch.arange(cw) + cx) % (ww * s)
        out[oy:oy + ch, ox:ox + cw] = y[ry][:, rx]
    return out


@functools.lru_cache(maxsize=None)
def tiled_reference(name):
    """(frame uint8 ndarray, float64 composition [h s, w s, 3], float32 composition, tol = 8 x max |f32 - f64|) of a TILED_CASES
    row, computed once."""
    _, (h, w), T, P, _ = tiled_case(name)
    case = C.by_name(name)
    frame = R.seeded_frame(h, w, 50 + h)
    y64 = tiled_float(case.sd, frame, T, P, torch.float64, **case.cfg)
    y32 = tiled_float(case.sd, frame, T, P, torch.float32, **case.cfg)
    return frame, y64, y32, 8 * float((y32.double() - y64).abs().max())
