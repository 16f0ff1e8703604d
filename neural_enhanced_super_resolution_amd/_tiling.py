"""Which tiles of a frame run together, in which order, on which stream: integer arithmetic, no torch.  A tile is ``(y0, y1, x0,
x1, payload)``, a window of the padded frame; a ``plan`` has one entry per stream, the batches (lists of tiles) it runs in order
on context slot ``slot_base + k`` (RealESRGANer._fan_out).  Also `Tile` and the fused 8-bit tile route's descriptors."""
from dataclasses import dataclass


@dataclass(frozen=True)
class Tile:
    index: int
    inp: tuple    # padded input window  (y0, y1, x0, x1) in frame coordinates
    out: tuple    # output window        (y0, y1, x0, x1) in output coordinates
    crop: tuple   # centre crop inside the tile's own output

    @property
    def area(self):
        return (self.inp[1] - self.inp[0]) * (self.inp[3] - self.inp[2])


def _area(t):
    return (t[1] - t[0]) * (t[3] - t[2])


def shape_group_plan(tiles, batch_for, tile_streams, small_job_tiles, small_job_streams, multi):
    """Batches of equal-shaped windows (`batch_for(th, tw, n)` per batch of a group of n), one shape group per stream; `multi`
    false (not the HIP backend, or one tile): one stream, the groups by descending h * w * count.
    A small job (a rank's share of a sharded frame: five tiles of an 8-way split 4K frame, often of one shape) is spread
    wider: every batch its own unit, the largest halved until each of `small_job_streams` streams has one -- one stream would
    run 351 launches of a few hundred workgroups each, five overlap their prologues, epilogues and tails (measured on one GPU
    with an 8-rank share: 25.6 -> 16.9 ms for the slowest rank).  A larger job of one shape stays on one stream."""
    groups = {}
    for t in tiles:
        groups.setdefault((t[1] - t[0], t[3] - t[2]), []).append(t)
    order = sorted(groups.items(), key=lambda kv: -kv[0][0] * kv[0][1] * len(kv[1]))
    units = []                                    # a unit = the batches of one shape group, run in order on one stream
    for shape, ts in order:
        nb = batch_for(shape[0], shape[1], len(ts))
        units.append([ts[i:i + nb] for i in range(0, len(ts), nb)])
    nstreams = 1
    if multi:
        nstreams = max(1, int(tile_streams))
        if len(tiles) <= small_job_tiles:
            nstreams = min(max(nstreams, int(small_job_streams)), len(tiles))
            units = [[b] for u in units for b in u]
            while len(units) < nstreams:
                k = max(range(len(units)), key=lambda i: len(units[i][0]))
                b = units[k][0]
                if len(b) < 2:
                    break
                units[k:k + 1] = [[b[:(len(b) + 1) // 2]], [b[(len(b) + 1) // 2:]]]
        elif len(units) == 1:
            nstreams = 1

    sized = sorted(((sum(_area(b[0]) * len(b) for b in u), u) for u in units), key=lambda su: -su[0])
    plan, load = [[] for _ in range(nstreams)], [0] * nstreams
    for size, u in sized:                         # largest unit first, each to the least-loaded stream
        k = load.index(min(load))
        load[k] += size
        plan[k].extend(u)
    return plan


def ragged_plan(tiles, nstreams, cap):
    """Batches of at most `cap` tiles of any shapes: largest first (stable), each to the least-loaded stream (first on ties)."""
    plan, load = [[] for _ in range(nstreams)], [0] * nstreams
    for t in sorted(tiles, key=lambda t: -_area(t)):
        k = load.index(min(load))
        load[k] += _area(t)
        if not plan[k] or len(plan[k][-1]) == cap:
            plan[k].append([])
        plan[k][-1].append(t)
    return plan


def windows(tiles, row0=0):
    """[(y0, x0, h, w)] of the padded tiles in a frame (or a band of it that starts at frame row `row0`)."""
    return [(t.inp[0] - row0, t.inp[2], t.inp[1] - t.inp[0], t.inp[3] - t.inp[2]) for t in tiles]


def canvas_pastes(tiles, out_w):
    """[(crop_y, crop_x, h, w, dst byte offset, dst row pitch)]: every tile's centre at its place in a uint8 HWC canvas `out_w` wide."""
    return [(t.crop[0], t.crop[2], t.crop[1] - t.crop[0], t.crop[3] - t.crop[2], (t.out[0] * out_w + t.out[2]) * 3, out_w * 3) for t in tiles]


def packed_pastes(tiles):
    """(pastes, offs): every tile's centre as a dense block of a packed uint8 buffer, tile i at bytes [offs[i], offs[i + 1])."""
    offs = [0]
    for t in tiles:
        offs.append(offs[-1] + (t.out[1] - t.out[0]) * (t.out[3] - t.out[2]) * 3)
    return [(t.crop[0], t.crop[2], t.crop[1] - t.crop[0], t.crop[3] - t.crop[2], offs[i], (t.out[3] - t.out[2]) * 3)
            for i, t in enumerate(tiles)], offs


def slid_window_axis(n, tile, tile_pad):
    """One axis of Swin2SR's tile plan: (S, [(w0, c0, c1)]).  Cores [c0, c1) of `tile` partition [0, n); every window is
    S = min(tile + 2 tile_pad, n) long and starts at w0 = clamp(c0 - tile_pad, 0, n - S): a window at the edge slides inward instead
    of shrinking, so the windows of an axis have one length."""
    if n < 1 or tile < 1 or tile_pad < 0:
        raise ValueError(f"slid_window_axis: n >= 1, tile >= 1, tile_pad >= 0, got {n}, {tile}, {tile_pad}")
    side = min(tile + 2 * tile_pad, n)
    return side, [(min(max(c0 - tile_pad, 0), n - side), c0, min(c0 + tile, n)) for c0 in range(0, n, tile)]


def overlap_axis(n, t, overlap):
    """The starts of one padded axis of Swin2SR's overlapped plan and of the x4 diffusion stage's window plan: 0, t - overlap, ...
    below n - t, then n - t (the last tile ends at n and is in general not on the stride)."""
    if not (1 <= t <= n and 0 <= overlap < t):
        raise ValueError(f"overlap_axis: 1 <= t <= n and 0 <= overlap < t, got n = {n}, t = {t}, overlap = {overlap}")
    return list(range(0, n - t, t - overlap)) + [n - t]


def blend_axis_weight(i, a, t, n, ramp):
    """The weight window [a, a + t) of an axis of n gives pixel i under the x4 diffusion stage's blend (nesr_sdx4_tile_plan): a ramp
    of `ramp` pixels on every side that is not on the frame's edge.  A fraction's numerator and denominator: (k, ramp) or (1, 1)."""
    left = min(i - a + 1, ramp) if a > 0 and ramp > 0 else ramp or 1
    right = min(a + t - i, ramp) if a + t < n and ramp > 0 else ramp or 1
    return min(left, right), ramp or 1


def sdx4_tile_plan(h, w, multiple, tile, tile_overlap, max_window=1 << 16):
    """The x4 diffusion stage's window plan of an h x w low-res frame, what nesr_sdx4_tile_plan computes: ((tiles_y, tiles_x), (ty,
    tx), [(y, x)] in row-major order).  h, w, tile and tile_overlap are multiples of `multiple` (the UNet's frame multiple, even);
    ty = min(tile, h), tx = min(tile, w); 0 <= tile_overlap < min(ty, tx); a window holds at most `max_window` pixels."""
    if multiple < 2 or multiple % 2 or h < 1 or w < 1 or h % multiple or w % multiple:
        raise ValueError(f"sdx4_tile_plan: h and w must be positive multiples of an even frame multiple, got {h} x {w}, multiple {multiple}")
    if tile < 1 or tile % multiple:
        raise ValueError(f"sdx4_tile_plan: tile must be a positive multiple of {multiple}, got {tile}")
    ty, tx = min(tile, h), min(tile, w)
    if not 0 <= tile_overlap < min(ty, tx) or tile_overlap % multiple:
        raise ValueError(f"sdx4_tile_plan: tile_overlap must be a multiple of {multiple} in 0 .. {min(ty, tx) - 1}, got {tile_overlap}")
    if ty * tx > max_window:
        raise ValueError(f"sdx4_tile_plan: a window of {ty} x {tx} exceeds {max_window} pixels")
    ys, xs = overlap_axis(h, ty, tile_overlap), overlap_axis(w, tx, tile_overlap)
    return (len(ys), len(xs)), (ty, tx), [(y, x) for y in ys for x in xs]


def overlap_plan(h, w, tile, tile_overlap, window_size, scale):
    """Swin2SR's overlapped plan of an h x w frame, what nesr_swin2sr_overlap_plan computes: ((tiles_y, tiles_x), t, (hp, wp), rows).
    The frame is padded once to hp x wp, multiples of the window; t = min(tile, hp, wp) must be a multiple of the window and
    0 <= tile_overlap < t; one row (win_y, win_x, out_y, out_x) per t x t window in row-major order, the origin in input pixels of
    the padded frame and in output pixels."""
    if h < 1 or w < 1 or tile < 1 or window_size < 1:
        raise ValueError(f"overlap_plan: h, w, tile and window_size must be positive, got {h}, {w}, {tile}, {window_size}")
    hp, wp = -(-h // window_size) * window_size, -(-w // window_size) * window_size
    t = min(tile, hp, wp)
    if t % window_size:
        raise ValueError(f"overlap_plan: the effective tile {t} must be a multiple of window_size {window_size}")
    if not 0 <= tile_overlap < t:
        raise ValueError(f"overlap_plan: tile_overlap must be 0 .. {t - 1}, got {tile_overlap}")
    ys, xs = overlap_axis(hp, t, tile_overlap), overlap_axis(wp, t, tile_overlap)
    return (len(ys), len(xs)), t, (hp, wp), [(y, x, y * scale, x * scale) for y in ys for x in xs]


def slid_window_plan(h, w, tile, tile_pad, scale):
    """Swin2SR's tile plan of an h x w frame, what nesr_swin2sr_tile_plan computes: ((tiles_y, tiles_x), (win_h, win_w), rows), one
    row (win_y, win_x, crop_y, crop_x, crop_h, crop_w, out_y, out_x) per tile in row-major order; the window's origin in input
    pixels, the core inside the window's output and its place in the result in output pixels."""
    sy, ys = slid_window_axis(h, tile, tile_pad)
    sx, xs = slid_window_axis(w, tile, tile_pad)
    rows = [(wy, wx, (y0 - wy) * scale, (x0 - wx) * scale, (y1 - y0) * scale, (x1 - x0) * scale, y0 * scale, x0 * scale)
            for wy, y0, y1 in ys for wx, x0, x1 in xs]
    return (len(ys), len(xs)), (sy, sx), rows
