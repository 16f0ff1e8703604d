"""The strip kernel's packing seen from the host (helpers of test_strip_schedule_host.py, test_gpu_strip_queue.py and
test_gpu_strip.py; no tests here): nesr_strip_schedule's arrays as a Plan, the properties every plan must have (`check`), an
independent walk of the workgroups' lists (`walk`), and the geometries the tests share.

A plan is a list of items per workgroup.  An item is (image, mailbox group, strip, h, w, pos0, pos1, row_lo, row_hi): strip
`strip` (16 columns) of image `image`, swept over positions pos0 .. pos1 - 1 of the image's own grid of 12-row positions,
storing rows row_lo .. row_hi - 1.  The strips of one row segment of an image form a UNIT (one mailbox group): they exchange
edge columns position by position, so they run in lockstep on as many workgroups."""
import ctypes
import types
from dataclasses import dataclass, replace

BH, BW = 12, 16          # rows of a position, columns of a strip (nesr_kernels.h: STRIP_BH, STRIP_BW)
TAG_POSITIONS = 256      # positions the tags of one launch tell apart: epoch step 2048 / 8 (tag = epoch + position * 8 + layer)


def npos_of(h):
    return (h + 4 + BH - 1) // BH


def nstrips_of(w):
    return (w + BW - 1) // BW


@dataclass(frozen=True)
class Plan:
    lists: tuple          # per workgroup: tuple of items (9-tuples, see the module's docstring)
    makespan: int
    grid: int
    smax: int
    nvimg: int
    applies: bool
    max_wait: int
    walk_makespan: int
    largest_pos1: int
    pos1_bound: int
    efficiency: float
    raw: tuple            # (items, wg_first) as the entry wrote them

    @property
    def items(self):
        return [it for lst in self.lists for it in lst]

    def most_items_per_workgroup(self):
        return max((len(lst) for lst in self.lists), default=0)

    def segments(self):
        """Units per image: {image: count}."""
        seen = {}
        for it in self.items:
            seen.setdefault(it[0], set()).add(it[1])
        return {k: len(v) for k, v in seen.items()}


def schedule(hw, cus, seg=0):
    """nesr_strip_schedule for images of hw[i] = (h, w) trunk pixels -> Plan.  The arrays are sized by a first call."""
    from neural_enhanced_super_resolution_amd import _lib
    lib = _lib.load()
    n = len(hw)
    flat = (ctypes.c_int * (2 * n))(*[int(v) for pair in hw for v in pair])
    info = (ctypes.c_int * 10)()
    eff = ctypes.c_double()
    rc = lib.nesr_strip_schedule(n, flat, cus, seg, None, 0, None, 0, info, ctypes.byref(eff))
    count, nfirst = info[4], (info[1] + 1 if info[4] else 0)
    assert rc == (0 if count == 0 else _lib.ERR_ARG), rc
    items = (ctypes.c_int * max(8 * count, 1))()
    first = (ctypes.c_int * max(nfirst, 1))()
    if count:
        _lib.check(lib.nesr_strip_schedule(n, flat, cus, seg, items, count, first, nfirst, info, ctypes.byref(eff)), "nesr_strip_schedule")
    raw_items, raw_first = tuple(items[:8 * count]), tuple(first[:nfirst])
    lists = []
    for g in range(max(nfirst - 1, 0)):
        lst = []
        for k in range(raw_first[g], raw_first[g + 1]):
            x, s, h, w, p0, p1, lo, hi = raw_items[8 * k:8 * k + 8]
            lst.append((x & 0xffff, (x >> 16) & 0xffff, s, h, w, p0, p1, lo, hi))
        lists.append(tuple(lst))
    return Plan(lists=tuple(lists), makespan=info[0], grid=info[1], smax=info[2], nvimg=info[3], applies=bool(info[5]), max_wait=info[6],
                walk_makespan=info[7], largest_pos1=info[8], pos1_bound=info[9], efficiency=eff.value, raw=(raw_items, raw_first))


def walk(lists):
    """Runs the lists as the workgroups do: a unit starts when every workgroup that holds one of its strips has it at the head
    of its list (until then those that arrived early idle), and takes pos1 - pos0 positions.  -> (makespan, largest idle time of a
    workgroup in front of an item, the units in starting order); AssertionError if items are left that can never start (a cycle
    of waits: no global order of the units that every list respects)."""
    head, t = [0] * len(lists), [0] * len(lists)
    left = sum(len(lst) for lst in lists)
    wait, order = 0, []
    while left:
        heads = {}
        for g, lst in enumerate(lists):
            if head[g] < len(lst):
                heads.setdefault(lst[head[g]][1], []).append(g)
        started = False
        for v, wgs in sorted(heads.items()):
            ns = nstrips_of(lists[wgs[0]][head[wgs[0]]][4])
            if len(wgs) < ns:
                continue
            start = max(t[g] for g in wgs)
            for g in wgs:
                it = lists[g][head[g]]
                wait = max(wait, start - t[g])
                t[g] = start + it[6] - it[5]
                head[g] += 1
                left -= 1
            order.append(v)
            started = True
        assert started, f"cycle: {left} items can never start (heads: {sorted(heads)})"
    return max(t, default=0), wait, order


def check(plan, hw, cus):
    """Every property of a plan that applies (the numbers are the issue's): AssertionError names the one that fails."""
    lists = plan.lists
    items = [it for lst in lists for it in lst]
    # 5. limits
    assert plan.grid <= cus, f"5: grid {plan.grid} > {cus} workgroups"
    assert plan.grid == len(lists) and all(lists), "5: grid + 1 == len(wg_first), no empty list"
    assert all(it[0] < 65536 and it[1] < 32768 for it in items) and len(hw) <= 65536 and plan.nvimg <= 32768, "5: image / mailbox group fields"
    units = {}
    for g, lst in enumerate(lists):
        for it in lst:
            units.setdefault(it[1], []).append((g, it))
    for v, members in units.items():
        img, _, _, h, w, p0, p1, lo, hi = members[0][1]
        ns, npos = nstrips_of(w), npos_of(h)
        # 1. the item's h, w are the image's
        assert img < len(hw) and (h, w) == tuple(hw[img]), f"1: unit {v} carries {h} x {w} for image {img}"
        # 3. a unit is one row segment of one image: ns strips, each once, on ns distinct workgroups
        assert all(m[1][0] == img and m[1][3:] == members[0][1][3:] for m in members), f"3: mailbox group {v} is used by two units"
        assert sorted(m[1][2] for m in members) == list(range(ns)), f"3: unit {v} of image {img}: strips {sorted(m[1][2] for m in members)} of {ns}"
        assert len({m[0] for m in members}) == ns, f"3: unit {v}: two strips on one workgroup"
        # 2. segments: the one from position a on starts one position early and stores rows from 12 a - 4
        assert 0 <= p0 < p1 <= npos, f"2: unit {v}: positions {p0} .. {p1} of {npos}"
        if lo == 0:
            assert p0 == 0, f"2: unit {v}: first segment starts at position {p0}"
        else:
            assert (lo + 4) % BH == 0 and p0 == (lo + 4) // BH - 1, f"2: unit {v}: rows from {lo} with a first position of {p0}"
        assert hi == (h if p1 == npos else BH * p1 - 4), f"2: unit {v}: rows to {hi} with an end position of {p1} (image of {h} rows)"
        # 5. mailboxes: vimg * smax + s, and the neighbours' at + 1 / - 1 for a strip that has one, inside nvimg * smax
        assert ns <= plan.smax and 0 <= v * plan.smax and v * plan.smax + ns - 1 < plan.nvimg * plan.smax, f"5: mailboxes of unit {v}"
    # 1. row coverage: per (image, strip) the segments partition [0, h)
    for i, (h, w) in enumerate(hw):
        for s in range(nstrips_of(w)):
            rows = sorted((it[7], it[8]) for it in items if it[0] == i and it[2] == s)
            assert rows, f"1: strip {s} of image {i} is missing"
            assert rows[0][0] == 0 and rows[-1][1] == h and all(a[1] == b[0] for a, b in zip(rows, rows[1:])) and all(a < b for a, b in rows), \
                f"1: strip {s} of image {i}: rows {rows} do not partition [0, {h})"
    # 4. no cycle, and the walk's makespan is the reported one
    mk, wait, _ = walk(lists)
    assert mk == plan.makespan, f"4: the walk takes {mk} positions, reported {plan.makespan}"
    assert plan.walk_makespan == mk and plan.max_wait == wait, f"4: the entry's walk ({plan.walk_makespan}, {plan.max_wait}) against ({mk}, {wait})"
    # 6. efficiency
    work = sum(nstrips_of(w) * npos_of(h) for h, w in hw)
    assert plan.efficiency == work / (cus * plan.makespan), f"6: efficiency {plan.efficiency} for {work} / ({cus} * {plan.makespan})"
    # 8. the entry's numbers about the tag space
    assert plan.largest_pos1 == max(it[6] for it in items) == max(npos_of(h) for h, _ in hw), "8: largest end position"
    return mk, wait


def expect_applies(hw, cus):
    """What applicability must be, from the images alone: none wider than the workgroups, none with more positions than the
    tags of a launch tell apart."""
    return all(nstrips_of(w) <= cus and npos_of(h) <= TAG_POSITIONS for h, w in hw)


def with_lists(plan, lists):
    return replace(plan, lists=tuple(tuple(lst) for lst in lists))


# ------------------------------------------------------------------------------------------------------------ geometries
def _tile_windows(height, width, unshuffle, tile, tile_pad):
    from neural_enhanced_super_resolution_amd.realesrganer import RealESRGANer
    grid = RealESRGANer.tile_grid(types.SimpleNamespace(tile_size=tile, tile_pad=tile_pad, scale=4 // unshuffle), height, width)
    return [(w[0], w[1], w[2], w[3], None) for w, _, _ in grid]


def tile_batches(height, width, unshuffle, tile=512, tile_pad=10, cap=64):
    """The ragged batches of a height x width frame as the tiling wrapper cuts and orders them (RealESRGANer.tile_grid,
    _tiling.ragged_plan on one stream), as trunk sizes: input pixels / unshuffle."""
    from neural_enhanced_super_resolution_amd import _tiling
    tiles = _tile_windows(height, width, unshuffle, tile, tile_pad)
    return [[((t[1] - t[0]) // unshuffle, (t[3] - t[2]) // unshuffle) for t in batch] for batch in _tiling.ragged_plan(tiles, 1, cap)[0]]


def tile_batches_u8(height, width, unshuffle, tile=512, tile_pad=10, cap=64):
    """The same for an 8-bit frame (RealESRGANer.tiles_u8_on_device): runs of `cap` tiles in the grid's own order."""
    sizes = [((t[1] - t[0]) // unshuffle, (t[3] - t[2]) // unshuffle) for t in _tile_windows(height, width, unshuffle, tile, tile_pad)]
    return [sizes[k:k + cap] for k in range(0, len(sizes), cap)]


def crowd():
    """12 small ragged images (trunk sizes)."""
    return [(13 + (i % 5) * 11, 9 + (i % 4) * 13) for i in range(12)]


def long_queue():
    """64 images whose packing for 4 workgroups is longer than 256 positions (trunk sizes)."""
    return [(40 + (i % 5) * 24, 16 + (i % 4) * 16) for i in range(64)]


SUITE_64 = [(3 + (7 * i) % 40, 5 + (11 * i) % 90) for i in range(64)]          # test_gpu_strip.py::test_strip_full_ragged_batch_of_64
RAGGED_SIX = [(132, 200), (40, 64), (132, 36), (2, 2), (66, 200), (130, 198)]   # test_gpu_ragged.py (x4: trunk = input)
SHAPES_X4 = [(1, 1), (5, 15), (11, 16), (12, 17), (13, 33), (23, 47), (24, 48), (25, 49), (100, 9), (9, 100)]
