"""CPU: the host side of the NESR stage's C entries (include/nesr_hip.h, csrc/nesr_stage_api.cpp) -- they are exported, declared and
bound; nesr_stage_tile_plan is nesr_adapter.tile_plan and nesr_stage_route is nesr_adapter.apply_esrgan's dispatch, integer for
integer; tile_plan is the loop process_with_tiling had before it (restated here); the refusals that need no device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nesr_forward_nesr_u8", "nesr_stage_route", "nesr_stage_tile_plan", "nesr_apply_esrgan_scratch_bytes", "nesr_apply_esrgan_u8")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


def test_entries_are_exported_declared_and_bound(lib):
    from neural_enhanced_super_resolution_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nesr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nesr_[a-z0-9_]+)\s*\(", text))
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/nesr_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} is not exported by libnesr_hip.so"
    assert (_lib.INPUT_12CH, _lib.INPUT_3CH_X4) == (0, 1) and re.search(r"NESR_INPUT_12CH = 0, NESR_INPUT_3CH_X4 = 1", text)


def c_plan(lib, h, w, tile, padding, uf, net_scale):
    n = ctypes.c_int(-1)
    assert lib.nesr_stage_tile_plan(h, w, tile, padding, uf, net_scale, None, 0, ctypes.byref(n)) == 0      # the count alone
    buf = (ctypes.c_int * (13 * n.value))()
    m = ctypes.c_int(-1)
    assert lib.nesr_stage_tile_plan(h, w, tile, padding, uf, net_scale, buf, n.value, ctypes.byref(m)) == 0 and m.value == n.value
    return [tuple(buf[13 * i:13 * i + 13]) for i in range(n.value)]


def test_tile_plan_sweep(lib):
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    sizes = (17, 24, 25, 40, 56, 100)
    cases = one_tile = lanczos = plain = 0
    for h in sizes:
        for w in sizes:
            for tile in (16, 24):
                for padding in (0, 4, 16):
                    for uf in (1.5, 2.0, 3.0, 4.0):
                        want = A.tile_plan(h, w, tile, padding, uf, 4)
                        assert c_plan(lib, h, w, tile, padding, uf, 4) == want, (h, w, tile, padding, uf)
                        cases += 1
                        one_tile += h <= tile and w <= tile
                        assert len(want) == (1 if h <= tile and w <= tile else math.ceil(h / tile) * math.ceil(w / tile))
                        for r in want:
                            same = (r[5] - r[4], r[7] - r[6]) == (r[9] - r[8], r[11] - r[10])
                            plain, lanczos = plain + same, lanczos + (not same)
    assert cases == 864 and one_tile > 0 and lanczos > 0 and plain > 0      # the sweep reaches every branch of the paste


def test_tile_plan_one_pixel_crop_and_skipped_rectangle(lib):
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    # A crop of one pixel.  The reference's clamps (at least one pixel, nesr.py:421-426) never bind for a processor of integer scale s:
    # between the sides it crops, a window keeps s x tile pixels or more.  One pixel is therefore reached with tile 1 and scale 1.
    want = A.tile_plan(5, 4, 1, 2, 1.0, 1)
    assert c_plan(lib, 5, 4, 1, 2, 1.0, 1) == want and len(want) == 20
    assert want[0] == (0, 3, 0, 3, 0, 1, 0, 1, 0, 1, 0, 1, 0) and want[19] == (2, 5, 1, 4, 2, 3, 2, 3, 4, 5, 3, 4, 0)
    assert min(r[5] - r[4] for r in want) == 1 and min(r[7] - r[6] for r in want) == 1
    assert c_plan(lib, 5, 4, 1, 2, 1.0, 4) == A.tile_plan(5, 4, 1, 2, 1.0, 4)
    # a skipped rectangle: a canvas of 0 x 1 rows for the first tile row
    want = A.tile_plan(40, 56, 16, 4, 0.02, 4)
    assert c_plan(lib, 40, 56, 16, 4, 0.02, 4) == want
    assert [r[12] for r in want] == [1] * 12 and A.tile_plan(40, 56, 16, 4, 0.05, 4)[0][12] == 0
    want = A.tile_plan(40, 56, 16, 4, 0.05, 4)
    assert c_plan(lib, 40, 56, 16, 4, 0.05, 4) == want and sorted(set(r[12] for r in want)) == [0, 1]


def loop_of_process_with_tiling(h, w, tile_size, padding, upscale_factor, scale):
    """process_with_tiling's loop as it stood before tile_plan existed, for a processor whose output is `scale` times its input."""
    rows = []
    nth, ntw = math.ceil(h / tile_size), math.ceil(w / tile_size)
    for i in range(nth):
        for j in range(ntw):
            y0, y1 = max(0, i * tile_size - padding), min(h, (i + 1) * tile_size + padding)
            x0, x1 = max(0, j * tile_size - padding), min(w, (j + 1) * tile_size + padding)
            tile_shape = (y1 - y0, x1 - x0)
            oy0, oy1 = int(y0 * upscale_factor), int(y1 * upscale_factor)
            ox0, ox1 = int(x0 * upscale_factor), int(x1 * upscale_factor)
            if padding > 0:
                pu = int(padding * upscale_factor)
                if y0 > 0:
                    oy0 += pu
                if y1 < h:
                    oy1 -= pu
                if x0 > 0:
                    ox0 += pu
                if x1 < w:
                    ox1 -= pu
            th, tw = scale * tile_shape[0], scale * tile_shape[1]
            sy, sx = th / tile_shape[0], tw / tile_shape[1]
            ty0 = 0 if y0 == 0 else int(padding * sy)
            ty1 = th if y1 == h else int(th - padding * sy)
            tx0 = 0 if x0 == 0 else int(padding * sx)
            tx1 = tw if x1 == w else int(tw - padding * sx)
            ty0 = max(0, min(ty0, th - 1))
            ty1 = max(ty0 + 1, min(ty1, th))
            tx0 = max(0, min(tx0, tw - 1))
            tx1 = max(tx0 + 1, min(tx1, tw))
            oh, ow = oy1 - oy0, ox1 - ox0
            rows.append((y0, y1, x0, x1, ty0, ty1, tx0, tx1, oy0, oy1, ox0, ox1, int(oh <= 0 or ow <= 0)))
    return rows


@pytest.mark.parametrize("h,w,tile,padding,uf", [(40, 52, 24, 4, 2.0), (48, 72, 32, 16, 2.0), (64, 64, 32, 16, 2.0), (80, 96, 48, 16, 2.0),
                                                 (160, 192, 48, 16, 2.0), (37, 53, 16, 3, 1.7)])
def test_tile_plan_is_the_loop_of_process_with_tiling(lib, h, w, tile, padding, uf):
    """The frames tests/test_nesr_adapter.py tiles (and one with nothing round in it)."""
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    want = loop_of_process_with_tiling(h, w, tile, padding, uf, 4)
    assert A.tile_plan(h, w, tile, padding, uf, 4) == want
    assert c_plan(lib, h, w, tile, padding, uf, 4) == want


def test_process_with_tiling_pastes_what_the_plan_says():
    """process_with_tiling through tile_plan's arithmetic: a processor that paints each call's output with the call's number."""
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    calls = []

    def processor(t):
        calls.append(tuple(t.shape[:2]))
        return torch.full((4 * t.shape[0], 4 * t.shape[1], 3), len(calls), dtype=torch.uint8)

    img = torch.zeros((40, 56, 3), dtype=torch.uint8)
    got = A.process_with_tiling(processor, img, 24, 16, 4.0, "cpu")
    plan = A.tile_plan(40, 56, 24, 16, 4.0, 4)
    assert calls == [(r[1] - r[0], r[3] - r[2]) for r in plan] and len(plan) == 6
    want = np.zeros((160, 224, 3), np.uint8)
    for k, r in enumerate(plan):
        assert (r[5] - r[4], r[7] - r[6]) == (r[9] - r[8], r[11] - r[10])      # upscale factor = the network's: plain pastes
        want[r[8]:r[9], r[10]:r[11]] = k + 1
    assert np.array_equal(got, want) and (got > 0).all()


def test_route_is_the_dispatch_of_apply_esrgan(lib):
    from neural_enhanced_super_resolution_amd import nesr_adapter as A

    class Net(torch.nn.Module):
        def forward(self, x):
            return torch.zeros(1, 3, x.shape[2] * 4, x.shape[3] * 4)

    class Up:
        model, device = Net(), torch.device("cpu")

    def c_route(h, w, tiling, force3, thr, large):
        tiled, mode = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.nesr_stage_route(h, w, tiling, force3, thr, large, ctypes.byref(tiled), ctypes.byref(mode)) == 0
        return bool(tiled.value), bool(mode.value)

    px = 32 * 32 / (1024 * 1024)              # the frame's "megapixels", exactly representable
    below, above = math.nextafter(px, 0.0), math.nextafter(px, 1.0)
    img = np.zeros((32, 32, 3), np.uint8)
    seen = set()
    for tiling in (True, False):
        for force3 in (False, True):
            for thr in (below, px, above):
                for large in (below, px, above):
                    trace = []
                    A.apply_esrgan(Up, img, {"enable_tiling": tiling, "force_3channel": force3, "cuda_megapixel_threshold": thr, "max_tile_size": 16},
                                   trace=trace, large_mp=large)
                    want = (trace[0]["tiled"], trace[0]["three_channel"])
                    assert c_route(32, 32, int(tiling), int(force3), thr, large) == want == A.stage_route(
                        32, 32, {"enable_tiling": tiling, "force_3channel": force3, "cuda_megapixel_threshold": thr}, "cuda", large)
                    assert want == ((tiling and px > thr) or px > large, force3 or px > large)
                    seen.add(want)
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    # the reference's literals: 8 "megapixels" for cuda, 16 for the forced branch (nesr.py:762-790)
    assert c_route(2896, 2896, 1, 0, 8.0, 16.0) == (False, False) and c_route(2897, 2897, 1, 0, 8.0, 16.0) == (True, False)
    assert c_route(4096, 4096, 1, 0, 8.0, 16.0) == (True, False) and c_route(4096, 4097, 0, 0, 8.0, 16.0) == (True, True)


def test_refusals_that_need_no_device(lib):
    fake = [ctypes.c_void_p(0x1000 * i) for i in (1, 2, 3)]      # never dereferenced
    n, a, b = ctypes.c_int(-7), ctypes.c_int(), ctypes.c_int()

    def refused(rc, text):
        assert rc == -1 and text in lib.nesr_last_error().decode(), (rc, lib.nesr_last_error().decode())

    refused(lib.nesr_forward_nesr_u8(None, fake[0], 36, 8, 12, 0, fake[1], 144, None), "null argument")
    refused(lib.nesr_apply_esrgan_u8(None, fake[0], 8, 12, 0, 1, 4, 16, 2.0, fake[1], 1 << 20, fake[2], None), "null argument")
    assert lib.nesr_apply_esrgan_scratch_bytes(None, 8, 12, 1, 4, 16) == 0 and b"null argument" in lib.nesr_last_error()
    refused(lib.nesr_stage_route(8, 12, 1, 0, 8.0, 16.0, None, ctypes.byref(b)), "null argument")
    refused(lib.nesr_stage_route(0, 12, 1, 0, 8.0, 16.0, ctypes.byref(a), ctypes.byref(b)), "sizes")
    refused(lib.nesr_stage_tile_plan(8, 12, 4, 16, 2.0, 4, None, 0, None), "null argument")
    for bad in ((0, 12, 4, 16, 2.0, 4), (8, 12, 0, 16, 2.0, 4), (8, 12, 4, -1, 2.0, 4), (8, 12, 4, 16, 0.0, 4), (8, 12, 4, 16, float("nan"), 4), (8, 12, 4, 16, 2.0, 0)):
        refused(lib.nesr_stage_tile_plan(*bad, None, 0, ctypes.byref(n)), "nesr_stage_tile_plan")
    assert n.value == -7
    # too small a table: the count is returned, nothing is written
    buf = (ctypes.c_int * 13)(*([-1] * 13))
    assert lib.nesr_stage_tile_plan(40, 56, 24, 16, 2.0, 4, buf, 1, ctypes.byref(n)) == 0 and n.value == 6 and list(buf) == [-1] * 13
