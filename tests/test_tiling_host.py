"""_tiling.py without a GPU: which tiles run together, in which order, on which stream, and the window / paste descriptors of the
fused 8-bit tile route.  Every expected value is a literal worked out from the rules (and, for the 4K grid, recorded from
run_tiles before the planning was split from the execution), never computed by the functions under test."""
from neural_enhanced_super_resolution_amd import RealESRGANer, _tiling
from neural_enhanced_super_resolution_amd.sharded import Tile


def _t(h, w, name):
    return (0, h, 0, w, name)


def test_ragged_plan_least_loaded_and_cap():
    t16, t8a, t8b, t4 = _t(4, 4, "16"), _t(2, 4, "8a"), _t(4, 2, "8b"), _t(2, 2, "4")
    # 16 -> stream 0; 8a -> stream 1; 8b -> stream 1 (8 < 16); 4 -> a tie at 16, the first stream
    assert _tiling.ragged_plan([t16, t8a, t8b, t4], 2, 64) == [[[t16, t4]], [[t8a, t8b]]]
    assert _tiling.ragged_plan([t16, t8a, t8b, t4], 1, 1) == [[[t16], [t8a], [t8b], [t4]]]
    assert _tiling.ragged_plan([t4, t8b, t16, t8a], 1, 3) == [[[t16, t8b, t8a], [t4]]]     # stable among equal areas


def test_small_job_is_halved_until_every_stream_has_a_batch():
    t = [_t(8, 8, i) for i in range(5)]
    # [5] -> [3, 2] -> [2, 1, 2] -> [1, 1, 1, 2] -> [1, 1, 1, 1, 1]: always the first of the largest batches
    plan = _tiling.shape_group_plan(t, lambda th, tw, n: 5, 3, 12, 5, True)
    assert plan == [[[t[0]]], [[t[1]]], [[t[2]]], [[t[3]]], [[t[4]]]]
    # three streams asked for, two tiles: no more streams than tiles
    assert _tiling.shape_group_plan(t[:2], lambda th, tw, n: 5, 3, 12, 5, True) == [[[t[0]]], [[t[1]]]]


def test_one_shape_group_stays_on_one_stream():
    t = [_t(8, 8, i) for i in range(13)]
    plan = _tiling.shape_group_plan(t, lambda th, tw, n: 4, 3, 12, 5, True)
    assert plan == [[t[0:4], t[4:8], t[8:12], t[12:13]]]


def test_not_multi_is_one_stream_in_group_order():
    a = [_t(4, 4, "a")]                                   # 16 * 1
    b = [_t(2, 2, f"b{i}") for i in range(5)]             # 4 * 5 = 20
    c = [_t(2, 4, "c")]                                   # 8 * 1
    plan = _tiling.shape_group_plan(a + c + b[:2] + b[2:], lambda th, tw, n: 2, 3, 12, 5, False)
    assert plan == [[b[0:2], b[2:4], b[4:5], a, c]]


def _grid_wrapper(tile, pad, scale):
    up = RealESRGANer.__new__(RealESRGANer)
    up.scale, up.tile_size, up.tile_pad = scale, tile, pad
    return up


def test_2160p_grid_over_three_streams():
    grid = _grid_wrapper(512, 10, 2).tile_grid(2160, 3840)
    tiles = [g[0] + (i,) for i, g in enumerate(grid)]
    assert len(tiles) == 40
    plan = _tiling.shape_group_plan(tiles, lambda th, tw, n: min(24, n), 3, 12, 5, True)
    got = [[((b[0][1] - b[0][0], b[0][3] - b[0][2]), [t[4] for t in b]) for b in lane] for lane in plan]
    # rows are 522, 532, 532, 532, 122 high and columns 522, 532 x 6, 266 wide: nine shape groups.  By descending h * w * count,
    # each to the then least-loaded stream: 5094432 -> 0; 1666224 -> 1; 833112, 424536, 389424, 272484 -> 2 (1919556);
    # 138852, 63684, 32452 -> 1 (1901212)
    assert got == [
        [((532, 532), [9, 10, 11, 12, 13, 14, 17, 18, 19, 20, 21, 22, 25, 26, 27, 28, 29, 30])],
        [((522, 532), [1, 2, 3, 4, 5, 6]), ((522, 266), [7]), ((122, 522), [32]), ((122, 266), [39])],
        [((532, 522), [8, 16, 24]), ((532, 266), [15, 23, 31]), ((122, 532), [33, 34, 35, 36, 37, 38]), ((522, 522), [0])],
    ]
    assert sorted(t[4] for lane in plan for b in lane for t in b) == list(range(40))
    # a cap below the largest group splits it into batches that stay together, in order
    plan = _tiling.shape_group_plan(tiles, lambda th, tw, n: min(8, n), 3, 12, 5, True)
    assert [[t[4] for t in b] for b in plan[0]] == [[9, 10, 11, 12, 13, 14, 17, 18], [19, 20, 21, 22, 25, 26, 27, 28], [29, 30]]


def test_descriptors_of_a_2x2_grid():
    # 12 x 14 frame, tile 8, pad 2, scale 2
    tiles = [Tile(0, (0, 10, 0, 10), (0, 16, 0, 16), (0, 16, 0, 16)), Tile(1, (0, 10, 6, 14), (0, 16, 16, 28), (0, 16, 4, 16)),
             Tile(2, (6, 12, 0, 10), (16, 24, 0, 16), (4, 12, 0, 16)), Tile(3, (6, 12, 6, 14), (16, 24, 16, 28), (4, 12, 4, 16))]
    assert [(t.inp, t.out, t.crop) for t in tiles] == _grid_wrapper(8, 2, 2).tile_grid(12, 14)
    assert _tiling.windows(tiles) == [(0, 0, 10, 10), (0, 6, 10, 8), (6, 0, 6, 10), (6, 6, 6, 8)]
    assert _tiling.windows(tiles[2:], row0=2) == [(4, 0, 6, 10), (4, 6, 6, 8)]           # a band that starts at frame row 2
    assert _tiling.canvas_pastes(tiles, 28) == [(0, 0, 16, 16, 0, 84), (0, 4, 16, 12, 48, 84),
                                                (4, 0, 8, 16, 1344, 84), (4, 4, 8, 12, 1392, 84)]
    assert _tiling.packed_pastes(tiles) == ([(0, 0, 16, 16, 0, 48), (0, 4, 16, 12, 768, 36), (4, 0, 8, 16, 1344, 48),
                                             (4, 4, 8, 12, 1728, 36)], [0, 768, 1344, 1728, 2016])
    assert _tiling.packed_pastes(tiles[1:3]) == ([(0, 4, 16, 12, 0, 36), (4, 0, 8, 16, 576, 48)], [0, 576, 960])
