"""RealESRGANer(devices=[...]): one wrapper spreading its tiles (enhance) or frames (enhance_many) over several device
contexts from one process.  Every case is compared BIT FOR BIT with devices=None on the same weights.  Repeated indices
([0, 0], [0, 0, 0], [0] * 8) run on one GPU; distinct devices are added where more than one is visible.

Sizes and the strip plan's limit (first item: a ragged batch whose strip schedule is too long falls back to the
per-layer kernels, which differ in bits): a lane's ragged batch is a subset of the one-device batch, so every size here
keeps the one-device batch inside the limit -- 2160p x2plus is one batch of 40 tiles of at most 532 x 532 (266 x 266
internal; test_gpu_f16 already pins it bitwise against single tiles), 1080p x4plus one batch of 12 such tiles at x4
(12 * 34 * 45 / 256 = 72 strip positions against the 383 of the 64-tile batch the advice names).  The 300 x 420 frames take
the generic route (f32 forms, equal-shape batches)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPEATED = [[0, 0], [0, 0, 0], [0] * 8]


def _lists(base):
    """`base` plus, where several GPUs are visible, the first k distinct devices (k = 2 and all of them, at most 8) and lists
    that repeat an index other than the first ([0, 1, 1], [0, 1, 0, 1]: several lanes read one copy of the frame there)."""
    n = min(torch.cuda.device_count(), 8)
    out = [list(b) for b in base]
    if n >= 2:
        out += [[0, 1], [0, 1, 1], [0, 1, 0, 1]] + ([list(range(n))] if n > 2 else [])
    return out


def _make(sd, model_fn, scale, devices=None, **kw):
    from neural_enhanced_super_resolution_amd import RealESRGANer
    args = dict(tile=512, tile_pad=10, pre_pad=0, half=False)
    args.update(kw)
    return RealESRGANer(scale=scale, model_path={"params_ema": sd}, model=model_fn(), device="cuda:0", devices=devices, **args)


def _record_calls(model):
    """Wraps the model's forward entries: every call appends (device index, slot, images in the call)."""
    calls = []
    for name in ("forward", "forward_ragged"):
        orig = getattr(model, name, None)
        if orig is None:
            continue

        def rec(x, *a, _orig=orig, **k):
            calls.append((x.device.index, k.get("slot", 0), x.shape[0]))
            return _orig(x, *a, **k)
        setattr(model, name, rec)
    return calls


def _lane_counts(up, frame, calls):
    """Each lane evaluated exactly its share, on exactly its own replicas: lane (device d, occurrence o) uses slot o on the
    fused 8-bit route and slots o * stride ... o * stride + stride - 1 on the generic route, and the images of its calls add
    up to its share of the tile grid (twice for BGRA: the alpha plane is a second pass)."""
    generic = hasattr(up, "img")                 # only the generic route keeps the padded image
    h, w = (up.img.shape[2], up.img.shape[3]) if generic else frame.shape[:2]
    _, shares = up.device_shares(h, w)
    stride = max(1, int(up.tile_streams), int(up.small_job_streams))
    passes = 2 if frame.ndim == 3 and frame.shape[2] == 4 else 1
    seen = {}
    for d, share in zip(up.devices, shares):
        o = seen.get(d, 0)
        seen[d] = o + 1
        slots = range(o * stride, (o + 1) * stride) if generic else range(o, o + 1)
        done = sum(n for dev, slot, n in calls if dev == d and slot in slots)
        assert done == passes * len(share), (up.devices, d, o, done, len(share))
    assert sum(n for _, _, n in calls) == passes * sum(len(sh) for sh in shares), "a tile ran outside its lane"


def _check_all(frame, sd, model_fn, scale, lists, **kw):
    ref = _make(sd, model_fn, scale, **kw)
    want, mode = ref.enhance(frame)
    for devices in lists:
        up = _make(sd, model_fn, scale, devices=devices, **kw)
        calls = _record_calls(up.model)
        got, gmode = up.enhance(frame)
        _lane_counts(up, frame, calls)
        assert gmode == mode and got.dtype == want.dtype and got.shape == want.shape
        diff = int(np.count_nonzero(got != want))
        assert diff == 0, f"devices={devices}: {diff} values differ from devices=None"
        again, _ = up.enhance(frame)                                 # a second frame on the same lanes and contexts
        assert np.array_equal(again, want), devices
        del up
    return want


@pytest.mark.parametrize("form", ["bf16", "f16"])
def test_2160p_x2plus_tile_parallel_is_bitwise(cuda_device, form):
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2)
    frame = synthetic_frame(2160, 3840, seed=0)
    dt = "f16" if form == "f16" else "f32"
    want = _check_all(frame, sd, lambda: RRDBNet(3, 3, scale=2, compute_dtype=dt), 2, _lists(REPEATED), half=True)
    assert want.shape == (4320, 7680, 3) and want.std() > 10


def test_1080p_x4plus_bf16_tile_parallel_is_bitwise(cuda_device):
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=1, num_in_ch=3, scale=4)
    frame = synthetic_frame(1080, 1920, seed=1)
    _check_all(frame, sd, lambda: RRDBNet(3, 3, scale=4), 4, _lists([[0, 0], [0, 0, 0]]), half=True)


def _small_frames():
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    bgr = synthetic_frame(300, 420, seed=3)
    bgra = synthetic_frame(300, 420, seed=4, channels=4)
    u16 = synthetic_frame(300, 420, seed=5).astype(np.uint16) * 250 + 3     # 3 .. 63753
    return bgr, bgra, u16


@pytest.mark.parametrize("case", ["u8", "u8_prepad", "bgra_prepad", "u16_prepad"])
def test_generic_route_f32_is_bitwise(cuda_device, case):
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=2, num_in_ch=3, scale=4, num_block=2)
    bgr, bgra, u16 = _small_frames()
    frame = {"u8": bgr, "u8_prepad": bgr, "bgra_prepad": bgra, "u16_prepad": u16}[case]
    pre = 0 if case == "u8" else 10
    want = _check_all(frame, sd, lambda: RRDBNet(3, 3, scale=4, num_block=2), 4, _lists([[0, 0], [0, 0, 0]]),
                      tile=128, tile_pad=10, pre_pad=pre)
    assert want.shape[:2] == (1200, 1680) and want.dtype == frame.dtype


def test_generic_route_x2plus_bf16_prepad_is_bitwise(cuda_device):
    """bf16 with pre_pad: the ragged batches of the generic route (run_tiles -> _run_tiles_ragged) on each lane's replicas."""
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=2, num_in_ch=3, scale=2, num_block=2)
    bgr, _, _ = _small_frames()
    _check_all(bgr, sd, lambda: RRDBNet(3, 3, scale=2, num_block=2), 2, _lists([[0, 0], [0] * 8]), tile=128, tile_pad=10,
               pre_pad=10, half=True)


def test_compact_animevideov3_is_bitwise(cuda_device):
    from neural_enhanced_super_resolution_amd import SRVGGNetCompact
    from neural_enhanced_super_resolution_amd.synth import synthetic_compact_state_dict
    sd = synthetic_compact_state_dict(seed=0, num_conv=16, upscale=4)
    bgr, _, _ = _small_frames()
    _check_all(bgr, sd, lambda: SRVGGNetCompact(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type="prelu"),
               4, _lists([[0, 0], [0, 0, 0]]), tile=128, tile_pad=10)


def test_enhance_many_over_devices_keeps_order(cuda_device):
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=2)
    frames = [synthetic_frame(192, 256, seed=10 + i) for i in range(5)]
    ref = _make(sd, lambda: RRDBNet(3, 3, scale=2, num_block=2), 2, tile=0, half=True)
    want = [ref.enhance(f)[0] for f in frames]
    assert all(not np.array_equal(want[0], w) for w in want[1:])
    for devices in _lists([[0, 0]]):
        up = _make(sd, lambda: RRDBNet(3, 3, scale=2, num_block=2), 2, devices=devices, tile=0, half=True)
        for inflight in (1, 2):
            got = up.enhance_many(frames, inflight=inflight)
            assert [m for _, m in got] == ["RGB"] * 5
            for i, (g, _) in enumerate(got):
                assert np.array_equal(g, want[i]), (devices, inflight, i)
        seen = {}
        for d in devices[:5]:                                        # every lane's first replica ran (inflight 2: slot occurrence * 2)
            o = seen.get(d, 0)
            seen[d] = o + 1
            assert up.model._handle(d, o * 2) is not None, (devices, d, o)
    # tiled frames go through enhance(), tile-parallel itself
    upt = _make(sd, lambda: RRDBNet(3, 3, scale=2, num_block=2), 2, devices=[0, 0], tile=128, tile_pad=10, half=True)
    reft = _make(sd, lambda: RRDBNet(3, 3, scale=2, num_block=2), 2, tile=128, tile_pad=10, half=True)
    for g, f in zip(upt.enhance_many(frames[:2], inflight=2), frames[:2]):
        assert np.array_equal(g[0], reft.enhance(f)[0])


def test_range_error_on_one_lane_then_clean(cuda_device):
    """An f16 model whose conv_first is scaled x3e5 (conv_last / 3e5): a bright input overflows f16, a black one does not.
    Only the bottom tile row is bright, so only the second lane's share overflows; the frame raises, the next one is clean."""
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd._lib import NesrRangeError
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=2)
    sd["conv_first.weight"] *= 3e5
    sd["conv_last.weight"] /= 3e5
    bad = synthetic_frame(256, 384, seed=7)
    bad[:140] = 0                     # rows the first tile row reads (tile 128 + pad 10) stay black
    clean = np.zeros_like(bad)
    clean[:100] = synthetic_frame(100, 384, seed=8) // 128  # dark content (values 0, 1) in the top rows
    mk = lambda: RRDBNet(3, 3, scale=2, num_block=2, compute_dtype="f16")   # noqa: E731
    ref = _make(sd, mk, 2, tile=128, tile_pad=10, half=True)
    want, _ = ref.enhance(clean)
    up = _make(sd, mk, 2, devices=[0, 0], tile=128, tile_pad=10, half=True)
    tiles, shares = up.device_shares(256, 384)
    assert all(tiles[i].inp[1] <= 140 for i in shares[0]) and all(tiles[i].inp[1] > 140 for i in shares[1])
    with pytest.raises(NesrRangeError):
        up.enhance(bad)
    got, _ = up.enhance(clean)
    assert np.array_equal(got, want)
    got, _ = up.enhance(clean)
    assert np.array_equal(got, want)


def test_bad_device_list_is_refused(cuda_device):
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=1)
    for bad in ([99], [], [0, torch.cuda.device_count()]):
        with pytest.raises(ValueError):
            _make(sd, lambda: RRDBNet(3, 3, scale=2, num_block=1), 2, devices=bad)


@pytest.mark.parametrize("route", ["shape_groups_f32", "ragged_bf16"])
def test_run_tiles_runs_the_plan(cuda_device, route):
    """run_tiles executes exactly _tiling's plan: the recorded (slot, images, input H, W) sequence is the plan's, stream by
    stream; every slot has a stream of its own; the bits are those of one stream and one tile per call.  64 x 96 at tile 32 /
    pad 10: six tiles of two shapes, a small job (five streams) for the shape groups, two ragged batches with tile_streams=2."""
    from neural_enhanced_super_resolution_amd import RRDBNet, _tiling
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=1)
    frame = synthetic_frame(64, 96, seed=9)
    ragged = route == "ragged_bf16"

    def make(**knobs):
        up = _make(sd, lambda: RRDBNet(3, 3, scale=2, num_block=1), 2, tile=32, tile_pad=10, half=ragged)
        for k, v in dict(knobs, **({"ragged_tiles": True} if ragged else {})).items():
            setattr(up, k, v)
        return up

    up = make(tile_streams=2) if ragged else make()
    calls = []
    for name in ("forward", "forward_ragged"):
        def rec(x, *a, _orig=getattr(up.model, name), **k):
            calls.append((k.get("slot", 0), x.shape[0], x.shape[2], x.shape[3], torch.cuda.current_stream(x.device).cuda_stream))
            return _orig(x, *a, **k)
        setattr(up.model, name, rec)
    got, _ = up.enhance(frame)

    tiles = [g[0] + (g[1:],) for g in up.tile_grid(64, 96)]
    assert len(tiles) == 6
    if ragged:
        plan = _tiling.ragged_plan(tiles, 2, up._ragged_cap())
    else:
        plan = _tiling.shape_group_plan(tiles, up.batch_for, up.tile_streams, up.small_job_tiles, up.small_job_streams, True)
    want = [(k, len(b), max(t[1] - t[0] for t in b), max(t[3] - t[2] for t in b)) for k, lane in enumerate(plan) for b in lane]
    assert len(plan) == (2 if ragged else 5)
    assert [c[:4] for c in calls] == want
    streams = {}
    for slot, *_, stream in calls:
        streams.setdefault(slot, set()).add(stream)
    assert all(len(v) == 1 for v in streams.values()), streams
    assert len({next(iter(v)) for v in streams.values()}) == len(plan), streams
    serial, _ = make(tile_streams=1, tile_batch=1).enhance(frame)
    assert np.array_equal(got, serial)
    assert got.shape == (128, 192, 3) and got.std() > 0
