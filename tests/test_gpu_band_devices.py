"""Row bands of one untiled frame over the contexts of ONE process: the peer-writing exchange (band_push_edges, nesr_band_land_aprons),
the whole frame below Python (nesr_forward_banded / _u8) and RealESRGANer(devices=[...], tile=0).  Everything is compared BIT FOR
BIT: with the existing pack / unpack, with the whole-frame forward, with devices=None.  Repeated indices ([0, 0], [0, 0, 0]) run on
one GPU (the links are then "local": the plain pointer); [0, 1] is added where two GPUs are visible, and only there is a link
written through a peer mapping -- every test prints which kind of link it ran."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_FORMS = ["f32", "f32-winograd", "f32-direct"]


def _lists(base):
    """`base` plus, where two GPUs are visible, the same number of lanes alternating over devices 0 and 1."""
    out = [list(b) for b in base]
    if torch.cuda.device_count() >= 2:
        out += [[j % 2 for j in range(len(b))] for b in base]
    return out


def _lanes(devices):
    return [(torch.device("cuda", d), devices[:j].count(d)) for j, d in enumerate(devices)]


def _net(algo, scale, num_block=2, seed=9):
    from neural_enhanced_super_resolution_amd import RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    net = RRDBNet(3, 3, scale=scale, num_block=num_block, compute_dtype=algo)
    net.load_state_dict(synthetic_state_dict(seed=seed, num_in_ch=3, scale=scale, num_block=num_block))
    return net.eval().to("cuda:0")


def _sync():
    for d in range(torch.cuda.device_count()):
        torch.cuda.synchronize(d)


@pytest.mark.parametrize("link", ["direct", "staged"])
@pytest.mark.parametrize("algo,world,scale,hw", [("f32", 2, 2, (96, 80)), ("f32", 3, 2, (132, 72)), ("f32", 2, 4, (40, 56)),
                                                 ("f32-direct", 3, 2, (132, 72)), ("f32-winograd", 2, 4, (40, 56)), ("bf16", 2, 2, (96, 80))])
def test_push_and_land_equal_pack_and_unpack(cuda_device, algo, world, scale, hw, link):
    """Linked contexts hold band images of different inputs and random feature buffers.  Pushed with one parity while another
    buffer is pushed with the other, a buffer's edge rows land in the neighbours' apron rows bitwise as band_rows reads them on
    the sender; band rows and the aprons at frame edges keep their bytes; `also` refreshes a second buffer from the same rows."""
    from neural_enhanced_super_resolution_amd import banded
    A = banded.APRON
    for devices in _lists([[0] * world]):
        net = _net(algo, scale)
        lanes = _lanes(devices)
        u = net.unshuffle
        bands = banded.band_split(hw[0] // u, world)
        tops = [A if r else 0 for r in range(world)]
        bots = [A if r < world - 1 else 0 for r in range(world)]
        gen = torch.Generator().manual_seed(11)
        for r, (dev, slot) in enumerate(lanes):
            rows = (bands[r][1] - bands[r][0] + tops[r] + bots[r]) * u
            net.band_begin(torch.rand(1, 3, rows, hw[1], generator=gen).to(dev), slot=slot)
        states = net.band_link(lanes)
        if link == "staged":
            for dev, slot in lanes:
                net.band_set_staged(True, slot, dev)
            states = [net.band_link_state(slot, dev) for dev, slot in lanes]
            assert all(v in (None, "staged") for st in states for v in st.values())
        else:
            assert all(v in (None, "local", "peer") for st in states for v in st.values())
            assert all(v != "local" or devices[r] == devices[r + (1 if k == "down" else -1)] for r, st in enumerate(states) for k, v in st.items() if v)
        print(f"\n{algo} {hw} devices={devices}: links {states}")
        assert states[0]["up"] is None and states[-1]["down"] is None and all(st["down"] for st in states[:-1]) and all(st["up"] for st in states[1:])
        heights = [bands[r][1] - bands[r][0] + tops[r] + bots[r] for r in range(world)]
        for r, (dev, slot) in enumerate(lanes):       # random bytes in every buffer: conv_first filled only 0 and 3
            n = heights[r] * net.band_row_bytes(slot, dev)
            for b in range(4):
                net.band_set_rows(b, 0, torch.randint(0, 256, (n,), dtype=torch.uint8, generator=gen), slot, dev)
        _sync()

        def rows(r, b, row0, n):
            return net.band_rows(b, row0, n, lanes[r][1], lanes[r][0]).cpu()

        def snapshot(b):
            return [dict(first=rows(r, b, tops[r], A), last=rows(r, b, heights[r] - bots[r] - A, A), band=rows(r, b, tops[r], heights[r] - tops[r] - bots[r]),
                         top=rows(r, b, 0, A), bottom=rows(r, b, heights[r] - A, A)) for r in range(world)]

        def landed(b, was, sent):
            for r in range(world):
                assert torch.equal(rows(r, b, tops[r], heights[r] - tops[r] - bots[r]), was[r]["band"]), (b, r, "band rows changed")
                if r > 0:
                    assert torch.equal(rows(r, b, 0, A), sent[r - 1]["last"]), (b, r, "top apron")
                else:
                    assert torch.equal(rows(r, b, 0, A), was[r]["top"]), (b, r, "frame edge changed")
                if r < world - 1:
                    assert torch.equal(rows(r, b, heights[r] - A, A), sent[r + 1]["first"]), (b, r, "bottom apron")
                else:
                    assert torch.equal(rows(r, b, heights[r] - A, A), was[r]["bottom"]), (b, r, "frame edge changed")

        for b in range(4):
            for parity in (0, 1):
                other = (b + 1) % 4
                was, was_other = snapshot(b), snapshot(other)
                assert not torch.equal(was[0]["last"], was_other[0]["last"])
                for r, (dev, slot) in enumerate(lanes):
                    net.band_push_edges(b, tops[r], bots[r], A, parity, slot, dev)
                    net.band_push_edges(other, tops[r], bots[r], A, 1 - parity, slot, dev)
                _sync()                                    # (one host thread: the devices' work is ordered by waiting for it)
                for r, (dev, slot) in enumerate(lanes):
                    net.band_land_aprons(b, tops[r], bots[r], A, parity, slot=slot, device=dev)
                _sync()
                landed(b, was, was)
                for r, (dev, slot) in enumerate(lanes):
                    net.band_land_aprons(other, tops[r], bots[r], A, 1 - parity, slot=slot, device=dev)
                _sync()
                landed(other, was_other, was_other)
        was0, was3 = snapshot(0), snapshot(3)               # step 0 of a frame: conv_first's rows also refresh the trunk-skip copy
        for r, (dev, slot) in enumerate(lanes):
            net.band_push_edges(0, tops[r], bots[r], A, 0, slot, dev)
        _sync()
        for r, (dev, slot) in enumerate(lanes):
            net.band_land_aprons(0, tops[r], bots[r], A, 0, also=(3,), slot=slot, device=dev)
        _sync()
        landed(0, was0, was0)
        landed(3, was3, was0)
        net.check_status()


@pytest.mark.parametrize("algo,world,scale,hw", [(a, *c) for a in F32_FORMS for c in [(2, 2, (96, 80)), (3, 2, (132, 72)), (2, 4, (40, 56))]]
                         + [("f32", 2, 2, (560, 544))])
def test_forward_banded_bitwise_equals_whole_frame(cuda_device, algo, world, scale, hw):
    """nesr_forward_banded on 2 and 3 lanes against the whole-frame forward of another model with the same weights; two frames on
    the same contexts (landing-buffer parity and events start over).  560 x 544: bands of several tile rows, and a whole frame that
    runs per-layer launches (the small ones compare against the fused dense-block kernel); the default form only."""
    ref = _net(algo, scale)
    xs = [torch.rand(1, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(4 + k)).to(cuda_device) for k in range(2)]
    want = [ref(x) for x in xs]
    assert not torch.equal(want[0], want[1])
    ref.check_status()
    for devices in _lists([[0] * world]):
        net = _net(algo, scale)
        lanes = _lanes(devices)
        for k, x in enumerate(xs):
            got = net.forward_banded(x, lanes)
            torch.cuda.synchronize()
            assert got.shape == want[k].shape and got.device == x.device
            assert torch.equal(got, want[k]), (devices, k, float((got - want[k]).abs().max()))
        print(f"\n{algo} {hw} devices={devices}: links {[net.band_link_state(s, d) for d, s in lanes]}")
        net.check_status()
        q = net.forward_banded_u8((xs[0][0].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous(), lanes)
        qw = ref.forward_u8((xs[0][0].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous())
        assert torch.equal(q, qw), devices
        net.check_status()
        ref.check_status()


def _make(sd, scale, devices=None, algo="f32", **kw):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    args = dict(tile=0, tile_pad=10, pre_pad=0, half=False)
    args.update(kw)
    return RealESRGANer(scale=scale, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=scale, num_block=2, compute_dtype=algo), device="cuda:0",
                        devices=devices, **args)


def _frames():
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    return {"bgr": (synthetic_frame(192, 256, seed=3), 0), "bgr_prepad": (synthetic_frame(191, 253, seed=4), 10),
            "gray": (synthetic_frame(192, 256, seed=5, channels=0), 0), "bgra": (synthetic_frame(192, 256, seed=6, channels=4), 0),
            "u16": (synthetic_frame(192, 256, seed=7).astype(np.uint16) * 250 + 3, 0)}


@pytest.mark.parametrize("case", ["bgr", "bgr_prepad", "gray", "bgra", "u16"])
def test_enhance_untiled_over_devices_is_banded_and_bitwise(cuda_device, case):
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(seed=2, num_in_ch=3, scale=2, num_block=2)
    frame, pre = _frames()[case]
    want, mode = _make(sd, 2, pre_pad=pre).enhance(frame)
    assert want.dtype == frame.dtype and want.shape[:2] == (2 * frame.shape[0], 2 * frame.shape[1])
    for devices in _lists([[0, 0]]):
        up = _make(sd, 2, devices=devices, pre_pad=pre)
        up.BAND_MIN_ROWS = 16
        for _ in range(2):                                 # a second frame on the same lanes
            got, gmode = up.enhance(frame)
            assert gmode == mode and got.dtype == want.dtype and np.array_equal(got, want), (devices, int(np.count_nonzero(got != want)))
            rows = (frame.shape[0] + pre + 1) // 2           # internal rows of the padded image
            assert up.last_bands is not None and len(up.last_bands) == 2 and up.last_bands[0][0] == 0 and up.last_bands[-1][1] == rows
        for d, o in _lanes(devices):
            assert up.model._handle(d.index, o) is not None, (devices, d, o)
        print(f"\n{case} devices={devices}: bands {up.last_bands}, links {[up.model.band_link_state(o, d) for d, o in _lanes(devices)]}")
        up.band_devices = False
        got, _ = up.enhance(frame)
        assert np.array_equal(got, want) and up.last_bands is None
        up.band_devices = True
        up.tile_size = 512                                 # a frame no larger than the tile is one evaluation too
        got, _ = up.enhance(frame)
        assert np.array_equal(got, want) and len(up.last_bands) == 2


def test_frame_below_the_row_floor_runs_on_one_lane(cuda_device):
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=2, num_in_ch=3, scale=2, num_block=2)
    frame = synthetic_frame(128, 96, seed=8)               # 64 internal rows: fewer than 2 x 48
    want, _ = _make(sd, 2).enhance(frame)
    up = _make(sd, 2, devices=[0, 0])
    got, _ = up.enhance(frame)
    assert np.array_equal(got, want) and up.last_bands is None
    assert up.model._handle(0, 1) is None                  # the second lane was never asked
    up.BAND_MIN_ROWS = 32
    got, _ = up.enhance(frame)
    assert np.array_equal(got, want) and up.last_bands == [(0, 32), (32, 64)]


def test_range_error_in_one_band_then_clean(cuda_device):
    """conv_first scaled x3e5 (conv_last / 3e5): a bright input overflows the f16 pair of the default f32 form, a black one does not.
    Only rows the lower band reads are bright; the frame raises, the next ones are clean and correct."""
    from neural_enhanced_super_resolution_amd._lib import NesrRangeError
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=2)
    sd["conv_first.weight"] *= 3e5
    sd["conv_last.weight"] /= 3e5
    bad = synthetic_frame(256, 384, seed=7)
    bad[:160] = 0                     # the upper band reads input rows [0, 2 * (64 + 6)) = [0, 140): black
    clean = np.zeros_like(bad)
    clean[:100] = synthetic_frame(100, 384, seed=8) // 128  # dark content (values 0, 1) in the top rows
    want, _ = _make(sd, 2).enhance(clean)
    up = _make(sd, 2, devices=[0, 0])
    with pytest.raises(NesrRangeError):
        up.enhance(bad)
    assert up.last_bands == [(0, 64), (64, 128)]
    for _ in range(2):
        got, _ = up.enhance(clean)
        assert np.array_equal(got, want) and len(up.last_bands) == 2


def test_c_host_runs_a_banded_frame(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "nesr_banded_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "banded_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    out = subprocess.run([exe, lib], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "banded vs whole frame: 0 bytes differ" in out.stdout


def test_bf16_model_keeps_the_first_entry_route(cuda_device):
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=2, num_in_ch=3, scale=2, num_block=2)
    frame = synthetic_frame(192, 256, seed=3)
    want, _ = _make(sd, 2, half=True).enhance(frame)
    up = _make(sd, 2, devices=[0, 0], half=True)
    up.BAND_MIN_ROWS = 16
    got, _ = up.enhance(frame)
    assert np.array_equal(got, want) and up.last_bands is None
    assert up.model._handle(0, 1) is None
