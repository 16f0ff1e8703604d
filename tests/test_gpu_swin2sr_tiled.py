"""GPU: Swin2SR's tiled upscale and the batch dimension of its three kernels.

  composition   upscale(frame, tile=T, tile_pad=P) equals, bit for bit, the paste of upscale(window) over the plan: both sides on
                the GPU, no tolerance
  float64       the same outputs, through the C entry into a guarded buffer, meet u8_check against the float64 composition of
                tests/swin2sr_tiled_ref.py: no wrong sample, at most 2 % thin
  batches       max_batch 1, 2, 5, 12 and the default give the same bits, in ceil(12 / B) x 19 launches
  one window    a frame no larger than T + 2 P gives the bits of the untiled upscale
  forward_batch three images as N = 3 equal three N = 1 forwards bit for bit and meet the case's tolerance against float64; one is
                all zeros and one all ones, so a halo, a shift or a mask that crosses into the neighbouring image shows
  workspace     a tiled frame after a large untiled one on one context, and the reverse, give the bits of fresh contexts
  refusals      tile < 1, tile_pad < 0, a capacity too small, a one-channel model, an H that is no multiple of the window: all
                NESR_ERR_ARG with the output untouched
  adapter       swin2sr_stage(model, tile=8, tile_pad=4) inside enhance_iterations equals the model's tiled call
"""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import Swin2SR, _lib
from neural_enhanced_super_resolution_amd import nesr_adapter as A
from tests import swin2sr_cases as C
from tests import swin2sr_ref as R
from tests import swin2sr_tiled_ref as TR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
NAMES = [t[0] for t in TR.TILED_CASES]
_cache = {}


def model(name):
    if name not in _cache:
        case = C.by_name(name)
        m = Swin2SR(**case.cfg).to(DEV)
        m.load_state_dict(case.sd)
        _cache[name] = m
    return _cache[name]


def fresh(name):
    case = C.by_name(name)
    m = Swin2SR(**case.cfg).to(DEV)
    m.load_state_dict(case.sd)
    return m


def guarded_tiled(m, frame, T, P, max_batch=0):
    """nesr_swin2sr_upscale_tiled_u8 into the middle of a buffer of sentinels; the guards are asserted."""
    h, w = frame.shape[:2]
    s = m.config["upscale"]
    n = h * s * w * s * 3
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    src = torch.from_numpy(frame).to(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().nesr_swin2sr_upscale_tiled_u8(m._context(src.device), ctypes.c_void_p(src.data_ptr()), h, w, T, P, max_batch,
                                                         ctypes.c_void_p(buf.data_ptr() + GUARD), n, stream), "nesr_swin2sr_upscale_tiled_u8")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n:] == 0xA5).all()), "the entry wrote outside the frame it reports"
    return buf[GUARD:GUARD + n].view(h * s, w * s, 3).cpu()


def pasted(m, frame, T, P):
    """The specification with the GPU's own untiled upscale as the window function."""
    h, w = frame.shape[:2]
    s = m.config["upscale"]
    p = m.tile_plan(h, w, T, P)
    sy, sx = p["window"]
    out = torch.zeros((h * s, w * s, 3), dtype=torch.uint8)
    for wy, wx, cy, cx, ch, cw, oy, ox in p["plan"].tolist():
        y = m.upscale(np.ascontiguousarray(frame[wy:wy + sy, wx:wx + sx])).cpu()
        out[oy:oy + ch, ox:ox + cw] = y[cy:cy + ch, cx:cx + cw]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_tiled_is_the_composition_bit_for_bit_and_meets_the_float64_route(name):
    _, (h, w), T, P, tiles = TR.tiled_case(name)
    m = model(name)
    frame, y64, _, tol = TR.tiled_reference(name)
    assert [tuple(r) for r in m.tile_plan(h, w, T, P)["plan"].tolist()] == TR.plan(h, w, T, P, m.config["upscale"])[2] and len(TR.plan(h, w, T, P, 1)[2]) == tiles
    got = m.upscale(frame, tile=T, tile_pad=P)
    assert got.is_cuda and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), pasted(m, frame, T, P))
    guarded = guarded_tiled(m, frame, T, P)
    assert torch.equal(guarded, got.cpu())
    excluded, wrong, n = R.u8_check(guarded, y64, tol)
    print(f"{name} {h}x{w} {T}/{P}: tol {tol:.3e}, {excluded} of {n} samples thin ({100.0 * excluded / n:.2f} %), {wrong} wrong")
    assert wrong == 0
    assert excluded <= C.MAX_THIN * n


def test_batch_size_changes_no_bit_and_tiles_share_launches():
    name = "small_shift"
    _, (h, w), T, P, tiles = TR.tiled_case(name)
    m = model(name)
    frame = torch.from_numpy(TR.tiled_reference(name)[0]).to(DEV)
    want = m.upscale(frame, tile=T, tile_pad=P, max_batch=1).cpu()
    m.kernel_time_ms()
    m.set_kernel_timing(True)
    try:
        for b in (1, 2, 5, 12, None):
            got = m.upscale(frame, tile=T, tile_pad=P, max_batch=b).cpu()
            launches = m.kernel_time_ms()["launches"]
            assert torch.equal(got, want), b
            assert launches == -(-tiles // (b or tiles)) * 19, (b, launches)      # the default holds all twelve windows
    finally:
        m.set_kernel_timing(False)
    assert torch.equal(m.upscale(frame, tile=T, tile_pad=P, max_batch=1000).cpu(), want)      # more than there are tiles


@pytest.mark.parametrize("name,hw,T,P", [("small_shift", (13, 18), 8, 5), ("small_shift", (16, 16), 8, 4), ("window_12_frame", (13, 18), 18, 0),
                                         ("published_width", (8, 9), 64, 16)])
def test_a_frame_of_one_window_gives_the_untiled_bits(name, hw, T, P):
    m = model(name)
    frame = R.seeded_frame(hw[0], hw[1], 50 + hw[0])
    assert hw[0] <= T + 2 * P and hw[1] <= T + 2 * P
    assert torch.equal(m.upscale(frame, tile=T, tile_pad=P).cpu(), m.upscale(frame).cpu())


@pytest.mark.parametrize("name", ["small_shift", "one_window_high", "window_7_odd", "published_width"])
def test_forward_batch_equals_single_forwards(name):
    case, m = C.by_name(name), model(name)
    x0 = case.x.to(DEV)
    x = torch.cat([torch.zeros_like(x0), x0, torch.ones_like(x0)])         # the case's own input between a black and a white image
    got = m.forward_batch(x)
    s = case.cfg["upscale"]
    assert got.shape == (3, 3, x0.shape[2] * s, x0.shape[3] * s)
    for i in range(3):
        assert torch.equal(got[i:i + 1], m(x[i:i + 1].contiguous())), i
    err, tol = C.error(got[1:2], case)
    print(f"{name}: err {err:.3e}, tol {tol:.3e}")
    assert err <= tol
    assert torch.equal(m.forward_batch(x0), m(x0))                         # N = 1


def test_forward_batch_of_three_different_seeded_inputs():
    case, m = C.by_name("small_shift"), model("small_shift")
    xs = [R.seeded_input(12, 20, seed).to(DEV) for seed in (71, 72, 73)]
    got = m.forward_batch(torch.cat(xs))
    for i, x in enumerate(xs):
        assert torch.equal(got[i:i + 1], m(x)), i


@pytest.mark.parametrize("name", ["small_shift", "published_width"])
def test_workspace_shared_between_tiled_and_untiled_leaves_no_trace(name):
    _, (h, w), T, P, _ = TR.tiled_case(name)
    frame = TR.tiled_reference(name)[0]
    big = R.seeded_frame(97, 99, 91)                                       # 104 x 104 tokens: more than all windows of the tiled frame together
    used, other = fresh(name), fresh(name)
    want_tiled, want_big = fresh(name).upscale(frame, tile=T, tile_pad=P).cpu(), fresh(name).upscale(big).cpu()
    assert torch.equal(used.upscale(big).cpu(), want_big)                  # large untiled, then tiled, then the large one again
    assert torch.equal(used.upscale(frame, tile=T, tile_pad=P).cpu(), want_tiled)
    assert torch.equal(used.upscale(big).cpu(), want_big)
    assert torch.equal(other.upscale(frame, tile=T, tile_pad=P, max_batch=3).cpu(), want_tiled)      # the reverse order
    assert torch.equal(other.upscale(big).cpu(), want_big)
    assert torch.equal(other.upscale(frame, tile=T, tile_pad=P).cpu(), want_tiled)
    assert used.workspace_bytes(16, 16, 2) > used.workspace_bytes(16, 16, 1) > 0


def test_refusals_leave_the_output_untouched():
    m = model("small_shift")                                             # window 4, x2
    lib, h = _lib.load(), m._context(torch.device(DEV))
    frame = torch.zeros(21, 30, 3, dtype=torch.uint8, device=DEV)
    o8 = torch.full((42 * 60 * 3,), 0xA5, dtype=torch.uint8, device=DEV)

    def tiled(handle, T, P, cap):
        return lib.nesr_swin2sr_upscale_tiled_u8(handle, ctypes.c_void_p(frame.data_ptr()), 21, 30, T, P, 0, ctypes.c_void_p(o8.data_ptr()), cap, None)

    for args, word in (((0, 4, o8.numel()), "tile must"), ((-8, 4, o8.numel()), "tile must"), ((8, -1, o8.numel()), "tile_pad must"),
                       ((8, 4, o8.numel() - 1), "capacity")):
        assert tiled(h, *args) == _lib.ERR_ARG and word in lib.nesr_last_error().decode(), (args, lib.nesr_last_error())
    gray = fresh("gray")
    assert tiled(gray._context(torch.device(DEV)), 8, 4, o8.numel()) == _lib.ERR_ARG
    assert "an RGB frame needs num_channels = num_channels_out = 3" in lib.nesr_last_error().decode()
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    out = torch.full((2 * 3 * 16 * 16,), -7.0, device=DEV)

    def batch(n, c, hh, ww, cap):
        return lib.nesr_swin2sr_forward_batch_f32(h, ctypes.c_void_p(x.data_ptr()), n, c, hh, ww, ctypes.c_void_p(out.data_ptr()), cap, None)

    assert batch(2, 3, 8, 6, out.numel()) == _lib.ERR_ARG and "H and W must be multiples of window_size 4" in lib.nesr_last_error().decode()
    assert batch(2, 3, 6, 8, out.numel()) == _lib.ERR_ARG and "H and W must be multiples of window_size 4" in lib.nesr_last_error().decode()
    assert batch(0, 3, 8, 8, out.numel()) == _lib.ERR_ARG and "N" in lib.nesr_last_error().decode()
    assert batch(2, 1, 8, 8, out.numel()) == _lib.ERR_ARG
    assert batch(2, 3, 8, 8, out.numel() - 1) == _lib.ERR_ARG and "capacity" in lib.nesr_last_error().decode()
    torch.cuda.synchronize()
    assert bool((o8 == 0xA5).all()) and bool((out == -7.0).all())           # refused before any launch
    with pytest.raises(_lib.NesrHipError, match="tile must"):
        m.upscale(frame, tile=-1)
    with pytest.raises(_lib.NesrHipError, match="tile_pad must"):
        m.upscale(frame, tile=8, tile_pad=-1)
    with pytest.raises(_lib.NesrHipError, match="multiples of window_size 4"):
        m.forward_batch(torch.zeros(2, 3, 10, 8, device=DEV))


def test_stage_with_tiles_in_enhance_iterations(cuda_device):
    name = "odd_depth_x4"
    m = model(name)
    img = R.seeded_frame(16, 24, 66)
    cfg = {"iterations": 1, "upscale_factor": 2.0}
    trace = []
    calls = m.calls
    got = A.enhance_iterations(None, img, cfg, "cuda", trace=trace, extra_upscalers=[A.swin2sr_stage(m, tile=8, tile_pad=4)], device=cuda_device)
    assert m.calls == calls + 1 and trace[0]["ensemble_n"] == 1
    want = m.upscale(img, tile=8, tile_pad=4).cpu().numpy()
    assert got.shape == (64, 96, 3) and np.array_equal(got, want)
    assert not np.array_equal(want, m.upscale(img).cpu().numpy())          # six tiles, not the whole frame
