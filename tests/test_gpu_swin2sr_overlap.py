"""GPU: Swin2SR's overlapped tiles with averaged seams (Swin2SR.upscale(tile=, tile_overlap=), nesr_swin2sr_upscale_overlapped_u8).

  composition   for the nine rows of swin2sr_overlap_ref.OVERLAP_CASES the route equals, bit for bit, a composition built on the
                device: frame / 255 (a true division, checked against numpy's) symmetric-padded by torch, model.forward on every
                window in plan order, E += y in float32, E / count, crop, clamp, x 255, round
  float64       the same output, through the C entry into a guarded buffer, meets u8_check against the float64 specification: no
                wrong sample, at most 2 % thin; the guards stay intact
  batches       max_batch 1, 2, 5, 35, 1000 and the default give the same bits, in ceil(35 / B) x 20 + 1 launches
  repeat        a repeated call gives the same bits
  one window    a frame no larger than the tile is the quantised forward of the padded frame; where the processor pads more than
                the window does, it differs from upscale(frame)
  O = 0         the paste of the quantised window outputs wherever one window covers the pixel (all but the slid last windows' overlap)
  fp16 form     the composition equality, with forward in the same form on the windows
  workspace     an overlapped call after a large untiled frame on one context, and the reverse, give the bits of fresh contexts
  refusals      tile < 1, an effective tile that is no multiple of the window, tile_overlap < 0 or >= the tile, a capacity too
                small, a one-channel model: NESR_ERR_ARG with the output untouched; the ValueErrors of upscale
  adapter       swin2sr_stage(model, tile=8, tile_overlap=4) inside enhance_iterations equals the model's own call
"""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import Swin2SR, _lib
from neural_enhanced_super_resolution_amd import nesr_adapter as A
from tests import swin2sr_cases as C
from tests import swin2sr_overlap_ref as OR
from tests import swin2sr_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
ROWS = list(range(len(OR.OVERLAP_CASES)))
_cache = {}


def fresh(name, compute_dtype="f32"):
    case = C.by_name(name)
    m = Swin2SR(compute_dtype=compute_dtype, **case.cfg).to(DEV)
    m.load_state_dict(case.sd)
    return m


def model(name, compute_dtype="f32"):
    if (name, compute_dtype) not in _cache:
        _cache[name, compute_dtype] = fresh(name, compute_dtype)
    return _cache[name, compute_dtype]


def sym(n_padded, n):
    """numpy's "symmetric" extension of an axis of n to n_padded, as indices."""
    i = torch.arange(n_padded) % (2 * n)
    return torch.where(i < n, i, 2 * n - 1 - i).to(DEV)


def padded_on_device(m, frame):
    """[1, 3, hp, wp] float32: frame / 255 by a true division on the device, symmetric-padded once to the window."""
    h, w = frame.shape[:2]
    ws = m.config["window_size"]
    x = torch.from_numpy(frame).to(DEV).float() / torch.tensor(255.0, device=DEV)       # a tensor divisor: no reciprocal
    assert np.array_equal(x.cpu().numpy(), frame.astype(np.float32) / np.float32(255.0)), "the device's division is not the IEEE one"
    x = x[sym(-(-h // ws) * ws, h)][:, sym(-(-w // ws) * ws, w)]
    return x.permute(2, 0, 1).unsqueeze(0).contiguous()


def windows_on_device(m, frame, T, O):
    """(plan, [forward(window)] in plan order, each [3, t s, t s] float32 on the device)."""
    h, w = frame.shape[:2]
    p = m.overlap_plan(h, w, T, O)
    t = p["tile"]
    x = padded_on_device(m, frame)
    assert tuple(x.shape[2:]) == p["padded"]
    return p, [m.forward(x[:, :, wy:wy + t, wx:wx + t].contiguous())[0] for wy, wx, _, _ in p["plan"].tolist()]


def composed(m, frame, T, O):
    """The specification with the GPU's own forward as the window function, all on the device."""
    h, w = frame.shape[:2]
    s = m.config["upscale"]
    p, ys = windows_on_device(m, frame, T, O)
    t, (hp, wp) = p["tile"], p["padded"]
    E = torch.zeros((3, hp * s, wp * s), dtype=torch.float32, device=DEV)
    for (_, _, oy, ox), y in zip(p["plan"].tolist(), ys):
        E[:, oy:oy + t * s, ox:ox + t * s] += y
    cy = torch.tensor(OR.counts(hp, t, O), dtype=torch.float32, device=DEV).repeat_interleave(s)
    cx = torch.tensor(OR.counts(wp, t, O), dtype=torch.float32, device=DEV).repeat_interleave(s)
    out = (E / (cy[:, None] * cx[None, :]))[:, :h * s, :w * s]
    return R.quantise(out.permute(1, 2, 0)).cpu()


def guarded_overlapped(m, frame, T, O, max_batch=0):
    """nesr_swin2sr_upscale_overlapped_u8 into the middle of a buffer of sentinels; the guards are asserted."""
    h, w = frame.shape[:2]
    s = m.config["upscale"]
    n = h * s * w * s * 3
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    src = torch.from_numpy(frame).to(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().nesr_swin2sr_upscale_overlapped_u8(m._context(src.device), ctypes.c_void_p(src.data_ptr()), h, w, T, O, max_batch,
                                                              ctypes.c_void_p(buf.data_ptr() + GUARD), n, stream), "nesr_swin2sr_upscale_overlapped_u8")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n:] == 0xA5).all()), "the entry wrote outside the frame it reports"
    return buf[GUARD:GUARD + n].view(h * s, w * s, 3).cpu()


@pytest.mark.parametrize("row", ROWS, ids=OR.row_id)
def test_overlapped_is_the_composition_bit_for_bit_and_meets_the_float64_route(row):
    name, (h, w), T, O, windows, _ = OR.OVERLAP_CASES[row]
    m = model(name)
    frame, y64, _, tol = OR.overlap_reference(row)
    p = m.overlap_plan(h, w, T, O)
    assert [tuple(r) for r in p["plan"].tolist()] == OR.plan(h, w, T, O, m.config["window_size"], m.config["upscale"])[3] and len(p["plan"]) == windows
    got = m.upscale(frame, tile=T, tile_overlap=O)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (h * m.config["upscale"], w * m.config["upscale"], 3)
    assert torch.equal(got.cpu(), composed(m, frame, T, O))
    guarded = guarded_overlapped(m, frame, T, O)
    assert torch.equal(guarded, got.cpu())
    excluded, wrong, n = R.u8_check(guarded, y64, tol)
    print(f"{OR.row_id(row)}: tol {tol:.3e}, {excluded} of {n} samples thin ({100.0 * excluded / n:.2f} %), {wrong} wrong")
    assert wrong == 0
    assert excluded <= C.MAX_THIN * n


def test_batch_size_changes_no_bit_and_a_repeat_neither():
    name, (h, w), T, O, windows, _ = OR.OVERLAP_CASES[0]
    assert (name, windows) == ("small_shift", 35)
    m = model(name)
    frame = torch.from_numpy(OR.overlap_reference(0)[0]).to(DEV)
    want = m.upscale(frame, tile=T, tile_overlap=O, max_batch=1).cpu()
    assert torch.equal(m.upscale(frame, tile=T, tile_overlap=O, max_batch=1).cpu(), want)       # a repeat
    m.kernel_time_ms()
    m.set_kernel_timing(True)
    try:
        for b in (1, 2, 5, 35, 1000, None):
            got = m.upscale(frame, tile=T, tile_overlap=O, max_batch=b).cpu()
            launches = m.kernel_time_ms()["launches"]
            assert torch.equal(got, want), b
            assert launches == -(-windows // min(b or windows, windows)) * 20 + 1, (b, launches)      # 19 of a forward, the add; the division once
    finally:
        m.set_kernel_timing(False)
    assert torch.equal(m.upscale(frame, tile=T, tile_overlap=O).cpu(), want)


def test_a_frame_of_one_window_is_the_forward_of_the_padded_frame():
    m = model("small_shift")                                             # window 4, x2
    for (h, w), same_as_processor in (((7, 6), True), ((8, 8), False)):
        frame = R.seeded_frame(h, w, 50 + h)
        p = m.overlap_plan(h, w, 8, 4)
        assert p["tiles"] == (1, 1) and p["tile"] == 8 and p["padded"] == (8, 8)
        y = m.forward(padded_on_device(m, frame))[0, :, :h * 2, :w * 2]
        got = m.upscale(frame, tile=8, tile_overlap=4).cpu()
        assert torch.equal(got, R.quantise(y.permute(1, 2, 0)).cpu())
        # 7 x 6: the processor's (n // 8 + 1) * 8 is 8 x 8 as well, the same symmetric extension; 8 x 8: it pads to 16 x 16
        assert torch.equal(got, m.upscale(frame).cpu()) == same_as_processor, (h, w)


def test_without_overlap_it_is_the_paste_except_under_the_slid_windows():
    m = model("small_shift")
    h, w, T = 13, 18, 8                                                  # 16 x 20: columns start at 0, 8 and (slid) 12
    frame = R.seeded_frame(h, w, 50 + h)
    p, ys = windows_on_device(m, frame, T, 0)
    assert p["tiles"] == (2, 3) and [r[1] for r in p["plan"].tolist()[:3]] == [0, 8, 12]
    paste = torch.zeros((32, 40, 3), dtype=torch.uint8)
    for (_, _, oy, ox), y in zip(p["plan"].tolist(), ys):
        paste[oy:oy + 16, ox:ox + 16] = R.quantise(y.permute(1, 2, 0)).cpu()
    once = (torch.tensor(OR.counts(16, 8, 0)).repeat_interleave(2)[:, None] * torch.tensor(OR.counts(20, 8, 0)).repeat_interleave(2)[None, :]) == 1
    once = once[:h * 2, :w * 2]
    assert bool(once.any()) and not bool(once.all()) and int((~once).sum()) == 26 * 8
    got = m.upscale(frame, tile=T, tile_overlap=0).cpu()
    assert torch.equal(got[once], paste[:h * 2, :w * 2][once])
    assert torch.equal(got, composed(m, frame, T, 0))


@pytest.mark.parametrize("row", [0, 4], ids=OR.row_id)
def test_fp16_form_is_the_composition_of_its_own_forwards(row):
    name, (h, w), T, O, _, _ = OR.OVERLAP_CASES[row]
    m = model(name, "fp16")
    frame = OR.overlap_reference(row)[0]
    got = m.upscale(frame, tile=T, tile_overlap=O).cpu()
    assert torch.equal(got, composed(m, frame, T, O))
    assert torch.equal(m.upscale(frame, tile=T, tile_overlap=O, max_batch=2).cpu(), got)


@pytest.mark.parametrize("row", [0, 4], ids=OR.row_id)
def test_workspace_shared_between_overlapped_and_untiled_leaves_no_trace(row):
    name, (h, w), T, O, _, _ = OR.OVERLAP_CASES[row]
    frame = OR.overlap_reference(row)[0]
    big = R.seeded_frame(97, 99, 91)                                       # 104 x 104 tokens: more than the overlapped frame's whole workspace
    used, other = fresh(name), fresh(name)
    want, want_big = fresh(name).upscale(frame, tile=T, tile_overlap=O).cpu(), fresh(name).upscale(big).cpu()
    assert torch.equal(used.upscale(big).cpu(), want_big)                  # large untiled, then overlapped, then the large one again
    assert torch.equal(used.upscale(frame, tile=T, tile_overlap=O).cpu(), want)
    assert torch.equal(used.upscale(big).cpu(), want_big)
    assert torch.equal(other.upscale(frame, tile=T, tile_overlap=O, max_batch=3).cpu(), want)      # the reverse order
    assert torch.equal(other.upscale(big).cpu(), want_big)
    assert torch.equal(other.upscale(frame, tile=T, tile_overlap=O).cpu(), want)
    s, (hp, wp) = used.config["upscale"], used.overlap_plan(h, w, T, O)["padded"]
    one, two = used.overlap_workspace_bytes(h, w, T, O, 1), used.overlap_workspace_bytes(h, w, T, O, 2)
    t = used.overlap_plan(h, w, T, O)["tile"]
    assert two > one > 12 * hp * s * wp * s + 12 * t * s * t * s           # the accumulator, a window's output, and the network's part
    assert two - one > 12 * t * s * t * s                                # a window more: its share of the network's workspace and its output


def test_refusals_leave_the_output_untouched():
    m = model("small_shift")                                             # window 4, x2
    lib, h = _lib.load(), m._context(torch.device(DEV))
    frame = torch.zeros(21, 30, 3, dtype=torch.uint8, device=DEV)
    o8 = torch.full((42 * 60 * 3,), 0xA5, dtype=torch.uint8, device=DEV)

    def overlapped(handle, T, O, cap):
        return lib.nesr_swin2sr_upscale_overlapped_u8(handle, ctypes.c_void_p(frame.data_ptr()), 21, 30, T, O, 0, ctypes.c_void_p(o8.data_ptr()), cap, None)

    for args, word in (((0, 0, o8.numel()), "tile must"), ((-8, 4, o8.numel()), "tile must"), ((6, 2, o8.numel()), "multiple of window_size 4"),
                       ((8, -1, o8.numel()), "tile_overlap must"), ((8, 8, o8.numel()), "tile_overlap must"), ((64, 24, o8.numel()), "tile_overlap must"),
                       ((8, 4, o8.numel() - 1), "capacity")):
        assert overlapped(h, *args) == _lib.ERR_ARG and word in lib.nesr_last_error().decode(), (args, lib.nesr_last_error())
    gray = fresh("gray")
    assert overlapped(gray._context(torch.device(DEV)), 8, 4, o8.numel()) == _lib.ERR_ARG
    assert "an RGB frame needs num_channels = num_channels_out = 3" in lib.nesr_last_error().decode()
    n = ctypes.c_size_t(7)
    assert lib.nesr_swin2sr_overlap_workspace_bytes(h, 21, 30, 6, 2, 1, ctypes.byref(n)) == _lib.ERR_ARG and n.value == 7
    assert lib.nesr_swin2sr_overlap_workspace_bytes(h, 21, 30, 8, 4, 0, ctypes.byref(n)) == _lib.ERR_ARG and "batch" in lib.nesr_last_error().decode()
    torch.cuda.synchronize()
    assert bool((o8 == 0xA5).all())                                        # refused before any launch
    with pytest.raises(ValueError, match="tile_overlap.*tile_pad"):
        m.upscale(frame, tile=8, tile_pad=4, tile_overlap=4)
    with pytest.raises(ValueError, match="tile_overlap.*tile"):
        m.upscale(frame, tile_overlap=4)
    with pytest.raises(_lib.NesrHipError, match="multiple of window_size 4"):
        m.upscale(frame, tile=6, tile_overlap=2)
    with pytest.raises(_lib.NesrHipError, match="tile_overlap must"):
        m.upscale(frame, tile=8, tile_overlap=8)


def test_stage_with_overlapped_tiles_in_enhance_iterations(cuda_device):
    name = "odd_depth_x4"
    m = model(name)
    img = R.seeded_frame(16, 24, 66)
    cfg = {"iterations": 1, "upscale_factor": 2.0}
    trace = []
    calls = m.calls
    got = A.enhance_iterations(None, img, cfg, "cuda", trace=trace, extra_upscalers=[A.swin2sr_stage(m, tile=8, tile_overlap=4)], device=cuda_device)
    assert m.calls == calls + 1 and trace[0]["ensemble_n"] == 1
    want = m.upscale(img, tile=8, tile_overlap=4).cpu().numpy()
    assert got.shape == (64, 96, 3) and np.array_equal(got, want)
    assert not np.array_equal(want, m.upscale(img, tile=8, tile_pad=4).cpu().numpy())      # the other tiled route
