"""GPU: Swin2SR's frame-level route and its edges.

  upscale     every crafted configuration on a 13 x 18 frame (both paddings and the crop) and an 8 x 8 frame (a multiple of 8, which
              the processor still pads by 8): the u8 result equals the float64 route's u8 wherever the float64 value x 255 lies
              farther than 255 tol from a rounding boundary, and is off by at most 1 elsewhere; at most 2 % of the samples are
              left out (tests/test_swin2sr_host.py holds that condition on the CPU).  Guard bytes surround the output.  The same on
              frames shorter than the processor's padding (1 x 1, 2 x 3, 3 x 17), where the symmetric extension bounces more than once
  ties        a model whose every output sample is a rounding tie (k + 0.5 exactly in float32) or clamped: the u8 frame is
              round-half-to-even on every sample, exactly
  workspace   a small frame after a large one on one context gives the bits of a fresh context, and the large frame its own again
  refusals    a missing weight at finalize, an unexpected key, every unsupported field, an H that is no multiple of the window,
              a capacity too small: all rejected before any launch
  the loop    swin2sr_stage inside enhance_iterations against the same loop with the float64 restatement as the callable
"""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import Swin2SR, _lib
from neural_enhanced_super_resolution_amd import nesr_adapter as A
from tests import swin2sr_cases as C
from tests import swin2sr_ref as R
from tests.test_swin2sr_host import BASE, UNSUPPORTED

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [c.name for c in C.frame_cases()]      # the RGB configurations; `gray` is refused (test_one_channel_model_refuses_an_rgb_frame)
GUARD = 4096
_cache = {}


def model(name):
    if name not in _cache:
        case = C.by_name(name)
        m = Swin2SR(**case.cfg).to(DEV)
        m.load_state_dict(case.sd)
        _cache[name] = m
    return _cache[name]


def guarded_upscale(m, frame):
    """nesr_swin2sr_upscale_u8 into the middle of a buffer of sentinels: the u8 frame [h s, w s, 3] on the host; the guards are asserted."""
    hw = frame.shape[:2]
    s = m.config["upscale"]
    oh, ow = hw[0] * s, hw[1] * s
    n = oh * ow * 3
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    src = torch.from_numpy(frame).to(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().nesr_swin2sr_upscale_u8(m._context(src.device), ctypes.c_void_p(src.data_ptr()), hw[0], hw[1],
                                                   ctypes.c_void_p(buf.data_ptr() + GUARD), n, stream), "nesr_swin2sr_upscale_u8")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n:] == 0xA5).all()), "the entry wrote outside the frame it reports"
    return buf[GUARD:GUARD + n].view(oh, ow, 3).cpu()


def upscale_against_the_float64_route(name, hw):
    m = model(name)
    frame, y64, tol = C.frame_reference(name, hw)
    src = torch.from_numpy(frame).to(DEV)
    got = guarded_upscale(m, frame)
    excluded, wrong, total = R.u8_check(got, y64, tol)
    print(f"{name} {hw}: tol {tol:.3e}, {excluded} of {total} samples thin ({100.0 * excluded / total:.2f} %), {wrong} wrong")
    assert wrong == 0
    assert excluded <= C.MAX_THIN * total
    via_module = m.upscale(frame)                                   # an ndarray is copied up once
    assert via_module.is_cuda and via_module.dtype == torch.uint8 and torch.equal(via_module.cpu(), got)
    assert torch.equal(m(src).cpu(), got)                           # a u8 HWC frame through __call__ is upscale


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("hw", C.FRAMES, ids=lambda hw: "%dx%d" % hw)
def test_upscale_against_the_float64_route(name, hw):
    upscale_against_the_float64_route(name, hw)


@pytest.mark.parametrize("name", C.SMALL_FRAME_CASES)
@pytest.mark.parametrize("hw", C.SMALL_FRAMES, ids=lambda hw: "%dx%d" % hw)
def test_upscale_of_frames_shorter_than_the_padding(name, hw):
    """The symmetric extension to 8 bounces more than once (1 x 1: seven times); window 12 then reflects 8 x 8 to 12 x 12."""
    upscale_against_the_float64_route(name, hw)


def test_u8_rounds_ties_to_even():
    """Exact: every sample of this model is k + 0.5 in float32 before the rounding, or outside [0, 1]; no sample is left out."""
    case = C.rounding_ties()
    m = Swin2SR(**case.cfg).to(DEV)
    m.load_state_dict(case.sd)
    got = guarded_upscale(m, case.frame)
    want = C.ties_expected_frame(case)
    assert got.shape == want.shape
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), got[:2, :2].tolist(), want[:2, :2].tolist())


def test_one_channel_model_refuses_an_rgb_frame():
    case = C.by_name("gray")
    m = Swin2SR(**case.cfg).to(DEV)
    m.load_state_dict(case.sd)
    lib, h = _lib.load(), m._context(torch.device(DEV))
    frame = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    o8 = torch.full((16 * 16 * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    assert lib.nesr_swin2sr_upscale_u8(h, ctypes.c_void_p(frame.data_ptr()), 8, 8, ctypes.c_void_p(o8.data_ptr()), o8.numel(), None) == _lib.ERR_ARG
    assert "an RGB frame needs num_channels = num_channels_out = 3" in lib.nesr_last_error().decode()
    torch.cuda.synchronize()
    assert bool((o8 == 0xA5).all())                                 # refused before any launch
    with pytest.raises(_lib.NesrHipError, match="an RGB frame needs num_channels"):
        m.upscale(frame)


@pytest.mark.parametrize("name", ["small_shift", "published_width"])      # pixelshuffle (both shuffle buffers) and nearest+conv
def test_workspace_reuse_leaves_no_trace(name):
    """The workspace only grows, and a smaller frame carves its buffers from the same base: a read past a frame's extent would meet
    what the larger frame left there.  Bit-equal to a context that never saw the large frame, and the large frame to itself."""
    case = C.by_name(name)
    used, fresh = Swin2SR(**case.cfg).to(DEV), Swin2SR(**case.cfg).to(DEV)
    used.load_state_dict(case.sd)
    fresh.load_state_dict(case.sd)
    big, small = R.seeded_input(24, 24, 61).to(DEV), R.seeded_input(8, 8, 62).to(DEV)
    y_big, y_small, y_again = used(big).cpu(), used(small).cpu(), used(big).cpu()
    assert torch.isfinite(y_big).all() and torch.equal(y_big, y_again)
    assert torch.equal(y_small, fresh(small).cpu())
    fbig, fsmall = R.seeded_frame(21, 19, 63), R.seeded_frame(3, 5, 64)
    u_big, u_small, u_again = used.upscale(fbig).cpu(), used.upscale(fsmall).cpu(), used.upscale(fbig).cpu()
    assert torch.equal(u_big, u_again)
    assert torch.equal(u_small, fresh.upscale(fsmall).cpu())
    assert torch.equal(fresh(big).cpu(), y_big)                     # and growing after a small frame changes nothing either


def test_finalize_and_load_weight_are_strict():
    case = C.by_name("small_shift")
    m = Swin2SR(**case.cfg)
    lib = _lib.load()
    h = m._create(0)
    try:
        assert lib.nesr_swin2sr_num_tensors(h) == len(case.sd)
        keys = list(case.sd)

        def load(key, t):
            t = t.contiguous()
            shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
            return lib.nesr_swin2sr_load_weight(h, key.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim())

        for k in keys[:-1]:
            assert load(k, case.sd[k]) == 0
        assert lib.nesr_swin2sr_finalize(h) == -3 and keys[-1] in lib.nesr_last_error().decode()        # NESR_ERR_STATE
        x = torch.zeros(1, 3, 8, 8, device=DEV)
        out = torch.zeros(1, 3, 16, 16, device=DEV)
        assert lib.nesr_swin2sr_forward_f32(h, ctypes.c_void_p(x.data_ptr()), 1, 3, 8, 8, ctypes.c_void_p(out.data_ptr()), out.numel(), None) == -3
        assert load("swin2sr.nothing.weight", torch.zeros(3)) == _lib.ERR_ARG and "unexpected key" in lib.nesr_last_error().decode()
        assert load(keys[-1], torch.zeros(2, 2)) == _lib.ERR_ARG and "size mismatch" in lib.nesr_last_error().decode()
        assert load("swin2sr.encoder.stages.0.layers.0.attention.self.relative_position_index", torch.zeros(16, 16)) == 0      # ignored
        assert load(keys[-1], case.sd[keys[-1]]) == 0
        assert lib.nesr_swin2sr_finalize(h) == 0
    finally:
        lib.nesr_swin2sr_destroy(h)


@pytest.mark.parametrize("field,change", UNSUPPORTED, ids=[f"{f}-{i}" for i, (f, _) in enumerate(UNSUPPORTED)])
def test_unsupported_configurations_name_the_field(field, change):
    m = Swin2SR(**dict(BASE, **change)).to(DEV)
    with pytest.raises(_lib.NesrUnsupportedError, match=field):
        m.upscale(np.zeros((8, 8, 3), np.uint8))


def test_shape_and_capacity_refusals():
    m = model("small_shift")                                        # window 4
    with pytest.raises(_lib.NesrHipError, match="multiples of window_size 4"):
        m(torch.zeros(1, 3, 10, 8, device=DEV))
    with pytest.raises(_lib.NesrHipError, match="multiples of window_size 4"):
        m(torch.zeros(1, 3, 8, 6, device=DEV))
    with pytest.raises(_lib.NesrHipError, match=r"expected \[1, 3, H, W\]"):
        m(torch.zeros(2, 3, 8, 8, device=DEV))
    lib, h = _lib.load(), m._context(torch.device(DEV))
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    out = torch.full((3 * 16 * 16,), -7.0, device=DEV)
    assert lib.nesr_swin2sr_forward_f32(h, ctypes.c_void_p(x.data_ptr()), 1, 3, 8, 8, ctypes.c_void_p(out.data_ptr()), out.numel() - 1, None) == _lib.ERR_ARG
    assert "capacity" in lib.nesr_last_error().decode()
    frame = torch.zeros(5, 7, 3, dtype=torch.uint8, device=DEV)
    o8 = torch.full((10 * 14 * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    assert lib.nesr_swin2sr_upscale_u8(h, ctypes.c_void_p(frame.data_ptr()), 5, 7, ctypes.c_void_p(o8.data_ptr()), o8.numel() - 1, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((o8 == 0xA5).all())   # refused before any launch
    with pytest.raises(ValueError):
        m.upscale(torch.zeros(5, 7, 4, dtype=torch.uint8, device=DEV))


def test_kernel_timing_and_launch_count():
    m = model("small_shift")                                        # two stages of two layers, pixelshuffle x2
    m.upscale(np.zeros((8, 8, 3), np.uint8))
    m.kernel_time_ms()
    m.set_kernel_timing(True)
    m.upscale(np.zeros((8, 8, 3), np.uint8))
    t = m.kernel_time_ms()
    m.set_kernel_timing(False)
    # first conv, embedding | per stage: 2 x (attention, MLP), conv, projection | LayerNorm, conv_after_body | before, shuffle step, final
    assert t["launches"] == 2 + 2 * (2 * 2 + 2) + 2 + 3
    assert list(t["groups"]) == ["conv", "projection", "attention", "mlp", "upsample"] and all(v > 0 for v in t["groups"].values())


def test_stage_in_enhance_iterations_against_the_restatement(cuda_device):
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    name = "odd_depth_x4"                                           # x4, the size the Real-ESRGAN stage gives: the ensemble resizes nothing
    case, m = C.by_name(name), model(name)
    sd = synthetic_state_dict(seed=6, num_in_ch=12, scale=4, num_block=2)
    up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(12, 3, num_block=2), tile=0, tile_pad=0, pre_pad=0, half=False,
                      device=cuda_device)
    img = synthetic_frame(14, 18, seed=5)[:, :, ::-1].copy()
    cfg = {"iterations": 1, "upscale_factor": 2.0}
    seen = {}

    def restated(frame):
        f = frame.cpu().numpy()
        y64 = R.upscale_float(case.sd, f, torch.float64, **case.cfg)
        y32 = R.upscale_float(case.sd, f, torch.float32, **case.cfg)
        seen["y64"], seen["tol"] = y64, 8 * float((y32.double() - y64).abs().max())
        return R.quantise(y64).to(frame.device)

    t_hip, t_ref = [], []
    calls = m.calls
    got = A.enhance_iterations(up, img, cfg, "cuda", trace=t_hip, extra_upscalers=[A.swin2sr_stage(m)])
    want = A.enhance_iterations(up, img, cfg, "cuda", trace=t_ref, extra_upscalers=[restated])
    assert m.calls == calls + 1 and t_hip[0]["ensemble_n"] == 2 and t_ref[0]["ensemble_n"] == 2
    assert got.shape == want.shape == (56, 72, 3) and got.dtype == np.uint8
    v = seen["y64"].clamp(0, 1) * 255.0
    firm = (((v - torch.floor(v)) - 0.5).abs() > 255.0 * seen["tol"]).numpy()
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(f"loop: {int((~firm).sum())} of {firm.size} samples thin, max |diff| {int(diff.max())}, {int((diff[firm] != 0).sum())} firm samples differ")
    assert int((diff[firm] != 0).sum()) == 0 and int(diff.max()) <= 1 and (~firm).sum() <= C.MAX_THIN * firm.size
    # upscaler=None: the only model
    t_only = []
    only = A.enhance_iterations(None, img, cfg, "cuda", trace=t_only, extra_upscalers=[A.swin2sr_stage(m)], device=cuda_device)
    assert t_only[0]["ensemble_n"] == 1 and np.array_equal(only, m.upscale(img).cpu().numpy())
