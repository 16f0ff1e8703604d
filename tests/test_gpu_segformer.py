"""GPU: SegFormer-B0 on the HIP path (csrc/segformer.hip, segformer_pre.hip) against the float64 restatement of
tests/segformer_ref.py, which test_segformer_host.py pins to ``transformers`` and PIL.

Tolerance of the logits, per input: 8 x the max abs deviation of the restatement run in float32 on the CPU from the same
restatement in float64 (the f32 MFMA is an fmaf chain; another valid summation order lands at the same order of magnitude).
Class maps: equal to the float64 argmax wherever the float64 top-2 margin is at least twice that tolerance, the positions left out
at most 1 % of the map (test_segformer_host.py asserts that share for these seeds on the CPU).
"""
import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import SegFormer, imgproc
from neural_enhanced_super_resolution_amd.nesr_adapter import enhance_iterations
from neural_enhanced_super_resolution_amd.segformer import pil_resize_u8
from tests import segformer_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


def weights():
    if "sd" not in _cache:
        _cache["sd"] = R.seeded_state_dict(seed=R.WEIGHT_SEED)
    return _cache["sd"]


def model():
    if "model" not in _cache:
        m = SegFormer().to(DEV)
        m.load_state_dict(weights())
        _cache["model"] = m
    return _cache["model"]


def reference(x):
    """(float64 logits, tolerance = 8 x |float32 CPU - float64|) of pixel_values x, computed once per input."""
    with torch.no_grad():
        l64 = R.segformer_forward(weights(), x.double())
        l32 = R.segformer_forward(weights(), x)
    return l64, 8 * float((l32.double() - l64).abs().max())


def forward_case(h, w, seed):
    key = ("fwd", h, w, seed)
    if key not in _cache:
        x = R.seeded_input(h, w, seed=seed)
        l64, tol = reference(x)
        got = model()(x.to(DEV))
        torch.cuda.synchronize()
        _cache[key] = (x, l64, tol, got.cpu())
    return _cache[key]


def frame_case(h, w, seed):
    key = ("frame", h, w, seed)
    if key not in _cache:
        frame = R.seeded_frame(h, w, seed=seed)
        x = R.preprocess(frame)
        _cache[key] = (frame, x) + reference(x)
    return _cache[key]


@pytest.mark.parametrize("h,w,seed", R.FORWARD_CASES)
def test_logits_against_float64(h, w, seed):
    x, l64, tol, got = forward_case(h, w, seed)
    assert got.shape == l64.shape == (1, 150, h // 4, w // 4) and got.dtype == torch.float32
    err = float((got.double() - l64).abs().max())
    print(f"logits {h}x{w}: max |gpu - f64| = {err:.3e}, tolerance {tol:.3e} (8 x f32 CPU), ratio to f32 CPU {8 * err / tol:.2f}")
    assert torch.isfinite(got).all()
    assert err <= tol


@pytest.mark.parametrize("h,w,seed", R.FORWARD_CASES)
def test_argmax_of_logits_under_the_margin_rule(h, w, seed):
    x, l64, tol, got = forward_case(h, w, seed)
    excluded, wrong = R.check_class_map(got[0].argmax(dim=0), l64, tol, R.MAX_THIN)
    print(f"argmax {h}x{w}: {excluded} thin positions left out, {wrong} wrong")
    assert wrong == 0


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: "%dx%d-%dx%d-f%d" % c)
def test_pil_resize_bit_for_bit(case):
    h, w, oh, ow, flt = case
    img = R.seeded_frame(h, w, seed=h)
    want = R.pil_resize(img, oh, ow, flt)
    got = pil_resize_u8(torch.from_numpy(img).to(DEV), oh, ow, flt).cpu().numpy()
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"pil resize {w}x{h} -> {ow}x{oh} filter {flt}: {int((diff > 0).sum())} bytes differ, max {int(diff.max())}")
    assert got.shape == want.shape and np.array_equal(got, want)


def test_pil_resize_single_channel_and_same_size():
    img = R.seeded_frame(70, 90, seed=1)
    one = np.ascontiguousarray(img[:, :, :1])
    got = pil_resize_u8(torch.from_numpy(one).to(DEV), 33, 47, R.PIL_LANCZOS).cpu().numpy()
    assert np.array_equal(got, R.pil_resize(one, 33, 47, R.PIL_LANCZOS))
    same = pil_resize_u8(torch.from_numpy(img).to(DEV), 70, 90, R.PIL_BILINEAR).cpu().numpy()
    assert np.array_equal(same, img)
    with pytest.raises(Exception, match="filter"):
        pil_resize_u8(torch.from_numpy(img).to(DEV), 10, 10, 3)


@pytest.mark.parametrize("h,w,seed", R.FRAME_CASES + [(512, 512, 6), (512, 300, 7)])
def test_pixel_values(h, w, seed):
    frame = R.seeded_frame(h, w, seed=seed)
    want = R.preprocess(frame)
    got = model().pixel_values(torch.from_numpy(frame).to(DEV)).cpu()
    err = float((got - want).abs().max())
    print(f"pixel_values of a {w}x{h} frame: max abs diff {err:.3e}, range [{float(want.min()):.3f}, {float(want.max()):.3f}]")
    assert got.shape == want.shape == (1, 3, 512, 512)
    assert err <= 1e-6


@pytest.mark.parametrize("h,w,seed", R.FRAME_CASES)
def test_segment_end_to_end(h, w, seed):
    frame, x, l64, tol = frame_case(h, w, seed)
    m = model()
    calls = m.calls
    got = m.segment(torch.from_numpy(frame).to(DEV))
    assert got.shape == (128, 128) and got.dtype == torch.uint8 and got.is_cuda and m.calls == calls + 1
    excluded, wrong = R.check_class_map(got, l64, tol, R.MAX_THIN)
    print(f"segment {w}x{h}: {excluded} thin positions left out, {wrong} wrong, {len(torch.unique(got))} classes")
    assert wrong == 0
    assert torch.equal(m(torch.from_numpy(frame).to(DEV)), got)      # __call__ on a uint8 HWC frame is segment


def test_segment_is_the_argmax_of_forward_on_its_pixel_values():
    frame = torch.from_numpy(R.seeded_frame(140, 100, seed=4)).to(DEV)
    m = model()
    logits = m(m.pixel_values(frame))
    assert torch.equal(m.segment(frame).long(), logits[0].argmax(dim=0))      # the fused argmax: the same logits, the lowest index


def test_enhance_iterations_with_the_segmenter():
    frame = R.seeded_frame(96, 120, seed=8)
    m = model()
    dev_frame = torch.from_numpy(frame).to(DEV)
    enhanced = imgproc.segment_enhance(dev_frame, m.segment(dev_frame))
    want = imgproc.resize_u8(enhanced, 192, 240, imgproc.INTER_CUBIC)      # upscaler=None: the loop's bicubic step follows
    calls = m.calls
    trace = []
    got = enhance_iterations(None, dev_frame, config={"iterations": 1, "upscale_factor": 2.0}, segmenter=m, device=DEV, trace=trace)
    assert m.calls == calls + 1 and trace[0]["segmented"] is True
    assert isinstance(got, np.ndarray) and np.array_equal(got, want.cpu().numpy())
    mask = (m.segment(dev_frame) > 0)
    assert bool(mask.any())      # the stage did something: some pixel is an object, so segment_enhance sharpened there
    assert not torch.equal(enhanced, dev_frame)


def test_forward_twice_gives_the_same_bits():
    x = R.seeded_input(96, 160, seed=1).to(DEV)
    m = model()
    a = m(x).clone()
    b = m(x)
    assert torch.equal(a, b)
    frame = torch.from_numpy(R.seeded_frame(140, 100, seed=4)).to(DEV)
    assert torch.equal(m.segment(frame).clone(), m.segment(frame))


def test_one_context_at_two_sizes_in_turn():
    m = model()
    small = forward_case(64, 64, 0)
    ragged = forward_case(96, 160, 1)
    for x, _, _, first in (small, ragged, small, ragged):
        assert torch.equal(m(x.to(DEV)).cpu(), first)
    assert len(m._handles) == 1


def test_old_and_new_names_give_the_same_bits():
    x, _, _, first = forward_case(96, 160, 1)
    old = SegFormer().to(DEV)
    old.load_state_dict(R.to_old_names(weights()))
    assert torch.equal(old(x.to(DEV)).cpu(), first)


def test_launch_counter():
    m = SegFormer().to(DEV)
    m.load_state_dict(weights())
    m.set_kernel_timing(True)
    for (h, w), expected_pre in (((512, 512), 1), ((140, 100), 2), ((900, 1300), 4)):
        frame = torch.from_numpy(R.seeded_frame(h, w, seed=9)).to(DEV)
        m.segment(frame)
        t = m.kernel_time_ms()
        print(f"segment of a {w}x{h} frame: {t['launches']} launches, ms per group {dict((k, round(v, 3)) for k, v in t['groups'].items())}")
        assert t["launches"] <= 80
        assert t["launches"] == 47 + expected_pre      # 4 patch embeds, 8 blocks of 5 (4 without a reduction), 4 stage ends, 1 head
        assert all(v > 0 for v in t["groups"].values())
    m.set_kernel_timing(False)
    m.segment(frame)
    t = m.kernel_time_ms()
    assert t["launches"] == 51 and sum(t["groups"].values()) == 0.0      # the counter always runs; no events without timing


@pytest.mark.parametrize("shape", [(1, 3, 64, 80), (1, 3, 48, 64), (2, 3, 64, 64), (1, 4, 64, 64), (1, 3, 32, 16)])
def test_forward_refuses_other_shapes(shape):
    with pytest.raises(Exception, match="multiples of 32|expected \\[1, 3"):
        model()(torch.zeros(shape, device=DEV))


def test_c_entry_takes_the_published_checkpoint_names():
    """nesr_segformer_load_weight renames transformers-4 keys itself: a C host loads the published checkpoint as it is."""
    import ctypes

    from neural_enhanced_super_resolution_amd import _lib
    lib = _lib.load()
    n = R.B0["num_encoder_blocks"]
    arr = lambda name: (ctypes.c_int * n)(*R.B0[name])      # noqa: E731
    handle = ctypes.c_void_p()
    _lib.check(lib.nesr_segformer_create(ctypes.byref(handle), 0, 3, n, arr("depths"), arr("sr_ratios"), arr("hidden_sizes"), arr("patch_sizes"),
                                         arr("strides"), arr("num_attention_heads"), arr("mlp_ratios"), 256, 150), "nesr_segformer_create")
    try:
        assert lib.nesr_segformer_num_tensors(handle) == 207
        def load(key, t):
            t = t.to(torch.float32).contiguous()
            shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
            return lib.nesr_segformer_load_weight(handle, key.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim())
        old = R.to_old_names(weights())
        assert load("segformer.encoder.block.0.0.attention.self.nothing.weight", torch.zeros(1)) == _lib.ERR_ARG
        assert b"segformer.encoder.block.0.0.attention.self.nothing.weight" in lib.nesr_last_error()
        held = "segformer.encoder.block.2.1.attention.self.sr.weight"
        for key, t in old.items():
            if key != held:
                assert load(key, t) == 0, key
        assert lib.nesr_segformer_finalize(handle) != 0 and b"sequence_reduction.sequence_reduction.weight" in lib.nesr_last_error()
        assert load(held, old[held]) == 0 and lib.nesr_segformer_finalize(handle) == 0
        x, _, _, first = forward_case(64, 64, 0)
        xd = x.to(DEV)
        out = torch.empty((1, 150, 16, 16), dtype=torch.float32, device=DEV)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.nesr_segformer_forward_f32(handle, ctypes.c_void_p(xd.data_ptr()), 1, 3, 64, 64, ctypes.c_void_p(out.data_ptr()), stream),
                   "nesr_segformer_forward_f32")
        assert torch.equal(out.cpu(), first)
    finally:
        lib.nesr_segformer_destroy(handle)
