"""CPU: the rest of enhance_image's loop (nesr/nesr.py:516-633) -- cv2's other 8-bit interpolations (nesr_resize_cv_u8,
imgproc.resize_u8), the mask stage (nesr_segment_enhance_u8, imgproc.segment_enhance) and the ensemble (nesr_ensemble_u8,
imgproc.ensemble_results): the C entries' refusals before any device is touched, the host tables, and the torch chains (the
specification of the kernels) on CPU tensors, bit for bit tests/cv2_stages_ref.py -- plus properties that need no restatement, so
that chain and restatement cannot be wrong in the same way.  No tolerance anywhere but the one stated for the cubic ramp."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cv2_stages_ref as R

ERR_ARG = -1
NEAREST, LINEAR, CUBIC, LANCZOS4 = 0, 1, 2, 4
INTERPS = (NEAREST, LINEAR, CUBIC, LANCZOS4)
FAKE = ctypes.c_void_p(0x1000)          # never dereferenced: every call that gets one fails its argument check first
FAKE2 = ctypes.c_void_p(0x2000)
FAKE3 = ctypes.c_void_p(0x3000)
FAKE4 = ctypes.c_void_p(0x4000)
AXES = [(1, 1), (1, 7), (7, 1), (5, 5), (8, 4), (37, 11), (11, 37), (64, 128), (1000, 1777)]
# 16x24 -> 8x12: both axes halve, cv2's area switch; 16x24 -> 8x13: one axis only, no switch
SHAPES = [((1, 1), (3, 5)), ((2, 3), (5, 7)), ((37, 41), (11, 13)), ((16, 24), (8, 12)), ((16, 24), (8, 13))]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


def _img(h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (h, w, c), dtype=torch.uint8, generator=g)


def _refused(lib, rc, text):
    assert rc == ERR_ARG
    assert text in lib.nesr_last_error().decode(), lib.nesr_last_error().decode()


def test_entries_declared_bound_and_exported(lib):
    from neural_enhanced_super_resolution_amd import _lib, imgproc as P
    from tests.test_cabi import header_symbols
    syms = header_symbols()
    for s in ("nesr_resize_cv_u8", "nesr_resize_cv_taps", "nesr_segment_enhance_scratch_bytes", "nesr_segment_enhance_u8", "nesr_ensemble_u8"):
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s)
    assert (_lib.INTER_NEAREST, _lib.INTER_LINEAR, _lib.INTER_CUBIC, _lib.INTER_LANCZOS4) == INTERPS
    assert (P.INTER_NEAREST, P.INTER_LINEAR, P.INTER_CUBIC, P.INTER_LANCZOS4) == INTERPS


def test_resize_cv_refusals_without_a_device(lib):
    fn = lib.nesr_resize_cv_u8
    sb, db = 10 * 3, 20 * 3
    for interp in (3, 5, -1, 6):
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, FAKE2, 16, 20, db, interp, None), f"interpolation {interp}")
    for good in INTERPS:
        _refused(lib, fn(0, FAKE, 8, 10, 2, 10 * 8, FAKE2, 16, 20, 20 * 8, good, None), "channels")
        _refused(lib, fn(0, None, 8, 10, 3, sb, FAKE2, 16, 20, db, good, None), "null")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, None, 16, 20, db, good, None), "null")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb - 1, FAKE2, 16, 20, db, good, None), "stride")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, FAKE2, 16, 20, db - 1, good, None), "stride")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, FAKE, 16, 20, db, good, None), "in place")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, FAKE, 8, 10, sb, good, None), "in place")      # equal sizes copy, but not onto themselves
        _refused(lib, fn(0, FAKE, 0, 10, 3, sb, FAKE2, 16, 20, db, good, None), "at least 1")
    n = ctypes.c_int()
    _refused(lib, lib.nesr_resize_cv_taps(5, 5, 3, None, None, 0, ctypes.byref(n)), "interp")
    _refused(lib, lib.nesr_resize_cv_taps(0, 5, CUBIC, None, None, 0, ctypes.byref(n)), "sizes")
    _refused(lib, lib.nesr_resize_cv_taps(5, 5, CUBIC, None, None, 0, None), "null")


def test_old_entries_keep_their_refusals(lib):
    """nesr_resize_u8 still takes Lanczos-4 only, in the words it used."""
    _refused(lib, lib.nesr_resize_u8(0, FAKE, 8, 10, 3, 30, FAKE2, 16, 20, 60, LINEAR, None), "u8 with NESR_INTER_LINEAR")
    _refused(lib, lib.nesr_resize_u8(0, FAKE, 8, 10, 3, 30, FAKE2, 16, 20, 60, CUBIC, None), "unknown interpolation (2)")
    _refused(lib, lib.nesr_resize_u8(0, FAKE, 8, 10, 3, 30, FAKE2, 16, 20, 60, NEAREST, None), "unknown interpolation (0)")


def test_ensemble_and_segment_refusals_without_a_device(lib):
    ptrs = (ctypes.c_void_p * 9)(*[0x1000 * (i + 1) for i in range(9)])
    out = ctypes.c_void_p(0xA000)
    _refused(lib, lib.nesr_ensemble_u8(0, ptrs, 0, 4, 4, 3, out, None), "0 images")
    _refused(lib, lib.nesr_ensemble_u8(0, ptrs, 9, 4, 4, 3, out, None), "9 images")
    _refused(lib, lib.nesr_ensemble_u8(0, None, 2, 4, 4, 3, out, None), "null")
    _refused(lib, lib.nesr_ensemble_u8(0, ptrs, 2, 4, 4, 3, None, None), "null")
    _refused(lib, lib.nesr_ensemble_u8(0, ptrs, 2, 0, 4, 3, out, None), "at least 1")
    holes = (ctypes.c_void_p * 2)(0x1000, None)
    _refused(lib, lib.nesr_ensemble_u8(0, holes, 2, 4, 4, 3, out, None), "null image")
    need = lib.nesr_segment_enhance_scratch_bytes(33, 47)
    assert need == 1792 and need >= 33 * 47 and lib.nesr_segment_enhance_scratch_bytes(0, 5) == 0
    seg = lib.nesr_segment_enhance_u8
    _refused(lib, seg(0, FAKE, 33, 47, FAKE2, 4, 4, FAKE3, need - 1, FAKE4, None), "scratch")
    _refused(lib, seg(0, FAKE, 33, 47, FAKE2, 4, 4, FAKE3, need, FAKE, None), "in place")
    _refused(lib, seg(0, FAKE, 33, 47, None, 4, 4, FAKE3, need, FAKE4, None), "null")
    _refused(lib, seg(0, FAKE, 33, 47, FAKE2, 4, 4, None, need, FAKE4, None), "null")
    _refused(lib, seg(0, FAKE, 33, 47, FAKE2, 0, 4, FAKE3, need, FAKE4, None), "at least 1")


def _cv_taps(lib, n_in, n_out, interp, per):
    n = ctypes.c_int()
    assert lib.nesr_resize_cv_taps(n_in, n_out, interp, None, None, 0, ctypes.byref(n)) == 0 and n.value == n_out     # size query
    first = (ctypes.c_int * n_out)()
    coef = (ctypes.c_int * (n_out * per))()
    assert lib.nesr_resize_cv_taps(n_in, n_out, interp, first, coef, n_out, ctypes.byref(n)) == 0
    return np.frombuffer(first, np.int32).astype(np.int64), np.frombuffer(coef, np.int32).reshape(n_out, per).astype(np.int64)


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_cv_taps_equal_the_restatement_and_the_chain(lib, n_in, n_out):
    from neural_enhanced_super_resolution_amd import imgproc as P
    for interp, per in ((NEAREST, 1), (LINEAR, 2), (CUBIC, 4)):
        first, coef = _cv_taps(lib, n_in, n_out, interp, per)
        rf, rc = R.axis_table(n_in, n_out, interp)
        assert np.array_equal(first, rf) and np.array_equal(coef, rc), (interp, n_in, n_out)
        pf, pc = P.resize_u8_tables(n_in, n_out, interp)
        assert np.array_equal(first, pf.numpy()) and np.array_equal(coef, pc.numpy())
    first, coef = _cv_taps(lib, n_in, n_out, LANCZOS4, 8)                        # interp 4: the Lanczos form's own 11-bit table
    pf, pc = P.resize_u8_tables(n_in, n_out, LANCZOS4)
    assert np.array_equal(first, pf.numpy()) and np.array_equal(coef, pc.numpy())


@pytest.mark.parametrize("src,dst", SHAPES)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_chain_equals_the_restatement(src, dst, C):
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(src[0], src[1], C, seed=src[0] * 100 + dst[1] + C)
    for interp in (NEAREST, LINEAR, CUBIC):
        got = P.resize_u8(img, dst[0], dst[1], interp).numpy()                   # a CPU tensor: the chain
        assert np.array_equal(got, R.resize(img.numpy(), dst[0], dst[1], interp)), interp
    assert torch.equal(P.resize_u8(img, dst[0], dst[1], LANCZOS4), P.lanczos4_resize(img, dst[0], dst[1], use_hip=False))


def test_area_switch_needs_both_axes():
    """16x24 -> 8x12 is the 2x2 mean, rounded once; with one axis halved only, the linear form's two truncating passes remain."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(16, 24, 3, seed=8)
    x = img.to(torch.int64)
    mean = ((x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2] + 2) >> 2).to(torch.uint8)
    assert torch.equal(P.resize_u8(img, 8, 12, LINEAR), mean)
    one_axis = P.resize_u8(img, 8, 24, LINEAR)                                    # rows halve, columns stay: the linear form
    assert np.array_equal(one_axis.numpy(), R.resize(img.numpy(), 8, 24, LINEAR))


def test_properties_without_a_restatement():
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(9, 7, 3, seed=2)
    flat = torch.full((6, 5, 3), 201, dtype=torch.uint8)
    for interp in INTERPS:
        for oh, ow in ((13, 4), (3, 11), (12, 10), (3, 2)):
            assert (P.resize_u8(flat, oh, ow, interp) == 201).all(), (interp, oh, ow)          # a constant stays constant
        assert torch.equal(P.resize_u8(img, 9, 7, interp), img)                               # equal sizes return the input
    up = P.resize_u8(img, 18, 14, NEAREST)
    assert torch.equal(up, img.repeat_interleave(2, 0).repeat_interleave(2, 1))               # nearest x2: every pixel 2 x 2
    # cubic x2 of the ramp 3 x: the Keys kernel reproduces a linear function, so away from the replicated border the output is the
    # ramp at the sample positions (d + 0.5) / 2 - 0.5, within 1 LSB (the 11-bit coefficients and the two roundings)
    w = 40
    ramp = (torch.arange(w) * 3).to(torch.uint8)[None, :, None].expand(6, w, 1).contiguous()
    got = P.resize_u8(ramp, 12, 2 * w, CUBIC)[:, :, 0].to(torch.int64)
    pos = (torch.arange(2 * w, dtype=torch.float64) + 0.5) / 2 - 0.5
    want = torch.round(pos * 3).to(torch.int64)
    inner = slice(4, 2 * w - 4)                                                               # taps that never touch the two border columns
    assert (got[:, inner] - want[None, inner]).abs().max() <= 1
    g = torch.Generator().manual_seed(5)
    for shape, out in (((4, 4), (33, 47)), ((18, 33), (70, 130)), ((64, 64), (32, 32)), ((50, 40), (7, 9))):
        m = (torch.rand(shape, generator=g) > 0.5).to(torch.uint8)[:, :, None]
        r = P.resize_u8(m, out[0], out[1], LINEAR)
        assert int(r.max()) <= 1, (shape, out)                                                # linear of {0, 1} yields only {0, 1}


def test_resize_u8_refuses_what_it_cannot_take():
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(5, 6, 3, seed=1)
    with pytest.raises(ValueError, match="interpolation 3"):
        P.resize_u8(img, 9, 9, 3)
    with pytest.raises(ValueError, match="HIP kernel takes"):
        P.resize_u8(img, 9, 9, CUBIC, use_hip=True)                                           # a CPU tensor
    with pytest.raises(ValueError, match="uint8"):
        P.resize_u8(img.float(), 9, 9, CUBIC)
    with pytest.raises(ValueError, match="out must be"):
        P.resize_u8(img, 9, 9, CUBIC, out=torch.zeros((9, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="no entry for it alone"):
        P.dilate3x3_u8(torch.zeros((3, 3), dtype=torch.uint8), use_hip=True)
    canvas = torch.full((12, 14, 3), 0xA5, dtype=torch.uint8)
    r = P.resize_u8(img, 7, 9, CUBIC, out=canvas[2:9, 3:12])
    assert r.data_ptr() == canvas[2:9, 3:12].data_ptr() and torch.equal(canvas[2:9, 3:12], P.resize_u8(img, 7, 9, CUBIC))
    canvas[2:9, 3:12] = 0xA5
    assert (canvas == 0xA5).all()


def test_dilate_equals_the_restatement():
    from neural_enhanced_super_resolution_amd import imgproc as P
    g = torch.Generator().manual_seed(4)
    for shape in ((1, 1), (1, 6), (5, 1), (7, 9)):
        m = (torch.rand(shape, generator=g) > 0.8).to(torch.uint8)
        assert np.array_equal(P.dilate3x3_u8(m).numpy(), R.dilate3x3(m.numpy()))
    one = torch.zeros((5, 5), dtype=torch.uint8)
    one[0, 4] = 1
    want = torch.zeros((5, 5), dtype=torch.uint8)
    want[0:2, 3:5] = 1
    assert torch.equal(P.dilate3x3_u8(one), want)


def test_ensemble_float32_recipe():
    from neural_enhanced_super_resolution_amd import imgproc as P
    ramp = torch.arange(256, dtype=torch.uint8).reshape(16, 16, 1)
    assert P.ensemble_results([ramp]) is ramp                                                 # n = 1: the image as it is
    got = P.ensemble_results([ramp, ramp.clone(), ramp.clone()])
    below = int((got.to(torch.int64) == ramp.to(torch.int64) - 1).sum())
    print(f"three copies of 0..255: {below} values come out one below the input, {int((got == ramp).sum())} equal")
    assert np.array_equal(got.numpy(), R.ensemble_mean([ramp.numpy()] * 3))
    for n in (2, 5, 7, 8):
        imgs = [_img(9, 11, 3, seed=20 + n + k) for k in range(n)]
        assert np.array_equal(P.ensemble_results(imgs).numpy(), R.ensemble_mean([i.numpy() for i in imgs])), n


def test_ensemble_aligns_to_the_tuple_max():
    """max over (h, w) tuples is lexicographic: (12, 8) beats (10, 20), the width 20 is NOT kept."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    a, b, c = _img(10, 20, 3, seed=1), _img(12, 8, 3, seed=2), _img(12, 6, 3, seed=3)
    assert R.ensemble_target([a.shape, b.shape, c.shape]) == (12, 8)
    got = P.ensemble_results([a, b, c])
    assert tuple(got.shape) == (12, 8, 3)
    aligned = [P.lanczos4_resize(a, 12, 8, use_hip=False).numpy(), b.numpy(), P.lanczos4_resize(c, 12, 8, use_hip=False).numpy()]
    assert np.array_equal(got.numpy(), R.ensemble_mean(aligned))
    with pytest.raises(ValueError, match="no image"):
        P.ensemble_results([])


def test_segment_enhance_cpu():
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(33, 47, 3, seed=6)
    sharp = torch.from_numpy(R.add_weighted_unsharp(img.numpy(), R.gaussian_blur_sigma3(img.numpy())))
    assert torch.equal(sharp, torch.round(img.float() * 1.5 - P.gaussian_blur_u8(img, 3.0, use_hip=False).float() * 0.5).clamp(0, 255).to(torch.uint8))
    assert torch.equal(P.segment_enhance(img, torch.zeros((4, 4), dtype=torch.int64)), img)   # nothing segmented: the input
    assert torch.equal(P.segment_enhance(img, np.full((4, 4), 7, np.int32)), sharp)           # everything: the sharpened frame
    assert not torch.equal(sharp, img)
    seg = np.zeros((4, 4), np.int64)
    seg[1, 2] = 150                                                                            # one positive cell
    got = P.segment_enhance(img, seg)
    assert np.array_equal(got.numpy(), R.segment_and_enhance(img.numpy(), seg))
    changed = (got != img).any(-1)
    assert changed.any() and not changed.all()
    with pytest.raises(ValueError, match="integer"):
        P.segment_enhance(img, torch.zeros((4, 4)))


def test_segment_enhance_large_frame_takes_the_nearest_step():
    """Above 1024 pixels a side the class map is resized with INTER_NEAREST (nesr/nesr.py:720-724), done on the mask; the stage runs
    (the reference's own call throws on its int64 map and skips it)."""
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = _img(1, 1030, 3, seed=7)
    seg = torch.zeros((1, 103), dtype=torch.int64)
    seg[0, 50:60] = 3
    got = P.segment_enhance(img, seg)
    mask = torch.from_numpy(R.dilate3x3(R.resize((seg.numpy() > 0).astype(np.uint8)[:, :, None], 1, 1030, NEAREST)[:, :, 0]))
    sharp = P.segment_enhance(img, torch.ones((1, 1), dtype=torch.int64))
    assert torch.equal(got, torch.where((mask == 1)[..., None], sharp, img)) and not torch.equal(got, img)


class _Up:
    """Minimal stand-in for a RealESRGANer, as tests/test_nesr_adapter.py's: the adapter touches only .model and .device."""

    def __init__(self, model):
        self.model, self.device = model, torch.device("cpu")


class _Net(torch.nn.Module):
    """A 12-channel x4 'network': nearest x4 of the first three input channels."""

    def forward(self, x):
        return x[:, :3].repeat_interleave(4, 2).repeat_interleave(4, 3)


def test_loop_without_a_model_is_the_cubic_step():
    from neural_enhanced_super_resolution_amd import imgproc as P, nesr_adapter as A
    img = _img(7, 9, 3, seed=9)
    trace = []
    got = A.enhance_iterations(None, img.numpy(), {"iterations": 2, "upscale_factor": 1.5}, trace=trace, device="cpu")
    step1 = P.resize_u8(img, 10, 13, CUBIC)                                                    # (int(9 x 1.5), int(7 x 1.5)) = (13, 10)
    step2 = P.resize_u8(step1, 15, 19, CUBIC)
    assert isinstance(got, np.ndarray) and np.array_equal(got, step2.numpy())
    assert [(t["iteration"], t["ensemble_n"], t["segmented"], t["model_calls"], t["out_shape"]) for t in trace] == \
        [(0, 0, False, 0, (10, 13)), (1, 0, False, 0, (15, 19))]
    assert np.array_equal(got, R.resize(R.resize(img.numpy(), 10, 13, CUBIC), 15, 19, CUBIC))


def test_loop_with_segmenter_and_extra_upscaler():
    from neural_enhanced_super_resolution_amd import imgproc as P, nesr_adapter as A
    img = _img(6, 8, 3, seed=10)
    up = _Up(_Net())
    seen = []

    def segmenter(frame):
        seen.append(tuple(frame.shape))
        return (frame[:, :, 0] > 128).to(torch.int64)

    def extra(frame):
        return P.resize_u8(frame, frame.shape[0] * 4, frame.shape[1] * 4 - 2, NEAREST)         # another size: aligned by Lanczos

    cfg = {"iterations": 1}
    plain_trace, trace = [], []
    plain = A.enhance_iterations(up, img.numpy(), cfg, trace=plain_trace)
    got = A.enhance_iterations(up, img.numpy(), cfg, trace=trace, segmenter=segmenter, extra_upscalers=[extra, lambda f: None])
    assert "segmented" not in plain_trace[0] and "ensemble_n" not in plain_trace[0]            # the defaults: today's trace
    assert seen == [(6, 8, 3)] and trace[0]["segmented"] is True and trace[0]["ensemble_n"] == 2 and trace[0]["out_shape"] == (24, 32)
    assert trace[0]["tiled"] is False and trace[0]["iteration"] == 0
    seg = P.segment_enhance(img, segmenter(img))
    esr = torch.from_numpy(A.enhance_iterations(up, seg.numpy(), cfg))
    assert np.array_equal(got, P.ensemble_results([esr, extra(seg)]).numpy())
    assert plain.shape == got.shape == (24, 32, 3) and not np.array_equal(plain, got)
    only = A.enhance_iterations(up, img.numpy(), cfg, extra_upscalers=[lambda f: None])        # a model that gave nothing: one result
    assert np.array_equal(only, plain)
