"""CPU: the resize entries of the C ABI (include/nesr_hip.h, csrc/resize_api.cpp) -- declared and exported, the host-side
coefficient tables equal to the imgproc.py functions and the oracle they restate, every argument error refused before any device
is touched (no GPU here: the library loads without one), and the Python route's refusals."""
import ctypes

import numpy as np
import pytest

ENTRIES = ("nesr_resize_u8", "nesr_resize_u16", "nesr_resize_f32", "nesr_resize_taps")
ERR_ARG = -1
LINEAR, LANCZOS4 = 1, 4
FAKE = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails its argument check first
FAKE2 = ctypes.c_void_p(0x2000)
# (n_in, n_out): the tiler's regions, the outscale cases of the 2160p frame, shrinking, enlarging, off by one, fewer samples than taps
AXES = [(2176, 1024), (2112, 1024), (544, 1024), (2160, 3780), (4320, 7560), (8640, 7560), (1000, 333), (333, 1000), (2048, 2047),
        (5, 17), (17, 5), (1, 7), (7, 1), (64, 64), (1080, 4320), (4320, 3240), (4320, 6480), (100, 101), (3, 8)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


def _taps(lib, n_in, n_out, interp):
    n = ctypes.c_int()
    assert lib.nesr_resize_taps(n_in, n_out, interp, None, None, 0, ctypes.byref(n)) == 0 and n.value == n_out     # size query
    first = (ctypes.c_int * n_out)()
    coef = (ctypes.c_float * (n_out * (16 if interp == LANCZOS4 else 2)))()
    assert lib.nesr_resize_taps(n_in, n_out, interp, first, coef, n_out, ctypes.byref(n)) == 0
    return np.frombuffer(first, np.int32).copy(), np.frombuffer(coef, np.float32).reshape(n_out, -1).copy()


def test_entries_declared_bound_and_exported(lib):
    from neural_enhanced_super_resolution_amd import _lib
    from tests.test_cabi import header_symbols
    syms = header_symbols()
    for s in ENTRIES:
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s)
    assert (_lib.INTER_LINEAR, _lib.INTER_LANCZOS4) == (LINEAR, LANCZOS4)


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_lanczos_taps_equal_imgproc_and_oracle(lib, n_in, n_out):
    import torch
    from neural_enhanced_super_resolution_amd import imgproc as P
    from oracle import cv2_ref
    first, coef = _taps(lib, n_in, n_out, LANCZOS4)
    idx, frac, i0 = P._axis_taps(n_in, n_out, torch.device("cpu"), 8, -3)
    assert np.array_equal(first, i0.numpy() - 3)
    assert np.array_equal(np.clip(first[:, None] + np.arange(8), 0, n_in - 1), idx.numpy())
    w = P._lanczos4_coeffs(frac)
    fixed = torch.round(w * 2048.0).clamp_(-32768, 32767).numpy()
    assert np.array_equal(coef[:, 8:], fixed)                                   # the 11-bit coefficients exactly
    want = np.array([cv2_ref._lanczos_weights(np.float32(f)) for f in frac.numpy()], np.float32)
    assert np.array_equal(coef[:, :8].view(np.uint32), want.view(np.uint32))    # the float32 ones bit for bit the oracle's


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_linear_taps_equal_imgproc(lib, n_in, n_out):
    import torch
    from neural_enhanced_super_resolution_amd import imgproc as P
    first, coef = _taps(lib, n_in, n_out, LINEAR)
    # linear_resize_f32 of the ramp 0, 1, .. n_in - 1 along one axis gives i0 (1 - f) + i1 f; compare the parts instead:
    pos = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).to(torch.float32)
    i0 = torch.floor(pos)
    f = pos - i0
    i0 = i0.long()
    lo, hi = i0 < 0, i0 >= n_in - 1
    f = torch.where(lo | hi, torch.zeros_like(f), f)
    i0 = torch.where(lo, torch.zeros_like(i0), torch.where(hi, torch.full_like(i0, n_in - 1), i0))
    i1 = (i0 + 1).clamp_(max=n_in - 1)
    assert np.array_equal(first, i0.numpy())
    assert np.array_equal(coef[:, 0].view(np.uint32), f.numpy().view(np.uint32))
    assert np.array_equal(first + coef[:, 1].astype(np.int64), i1.numpy())
    # and through the function itself: a one-row ramp
    ramp = torch.arange(n_in, dtype=torch.float32)[None, :]
    got = P.linear_resize_f32(ramp, 1, n_out, use_hip=False)[0].numpy()
    a, b = i0.numpy().astype(np.float32), i1.numpy().astype(np.float32)
    ff = f.numpy()
    assert np.array_equal(got, a * (np.float32(1) - ff) + b * ff)


def _refused(lib, rc, text):
    assert rc == ERR_ARG
    assert text in lib.nesr_last_error().decode(), lib.nesr_last_error().decode()


def test_argument_errors_without_a_device(lib):
    n = ctypes.c_int()
    for name, S, good, bad, bad_name in (("nesr_resize_u8", 1, LANCZOS4, LINEAR, "u8 with NESR_INTER_LINEAR"),
                                         ("nesr_resize_u16", 2, LANCZOS4, LINEAR, "u16 with NESR_INTER_LINEAR"),
                                         ("nesr_resize_f32", 4, LINEAR, LANCZOS4, "f32 with NESR_INTER_LANCZOS4")):
        fn = getattr(lib, name)
        sb, db = 10 * 3 * S, 20 * 3 * S
        _refused(lib, fn(0, None, 8, 10, 3, sb, FAKE2, 16, 20, db, good, None), "null")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, None, 16, 20, db, good, None), "null")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, FAKE2, 16, 20, db, bad, None), bad_name)
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, FAKE2, 16, 20, db, 2, None), "unknown interpolation (2)")       # INTER_CUBIC: not in scope
        for sizes in ((0, 10, 16, 20), (8, 0, 16, 20), (8, 10, 0, 20), (8, 10, 16, -1)):
            _refused(lib, fn(0, FAKE, sizes[0], sizes[1], 3, sb, FAKE2, sizes[2], sizes[3], db, good, None), "at least 1")
        for C in (0, 5, -3) + ((2,) if S < 4 else ()):
            _refused(lib, fn(0, FAKE, 8, 10, C, 10 * 8 * S, FAKE2, 16, 20, 20 * 8 * S, good, None), "channels")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb - S, FAKE2, 16, 20, db, good, None), "stride")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, FAKE2, 16, 20, db - S, good, None), "stride")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, FAKE, 16, 20, db, good, None), "in place")
        _refused(lib, fn(0, FAKE, 8, 10, 3, sb, FAKE, 8, 10, sb, good, None), "in place")                     # equal sizes copy, but not onto themselves
        if S > 1:
            _refused(lib, fn(0, ctypes.c_void_p(0x1001), 8, 10, 3, sb, FAKE2, 16, 20, db, good, None), "multiples of the sample size")
            _refused(lib, fn(0, FAKE, 8, 10, 3, sb + 1, FAKE2, 16, 20, db, good, None), "multiples of the sample size")
    _refused(lib, lib.nesr_resize_taps(0, 5, LANCZOS4, None, None, 0, ctypes.byref(n)), "sizes")
    _refused(lib, lib.nesr_resize_taps(5, 0, LINEAR, None, None, 0, ctypes.byref(n)), "sizes")
    _refused(lib, lib.nesr_resize_taps(5, 5, 2, None, None, 0, ctypes.byref(n)), "interp")
    _refused(lib, lib.nesr_resize_taps(5, 5, LINEAR, None, None, 0, None), "null")


def test_forced_hip_route_refuses_what_the_kernels_cannot_take():
    import torch
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = torch.zeros((5, 6, 3), dtype=torch.uint8)
    for call in (lambda: P.lanczos4_resize(img, 9, 9, use_hip=True), lambda: P.lanczos4_resize(img.int(), 9, 9, use_hip=True),
                 lambda: P.linear_resize_f32(img.float(), 9, 9, use_hip=True), lambda: P.linear_resize_f32(img.float()[:, :, 0], 9, 9, use_hip=True)):
        with pytest.raises(ValueError, match="HIP kernel takes"):
            call()
    with pytest.raises(ValueError, match="out must be"):
        P.lanczos4_resize(img, 9, 9, out=torch.zeros((9, 8, 3), dtype=torch.uint8))


def test_default_route_on_cpu_tensors_is_the_torch_chain():
    """use_hip=None on CPU tensors: today's values (the oracle's), also through out= a view of a canvas."""
    import torch
    from neural_enhanced_super_resolution_amd import imgproc as P
    from oracle import cv2_ref
    g = torch.Generator().manual_seed(11)
    for C in (1, 3, 4):
        a = torch.randint(0, 256, (13, 9, C), dtype=torch.uint8, generator=g)
        assert np.array_equal(P.lanczos4_resize(a, 7, 20).numpy(), cv2_ref.resize_lanczos4(a.numpy(), 7, 20))
    a = torch.randint(0, 256, (13, 9, 3), dtype=torch.uint8, generator=g)
    canvas = torch.full((12, 25, 3), 77, dtype=torch.uint8)
    r = P.lanczos4_resize(a[2:11, 1:8], 7, 20, out=canvas[3:10, 4:24])
    assert r.data_ptr() == canvas[3:10, 4:24].data_ptr()
    want = torch.full((12, 25, 3), 77, dtype=torch.uint8)
    want[3:10, 4:24] = torch.from_numpy(cv2_ref.resize_lanczos4(a[2:11, 1:8].contiguous().numpy(), 7, 20))
    assert torch.equal(canvas, want)
    b = torch.randint(0, 65536, (9, 8, 3), dtype=torch.int32, generator=g)
    got = P.lanczos4_resize(b, 14, 5).numpy()
    ref = cv2_ref.resize_lanczos4(b.numpy().astype(np.uint16), 14, 5).astype(np.int64)
    assert np.abs(got - ref).max() <= 1                                         # torch's sum order: tests/test_imgproc.py
    f = torch.rand((9, 11), generator=g)
    assert np.array_equal(P.linear_resize_f32(f, 5, 20).numpy(), cv2_ref.resize_linear_f32(f.numpy(), 5, 20))


def test_tiler_keyword_keeps_cpu_route():
    """process_with_tiling on CPU tensors: use_hip=None and use_hip=False are the same (present) code."""
    import torch
    from neural_enhanced_super_resolution_amd import nesr_adapter as A
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (40, 52, 3), dtype=torch.uint8, generator=g)

    def proc(t):
        t = torch.as_tensor(t)
        return t.repeat_interleave(4, 0).repeat_interleave(4, 1)

    a = A.process_with_tiling(proc, img, 16, 4, 2, torch.device("cpu"), as_numpy=False)
    b = A.process_with_tiling(proc, img, 16, 4, 2, torch.device("cpu"), as_numpy=False, use_hip=False)
    assert a.shape == (80, 104, 3) and torch.equal(a, b)
