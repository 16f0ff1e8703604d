"""CPU: the filter entries of the C ABI (include/nesr_hip.h, csrc/filters_api.cpp) -- declared and exported, the host-side
tables equal to the imgproc.py functions they restate, and every argument error refused before any device is touched
(no GPU here: the library loads without one, as tests/test_cabi.py shows)."""
import ctypes

import numpy as np
import pytest

ENTRIES = ("nesr_lab_u8", "nesr_gaussian_u8", "nesr_gaussian_taps", "nesr_nl_means_weights", "nesr_preprocess_scratch_bytes",
           "nesr_preprocess_u8", "nesr_postprocess_u8")
ERR_ARG = -1
FAKE = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails its argument check first
FAKE2 = ctypes.c_void_p(0x2000)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import _lib
    return _lib.load()


def test_entries_declared_bound_and_exported(lib):
    from neural_enhanced_super_resolution_amd import _lib
    from tests.test_cabi import header_symbols
    syms = header_symbols()
    for s in ENTRIES:
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s)


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("template,search", [(7, 21), (5, 11), (3, 7)])
def test_nl_means_weights_equal_imgproc(lib, C, template, search):
    from neural_enhanced_super_resolution_amd import imgproc as P
    for h in np.arange(0.5, 10.01, 0.5):
        nb, sh = ctypes.c_int(), ctypes.c_int()
        assert lib.nesr_nl_means_weights(C, float(h), template, search, None, 0, ctypes.byref(nb), ctypes.byref(sh)) == 0
        table = (ctypes.c_int * nb.value)()
        assert lib.nesr_nl_means_weights(C, float(h), template, search, table, nb.value, ctypes.byref(nb), ctypes.byref(sh)) == 0
        want, shift = P.nl_means_weights(C, float(h), template, search)
        assert sh.value == shift and nb.value == want.numel()
        assert np.array_equal(np.frombuffer(table, np.int32), want.numpy()), h


def test_gaussian_taps_equal_imgproc(lib):
    from neural_enhanced_super_resolution_amd import imgproc as P
    cases = [(0.0, k) for k in range(1, 32, 2)] + [(s, 0) for s in (0.8, 1.0, 2.0, 3.0, 4.5)] + [(1.3, 9), (2.7, 31)]
    for sigma, ksize in cases:
        n = ctypes.c_int()
        taps = (ctypes.c_int * 31)()
        assert lib.nesr_gaussian_taps(sigma, ksize, taps, 31, ctypes.byref(n)) == 0
        assert list(taps[:n.value]) == P.gaussian_kernel_u8(sigma, ksize).tolist(), (sigma, ksize)
    assert lib.nesr_gaussian_taps(3.0, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 19     # size query


def test_preprocess_scratch_formula(lib):
    for h, w in ((1, 1), (18, 22), (64, 96), (1000, 1777), (8192, 8192)):
        planes = (3 * h * w + 255) // 256 * 256
        assert lib.nesr_preprocess_scratch_bytes(h, w) == 2 * planes + 8 * 8 * 256 * 4
    assert lib.nesr_preprocess_scratch_bytes(0, 5) == 0


def _refused(lib, rc, text):
    assert rc == ERR_ARG
    assert text in lib.nesr_last_error().decode()


def test_argument_errors_without_a_device(lib):
    n, sh = ctypes.c_int(), ctypes.c_int()
    _refused(lib, lib.nesr_lab_u8(0, FAKE, 4, 4, 16, FAKE2, None), "mode")
    _refused(lib, lib.nesr_lab_u8(0, FAKE, 0, 4, 0, FAKE2, None), "at least 1")
    _refused(lib, lib.nesr_lab_u8(0, FAKE, 4, 4, 8, FAKE, None), "in place")
    _refused(lib, lib.nesr_lab_u8(0, None, 4, 4, 0, FAKE2, None), "null")
    _refused(lib, lib.nesr_gaussian_u8(0, FAKE, 4, 4, 3, 0.0, 4, FAKE2, None), "odd")
    _refused(lib, lib.nesr_gaussian_u8(0, FAKE, 4, 4, 3, 0.0, 33, FAKE2, None), "at most 31")
    _refused(lib, lib.nesr_gaussian_u8(0, FAKE, 4, 4, 3, 6.0, 0, FAKE2, None), "too large")
    _refused(lib, lib.nesr_gaussian_u8(0, FAKE, 4, 4, 2, 2.0, 0, FAKE2, None), "C = 1 or 3")
    _refused(lib, lib.nesr_gaussian_u8(0, FAKE, 0, 4, 3, 2.0, 0, FAKE2, None), "H, W")
    _refused(lib, lib.nesr_gaussian_u8(0, FAKE, 4, 4, 3, 2.0, 0, FAKE, None), "in place")
    _refused(lib, lib.nesr_gaussian_taps(0.0, 2, None, 0, ctypes.byref(n)), "odd")
    for sigma in (-0.3, -1.0, -1e300):                        # round(6 sigma + 1) | 1 < 1: no kernel
        _refused(lib, lib.nesr_gaussian_taps(sigma, 0, None, 0, ctypes.byref(n)), "negative")
        _refused(lib, lib.nesr_gaussian_u8(0, FAKE, 4, 4, 3, sigma, 0, FAKE2, None), "negative")
    for sigma in (-0.1, -0.25):                               # round(0.4) | 1 = round(-0.5) | 1 = 1, as imgproc
        assert lib.nesr_gaussian_taps(sigma, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 1
    _refused(lib, lib.nesr_nl_means_weights(4, 5.0, 7, 21, None, 0, ctypes.byref(n), ctypes.byref(sh)), "channels")
    _refused(lib, lib.nesr_nl_means_weights(1, 0.0, 7, 21, None, 0, ctypes.byref(n), ctypes.byref(sh)), "positive")
    need = lib.nesr_preprocess_scratch_bytes(20, 30)
    _refused(lib, lib.nesr_preprocess_u8(0, FAKE, 20, 30, 0.5, FAKE2, need - 1, FAKE, None), "scratch")
    _refused(lib, lib.nesr_preprocess_u8(0, FAKE, 0, 30, 0.5, FAKE2, need, FAKE, None), "at least 1")
    _refused(lib, lib.nesr_preprocess_u8(0, FAKE, 20, 30, float("nan"), FAKE2, need, FAKE, None), "finite")
    _refused(lib, lib.nesr_postprocess_u8(0, FAKE, 20, 30, 1, FAKE, None), "in place")
    _refused(lib, lib.nesr_postprocess_u8(0, FAKE, 20, 0, 1, FAKE2, None), "at least 1")


def test_forced_hip_route_refuses_what_the_kernels_cannot_take():
    """use_hip=True on a CPU tensor, a wrong dtype or a wrong layout raises before any launch."""
    import torch
    from neural_enhanced_super_resolution_amd import imgproc as P
    img = torch.zeros((5, 6, 3), dtype=torch.uint8)
    for call in (lambda: P.rgb2lab_u8(img, use_hip=True), lambda: P.lab2rgb_u8(img, use_hip=True),
                 lambda: P.gaussian_blur_u8(img, 2.0, use_hip=True), lambda: P.preprocess_image(img, 0.5, use_hip=True),
                 lambda: P.postprocess_image(img, use_hip=True)):
        with pytest.raises(ValueError, match="HIP kernel takes"):
            call()
