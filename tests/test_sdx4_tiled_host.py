"""The x4 diffusion stage over windows without a GPU: the host entries nesr_sdx4_tile_plan and nesr_sdx4_tiled_workspace_bytes
against the package's twin (_tiling.sdx4_tile_plan) and the specification (tests/sdx4_tiled_ref.py); the normaliser against the
brute-force weight sum; every named fault of the specification against a case tests/test_gpu_sdx4_tiled_kernels.py runs on the
device; the crafted tiled pipeline's float32 restatement against float64; the refusals that need no device.

The tolerance of a case is the project's rule, 8 x max |float32 CPU restatement - float64|, computed here; a fault has to exceed
10 x that (DESIGN section 21's bar) in the case FAULT_CASES names for it.

The tests of the normaliser, of the faults and of the crafted float32 restatement check the specification itself (tests/
sdx4_tiled_ref.py): they are what gives the device tests' reference and tolerances their standing, and they need nothing of the
library.  The tests that need the feature are those of nesr_sdx4_tile_plan and its twin, of the refusals and of the workspace query.

The share recorded for the crafted tiled frame (24 x 40, tile 16, overlap 8, 3 steps; float32 CPU restatement against float64,
printed by test_thin_samples_of_the_tiled_frame_stay_under_the_cap) stands in that test's docstring; the cap is 2 %."""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import _lib, _tiling
from tests import sdx4_cases as C
from tests import sdx4_tiled_ref as T
from tests import vae_ref as VR
from tests.swin2sr_ref import u8_check


@pytest.fixture(scope="module", autouse=True)
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


# (h, w, multiple, tile, overlap): n = t on both axes and on one; an off-stride last window; overlap 0; the device's plans; the
# published multiple; a frame above the VAE's limit
SHAPES = ((8, 8, 2, 8, 0), (16, 24, 2, 32, 0), (16, 24, 2, 16, 8), (12, 22, 2, 8, 2), (8, 24, 2, 8, 4), (40, 16, 2, 16, 8), (8, 22, 2, 6, 4), (24, 40, 2, 16, 8),
          (24, 40, 2, 16, 0), (30, 50, 2, 16, 6), (264, 256, 8, 64, 8), (512, 512, 8, 128, 16), (512, 512, 8, 256, 32), (256, 2048, 8, 256, 248))


def c_plan(lib, h, w, multiple, tile, overlap):
    counts = [ctypes.c_int(0) for _ in range(4)]
    assert lib.nesr_sdx4_tile_plan(h, w, multiple, tile, overlap, *counts, None, 0) == 0, lib.nesr_last_error()
    ky, kx, ty, tx = (c.value for c in counts)
    rows = (ctypes.c_int32 * (2 * ky * kx))()
    assert lib.nesr_sdx4_tile_plan(h, w, multiple, tile, overlap, *counts, rows, len(rows)) == 0, lib.nesr_last_error()
    return (ky, kx), (ty, tx), [(rows[2 * i], rows[2 * i + 1]) for i in range(ky * kx)]


@pytest.mark.parametrize("shape", SHAPES)
def test_the_three_plans_agree(lib, shape):
    h, w, multiple, tile, overlap = shape
    want = T.plan(h, w, tile, overlap)
    assert c_plan(lib, *shape) == want and _tiling.sdx4_tile_plan(*shape) == want
    (ky, kx), (ty, tx), rows = want
    assert rows[0] == (0, 0) and rows[-1] == (h - ty, w - tx) and len(rows) == ky * kx and rows == sorted(rows)
    covered = np.zeros((h, w), dtype=bool)
    for y, x in rows:
        assert 0 <= y <= h - ty and 0 <= x <= w - tx and y % multiple == 0 and x % multiple == 0
        covered[y:y + ty, x:x + tx] = True
    assert covered.all()


def test_an_off_stride_last_window_and_an_origin_2_mod_4():
    (_, kx), (_, tx), rows = T.plan(12, 22, 8, 2)
    xs = [x for y, x in rows if y == 0]
    assert xs == [0, 6, 12, 14] and (xs[-1] - xs[-2]) != tx - 2 and {x % 4 for x in xs} == {0, 2}
    assert _tiling.overlap_axis(22, 8, 2) == xs      # the axis is Swin2SR's, shared


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] * s[1] <= 4096])
@pytest.mark.parametrize("scale", [1, 4])
def test_the_normaliser_is_positive_and_the_brute_force_sum(shape, scale):
    h, w, _, tile, overlap = shape
    s, brute = T.normaliser(h, w, tile, overlap, scale), T.brute_force_sum(h, w, tile, overlap, scale)
    assert s.shape == (h * scale, w * scale) and float(s.min()) > 0 and float(np.abs(s - brute).max()) <= 1e-12
    # the twin's fractions are the specification's weights
    ty = min(tile, h)
    for a in T.axis_starts(h, ty, overlap):
        got = [k / r for k, r in (_tiling.blend_axis_weight(i, a, ty, h, overlap) for i in range(a, a + ty))]
        assert np.array_equal(np.array(got), T.axis_weight(h, ty, a, overlap))


# fault -> ("chain" | "blend", plan): a case of tests/test_gpu_sdx4_tiled_kernels.py in which it exceeds 10 x the tolerance
FAULT_CASES = {"uniform_weights": ("chain", T.PLANS[1]), "ramp_on_frame_edge": ("chain", T.PLANS[4]), "last_window_on_stride": ("chain", T.PLANS[2]),
               "normalise_by_count": ("chain", T.PLANS[3]), "normalise_by_sy_only": ("chain", T.PLANS[2]), "acc_not_cleared": ("chain", T.PLANS[3]),
               "image_from_origin_0": ("chain", T.PLANS[2]), "window_stride_as_plane_stride": ("chain", T.PLANS[1]), "output_ramp_unscaled": ("blend", T.BLEND_PLANS[1])}
_cases = {}


def case(kind, plan, n=2):
    """(float64 result, tol, run(fault)) of a device case, computed once."""
    key = (kind, plan, n)
    if key not in _cases:
        h, w, tile, overlap = plan
        if kind == "chain":
            frame = T.chain_case(h, w, T.PLANS.index(plan), False)
            run = lambda dtype=np.float64, fault=None: T.chain(frame, h, w, tile, overlap, n, 2, False, dtype, fault)
        else:
            samples = T.blend_case(h, w, tile, overlap, T.PLANS.index(plan))
            run = lambda dtype=np.float64, fault=None: T.blend_chain(samples, h, w, tile, overlap, dtype, fault)
        want = run()
        _cases[key] = (want, 8.0 * float(np.abs(run(np.float32).astype(np.float64) - want).max()), run)
    return _cases[key]


def test_every_fault_has_a_case():
    assert set(FAULT_CASES) == set(T.FAULTS)


@pytest.mark.parametrize("fault", T.FAULTS)
def test_fault_exceeds_ten_tolerances_of_a_device_case(fault):
    kind, plan = FAULT_CASES[fault]
    want, tol, run = case(kind, plan)
    err = float(np.abs(run(np.float64, fault) - want).max())
    print(f"{fault}: {kind} {plan}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.0f}")
    assert 0 < tol < 1e-3 and err > 10.0 * tol


@pytest.mark.parametrize("fault", ["uniform_weights", "last_window_on_stride", "normalise_by_count", "acc_not_cleared", "image_from_origin_0"])
def test_fault_fails_the_crafted_tiled_loop(fault):
    """The same faults in the windowed loop on the real UNet restatement: the final latents of the crafted tiled call."""
    lat64, _, tol, _, _ = T.reference()
    frame, noise, latents = T.crafted()
    with torch.no_grad():
        text = T.TR.forward(C.models()["text"][0], C.ids(), torch.float64, **C.TEXT)
    # the last window of the crafted plan is on the stride: that fault is run on a 24 x 36 crop, against its own reference
    if fault == "last_window_on_stride":
        frame, noise, latents = frame[:, :36], noise[:, :, :36], latents[:, :, :36]
        args = (C.models()["unet"], frame, text, noise, latents, C.NOISE_LEVEL, T.STEPS, C.GUIDANCE, T.TILE, T.OVERLAP)
        lat64 = T.loop(*args)
        tol = 8.0 * float((T.loop(*args, torch.float32).double() - lat64).abs().max())
    bad = T.loop(C.models()["unet"], frame, text, noise, latents, C.NOISE_LEVEL, T.STEPS, C.GUIDANCE, T.TILE, T.OVERLAP, torch.float64, fault)
    err = float((bad - lat64).abs().max())
    print(f"{fault}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.0f}")
    assert err > 10.0 * tol


@pytest.mark.parametrize("guidance", [C.GUIDANCE, 1.0])
def test_thin_samples_of_the_tiled_frame_stay_under_the_cap(guidance):
    """Recorded: guidance 7.5: 197 of 46080 samples thin (0.43 %), 0 wrong; guidance 1.0: 72 thin (0.16 %), 0 wrong."""
    lat64, y64, tol_lat, tol, y32 = T.reference(guidance)
    excluded, wrong, n = u8_check(VR.quantise(y32), y64, tol)
    clamped = float(((y64 <= 0) | (y64 >= 1)).double().mean())
    print(f"guidance {guidance}: latents tol {tol_lat:.3e}, frame tol {tol:.3e}, {excluded} of {n} samples thin ({100.0 * excluded / n:.2f} %), {wrong} wrong (f32 CPU), "
          f"{100 * clamped:.1f} % on the clamp, latents std {float(lat64.std()):.3f}")
    assert tuple(y64.shape) == (4 * T.H, 4 * T.W, 3) and excluded <= C.MAX_THIN * n and wrong == 0 and tol_lat > 0
    assert clamped < 0.5 and float(y64.std()) > 0.02      # an image, not a constant


def test_one_window_is_the_untiled_specification():
    noise, latents = C.draws()
    args = (C.models(), C.frame(), C.ids(), noise, latents, C.NOISE_LEVEL, 2, C.GUIDANCE)
    lat, y = T.upscale(*args, 32, 0)
    lat0, y0 = T.R.upscale(*args)
    assert torch.equal(lat, lat0) and float((y - y0).abs().max()) < 1e-12


def test_what_the_host_entries_refuse(lib):
    counts = [ctypes.c_int(0) for _ in range(4)]
    for args, match in (((24, 40, 2, 15, 0), "tile must be a positive multiple of 2, got 15"), ((24, 40, 2, 0, 0), "tile must be"), ((24, 40, 2, 16, 16), "tile_overlap must be"),
                        ((24, 40, 2, 16, 7), "tile_overlap must be a multiple of 2"), ((24, 40, 2, 16, -2), "got -2"), ((23, 40, 2, 16, 8), "multiples of 2"),
                        ((512, 512, 8, 512, 0), "a window of 512 x 512 exceeds NESR_VAE_MAX_TOKENS"), ((4096, 2048, 8, 128, 0), "2^22"), ((24, 40, 1, 16, 8), "frame multiple")):
        assert lib.nesr_sdx4_tile_plan(*args, *counts, None, 0) == _lib.ERR_ARG and match in lib.nesr_last_error().decode(), (args, lib.nesr_last_error())
        if "2^22" not in match:      # the twin has no frame cap of its own
            with pytest.raises(ValueError):
                _tiling.sdx4_tile_plan(*args)
    rows = (ctypes.c_int32 * 16)()
    assert lib.nesr_sdx4_tile_plan(24, 40, 2, 16, 8, *counts, rows, 15) == _lib.ERR_ARG and "capacity" in lib.nesr_last_error().decode()
    assert lib.nesr_sdx4_tile_plan(24, 40, 2, 16, 8, None, *counts[1:], rows, 16) == _lib.ERR_ARG


def test_the_workspace_grows_with_the_frame_and_the_window(lib):
    def size(n, h, w, tile, overlap, vae_tile=0, vae_overlap=-1):
        out = ctypes.c_size_t(0)
        assert lib.nesr_sdx4_tiled_workspace_bytes(n, 4, 32, 4, h, w, C.TOKENS, 2, tile, overlap, vae_tile, vae_overlap, ctypes.byref(out)) == 0, lib.nesr_last_error()
        return out.value
    base = size(2, 24, 40, 16, 8)
    # at least: the full-frame buffer, the accumulator and the f32 frame
    assert base >= (7 + 4) * 24 * 40 * 4 + 3 * 96 * 160 * 4
    assert size(2, 24, 40, 16, 8) > size(1, 24, 40, 16, 8) and size(2, 48, 40, 16, 8) > base and size(2, 24, 40, 24, 8) > base > size(2, 24, 40, 16, 8, 8, 4)
    out = ctypes.c_size_t(0)
    assert lib.nesr_sdx4_tiled_workspace_bytes(2, 4, 32, 4, 24, 40, C.TOKENS, 2, 16, 8, 10, 12, ctypes.byref(out)) == _lib.ERR_ARG and "vae_tile_overlap" in lib.nesr_last_error().decode()
    assert lib.nesr_sdx4_tiled_workspace_bytes(3, 4, 32, 4, 24, 40, C.TOKENS, 2, 16, 8, 0, -1, ctypes.byref(out)) == _lib.ERR_ARG
