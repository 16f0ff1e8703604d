"""GPU: the five window kernels of csrc/sdx4_tiled.hip, one launch at a time through the nesr_sdx4_k_* hooks, against the emulations
of tests/sdx4_tiled_ref.py.

  exact    integer data, power-of-two ramps, coefficients and guidance 8: every intermediate is a float32, so the device equals
           float64 bit for bit.  The step and the finish divide by S, so their accumulators are built as S x a value: the quotient
           is that value again
  random   the kernels chained as the tiled call chains them (gather -> a toy model -> accumulate per window, then the step), and
           the blend chain at s = 4, within 8 x max |float32 CPU restatement - float64|, computed here
  plans    tests/sdx4_tiled_ref.PLANS: 8 x 8 / 8 (one window), 8 x 24 / 8 / 4, 12 x 22 / 8 / 2 (x starts 0, 6, 12, 14: off the stride,
           6 and 14 are 2 mod 4), 40 x 16 / 16 / 8, 8 x 22 / 6 / 4 (rows of 6 floats, three windows a pixel), each at n = 1 and 2
  refused  what the launchers refuse leaves the buffers as they were
"""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import _lib
from tests import sdx4_tiled_ref as T
from tests.sdx4_kernel_ref import representable
from tests.swin2sr_ref import u8_check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LC = T.LC
MAX_THIN = 0.02


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def ints(ax):
    return (ctypes.c_int * 8)(*ax)


def run(name, *args):
    lib = _lib.load()
    _lib.check(getattr(lib, name)(*args, None), name)


def gather(src, n, ax):
    channels = src.shape[0]
    dst = torch.full((n, channels, ax[1], ax[5]), T.SENTINEL, dtype=torch.float32, device=DEV)
    run("nesr_sdx4_k_window_gather", ptr(src), n, channels, ints(ax), ptr(dst))
    return dst


def windows(plan):
    h, w, tile, overlap = plan
    return [T.axes(h, w, tile, overlap, y, x) for y, x in T.plan(h, w, tile, overlap)[2]]


# ---------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("plan", T.PLANS)
def test_gather_copies_every_window(plan, n):
    h, w, _, _ = plan
    rng = np.random.default_rng(1000 + h + w)
    for channels in (LC + 3, LC):
        src = rng.standard_normal((channels, h, w)).astype(np.float32)
        d = dev(src)
        for ax in windows(plan):
            got = gather(d, n, ax).cpu().numpy()
            assert np.array_equal(got.astype(np.float64), T.k_gather(src, n, ax)), (plan, n, channels, ax)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("plan", T.PLANS)
def test_accumulate_is_exact_on_integers(plan, n):
    h, w, _, _ = plan
    rng = np.random.default_rng(1100 + h + w + n)
    acc = rng.integers(-8, 9, size=(LC, h, w)).astype(np.float32)
    want, got = acc.astype(np.float64), dev(acc)
    for ax in windows(plan):
        model = rng.integers(-8, 9, size=(n, LC, ax[1], ax[5])).astype(np.float32)
        want = T.k_accumulate(model, want, ax, T.EXACT_G)
        run("nesr_sdx4_k_accumulate", ptr(dev(model)), n, LC, ints(ax), ctypes.c_float(T.EXACT_G), ptr(got))
    assert representable(want) and np.array_equal(got.cpu().numpy().astype(np.float64), want)


@pytest.mark.parametrize("plan", T.PLANS)
def test_tiled_step_is_exact_and_clears_the_accumulator(plan):
    h, w, tile, overlap = plan
    rng = np.random.default_rng(1200 + h + w)
    ax = T.axes(h, w, tile, overlap)
    s = T.normaliser(h, w, tile, overlap)
    acc = rng.integers(-8, 9, size=(LC, h, w)).astype(np.float64) * s[None]      # acc / S is the integer again
    frame = rng.integers(-8, 9, size=(LC + 3, h, w)).astype(np.float32)
    assert representable(acc)
    want_acc, want = T.k_tiled_step(acc, frame, LC, ax, T.EXACT_COEF)
    got_acc, got = dev(acc.astype(np.float32)), dev(frame)
    run("nesr_sdx4_k_tiled_step", ptr(got_acc), ptr(got), LC, ints(ax), (ctypes.c_float * 6)(*T.EXACT_COEF))
    assert representable(want) and np.array_equal(got.cpu().numpy().astype(np.float64), want) and not bool(got_acc.any())
    assert np.array_equal(got.cpu().numpy()[LC:], frame[LC:]) and not want_acc.any()      # the noised image stays


@pytest.mark.parametrize("plan", T.BLEND_PLANS + (T.PLANS[0], T.PLANS[4]))
def test_blend_add_and_finish_are_exact(plan):
    h, w, tile, overlap = plan
    rng = np.random.default_rng(1300 + h + w)
    acc = rng.integers(-8, 9, size=(4 * h, 4 * w, 3)).astype(np.float32)
    want, got = acc.astype(np.float64), dev(acc)
    for y, x in T.plan(h, w, tile, overlap)[2]:
        ax = T.axes(h, w, tile, overlap, y, x, 4)
        sample = rng.integers(-8, 9, size=(3, ax[1], ax[5])).astype(np.float32)
        want = T.k_blend_add(sample, want, ax)
        run("nesr_sdx4_k_blend_add", ptr(dev(sample)), ints(ax), ptr(got))
    assert representable(want) and np.array_equal(got.cpu().numpy().astype(np.float64), want)
    # the finish: values on a grid of 1 / 64 over [-2, 2] (v / 2 + 0.5 and x 255 are exact; halves round to even), times S
    ax = T.axes(h, w, tile, overlap, 0, 0, 4)
    v = rng.integers(-128, 129, size=(4 * h, 4 * w, 3)).astype(np.float64) / 64.0
    acc = v * T.normaliser(h, w, tile, overlap, 4)[:, :, None]
    assert representable(acc)
    out = torch.full((4 * h, 4 * w, 3), 201, dtype=torch.uint8, device=DEV)
    run("nesr_sdx4_k_blend_finish", ptr(dev(acc.astype(np.float32))), ints(ax), ptr(out))
    want_u8 = T.quantise(T.k_blend_finish_float(acc, ax))
    assert np.array_equal(out.cpu().numpy(), want_u8) and np.array_equal(want_u8, T.quantise(v / 2 + 0.5))
    assert ((v * 255 / 2 + 127.5) % 1 == 0.5).any()      # a tie was among them


# ---------------------------------------------------------------------------------------------- random, chained
def toy_model(window, n):
    k = (0.37, 0.61, 0.05)
    ty, tx = window.shape[-2:]
    pos = (torch.arange(ty)[:, None] - torch.arange(tx)[None, :]).to(torch.float32).to(DEV)
    return torch.stack([window[s, :LC] * k[0] + window[s, LC + s % 3][None] * (k[1] * (s + 1)) + pos[None] * k[2] for s in range(n)]).contiguous()


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("plan", T.PLANS)
def test_the_chained_kernels_follow_float64(plan, n):
    h, w, tile, overlap = plan
    start = T.chain_case(h, w, T.PLANS.index(plan), False)
    want = T.chain(start, h, w, tile, overlap, n, 2, False)
    tol = 8.0 * float(np.abs(T.chain(start, h, w, tile, overlap, n, 2, False, np.float32).astype(np.float64) - want).max())
    frame, acc = dev(start), torch.zeros((LC, h, w), dtype=torch.float32, device=DEV)
    for _ in range(2):
        for ax in windows(plan):
            model = toy_model(gather(frame, n, ax), n)
            run("nesr_sdx4_k_accumulate", ptr(model), n, LC, ints(ax), ctypes.c_float(T.RANDOM_G), ptr(acc))
        run("nesr_sdx4_k_tiled_step", ptr(acc), ptr(frame), LC, ints(T.axes(h, w, tile, overlap)), (ctypes.c_float * 6)(*T.RANDOM_COEF))
    err = float(np.abs(frame.cpu().numpy().astype(np.float64) - want).max())
    print(f"chain {plan} n = {n}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.3f}")
    assert 0 < tol < 1e-3 and err <= tol and not bool(acc.any())


@pytest.mark.parametrize("plan", T.BLEND_PLANS + (T.PLANS[4],))
def test_the_blend_chain_follows_float64(plan):
    h, w, tile, overlap = plan
    samples = T.blend_case(h, w, tile, overlap, T.PLANS.index(plan))
    want = T.blend_chain(samples, h, w, tile, overlap)
    tol = 8.0 * float(np.abs(T.blend_chain(samples, h, w, tile, overlap, np.float32).astype(np.float64) - want).max())
    acc = torch.zeros((4 * h, 4 * w, 3), dtype=torch.float32, device=DEV)
    for y, x, v in samples:
        run("nesr_sdx4_k_blend_add", ptr(dev(v)), ints(T.axes(h, w, tile, overlap, y, x, 4)), ptr(acc))
    out = torch.empty((4 * h, 4 * w, 3), dtype=torch.uint8, device=DEV)
    run("nesr_sdx4_k_blend_finish", ptr(acc), ints(T.axes(h, w, tile, overlap, 0, 0, 4)), ptr(out))
    excluded, wrong, count = u8_check(out.cpu(), torch.from_numpy(want), tol)
    print(f"blend {plan}: tol {tol:.3e}, {excluded} of {count} thin, {wrong} wrong")
    assert 0 < tol < 1e-4 and wrong == 0 and excluded <= MAX_THIN * count
    assert 0.2 < float(((want > 0) & (want < 1)).mean()) < 0.9      # both the clamp and the interior are reached


# ---------------------------------------------------------------------------------------------- refused
def test_what_the_launchers_refuse_leaves_the_buffers():
    lib = _lib.load()
    h, w = 12, 22
    src = torch.zeros((LC + 3, h, w), dtype=torch.float32, device=DEV)
    dst = torch.full((2, LC + 3, 8, 8), T.SENTINEL, dtype=torch.float32, device=DEV)
    acc = torch.full((LC, h, w), T.SENTINEL, dtype=torch.float32, device=DEV)
    good = T.axes(h, w, 8, 2, 4, 6)

    def changed(**kw):
        ax = list(good)
        for k, v in kw.items():
            ax[dict(yn=0, yt=1, yr=2, ya=3, xn=4, xt=5, xr=6, xa=7)[k]] = v
        return ints(ax)

    for bad in (changed(xa=5), changed(xa=16), changed(ya=6), changed(xr=8), changed(xt=7), changed(xn=21), changed(yr=-2), changed(xt=24)):
        assert lib.nesr_sdx4_k_window_gather(ptr(src), 2, LC + 3, bad, ptr(dst), None) == _lib.ERR_ARG and "refused" in lib.nesr_last_error().decode()
        assert lib.nesr_sdx4_k_accumulate(ptr(dst), 2, LC, bad, 7.5, ptr(acc), None) == _lib.ERR_ARG
    assert lib.nesr_sdx4_k_window_gather(ptr(src), 3, LC + 3, ints(good), ptr(dst), None) == _lib.ERR_ARG
    assert lib.nesr_sdx4_k_window_gather(ctypes.c_void_p(src.data_ptr() + 4), 2, LC + 3, ints(good), ptr(dst), None) == _lib.ERR_ARG
    assert lib.nesr_sdx4_k_window_gather(ptr(src), 2, LC + 3, None, ptr(dst), None) == _lib.ERR_ARG
    assert lib.nesr_sdx4_k_accumulate(ptr(dst), 2, LC, ints(good), float("nan"), ptr(acc), None) == _lib.ERR_ARG
    assert lib.nesr_sdx4_k_tiled_step(ptr(acc), ptr(src), LC, ints(good), None, None) == _lib.ERR_ARG
    out = torch.full((h, w, 3), 201, dtype=torch.uint8, device=DEV)
    assert lib.nesr_sdx4_k_blend_finish(ptr(src), ints(good), ptr(out), None) == _lib.ERR_ARG      # 22 is no multiple of 4
    torch.cuda.synchronize()
    assert bool((dst == T.SENTINEL).all()) and bool((acc == T.SENTINEL).all()) and bool((out == 201).all())
