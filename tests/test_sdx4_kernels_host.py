"""The kernel emulations of tests/sdx4_kernel_ref.py without a GPU: the streamed causal attention is the causal softmax, the
exact cases are exact in float32 and float64 alike, and every named indexing fault is seen by a case that
tests/test_gpu_sdx4_kernels.py runs on the device."""
import numpy as np
import pytest

from tests import sdx4_kernel_ref as K


@pytest.mark.parametrize("tokens", K.KEY_COUNTS)
def test_streamed_causal_attention_is_the_causal_softmax(tokens):
    rng = np.random.default_rng(900 + tokens)
    q, k, v = (rng.standard_normal((2, tokens, 48)).astype(np.float32) for _ in range(3))
    want = K.softmax_attention(q, 3.0 * k, v, 2, 24)
    assert float(np.abs(K.causal_attention(q, 3.0 * k, v, 2, 24) - want).max()) < 1e-12
    assert np.array_equal(K.causal_attention(q, k, v, 2, 24)[:, 0], v[:, 0].astype(np.float64))      # query 0: its single key, exactly


@pytest.mark.parametrize("tokens", K.KEY_COUNTS)
def test_the_selector_case_selects_exactly(tokens):
    q, k, v = K.selector_case(tokens, samples=2)
    for dtype in (np.float64, np.float32):
        assert np.array_equal(K.causal_attention(q, k, v, 2, 16, dtype), v.astype(dtype))
    assert np.array_equal(K.softmax_attention(q, k, v, 2, 16), v.astype(np.float64))
    if tokens > 1:      # a scored future key wins by the lead and wipes what the query may read
        bad = K.causal_attention(q, k, v, 2, 16, np.float32, fault="future_key_scored")
        last = np.minimum((np.arange(tokens) // K.CHUNK + 1) * K.CHUNK, tokens) - 1
        assert np.array_equal(bad, v[:, last]) and not np.array_equal(bad, v)


@pytest.mark.parametrize("tokens", [1, 33, 77])
def test_a_ragged_chunk_scored_zero_is_seen(tokens):
    rng = np.random.default_rng(910 + tokens)
    q, k, v = (rng.standard_normal((1, tokens, 16)).astype(np.float32) for _ in range(3))
    good, bad = K.causal_attention(q, k, v, 2, 8), K.causal_attention(q, k, v, 2, 8, fault="ragged_chunk_scored_zero")
    assert float(np.abs(good - bad).max()) > 1e-3


@pytest.mark.parametrize("h, w", K.EXTENTS)
@pytest.mark.parametrize("n", [1, 2])
def test_exact_cases_are_exact_and_see_the_faults(h, w, n):
    model, latents, sample, g, coef = K.exact_step_case(h, w, n, h + n)
    new64, out64 = K.step(model, latents, sample, g, coef, np.float64)
    new32, out32 = K.step(model, latents, sample, g, coef, np.float32)
    assert np.array_equal(new64, new32) and np.array_equal(out64, out32) and K.representable(new64, out64)
    assert np.array_equal(out64[:, 4:], sample[:, 4:]) and all(np.array_equal(out64[s, :4], new64) for s in range(n))
    assert not np.array_equal(K.step(model, latents, sample, g, coef, fault="image_overwritten_by_step")[1], out64)
    frame, noise, lat, sa, sb, sigma = K.exact_prepare_case(h, w, n, h + n)
    s64, l64 = K.prepare(frame, noise, lat, n, sa, sb, sigma, np.float64)
    s32, l32 = K.prepare(frame, noise, lat, n, sa, sb, sigma, np.float32)
    assert np.array_equal(s64, s32) and np.array_equal(l64, l32) and K.representable(s64, l64) and not (s64 == K.SENTINEL).any()
    if n == 2:
        for fault in ("plane_stride", "sample_one_not_written"):
            assert not np.array_equal(K.step(model, latents, sample, g, coef, fault=fault)[1], out64)
            assert not np.array_equal(K.prepare(frame, noise, lat, n, sa, sb, sigma, fault=fault)[0], s64)


def test_every_u8_value_maps_into_the_unit_range():
    frame = np.arange(256, dtype=np.uint8).repeat(3).reshape(256, 3)
    zeros = np.zeros((3, 256), dtype=np.float32)
    s64, _ = K.prepare(frame, zeros, np.zeros((4, 256), dtype=np.float32), 1, 1.0, 0.0, 1.0, np.float64)
    s32, _ = K.prepare(frame, zeros, np.zeros((4, 256), dtype=np.float32), 1, 1.0, 0.0, 1.0, np.float32)
    assert s64[0, 4, 0] == -1.0 and s64[0, 4, 255] == 1.0 and bool((np.diff(s64[0, 5]) > 0).all())
    assert float(np.abs(s32.astype(np.float64) - s64).max()) <= 2.0 ** -23      # two roundings of values under 2


def test_the_embedding_emulation_pads_with_zeros():
    rng = np.random.default_rng(920)
    tok, pos = rng.standard_normal((10, 40)).astype(np.float32), rng.standard_normal((7, 40)).astype(np.float32)
    out = K.embed([3, 3, 0, 9, 9, 1], tok, pos, 3, 48)
    assert out.shape == (6, 48) and not out[:, 40:].any() and np.array_equal(out[4, :40], tok[9].astype(np.float64) + pos[1]) and np.array_equal(out[0, :40] - out[1, :40], (pos[0].astype(np.float64) - pos[1]))


def test_every_fault_is_named():
    assert set(K.FAULTS) == {"plane_stride", "sample_one_not_written", "image_overwritten_by_step", "future_key_scored", "ragged_chunk_scored_zero"}
