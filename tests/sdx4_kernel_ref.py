"""Emulations of the indexing of the four kernels the diffusion stage's part 3 adds (csrc/sdx4_step.hip: prepare, step; csrc/
clip_text.hip: the embedding gather, the causal attention), on flat buffers with the kernels' own offsets, in whatever float dtype
they are asked for.  `fault` names one deliberate indexing mistake (FAULTS); tests/test_sdx4_kernels_host.py shows that each one is
seen by the cases tests/test_gpu_sdx4_kernels.py runs on the device.

  plane_stride               a sample of the UNet's input is taken to be lc planes apart, not lc + 3
  sample_one_not_written     only sample 0 of the UNet's input is written
  image_overwritten_by_step  the step writes lc + 3 planes of a sample: the noised image is lost
  future_key_scored          the diagonal chunk is not masked
  ragged_chunk_scored_zero   a key past the last one (zero filled in LDS) scores 0 instead of -inf, whatever the causal mask says
"""
from __future__ import annotations

import math

import numpy as np

FAULTS = ("plane_stride", "sample_one_not_written", "image_overwritten_by_step", "future_key_scored", "ragged_chunk_scored_zero")
SENTINEL = -777.0
CHUNK = 32


def prepare(frame, noise, latents, n, sa, sb, sigma, dtype=np.float64, fault=None):
    """frame [hw, 3] u8, noise [3, hw], latents [lc, hw] -> (sample [n, lc + 3, hw], latents_out [lc, hw]); what is not written
    keeps SENTINEL."""
    hw, lc = frame.shape[0], latents.shape[0]
    planes = lc + 3
    stride = (lc if fault == "plane_stride" else planes) * hw
    sample = np.full(n * planes * hw, SENTINEL, dtype=dtype)
    one = dtype(1.0)
    for s in range(1 if fault == "sample_one_not_written" else n):
        for c in range(3):
            x = frame[:, c].astype(dtype) / dtype(127.5) - one
            at = s * stride + (lc + c) * hw
            sample[at:at + hw] = dtype(sa) * x + dtype(sb) * noise[c].astype(dtype)
        for k in range(lc):
            at = s * stride + k * hw
            sample[at:at + hw] = dtype(sigma) * latents[k].astype(dtype)
    return sample.reshape(n, planes, hw), (dtype(sigma) * latents.astype(dtype))


def step(model, latents, sample, g, coef, dtype=np.float64, fault=None):
    """model [n, lc, hw], latents [lc, hw], sample [n, lc + 3, hw] (updated in a copy), coef = (c0x, c0m, cex, cem, sp, sq) ->
    (latents_out [lc, hw], sample)."""
    n, lc, hw = model.shape
    planes = lc + 3
    c0x, c0m, cex, cem, sp, sq = (dtype(v) for v in coef)
    x, m = latents.astype(dtype), model.astype(dtype)
    mm = m[0] + dtype(g) * (m[1] - m[0]) if n == 2 else m[0]
    x0, e = c0x * x + c0m * mm, cex * x + cem * mm
    new = sp * x0 + sq * e
    out = sample.astype(dtype).copy().reshape(-1)
    stride = (lc if fault == "plane_stride" else planes) * hw
    for s in range(1 if fault == "sample_one_not_written" else n):
        out[s * stride:s * stride + lc * hw] = new.reshape(-1)
        if fault == "image_overwritten_by_step":
            out[s * stride + lc * hw:s * stride + planes * hw] = 0
    return new, out.reshape(n, planes, hw)


def embed(ids, tok, pos, tokens, cs, dtype=np.float64):
    """ids [rows], tok [vocab, c], pos [positions, c] -> rows [rows, cs], zero past c."""
    rows, c = len(ids), tok.shape[1]
    out = np.zeros((rows, cs), dtype=dtype)
    for r in range(rows):
        out[r, :c] = tok[ids[r]].astype(dtype) + pos[r % tokens].astype(dtype)
    return out


def causal_attention(q, k, v, heads, d, dtype=np.float64, fault=None):
    """q, k, v [samples, tokens, heads d] -> [samples, tokens, heads d]: per query block of 32 the key chunks of 32 up to its own,
    a running maximum and sum, the accumulator rescaled with every chunk; a future key of the diagonal chunk scores -inf."""
    samples, tokens, _ = q.shape
    out = np.zeros((samples, tokens, heads * d), dtype=dtype)
    root = dtype(math.sqrt(d))
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(samples):
            for h in range(heads):
                cols = slice(h * d, (h + 1) * d)
                for q0 in range(0, tokens, CHUNK):
                    qi = np.arange(q0, min(q0 + CHUNK, tokens))
                    m_run = np.full(len(qi), -np.inf, dtype=dtype)
                    l_run = np.zeros(len(qi), dtype=dtype)
                    acc = np.zeros((len(qi), d), dtype=dtype)
                    for k0 in range(0, min(q0 + CHUNK, tokens), CHUNK):
                        kj = np.arange(k0, k0 + CHUNK)
                        real = kj < tokens
                        kk = np.zeros((CHUNK, d), dtype=dtype)
                        vv = np.zeros((CHUNK, d), dtype=dtype)
                        kk[real], vv[real] = k[s, kj[real], cols].astype(dtype), v[s, kj[real], cols].astype(dtype)
                        sc = (q[s, qi, cols].astype(dtype) @ kk.T) / root
                        sc[:, ~real] = -np.inf
                        if fault != "future_key_scored":
                            sc[kj[None, :] > qi[:, None]] = -np.inf
                        if fault == "ragged_chunk_scored_zero":      # after the mask: the zero-filled keys count with score 0
                            sc[:, ~real] = 0.0
                        m_new = np.maximum(m_run, sc.max(axis=1))
                        p = np.exp(sc - m_new[:, None])
                        alpha = np.exp(m_run - m_new)
                        l_run = l_run * alpha + p.sum(axis=1)
                        acc = acc * alpha[:, None] + p @ vv
                        m_run = m_new
                    out[s, qi, cols] = acc / l_run[:, None]
    return out


def softmax_attention(q, k, v, heads, d):
    """The same in float64 as the plain causal softmax: what the streamed form must equal."""
    samples, tokens, _ = q.shape
    out = np.zeros((samples, tokens, heads * d))
    ok = np.arange(tokens)[None, :] <= np.arange(tokens)[:, None]
    for s in range(samples):
        for h in range(heads):
            cols = slice(h * d, (h + 1) * d)
            sc = np.where(ok, (q[s, :, cols].astype(np.float64) @ k[s, :, cols].astype(np.float64).T) / math.sqrt(d), -np.inf)
            p = np.exp(sc - sc.max(axis=1, keepdims=True))
            out[s, :, cols] = (p / p.sum(axis=1, keepdims=True)) @ v[s, :, cols].astype(np.float64)
    return out


def representable(*arrays):
    """Every value of every array is a float32."""
    return all(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)) for a in arrays)


# ------------------------------------------------------------------------------------------------ the cases both test files run
EXTENTS = ((8, 8), (8, 24), (40, 16))
KEY_COUNTS = (1, 32, 33, 77)
SELECT_LEAD = 176.0        # >= 175: exp(-lead) is 0 in float32 and 1e-77 in float64, far under a rounding of 1


def exact_step_case(h, w, n, seed):
    """Integer latents and model outputs, power-of-two coefficients and guidance: every intermediate is a float32."""
    rng = np.random.default_rng(800 + seed)
    hw, lc = h * w, 4
    model = rng.integers(-8, 9, size=(n, lc, hw)).astype(np.float32)
    latents = rng.integers(-8, 9, size=(lc, hw)).astype(np.float32)
    sample = rng.integers(-8, 9, size=(n, lc + 3, hw)).astype(np.float32)
    g, coef = 8.0, (0.5, -2.0, 4.0, 0.25, 2.0, -0.5)
    m = model.astype(np.float64)
    mm = m[0] + g * (m[1] - m[0]) if n == 2 else m[0]
    x0, e = coef[0] * latents + coef[1] * mm, coef[2] * latents + coef[3] * mm
    assert representable(mm, coef[1] * mm, x0, coef[3] * mm, e, coef[5] * e, coef[4] * x0 + coef[5] * e)
    return model, latents, sample, g, coef


def exact_prepare_case(h, w, n, seed):
    """A frame of 0 and 255 (v / 127.5 - 1 is -1 or 1 exactly), integer noise and latents, power-of-two coefficients."""
    rng = np.random.default_rng(810 + seed)
    hw, lc = h * w, 4
    frame = (rng.integers(0, 2, size=(hw, 3)) * 255).astype(np.uint8)
    noise = rng.integers(-8, 9, size=(3, hw)).astype(np.float32)
    latents = rng.integers(-8, 9, size=(lc, hw)).astype(np.float32)
    return frame, noise, latents, 0.5, 0.25, 2.0


def selector_case(tokens, samples=1, heads=2, d=16):
    """q = 32 e0 for every query, k_j = 22 j e0: key j scores 176 j, so the latest key a query may read leads every earlier one by
    SELECT_LEAD and its weight is exactly 1; a future key, if scored, would lead by as much and wipe the accumulator.  v nonzero integers:
    out_i = v_i, bit for bit, in float32 and in float64."""
    rng = np.random.default_rng(820 + tokens)
    dim = heads * d
    q = np.zeros((samples, tokens, dim), dtype=np.float32)
    k = np.zeros((samples, tokens, dim), dtype=np.float32)
    for h in range(heads):
        q[:, :, h * d] = 32.0
        k[:, :, h * d] = 22.0 * np.arange(tokens)[None, :]
    v = (rng.integers(1, 65, size=(samples, tokens, dim)) * rng.choice([-1, 1], size=(samples, tokens, dim))).astype(np.float32)      # no zero: float64's 1e-77 would show
    assert 32.0 * 22.0 / math.sqrt(d) == SELECT_LEAD
    return q, k, v
