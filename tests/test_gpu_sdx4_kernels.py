"""GPU: the four kernels of the diffusion stage's part 3, one launch each through their hooks (nesr_sdx4_k_prepare, nesr_sdx4_k_step,
nesr_clip_text_k_embed, nesr_clip_text_k_attention), against the emulations of tests/sdx4_kernel_ref.py in float64.

  exact      integer inputs, power-of-two coefficients and guidance, every intermediate a float32 (asserted by the case): the device
             equals float64 bit for bit.  The causal selector case makes the latest key a query may read lead by 176: its weight is
             exactly 1, and a future key, if it were scored, would wipe the accumulator.
  u8         the prepare kernel on all 256 values: the two-rounding float32 formula bit for bit, float64 to two roundings
  toleranced random cases within 8 x max |float32 emulation - float64|
  guards     every output lies in a buffer of sentinels; channels lc .. of the UNet's input survive a step
  refusals   what a launcher refuses launches nothing
"""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import _lib
from tests import sdx4_kernel_ref as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 1024


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def guarded(count, fill=K.SENTINEL):
    buf = torch.full((GUARD + count + GUARD,), fill, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + count]


def guards_intact(buf, count, fill=K.SENTINEL):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + count:] == fill).all())


def run_prepare(frame, noise, latents, n, sa, sb, sigma):
    hw, lc = frame.shape[0], latents.shape[0]
    sbuf, sample = guarded(n * (lc + 3) * hw)
    lbuf, lat = guarded(lc * hw)
    f, nz, lt = dev(frame), dev(noise), dev(latents)
    rc = _lib.load().nesr_sdx4_k_prepare(ptr(f), ptr(nz), ptr(lt), n, hw, lc, sa, sb, sigma, ptr(sample), ptr(lat), None)
    torch.cuda.synchronize()
    assert guards_intact(sbuf, sample.numel()) and guards_intact(lbuf, lat.numel())
    return rc, sample.cpu().numpy().reshape(n, lc + 3, hw), lat.cpu().numpy().reshape(lc, hw)


def run_step(model, latents, sample, g, coef, in_place=False):
    n, lc, hw = model.shape
    sbuf, smp = guarded(n * (lc + 3) * hw)
    smp.copy_(dev(sample).reshape(-1))
    lbuf, lat = guarded(lc * hw)
    m, lt = dev(model), dev(latents)
    if in_place:
        lat.copy_(lt.reshape(-1))
        lt = lat
    co = (ctypes.c_float * 6)(*coef)
    rc = _lib.load().nesr_sdx4_k_step(ptr(m), ptr(lt), n, hw, lc, g, co, ptr(lat), ptr(smp), None)
    torch.cuda.synchronize()
    assert guards_intact(sbuf, smp.numel()) and guards_intact(lbuf, lat.numel())
    return rc, lat.cpu().numpy().reshape(lc, hw), smp.cpu().numpy().reshape(n, lc + 3, hw)


def run_attention(q, k, v, heads, d, pad=0):
    """q, k, v [samples, tokens, heads d] packed side by side as the encoder does; `pad` zero columns behind each part."""
    samples, tokens, dim = q.shape
    ld = dim + pad
    qkv = np.zeros((samples, tokens, 3 * ld), dtype=np.float32)
    qkv[:, :, :dim], qkv[:, :, ld:ld + dim], qkv[:, :, 2 * ld:2 * ld + dim] = q, k, v
    t = dev(qkv)
    obuf, out = guarded(samples * tokens * ld)
    rc = _lib.load().nesr_clip_text_k_attention(samples, tokens, heads, d, ptr(t), ctypes.c_void_p(t.data_ptr() + 4 * ld), ctypes.c_void_p(t.data_ptr() + 8 * ld),
                                                3 * ld, 3 * ld, ld, ptr(out), None)
    torch.cuda.synchronize()
    assert guards_intact(obuf, out.numel())
    got = out.cpu().numpy().reshape(samples, tokens, ld)
    assert rc != 0 or not got[:, :, dim:].any()      # the pad columns are zeroed
    return rc, got[:, :, :dim]


# ---------------------------------------------------------------------------------------------- prepare and step
@pytest.mark.parametrize("h, w", K.EXTENTS)
@pytest.mark.parametrize("n", [1, 2])
def test_exact_cases_equal_float64_bit_for_bit(h, w, n):
    model, latents, sample, g, coef = K.exact_step_case(h, w, n, h + n)
    new64, out64 = K.step(model, latents, sample, g, coef, np.float64)
    for in_place in (False, True):
        rc, new, out = run_step(model, latents, sample, g, coef, in_place)
        assert rc == 0 and np.array_equal(new.astype(np.float64), new64) and np.array_equal(out.astype(np.float64), out64)
    assert np.array_equal(out[:, 4:], sample[:, 4:])      # the noised image stays
    frame, noise, lat, sa, sb, sigma = K.exact_prepare_case(h, w, n, h + n)
    s64, l64 = K.prepare(frame, noise, lat, n, sa, sb, sigma, np.float64)
    rc, s, l = run_prepare(frame, noise, lat, n, sa, sb, sigma)
    assert rc == 0 and np.array_equal(s.astype(np.float64), s64) and np.array_equal(l.astype(np.float64), l64)


def test_prepare_on_every_u8_value():
    frame = np.stack([np.arange(256), np.arange(256)[::-1], (np.arange(256) * 7) % 256], axis=1).astype(np.uint8)
    zeros, lat = np.zeros((3, 256), dtype=np.float32), np.zeros((4, 256), dtype=np.float32)
    rc, s, _ = run_prepare(frame, zeros, lat, 1, 1.0, 0.0, 1.0)
    want32 = (frame.T.astype(np.float32) / np.float32(127.5) - np.float32(1.0))
    want64 = frame.T.astype(np.float64) / 127.5 - 1.0
    assert rc == 0 and np.array_equal(s[0, 4:], want32) and float(np.abs(s[0, 4:].astype(np.float64) - want64).max()) <= 2.0 ** -23
    assert s[0, 4, 0] == -1.0 and s[0, 4, 255] == 1.0


@pytest.mark.parametrize("h, w", K.EXTENTS)
@pytest.mark.parametrize("n", [1, 2])
def test_random_cases_within_the_float32_emulation_s_error(h, w, n):
    rng = np.random.default_rng(700 + h + n)
    hw, lc = h * w, 4
    frame = rng.integers(0, 256, size=(hw, 3)).astype(np.uint8)
    noise, lat = rng.standard_normal((3, hw)).astype(np.float32), rng.standard_normal((lc, hw)).astype(np.float32)
    sa, sb, sigma = np.float32(0.99853), np.float32(0.05421), np.float32(1.0)
    s64, l64 = K.prepare(frame, noise, lat, n, sa, sb, sigma, np.float64)
    s32, _ = K.prepare(frame, noise, lat, n, sa, sb, sigma, np.float32)
    tol = 8.0 * float(np.abs(s32.astype(np.float64) - s64).max())
    rc, s, l = run_prepare(frame, noise, lat, n, float(sa), float(sb), float(sigma))
    err = float(np.abs(s.astype(np.float64) - s64).max())
    print(f"prepare {h}x{w} n={n}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.3f}")
    assert rc == 0 and 0 < tol and err <= tol and np.array_equal(l, lat)
    model = rng.standard_normal((n, lc, hw)).astype(np.float32)
    a, p = 0.0413, 0.0627
    coef = tuple(np.float32(v) for v in (np.sqrt(a), -np.sqrt(1 - a), np.sqrt(1 - a), np.sqrt(a), np.sqrt(p), np.sqrt(1 - p)))
    new64, out64 = K.step(model, lat, s, 7.5, coef, np.float64)
    new32, _ = K.step(model, lat, s, 7.5, coef, np.float32)
    tol = 8.0 * float(np.abs(new32.astype(np.float64) - new64).max())
    rc, new, out = run_step(model, lat, s, 7.5, [float(c) for c in coef])
    err = float(np.abs(new.astype(np.float64) - new64).max())
    print(f"step {h}x{w} n={n}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.3f}")
    assert rc == 0 and 0 < tol and err <= tol
    assert np.array_equal(out[:, 4:], s[:, 4:]) and all(np.array_equal(out[i, :4], new) for i in range(n))


def test_launchers_refuse_what_they_cannot_take():
    lib = _lib.load()
    frame, noise, lat, sa, sb, sigma = K.exact_prepare_case(8, 8, 1, 0)
    f, nz, lt = dev(frame), dev(noise), dev(lat)
    sbuf, sample = guarded(2 * 7 * 64)
    lbuf, out = guarded(4 * 64)
    off = ctypes.c_void_p(sample.data_ptr() + 4)      # not 16-byte aligned
    for args in ((ptr(f), ptr(nz), ptr(lt), 3, 64, 4), (ptr(f), ptr(nz), ptr(lt), 1, 62, 4), (ptr(f), ptr(nz), ptr(lt), 1, 64, 9), (ptr(f), ptr(nz), ptr(lt), 0, 64, 4),
                 (None, ptr(nz), ptr(lt), 1, 64, 4)):
        assert lib.nesr_sdx4_k_prepare(*args, sa, sb, sigma, ptr(sample), ptr(out), None) == _lib.ERR_ARG and b"launch_sdx4_prepare" in lib.nesr_last_error()
    assert lib.nesr_sdx4_k_prepare(ptr(f), ptr(nz), ptr(lt), 1, 64, 4, sa, sb, sigma, off, ptr(out), None) == _lib.ERR_ARG
    co = (ctypes.c_float * 6)(1, 1, 1, 1, 1, 1)
    m = dev(np.zeros((2, 4, 64), dtype=np.float32))
    assert lib.nesr_sdx4_k_step(ptr(m), ptr(lt), 3, 64, 4, 1.0, co, ptr(out), ptr(sample), None) == _lib.ERR_ARG
    assert lib.nesr_sdx4_k_step(ptr(m), ptr(lt), 2, 64, 4, 1.0, None, ptr(out), ptr(sample), None) == _lib.ERR_ARG
    assert lib.nesr_sdx4_k_step(ptr(m), ptr(lt), 2, 64, 4, float("nan"), co, ptr(out), ptr(sample), None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((sbuf == K.SENTINEL).all()) and bool((lbuf == K.SENTINEL).all())


# ---------------------------------------------------------------------------------------------- the text encoder's kernels
@pytest.mark.parametrize("tokens", K.KEY_COUNTS)
def test_causal_selector_is_exact(tokens):
    q, k, v = K.selector_case(tokens, samples=2)
    want = K.causal_attention(q, k, v, 2, 16, np.float64)
    assert np.array_equal(want, v.astype(np.float64))
    rc, got = run_attention(q, k, v, 2, 16)
    assert rc == 0 and np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("tokens", K.KEY_COUNTS)
@pytest.mark.parametrize("heads, d, pad", [(4, 8, 0), (5, 8, 8), (2, 64, 0), (1, 24, 8)])
def test_causal_attention_within_the_float32_emulation_s_error(tokens, heads, d, pad):
    rng = np.random.default_rng(600 + tokens + d)
    q, k, v = (rng.standard_normal((2, tokens, heads * d)).astype(np.float32) for _ in range(3))
    k = 2.0 * k
    want = K.causal_attention(q, k, v, heads, d, np.float64)
    tol = 8.0 * float(np.abs(K.causal_attention(q, k, v, heads, d, np.float32).astype(np.float64) - want).max())
    rc, got = run_attention(q, k, v, heads, d, pad)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"attention {tokens} keys, {heads} x {d}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol if tol else 0:.3f}")
    assert rc == 0 and np.array_equal(got[:, 0], v[:, 0])      # query 0 with its single key is exact
    assert err <= tol or tokens == 1
    both = got
    rc, alone = run_attention(q[1:], k[1:], v[1:], heads, d, pad)
    assert np.array_equal(alone[0], both[1])                   # a sample does not depend on n


@pytest.mark.parametrize("tokens, c", [(1, 32), (7, 40), (77, 128)])
def test_embedding_gather_is_exact(tokens, c):
    rng = np.random.default_rng(500 + tokens)
    vocab, positions, cs = 50, 77, (c + 15) // 16 * 16
    tok, pos = rng.integers(-99, 100, size=(vocab, c)).astype(np.float32), rng.integers(-99, 100, size=(positions, c)).astype(np.float32)
    ids = rng.integers(0, vocab, size=2 * tokens)
    ids[0], ids[-1] = 0, vocab - 1
    if tokens > 2:
        ids[2] = ids[1]
    t, p = dev(tok), dev(pos)
    obuf, out = guarded(2 * tokens * cs)
    host = (ctypes.c_int32 * len(ids))(*ids.tolist())
    lib = _lib.load()
    assert lib.nesr_clip_text_k_embed(host, 2 * tokens, tokens, ptr(t), vocab, ptr(p), positions, c, cs, ptr(out), None) == 0
    torch.cuda.synchronize()
    assert guards_intact(obuf, out.numel())
    assert np.array_equal(out.cpu().numpy().reshape(2 * tokens, cs).astype(np.float64), K.embed(ids, tok, pos, tokens, cs))
    out.fill_(K.SENTINEL)
    bad = (ctypes.c_int32 * len(ids))(*ids.tolist())
    bad[len(ids) // 2] = vocab
    for args in ((bad, 2 * tokens, tokens, ptr(t), vocab, ptr(p), positions, c, cs), (host, 2 * tokens, tokens, ptr(t), vocab, ptr(p), tokens - 1, c, cs),
                 (host, 2 * tokens, tokens, ptr(t), vocab, ptr(p), positions, c, cs + 16), (host, 513, tokens, ptr(t), vocab, ptr(p), positions, c, cs)):
        assert lib.nesr_clip_text_k_embed(*args, ptr(out), None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((obuf == K.SENTINEL).all())
