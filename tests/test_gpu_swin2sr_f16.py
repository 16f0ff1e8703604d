"""GPU: Swin2SR's fp16 compute form (Swin2SR(compute_dtype="fp16"), csrc/swin2sr.hip) against tests/swin2sr_f16_emu.py;
tests/test_swin2sr_f16_host.py shows on the CPU that every named fault of the emulation fails a (case, part) by 10 x its tolerance.

  part          one launch (attention block, MLP block, a stage's 3x3 conv) on seeded N(0, 1) tokens against the float64 emulation:
                max |gpu - emulation64| <= 8 x max |emulation32 - emulation64|, per case and part (printed as err / tol); the f32
                form's part against swin2sr_ref in float64 at the f32 tolerance 8 x max |f32 CPU - f64|
  forward       max |gpu - f64 unrounded| <= max |emulation64 - f64| + 8 x max |emulation32 - emulation64|: a bound, not a pin (an
                activation within a float32 error of an f16 rounding boundary flips and the later layers amplify it)
  upscale       no sample farther than ceil(255 x that bound) levels from quantise(emulation64); the share of differing samples is
                printed, not capped: with random weights nothing derives a cap
  composition   tiled == paste of upscale(window), forward_batch == each forward, a forward repeated == itself, bit for bit
  range         an input scaled until first_convolution's output passes 65504 raises NesrRangeError in fp16 and runs in f32
  f32           the default form gives the sha256 of the parent commit's 64 x 64 upscale (classical x2, seed 7)

Measured on the MI355X: every part passes, err / tol 0.000 to 0.504.  x3_range255 / attention is the sharpest pair (tolerance
7.2e-06, the bare float32 noise: the float32 emulation flips no f16 rounding in that launch).  It is what made the kernel normalise
q and k in double: q^[token 3, head 3, dim 5] lies 1.4e-07 (relative) from an f16 rounding boundary, an f32 normalisation chain
rounds it the other way, and that one f16 ulp times a temperature near 100 moves the token by 2.5e-03.  DESIGN section 17 has the
account.
"""
import ctypes
import hashlib
import math

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import Swin2SR, _lib
from tests import swin2sr_cases as C
from tests import swin2sr_f16_emu as E
from tests import swin2sr_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
FORWARD = [c.name for c in C.forward_cases()]
# one stage conv per distinct width: 24, 60, 180, 36, 32, 128, 40, 64, 48
CONV_CASES = ["small_shift", "one_window_high", "published_width", "odd_depth_x4", "x3_range255", "window_6_wide", "window_7_odd", "window_10_one_high",
              "window_5_one_head"]
PART_CASES = [(n, p) for n in FORWARD for p in ("attention", "mlp")] + [(n, "stage_conv") for n in CONV_CASES]
PARENT_SHA256 = "1347083324e12bd13db7b8562c830957bb455012fa96f8dc28f8d69dd5859e2e"
CLASSICAL = dict(embed_dim=180, depths=(6,) * 6, num_heads=(6,) * 6, window_size=8, upsampler="pixelshuffle", upscale=2, image_size=64)
_cache = {}


def model(case, form="fp16"):
    if (case.name, form) not in _cache:
        m = Swin2SR(compute_dtype=form, **case.cfg).to(DEV)
        m.load_state_dict(case.sd)
        _cache[case.name, form] = m
    return _cache[case.name, form]


def guarded(m, entry, shape, dtype, call):
    """An entry's output written into the middle of a buffer of sentinels; the guards are asserted."""
    n = int(np.prod(shape))
    fill = -7.0 if dtype == torch.float32 else 0x5A
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = ctypes.c_void_p(buf.data_ptr() + buf.element_size() * GUARD)
    _lib.check(call(_lib.load(), m._context(torch.device(DEV)), out, n, stream), entry)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), f"{entry} wrote outside the extent it reports"
    return buf[GUARD:GUARD + n].view(shape).cpu()


def guarded_part(m, part, layer, tokens):
    x = tokens.to(DEV).contiguous()
    n, h, w, _ = x.shape
    return guarded(m, "nesr_swin2sr_part_f32", tuple(x.shape), torch.float32,
                   lambda lib, ctx, out, cap, s: lib.nesr_swin2sr_part_f32(ctx, E.PARTS.index(part), 0, layer, ctypes.c_void_p(x.data_ptr()), n, h, w, out, cap, s))


def guarded_upscale(m, frame):
    f = torch.from_numpy(np.ascontiguousarray(frame)).to(DEV)
    h, w = f.shape[:2]
    s = m.config["upscale"]
    return guarded(m, "nesr_swin2sr_upscale_u8", (h * s, w * s, 3), torch.uint8,
                   lambda lib, ctx, out, cap, st: lib.nesr_swin2sr_upscale_u8(ctx, ctypes.c_void_p(f.data_ptr()), h, w, out, cap, st))


@pytest.mark.parametrize("name,part", PART_CASES)
def test_part_against_the_float64_emulation(name, part):
    case = C.by_name(name)
    tokens, layer, e64, tol = E.part_reference(case, part)
    m = model(case)
    got = guarded_part(m, part, layer, tokens)
    err = float((got.double() - e64).abs().max())
    print(f"{name} / {part} (layer {layer}): max |gpu - emulation64| = {err:.3e}, tol {tol:.3e}, err / tol = {err / tol:.3f}")
    assert torch.isfinite(got).all()
    assert err <= tol
    assert torch.equal(m.part(part, 0, layer, tokens.to(DEV)).cpu(), got), "the module's part gives the entry's bits, and the same twice"


@pytest.mark.parametrize("name,part", PART_CASES)
def test_part_in_the_f32_form_against_float64(name, part):
    case = C.by_name(name)
    tokens, layer = E.seeded_tokens(case), E.part_layer(case, part)
    y64 = E.part(part, case.sd, 0, layer, tokens.double(), torch.float64, **case.cfg)
    y32 = E.part(part, case.sd, 0, layer, tokens, torch.float64, **case.cfg)
    tol = 8 * float((y32.double() - y64).abs().max())
    got = guarded_part(model(case, "f32"), part, layer, tokens)
    err = float((got.double() - y64).abs().max())
    print(f"{name} / {part} f32: max |gpu - f64| = {err:.3e}, tol {tol:.3e}, err / tol = {err / tol:.3f}")
    assert torch.isfinite(got).all() and err <= tol


def test_part_takes_a_batch_and_every_layer():
    case = C.by_name("small_shift")
    m = model(case)
    tokens = E.seeded_tokens(case, seed=9, n=3)
    for part, stage, layer in (("attention", 1, 0), ("attention", 1, 1), ("mlp", 1, 1), ("stage_conv", 1, 0)):
        got = m.part(part, stage, layer, tokens.to(DEV)).cpu()
        for i in range(3):
            assert torch.equal(got[i:i + 1], m.part(part, stage, layer, tokens[i:i + 1].to(DEV)).cpu())
        e64 = E.part(part, case.sd, stage, layer, tokens.double(), **case.cfg)
        e32 = E.part(part, case.sd, stage, layer, tokens, **case.cfg)
        assert float((got.double() - e64).abs().max()) <= 8 * float((e32.double() - e64).abs().max())
    with pytest.raises(_lib.NesrHipError, match="stage"):
        m.part("mlp", 2, 0, tokens.to(DEV))
    with pytest.raises(_lib.NesrHipError, match="layer"):
        m.part("mlp", 0, 2, tokens.to(DEV))
    with pytest.raises(_lib.NesrHipError, match="window_size"):
        m.part("mlp", 0, 0, torch.zeros(1, 6, 8, 24, device=DEV))


@pytest.mark.parametrize("name", FORWARD)
def test_forward_within_the_bound(name):
    case = C.by_name(name)
    y64, _, bound = E.network_reference(case)
    m = model(case)
    x = case.x.to(DEV)
    got = m(x).cpu()
    err = float((got.double() - y64).abs().max())
    print(f"{name}: max |gpu - f64 unrounded| = {err:.3e}, bound {bound:.3e}, err / bound = {err / bound:.3f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= bound
    assert torch.equal(m(x).cpu(), got), "a forward repeated gives the same bits"
    assert not torch.equal(model(case, "f32")(x).cpu(), got), "the form changes the result"


@pytest.mark.parametrize("name", [c.name for c in C.frame_cases()])
def test_upscale_against_the_quantised_emulation(name):
    case = C.by_name(name)
    frame = case.frame if case.via == "upscale" else R.seeded_frame(13, 18, 63)
    y64 = R.upscale_float(case.sd, frame, torch.float64, **case.cfg)
    e64 = E.upscale_float(case.sd, frame, torch.float64, **case.cfg)
    e32 = E.upscale_float(case.sd, frame, torch.float32, **case.cfg)
    bound = float((e64 - y64).abs().max()) + 8 * float((e32.double() - e64).abs().max())
    levels = math.ceil(255 * bound)
    got = guarded_upscale(model(case), frame)
    want = R.quantise(e64)
    diff = (got.to(torch.int64) - want.to(torch.int64)).abs()
    print(f"{name}: {tuple(got.shape)}, bound {bound:.3e} = {levels} level(s); largest difference {int(diff.max())}, "
          f"{100.0 * float((diff > 0).float().mean()):.3f} % of the samples differ")
    assert got.shape == want.shape and int(diff.max()) <= levels


def test_tiled_is_the_paste_of_its_windows_bit_for_bit():
    case = C.by_name("small_shift")
    m = model(case)
    frame = torch.from_numpy(R.seeded_frame(21, 30, 64)).to(DEV)
    T, P, s = 8, 4, m.config["upscale"]
    p = m.tile_plan(21, 30, T, P)
    sy, sx = p["window"]
    want = torch.zeros((21 * s, 30 * s, 3), dtype=torch.uint8)
    for wy, wx, cy, cx, ch, cw, oy, ox in p["plan"].tolist():
        win = m.upscale(frame[wy:wy + sy, wx:wx + sx].contiguous()).cpu()
        want[oy:oy + ch, ox:ox + cw] = win[cy:cy + ch, cx:cx + cw]
    got = m.upscale(frame, tile=T, tile_pad=P)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(m.upscale(frame, tile=T, tile_pad=P, max_batch=5).cpu(), want)


def test_forward_batch_gives_each_image_its_own_bits():
    case = C.by_name("window_7_odd")
    m = model(case)
    _, ch, h, w = case.x.shape
    x = torch.stack([torch.zeros(ch, h, w), case.x[0], R.seeded_input(h, w, 77)[0]]).to(DEV)
    got = m.forward_batch(x).cpu()
    for i in range(3):
        assert torch.equal(got[i:i + 1], m(x[i:i + 1]).cpu())


def test_an_activation_f16_cannot_carry_raises_in_fp16_and_runs_in_f32():
    case = C.by_name("small_shift")
    scale = 1.0      # found on the CPU: first_convolution's output, which the patch embedding's projection rounds, passes 65504
    while float(E.first_conv(case.sd, case.x * scale, **case.cfg).abs().max()) <= 2 * 65504.0:
        scale *= 2.0
    assert float(E.first_conv(case.sd, case.x * (scale / 8), **case.cfg).abs().max()) < 65504.0
    m = model(case)
    x = (case.x * scale).to(DEV)
    with pytest.raises(_lib.NesrRangeError, match="65504"):
        m(x)
    assert torch.isfinite(model(case, "f32")(x)).all()
    with pytest.raises(_lib.NesrRangeError):
        m.forward_batch(torch.cat([case.x.to(DEV), x]))
    tokens = E.seeded_tokens(case)
    for part in E.PARTS:
        bad = tokens.clone()
        bad[0, 3, 5, 2] = float("nan") if part == "mlp" else 7e4
        with pytest.raises(_lib.NesrRangeError):
            m.part(part, 0, 0, bad.to(DEV))
    # the word is per call: the next forward is clean, and below the limit the same input runs
    y64, _, bound = E.network_reference(case)
    assert float((m(case.x.to(DEV)).cpu().double() - y64).abs().max()) <= bound
    assert torch.isfinite(m((case.x * (scale / 8)).to(DEV))).all()


def test_a_weight_f16_cannot_carry_is_refused_when_the_context_is_made():
    case = C.by_name("small_shift")
    sd = {k: v.clone() for k, v in case.sd.items()}
    sd["swin2sr.encoder.stages.0.layers.0.intermediate.dense.weight"][1, 2] = -65600.0
    m = Swin2SR(compute_dtype="fp16", **case.cfg).to(DEV)
    m.load_state_dict(sd)
    with pytest.raises(_lib.NesrRangeError, match="intermediate.dense.weight"):
        m(case.x.to(DEV))
    ctx = model(case)._context(torch.device(DEV))
    assert _lib.load().nesr_swin2sr_set_dtype(ctx, _lib.DTYPE_F32) == -3      # NESR_ERR_STATE: after finalize


def test_the_f32_form_gives_the_parent_commits_bits():
    m = Swin2SR(**CLASSICAL).to(DEV)
    m.load_state_dict(R.seeded_state_dict(seed=7, **CLASSICAL))
    frame = torch.from_numpy(R.seeded_frame(64, 64, seed=11)).to(DEV)
    assert hashlib.sha256(m.upscale(frame).cpu().numpy().tobytes()).hexdigest() == PARENT_SHA256
    m.kernel_time_ms()                               # the counter always runs: start it afresh
    m.upscale(frame)
    assert m.kernel_time_ms()["launches"] == 91      # the launches of DESIGN section 17, unchanged
