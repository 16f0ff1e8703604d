"""GPU: `StableDiffusionX4Upscaler.upscale(tile=...)` and `VaeDecoder.decode_latents_u8(tile=...)` on the crafted pipeline of
tests/sdx4_cases.py (UNet of two levels: the frame multiple is 2).

  (a) one window   tile >= frame on the 16 x 24 frame goes through the window kernels and returns the untiled upscale's bits
  (b) composed     a 24 x 40 frame, tile 16, overlap 8 (2 x 4 windows), 3 steps: bit-equal to the same loop composed in Python from
                   the five hooks, UNet2DCondition.forward and VaeDecoder.decode; guidance 7.5 and 1
  (c) float64      the same call against tests/sdx4_tiled_ref.py: latents within 8 x max |float32 restatement - float64|, the frame
                   through u8_check with 0 wrong and at most 2 % left out
  (d) repeats      the same bits twice; unet.calls rises by steps x windows; last_launches() is text + 1 + steps (windows (1 + UNet
                   + 1) + 1) + vae_windows (1 + VAE + 1) + 1
  (e) large        264 x 256 (67584 pixels, above the limit), tile 64, overlap 8, 2 steps -> [1056, 1024, 3], the same bits twice;
                   without `tile` the refusal naming 65536 stands
  (f) VAE alone    decode_latents_u8(tile=) on 24 x 40 latents against float64; one window is the untiled decode; 264 x 256 runs
  (g) stage        diffusion_stage(pipe, tile=16, tile_overlap=8) inside enhance_iterations
  (h) fp16 UNet    the tiled call equals the loop composed from the same fp16 forward, bit for bit, and lies within max |emulation64
                   - float64| + 8 max |emulation32 - emulation64| of the float64 loop, the emulation being the specification's loop
                   with tests/unet_f16_emu.forward; the crafted over-range weights raise NesrRangeError once, after the call
  (i) refusals     every refusal names the value and leaves the sentinels intact
"""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import ClipTextEncoder, StableDiffusionX4Upscaler, UNet2DCondition, VaeDecoder, _lib, nesr_adapter
from neural_enhanced_super_resolution_amd import clip_text, sdx4, unet
from tests import sdx4_cases as C
from tests import sdx4_tiled_ref as T
from tests.swin2sr_ref import u8_check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


def pipe(dtype="f32", conv_out_scale=1.0):
    key = (dtype, conv_out_scale)
    if key not in _cache:
        m = C.models()
        text = ClipTextEncoder(**m["text"][1]).to(DEV)
        text.load_state_dict(m["text"][0])
        vae = VaeDecoder(**m["vae"][1]).to(DEV)
        vae.load_state_dict(m["vae"][0])
        sd = {k: v.clone() for k, v in m["unet"][0].items()}
        if conv_out_scale != 1.0:      # tests/test_gpu_sdx4_f16.py's over-range UNet
            for name in ("conv_out.weight", "conv_out.bias"):
                sd[name] *= conv_out_scale
            sd["conv_norm_out.weight"] *= 100.0
        net = UNet2DCondition(compute_dtype="fp16" if dtype == "fp16" else "f32", **m["unet"][1]).to(DEV)
        net.load_state_dict(sd)
        _cache[key] = StableDiffusionX4Upscaler(text, net, vae, max_noise_level=C.MAX_NOISE_LEVEL)
    return _cache[key]


def call(p, guidance=C.GUIDANCE, steps=T.STEPS, tile=T.TILE, overlap=T.OVERLAP, **kw):
    frame, noise, latents = T.crafted()
    ids = C.ids()
    return p.upscale(frame.to(DEV), prompt_ids=ids[1], negative_ids=ids[0], noise_level=C.NOISE_LEVEL, num_inference_steps=steps, guidance_scale=guidance,
                     noise=noise.to(DEV), latents=latents.to(DEV), return_latents=True, tile=tile, tile_overlap=overlap, **kw)


ptr = lambda t: ctypes.c_void_p(t.data_ptr())
ints = lambda ax: (ctypes.c_int * 8)(*ax)


def hook(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def composed_decode(p, lat, h, w, tile, overlap):
    """The tiled decode from the gather and blend hooks and VaeDecoder.decode; lat [4, h, w] on the device."""
    sf = float(p.vae.config["scaling_factor"])
    acc = torch.zeros((4 * h, 4 * w, 3), dtype=torch.float32, device=DEV)
    for y, x in T.plan(h, w, tile, overlap)[2]:
        ax = T.axes(h, w, tile, overlap, y, x)
        win = torch.empty((1, 4, ax[1], ax[5]), dtype=torch.float32, device=DEV)
        hook("nesr_sdx4_k_window_gather", ptr(lat), 1, 4, ints(ax), ptr(win))
        z = torch.from_numpy(win.cpu().numpy() / np.float32(sf)).to(DEV)      # the kernel's own division (torch multiplies by a reciprocal)
        sample = p.vae.decode(z)
        hook("nesr_sdx4_k_blend_add", ptr(sample), ints(T.axes(h, w, tile, overlap, y, x, 4)), ptr(acc))
    out = torch.empty((4 * h, 4 * w, 3), dtype=torch.uint8, device=DEV)
    hook("nesr_sdx4_k_blend_finish", ptr(acc), ints(T.axes(h, w, tile, overlap, 0, 0, 4)), ptr(out))
    return out


def composed(p, guidance, steps=T.STEPS, tile=T.TILE, overlap=T.OVERLAP):
    """The tiled loop from the parts: the networks' own forwards, sdx4_prepare at n = 1 and the five window hooks."""
    frame, noise, latents = T.crafted()
    frame, noise, latents = frame.to(DEV), noise.to(DEV), latents.to(DEV)
    h, w = T.H, T.W
    ids = C.ids() if guidance > 1.0 else C.ids()[1:]
    n = ids.shape[0]
    text = p.text_encoder(ids, device=DEV)
    full = torch.empty((7, h, w), dtype=torch.float32, device=DEV)
    acc = torch.empty((4, h, w), dtype=torch.float32, device=DEV)
    sa, sb = sdx4.noise_coefficients(C.NOISE_LEVEL)[1]
    hook("nesr_sdx4_k_prepare", ptr(frame), ptr(noise), ptr(latents), 1, h * w, 4, float(sa), float(sb), 1.0, ptr(full), ptr(acc))
    acc.zero_()
    ts, _, coef = sdx4.schedule(steps)
    rows = T.plan(h, w, tile, overlap)[2]
    for i, t in enumerate(ts):
        for y, x in rows:
            ax = T.axes(h, w, tile, overlap, y, x)
            win = torch.empty((n, 7, ax[1], ax[5]), dtype=torch.float32, device=DEV)
            hook("nesr_sdx4_k_window_gather", ptr(full), n, 7, ints(ax), ptr(win))
            m = p.unet(win, float(t), text, C.NOISE_LEVEL)
            hook("nesr_sdx4_k_accumulate", ptr(m), n, 4, ints(ax), ctypes.c_float(guidance), ptr(acc))
        hook("nesr_sdx4_k_tiled_step", ptr(acc), ptr(full), 4, ints(T.axes(h, w, tile, overlap)), (ctypes.c_float * 6)(*[float(v) for v in coef[i]]))
    lat = full[:4].contiguous()
    return composed_decode(p, lat, h, w, tile, overlap), lat[None].clone()


def test_one_window_returns_the_untiled_bits():                                                         # (a)
    p = pipe()
    noise, latents = C.draws()
    ids = C.ids()
    kw = dict(prompt_ids=ids[1], negative_ids=ids[0], noise_level=C.NOISE_LEVEL, num_inference_steps=C.STEPS, noise=noise.to(DEV), latents=latents.to(DEV), return_latents=True)
    for guidance in (C.GUIDANCE, 1.0):
        want, want_lat = p.upscale(C.frame().to(DEV), guidance_scale=guidance, **kw)
        p.kernel_time_ms()
        for tile in (24, 64):
            got, lat = p.upscale(C.frame().to(DEV), guidance_scale=guidance, tile=tile, **kw)
            assert torch.equal(lat, want_lat) and torch.equal(got, want)
        assert p.kernel_time_ms()["launches"] == 2 * (1 + C.STEPS * 3 + 3)      # the window kernels ran: prepare, (gather, accumulate, step) a step, gather, add, finish
    assert p.tile_plan(C.H, C.W, 64) == ((1, 1), (C.H, C.W), [(0, 0)])


@pytest.mark.parametrize("guidance", [C.GUIDANCE, 1.0])
def test_the_tiled_call_is_the_composed_loop_and_the_float64_loop(guidance):
    p = pipe()
    out, lat = call(p, guidance)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (4 * T.H, 4 * T.W, 3) and tuple(lat.shape) == (1, 4, T.H, T.W)
    want_out, want_lat = composed(p, guidance)
    assert torch.equal(lat, want_lat) and torch.equal(out, want_out)                                   # (b)
    lat64, y64, tol_lat, tol, _ = T.reference(guidance)
    err = float((lat.cpu().double() - lat64).abs().max())
    excluded, wrong, n = u8_check(out.cpu(), y64, tol)
    print(f"guidance {guidance}: latents err {err:.3e}, tol {tol_lat:.3e}, err / tol {err / tol_lat:.3f}; frame: {excluded} of {n} thin, {wrong} wrong")
    assert err <= tol_lat and wrong == 0 and excluded <= C.MAX_THIN * n                                 # (c)


def test_repeats_calls_and_launches():                                                                  # (d)
    p = pipe()
    p.vae.kernel_time_ms()
    p.vae.decode_latents_u8(torch.zeros((1, 4, 16, 16), device=DEV))
    vae_launches = p.vae.kernel_time_ms()["launches"]
    (ky, kx), (ty, tx), rows = p.tile_plan(T.H, T.W, T.TILE, T.OVERLAP)
    assert (ky, kx, ty, tx) == (2, 4, 16, 16) and rows == T.plan(T.H, T.W, T.TILE, T.OVERLAP)[2]
    for guidance, steps in ((C.GUIDANCE, T.STEPS), (1.0, 2)):
        before, vae_before = p.unet.calls, p.vae.calls
        p.kernel_time_ms()
        out, lat = call(p, guidance, steps)
        own = p.kernel_time_ms()
        assert p.unet.calls - before == steps * 8 and p.vae.calls - vae_before == 8
        want = clip_text.launches_per_forward(**C.TEXT) + 1 + steps * (8 * (1 + unet.launches_per_forward(**C.UNET) + 1) + 1) + 8 * (1 + vae_launches + 1) + 1
        assert p.last_launches() == want and own["launches"] == 1 + steps * (8 * 2 + 1) + 8 * 2 + 1
        assert tuple(own["groups"]) == sdx4.KERNEL_GROUPS and sdx4.KERNEL_GROUPS[:2] == ("prepare", "step")
        again, lat_again = call(p, guidance, steps)
        assert torch.equal(again, out) and torch.equal(lat_again, lat)
    # a VAE plan of its own: 16 / 0 has 2 x 3 windows
    before = p.vae.calls
    out2, lat2 = call(p, vae_tile=16, vae_overlap=0)
    assert p.vae.calls - before == 6 and torch.equal(lat2, call(p)[1]) and not torch.equal(out2, call(p)[0])
    assert p.workspace_bytes(2, T.H, T.W, C.TOKENS, tile=16, tile_overlap=8) > p.workspace_bytes(1, T.H, T.W, C.TOKENS, tile=16, tile_overlap=8) > 0


def test_a_frame_above_the_limit():                                                                     # (e)
    p, ids = pipe(), C.ids()
    h, w = 264, 256
    frame = C.frame(h, w, 76).to(DEV)
    noise, latents = C.draws(h, w, 77)
    kw = dict(prompt_ids=ids[1], negative_ids=ids[0], noise_level=C.NOISE_LEVEL, num_inference_steps=2, noise=noise.to(DEV), latents=latents.to(DEV))
    out = p.upscale(frame, tile=64, tile_overlap=8, **kw)
    assert tuple(out.shape) == (1056, 1024, 3) and out.dtype == torch.uint8 and float(out.float().std()) > 1.0
    assert torch.equal(p.upscale(frame, tile=64, tile_overlap=8, **kw), out)
    with pytest.raises(_lib.NesrHipError, match="65536"):
        p.upscale(frame, **kw)
    with pytest.raises(_lib.NesrUnsupportedError, match="65536"):
        p.upscale_frame(frame, prompt_ids=ids[1], negative_ids=ids[0], num_inference_steps=2)
    # upscale_frame with `tile` passes the limit, pads to the multiple and crops
    small = p.upscale_frame(C.frame(23, 37, 78).to(DEV), prompt_ids=ids[1], negative_ids=ids[0], noise_level=C.NOISE_LEVEL, num_inference_steps=2, tile=16, tile_overlap=8,
                            generator=torch.Generator(device=DEV).manual_seed(5))
    assert tuple(small.shape) == (92, 148, 3)


def test_the_vae_decodes_over_windows():                                                                # (f)
    p = pipe()
    lat64 = T.reference()[0]
    lat = lat64.float().to(DEV)
    got = p.vae.decode_latents_u8(lat, tile=T.TILE, tile_overlap=T.OVERLAP)
    assert torch.equal(got, composed_decode(p, lat[0].contiguous(), T.H, T.W, T.TILE, T.OVERLAP))
    args = (C.models()["vae"], lat.cpu(), T.TILE, T.OVERLAP)
    y64 = T.decode(*args)
    tol = 8.0 * float((T.decode(*args, torch.float32).double() - y64).abs().max())
    excluded, wrong, n = u8_check(got.cpu(), y64, tol)
    print(f"tiled decode: tol {tol:.3e}, {excluded} of {n} thin, {wrong} wrong")
    assert wrong == 0 and excluded <= C.MAX_THIN * n
    assert torch.equal(p.vae.decode_latents_u8(lat, tile=64), p.vae.decode_latents_u8(lat))      # one window: the untiled bytes
    big = torch.randn((1, 4, 264, 256), generator=torch.Generator().manual_seed(79)).mul(0.08333).to(DEV)
    with pytest.raises(_lib.NesrHipError, match="65536"):
        p.vae.decode_latents_u8(big)
    out = p.vae.decode_latents_u8(big, tile=64, tile_overlap=8)
    assert tuple(out.shape) == (1056, 1024, 3) and float(out.float().std()) > 1.0
    for kw, match in ((dict(tile=15), "tile must be a positive multiple of 2, got 15"), (dict(tile=16, tile_overlap=16), "tile_overlap must be"), (dict(tile=512), "exceeds NESR_VAE_MAX_TOKENS")):
        with pytest.raises(_lib.NesrHipError, match=match):
            p.vae.decode_latents_u8(torch.zeros((1, 4, 512, 512), device=DEV) if kw.get("tile") == 512 else lat, **kw)


def test_diffusion_stage_with_tiles_in_enhance_iterations():                                            # (g)
    p, ids = pipe(), C.ids()
    stage = nesr_adapter.diffusion_stage(p, prompt_ids=ids[1], negative_ids=ids[0], noise_level=C.NOISE_LEVEL, num_inference_steps=2, seed=11, tile=16, tile_overlap=8)
    before, trace = p.unet.calls, []
    image = C.frame(T.H, T.W, T.FRAME_SEED).numpy()
    out = nesr_adapter.enhance_iterations(None, image, config={"iterations": 1}, extra_upscalers=[stage], device=torch.device(DEV), trace=trace)
    assert isinstance(out, np.ndarray) and out.shape == (96, 160, 3) and out.dtype == np.uint8
    assert p.unet.calls - before == 2 * 8 and trace[0]["ensemble_n"] == 1 and trace[0]["out_shape"] == (96, 160)
    assert np.array_equal(out, stage(torch.from_numpy(image).to(DEV)).cpu().numpy())      # the seed: the same frame again


def test_an_fp16_unet_over_windows():                                                                   # (h)
    p = pipe("fp16")
    assert p.unet.compute_dtype == "fp16"
    out, lat = call(p, C.GUIDANCE, 2)
    want_out, want_lat = composed(p, C.GUIDANCE, 2)
    assert torch.equal(lat, want_lat) and torch.equal(out, want_out)
    # the specification's loop with the fp16 form's emulated forward (tests/unet_f16_emu.py), under that file's bound for a network
    lat64, emu64, bound = T.reference_f16(C.GUIDANCE, 2)
    err, own = float((lat.cpu().double() - lat64).abs().max()), float((lat.cpu().double() - emu64).abs().max())
    print(f"fp16 tiled: |gpu - f64| {err:.3e}, bound {bound:.3e}, err / bound {err / bound:.3f}, |gpu - emu64| {own:.3e}, |emu64 - f64| {float((emu64 - lat64).abs().max()):.3e}")
    assert err <= bound
    assert not torch.equal(lat, call(pipe(), C.GUIDANCE, 2)[1])      # the fp16 form ran, not the f32 one
    bad = pipe("fp16", 1e5)
    first, lat1 = call(bad, C.GUIDANCE, 1)                 # a first step alone: every operand in range
    assert bool(torch.isfinite(lat1).all())
    with pytest.raises(_lib.NesrRangeError, match="nesr_sdx4_upscale_tiled_u8") as info:
        call(bad, C.GUIDANCE, 2)
    assert str(info.value).count("65504") == 1
    assert torch.equal(call(bad, C.GUIDANCE, 1)[0], first)      # the word is cleared in front of the next call


def test_refusals_name_the_value_and_leave_the_sentinels():                                             # (i)
    p, lib = pipe(), _lib.load()
    handle = p._pipeline(torch.device(DEV))
    frame, noise, latents = T.crafted()
    frame, noise, latents = frame.to(DEV), noise.to(DEV), latents.to(DEV)
    cap = 4 * T.H * 4 * T.W * 3
    out = torch.full((cap + 64,), 201, dtype=torch.uint8, device=DEV)
    lat = torch.full((4 * T.H * T.W,), -777.0, device=DEV)
    ids = C.ids()
    host = (ctypes.c_int32 * ids.numel())(*ids.reshape(-1).tolist())
    good = dict(h=T.H, w=T.W, tile=16, overlap=8, vt=0, vo=-1, cap=cap, noise=noise.data_ptr())
    big = torch.zeros((512, 512, 3), dtype=torch.uint8, device=DEV)
    for change, match in ((dict(tile=15), "tile must be a positive multiple of 2, got 15"), (dict(tile=0), "tile must be"), (dict(overlap=16), "tile_overlap must be a multiple of 2 in 0 .. 15"),
                          (dict(overlap=3), "got 3"), (dict(vt=10, vo=12), "vae_tile_overlap must be"), (dict(vt=7), "vae_tile must be a positive multiple of 2, got 7"),
                          (dict(h=512, w=512, tile=512, overlap=0), "a window of 512 x 512 exceeds NESR_VAE_MAX_TOKENS"), (dict(h=23), "multiples of 2"),
                          (dict(h=4096, w=2048), "2^22"), (dict(cap=cap - 1), "capacity is " + str(cap - 1)), (dict(noise=noise.data_ptr() + 4), "aligned")):
        a = dict(good, **change)
        rc = lib.nesr_sdx4_upscale_tiled_u8(handle, ptr(big if a["h"] >= 512 else frame), a["h"], a["w"], host, C.TOKENS, ctypes.c_void_p(a["noise"]), ptr(latents), C.NOISE_LEVEL, 2,
                                            7.5, a["tile"], a["overlap"], a["vt"], a["vo"], ptr(out), a["cap"], ptr(lat), None)
        assert rc == _lib.ERR_ARG and match in lib.nesr_last_error().decode(), (change, lib.nesr_last_error())
    torch.cuda.synchronize()
    assert bool((out == 201).all()) and bool((lat == -777.0).all())
    with pytest.raises(ValueError, match="need tile"):
        p.upscale(frame, prompt_ids=ids[1], negative_ids=ids[0], tile_overlap=8)
    for kw, match in ((dict(vae_tile=0), "vae_tile must be positive"), (dict(vae_overlap=-1), "vae_overlap must not be negative")):
        with pytest.raises(ValueError, match=match):
            p.upscale(frame, prompt_ids=ids[1], negative_ids=ids[0], tile=16, tile_overlap=8, **kw)
