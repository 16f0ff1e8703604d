"""GPU: `StableDiffusionX4Upscaler` on the crafted pipeline of tests/sdx4_cases.py (text hidden 32 x 2 layers, UNet (32, 64), VAE
(32, 32, 64); a 16 x 24 frame -> 64 x 96, 3 steps, noise level 5).

  (a) composed    one `upscale` call equals, bit for bit in latents and frame, the same loop composed in Python from ClipTextEncoder,
                  UNet2DCondition.forward, the two kernel hooks and VaeDecoder.decode_latents_u8
  (b) float64     the final latents within 8 x max |float32 restatement - float64| of the float64 loop; the frame passes u8_check
                  with 0 wrong, at most 2 % left out (84 of 18432 samples, 0.46 %, at guidance 7.5; 28, 0.15 %, at guidance 1:
                  tests/test_sdx4_host.py)
  (c) guidance 1  runs n = 1 and matches its own reference
  (d) repeats     a repeated call gives the same bits; a generator seed gives the same frame twice
  (e) launches    text + 1 + steps (UNet + 1) + VAE, asserted on the device
  (f) __call__    an ndarray, and a 13 x 18 frame (pad, crop) -> .images[0] of 52 x 72
  (g) stage       diffusion_stage inside enhance_iterations(extra_upscalers=[...]); the UNet ran once a step
  (h) refusals    every refusal leaves the sentinels intact
"""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import ClipTextEncoder, StableDiffusionX4Upscaler, UNet2DCondition, VaeDecoder, _lib, nesr_adapter
from neural_enhanced_super_resolution_amd import clip_text, sdx4, unet
from tests import sdx4_cases as C
from tests.swin2sr_ref import u8_check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


def pipe():
    if "pipe" not in _cache:
        m = C.models()
        nets = []
        for cls, key in ((ClipTextEncoder, "text"), (UNet2DCondition, "unet"), (VaeDecoder, "vae")):
            net = cls(**m[key][1]).to(DEV)
            net.load_state_dict(m[key][0])
            nets.append(net)
        _cache["pipe"] = StableDiffusionX4Upscaler(*nets, max_noise_level=C.MAX_NOISE_LEVEL)
    return _cache["pipe"]


def call(guidance=C.GUIDANCE, **kw):
    noise, latents = C.draws()
    ids = C.ids()
    return pipe().upscale(C.frame().to(DEV), prompt_ids=ids[1], negative_ids=ids[0], noise_level=C.NOISE_LEVEL, num_inference_steps=C.STEPS, guidance_scale=guidance,
                          noise=noise.to(DEV), latents=latents.to(DEV), return_latents=True, **kw)


def composed(guidance):
    """The same loop from the parts: the three networks' own forwards and the two kernel hooks."""
    p, lib = pipe(), _lib.load()
    noise, latents = C.draws()
    noise, latents, frame = noise.to(DEV), latents.to(DEV), C.frame().to(DEV)
    ids = C.ids() if guidance > 1.0 else C.ids()[1:]
    n, hw = ids.shape[0], C.H * C.W
    text = p.text_encoder(ids, device=DEV)
    sample = torch.empty((n, 7, C.H, C.W), dtype=torch.float32, device=DEV)
    lat = torch.empty((4, C.H, C.W), dtype=torch.float32, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sa, sb = sdx4.noise_coefficients(C.NOISE_LEVEL)[1]
    _lib.check(lib.nesr_sdx4_k_prepare(ptr(frame), ptr(noise), ptr(latents), n, hw, 4, float(sa), float(sb), 1.0, ptr(sample), ptr(lat), stream), "nesr_sdx4_k_prepare")
    ts, _, coef = sdx4.schedule(C.STEPS)
    for i, t in enumerate(ts):
        m = p.unet(sample, float(t), text, C.NOISE_LEVEL)
        co = (ctypes.c_float * 6)(*[float(v) for v in coef[i]])
        _lib.check(lib.nesr_sdx4_k_step(ptr(m), ptr(lat), n, hw, 4, float(guidance), co, ptr(lat), ptr(sample), stream), "nesr_sdx4_k_step")
    return p.vae.decode_latents_u8(lat[None]), lat[None].clone()


@pytest.mark.parametrize("guidance", [C.GUIDANCE, 1.0])
def test_upscale_is_the_composed_loop_and_the_float64_loop(guidance):
    out, lat = call(guidance)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (4 * C.H, 4 * C.W, 3) and tuple(lat.shape) == (1, 4, C.H, C.W)
    want_out, want_lat = composed(guidance)
    assert torch.equal(lat, want_lat) and torch.equal(out, want_out)                                   # (a), and (c) at guidance 1
    lat64, y64, tol_lat, tol, _ = C.reference(guidance)
    err = float((lat.cpu().double() - lat64).abs().max())
    excluded, wrong, n = u8_check(out.cpu(), y64, tol)
    print(f"guidance {guidance}: latents err {err:.3e}, tol {tol_lat:.3e}, err / tol {err / tol_lat:.3f}; frame: {excluded} of {n} thin, {wrong} wrong")
    assert err <= tol_lat and wrong == 0 and excluded <= C.MAX_THIN * n                                 # (b)
    again, lat_again = call(guidance)
    assert torch.equal(again, out) and torch.equal(lat_again, lat)                                     # (d)


def test_a_generator_seed_gives_the_same_frame_twice():
    ids, frame = C.ids(), C.frame().to(DEV)
    frames = []
    for seed in (7, 7, 8):
        g = torch.Generator(device=DEV).manual_seed(seed)
        frames.append(pipe().upscale(frame, prompt_ids=ids[1], negative_ids=ids[0], noise_level=C.NOISE_LEVEL, num_inference_steps=2, generator=g))
    assert torch.equal(frames[0], frames[1]) and not torch.equal(frames[0], frames[2])


def test_launch_count_is_the_sum_of_the_parts():
    p = pipe()
    p.vae.kernel_time_ms()
    p.vae.decode_latents_u8(torch.zeros((1, 4, C.H, C.W), device=DEV))
    vae_launches = p.vae.kernel_time_ms()["launches"]
    for guidance, steps in ((C.GUIDANCE, C.STEPS), (1.0, 2)):
        noise, latents = C.draws()
        p.kernel_time_ms()
        p.upscale(C.frame().to(DEV), prompt_ids=C.ids()[1], negative_ids=C.ids()[0], noise_level=C.NOISE_LEVEL, num_inference_steps=steps, guidance_scale=guidance,
                  noise=noise.to(DEV), latents=latents.to(DEV))
        want = clip_text.launches_per_forward(**C.TEXT) + 1 + steps * (unet.launches_per_forward(**C.UNET) + 1) + vae_launches
        assert p.last_launches() == want and p.kernel_time_ms()["launches"] == 1 + steps
    assert p.workspace_bytes(2, C.H, C.W, C.TOKENS) > p.workspace_bytes(1, C.H, C.W, C.TOKENS) > 0


def test_the_reference_s_call():
    p, ids = pipe(), C.ids()
    res = p(prompt_ids=ids[1], negative_ids=ids[0], image=C.frame().numpy(), noise_level=C.NOISE_LEVEL, num_inference_steps=2, guidance_scale=7.5,
            generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    img = np.array(res.images[0])
    assert isinstance(res.images[0], np.ndarray) and img.dtype == np.uint8 and img.shape == (64, 96, 3)
    small = p(prompt_ids=ids[1], negative_ids=ids[0], image=C.frame(13, 18).numpy(), noise_level=C.NOISE_LEVEL, num_inference_steps=2, device=DEV).images[0]
    assert small.shape == (52, 72, 3) and small.dtype == np.uint8 and small.std() > 0
    with pytest.raises(RuntimeError, match="prompt_ids"):
        p(prompt="a photograph", image=C.frame().numpy())


def test_diffusion_stage_in_enhance_iterations():
    p, ids = pipe(), C.ids()
    stage = nesr_adapter.diffusion_stage(p, prompt_ids=ids[1], negative_ids=ids[0], noise_level=C.NOISE_LEVEL, num_inference_steps=2, seed=11)
    before, trace = p.unet.calls, []
    out = nesr_adapter.enhance_iterations(None, C.frame().numpy(), config={"iterations": 1}, extra_upscalers=[stage], device=torch.device(DEV), trace=trace)
    assert isinstance(out, np.ndarray) and out.shape == (64, 96, 3) and out.dtype == np.uint8
    assert p.unet.calls - before == 2 and trace[0]["ensemble_n"] == 1 and trace[0]["out_shape"] == (64, 96)
    assert np.array_equal(out, stage(C.frame().to(DEV)).cpu().numpy())      # the seed: the same frame again
    with pytest.raises(_lib.NesrUnsupportedError, match="65536"):
        stage(torch.zeros((264, 256, 3), dtype=torch.uint8, device=DEV))


def test_refusals_leave_the_sentinels_intact():
    p, lib = pipe(), _lib.load()
    handle = p._pipeline(torch.device(DEV))
    noise, latents = C.draws()
    noise, latents, frame = noise.to(DEV), latents.to(DEV), C.frame().to(DEV)
    out = torch.full((4 * C.H * 4 * C.W * 3 + 64,), 201, dtype=torch.uint8, device=DEV)
    lat = torch.full((4 * C.H * C.W,), -777.0, device=DEV)
    ids = C.ids()
    host = lambda t: (ctypes.c_int32 * t.numel())(*t.reshape(-1).tolist())
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(h=C.H, w=C.W, ids=ids, tokens=C.TOKENS, level=C.NOISE_LEVEL, steps=C.STEPS, g=7.5, cap=4 * C.H * 4 * C.W * 3)
    bad_ids = ids.clone()
    bad_ids[1, 3] = 50
    for change, match in ((dict(h=15), "multiples of 2"), (dict(w=0), "multiples of 2"), (dict(h=512, w=256), "NESR_VAE_MAX_TOKENS"), (dict(tokens=78), "tokens must be"),
                          (dict(tokens=0), "tokens must be"), (dict(ids=bad_ids), "id 50 at position 3 of sample 1"), (dict(level=32), "noise_level must be 0 .. 31"),
                          (dict(level=-1), "noise_level"), (dict(steps=0), "steps must be"), (dict(steps=1000), "past the table"), (dict(g=float("nan")), "guidance_scale"),
                          (dict(cap=4 * C.H * 4 * C.W * 3 - 1), "capacity")):
        a = dict(good, **change)
        rc = lib.nesr_sdx4_upscale_u8(handle, ptr(frame), a["h"], a["w"], host(a["ids"]), a["tokens"], ptr(noise), ptr(latents), a["level"], a["steps"], a["g"], ptr(out),
                                      a["cap"], ptr(lat), None)
        assert rc == _lib.ERR_ARG and match in lib.nesr_last_error().decode(), (change, lib.nesr_last_error())
    rc = lib.nesr_sdx4_upscale_u8(handle, ptr(frame), C.H, C.W, host(ids), C.TOKENS, ctypes.c_void_p(noise.data_ptr() + 4), ptr(latents), 5, 3, 7.5, ptr(out), good["cap"],
                                  ptr(lat), None)
    assert rc == _lib.ERR_ARG and "aligned" in lib.nesr_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 201).all()) and bool((lat == -777.0).all())
    # what nesr_sdx4_create refuses: parts that do not fit each other, scheduler fields by name
    m = C.models()
    wide = ClipTextEncoder(**dict(C.TEXT, hidden_size=64)).to(DEV)
    with pytest.raises(_lib.NesrHipError, match="cross_attention_dim 32 is not the text encoder's hidden_size 64"):
        StableDiffusionX4Upscaler(wide, p.unet, p.vae, max_noise_level=31)._pipeline(torch.device(DEV))
    with pytest.raises(_lib.NesrHipError, match="class table of 32"):
        StableDiffusionX4Upscaler(p.text_encoder, p.unet, p.vae)._pipeline(torch.device(DEV))      # max_noise_level 350
    vae2 = VaeDecoder(**dict(C.VAE, latent_channels=5)).to(DEV)
    with pytest.raises(_lib.NesrHipError, match="in_channels 7 is not the VAE's latent_channels 5"):
        StableDiffusionX4Upscaler(p.text_encoder, p.unet, vae2, max_noise_level=31)._pipeline(torch.device(DEV))
    with pytest.raises(_lib.NesrUnsupportedError, match="clip_sample"):
        StableDiffusionX4Upscaler(p.text_encoder, p.unet, p.vae, scheduler=dict(clip_sample=True), max_noise_level=31)._pipeline(torch.device(DEV))
    with pytest.raises(_lib.NesrUnsupportedError, match="prediction_type"):
        StableDiffusionX4Upscaler(p.text_encoder, p.unet, p.vae, scheduler=dict(prediction_type="sample"), max_noise_level=31)._pipeline(torch.device(DEV))
