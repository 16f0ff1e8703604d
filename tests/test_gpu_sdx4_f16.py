"""GPU: `StableDiffusionX4Upscaler` with a UNet in its fp16 compute form, on the crafted pipeline of tests/sdx4_cases.py.

  composed   one `upscale` call equals, bit for bit in latents and frame, the loop composed in Python from the text encoder, the
             same fp16 `UNet2DCondition.forward`, the two kernel hooks with the pipeline's own coefficients and the VAE decoder:
             2 and 3 steps, guidance 7.5 and 1
  launches   text + 1 + steps (UNet + 1) + VAE: the f32 pipeline's formula
  range      a UNet whose conv_out is scaled by 1e5 and whose last GroupNorm gain by 100 has every operand in range during a
             step (conv_out reads silu of at most a few hundred, its weights stay below 65504) and predicts noise of the order
             of 1e7: `upscale` with one step returns, with two steps the second step's conv_in rounds latents beyond 65504 and
             the call raises NesrRangeError, once, after its last launch
"""
import ctypes

import pytest
import torch

from neural_enhanced_super_resolution_amd import ClipTextEncoder, StableDiffusionX4Upscaler, UNet2DCondition, VaeDecoder, _lib
from neural_enhanced_super_resolution_amd import clip_text, sdx4, unet
from tests import sdx4_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


def pipe(conv_out_scale=1.0):
    if conv_out_scale not in _cache:
        m = C.models()
        text = ClipTextEncoder(**m["text"][1]).to(DEV)
        text.load_state_dict(m["text"][0])
        vae = VaeDecoder(**m["vae"][1]).to(DEV)
        vae.load_state_dict(m["vae"][0])
        sd = {k: v.clone() for k, v in m["unet"][0].items()}
        for key in ("conv_out.weight", "conv_out.bias"):
            sd[key] *= conv_out_scale
        if conv_out_scale != 1.0:
            assert float(sd["conv_out.weight"].abs().max()) < 65504.0
            sd["conv_norm_out.weight"] *= 100.0
        net = UNet2DCondition(compute_dtype="fp16", **m["unet"][1]).to(DEV)
        net.load_state_dict(sd)
        _cache[conv_out_scale] = StableDiffusionX4Upscaler(text, net, vae, max_noise_level=C.MAX_NOISE_LEVEL)
    return _cache[conv_out_scale]


def call(p, guidance, steps):
    noise, latents = C.draws()
    ids = C.ids()
    return p.upscale(C.frame().to(DEV), prompt_ids=ids[1], negative_ids=ids[0], noise_level=C.NOISE_LEVEL, num_inference_steps=steps, guidance_scale=guidance,
                     noise=noise.to(DEV), latents=latents.to(DEV), return_latents=True)


def composed(p, guidance, steps):
    lib = _lib.load()
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
    ts, _, coef = sdx4.schedule(steps)
    for i, t in enumerate(ts):
        m = p.unet(sample, float(t), text, C.NOISE_LEVEL)
        co = (ctypes.c_float * 6)(*[float(v) for v in coef[i]])
        _lib.check(lib.nesr_sdx4_k_step(ptr(m), ptr(lat), n, hw, 4, float(guidance), co, ptr(lat), ptr(sample), stream), "nesr_sdx4_k_step")
    return p.vae.decode_latents_u8(lat[None]), lat[None].clone()


@pytest.mark.parametrize("steps", [2, 3])
@pytest.mark.parametrize("guidance", [C.GUIDANCE, 1.0])
def test_upscale_is_the_loop_composed_from_the_fp16_forward(guidance, steps):
    p = pipe()
    assert p.unet.compute_dtype == "fp16"
    out, lat = call(p, guidance, steps)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (4 * C.H, 4 * C.W, 3) and tuple(lat.shape) == (1, 4, C.H, C.W)
    want_out, want_lat = composed(p, guidance, steps)
    assert torch.equal(lat, want_lat) and torch.equal(out, want_out)
    again, lat_again = call(p, guidance, steps)
    assert torch.equal(again, out) and torch.equal(lat_again, lat)


def test_launch_count_is_the_f32_pipelines_formula():
    p = pipe()
    p.vae.kernel_time_ms()
    p.vae.decode_latents_u8(torch.zeros((1, 4, C.H, C.W), device=DEV))
    vae_launches = p.vae.kernel_time_ms()["launches"]
    for guidance, steps in ((C.GUIDANCE, 3), (1.0, 2)):
        call(p, guidance, steps)
        assert p.last_launches() == clip_text.launches_per_forward(**C.TEXT) + 1 + steps * (unet.launches_per_forward(**C.UNET) + 1) + vae_launches


def test_an_overflow_inside_step_two_raises_once_after_the_call():
    p = pipe(1e5)
    out, lat = call(p, C.GUIDANCE, 1)                     # a first step alone: every operand in range
    assert bool(torch.isfinite(lat).all())
    with pytest.raises(_lib.NesrRangeError, match="nesr_sdx4_upscale_u8") as info:
        call(p, C.GUIDANCE, 2)
    assert str(info.value).count("65504") == 1
    good, _ = call(p, C.GUIDANCE, 1)                      # the word is cleared in front of the next call
    assert torch.equal(good, out)
