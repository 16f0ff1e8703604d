"""The x4 diffusion pipeline without a GPU.  None of the first group of checks depends on the transcription of tests/sdx4_ref.py:
the timestep tables, the alpha-bars' shape, the closed-form identity of the DDIM step and the guidance at g = 1 hold for the
restatement AND for the tables the library computes (nesr_sdx4_schedule, nesr_sdx4_noise_coefficients: host code, no device).  Then:
the library's tables against the restatement's, every named fault of the loop fails the crafted pipeline, the share of samples
u8_check may leave out stays under the cap, and the Python class's refusals.

The share recorded for the crafted frame (float32 CPU restatement against float64, printed by test_thin_samples_stay_under_the_cap):
guidance 7.5: 84 of 18432 samples thin (0.46 %), 0 wrong; guidance 1.0: 28 thin (0.15 %), 0 wrong; the cap is 2 %."""
import json
import math

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import ClipTextEncoder, StableDiffusionX4Upscaler, UNet2DCondition, VaeDecoder, _lib
from neural_enhanced_super_resolution_amd import sdx4 as S
from tests import sdx4_cases as C
from tests import sdx4_ref as R
from tests import vae_ref as VR
from tests.swin2sr_ref import u8_check


@pytest.fixture(scope="module", autouse=True)
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------- independent of the transcription
@pytest.mark.parametrize("N, ratio, first", [(10, 100, 901), (15, 66, 925), (20, 50, 951)])
def test_timestep_tables(N, ratio, first):
    want = [first - ratio * i for i in range(N)]
    assert want[-1] == 1 and R.timesteps(N).tolist() == want and S.schedule(N)[0].tolist() == want
    assert R.timesteps(N, steps_offset=0).tolist() == [w - 1 for w in want] == S.schedule(N, steps_offset=0)[0].tolist()


def test_alpha_bars_fall_from_one():
    abar, low = R.ddim_alpha_bars(), R.low_res_alpha_bars()
    assert abar[0] == 1.0 - 1e-4 and bool((np.diff(abar) < 0).all()) and 0 < abar[-1] < 0.01
    assert bool((np.diff(low) < 0).all()) and 0.999 < low[0] < 1 and 0 <= low[-1] < 1e-6
    ts, ab, _ = S.schedule(20)
    assert bool((ab[:, 0] < ab[:, 1]).all()) and bool((np.diff(ab[:, 0]) > 0).all())      # every step moves towards the image
    assert ab[-1, 1] == pytest.approx(1.0 - 1e-4, abs=1e-15)                                  # the final alpha-bar is alpha-bar[0]
    assert S.schedule(20, set_alpha_to_one=True)[1][-1, 1] == 1.0


@pytest.mark.parametrize("prediction", ["v_prediction", "epsilon"])
@pytest.mark.parametrize("N", [10, 15, 20])
def test_the_step_follows_the_closed_form(prediction, N):
    """A model that returns the true v (or the true epsilon) of a fixed (x0, eps): every step lands on sqrt(p) x0 + sqrt(1 - p) eps."""
    g = torch.Generator().manual_seed(71)
    x0, eps = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    abar = R.ddim_alpha_bars()
    ts, ab, co = S.schedule(N, prediction_type=prediction)
    x = x_lib = math.sqrt(abar[ts[0]]) * x0 + math.sqrt(1 - abar[ts[0]]) * eps
    for i, t in enumerate(R.timesteps(N)):
        a, p = R.step_alphas(t, N, abar)
        assert (a, p) == (pytest.approx(ab[i, 0], rel=1e-12), pytest.approx(ab[i, 1], rel=1e-12))
        model = (lambda s: math.sqrt(a) * eps - math.sqrt(1 - a) * x0) if prediction == "v_prediction" else (lambda s: eps)
        x = R.ddim_step(x, model(x), a, p, prediction)
        want = math.sqrt(p) * x0 + math.sqrt(1 - p) * eps
        assert float((x - want).abs().max()) < 1e-12
        c = co[i].astype(np.float64)                     # the library's six coefficients, f32: the same step to their rounding
        m = model(x_lib)
        x_lib = c[4] * (c[0] * x_lib + c[1] * m) + c[5] * (c[2] * x_lib + c[3] * m)
        assert float((x_lib - want).abs().max()) < 2e-6 * (i + 1)
    assert p == abar[0]                                  # the last step returns it at the final alpha-bar


def test_guidance_of_one_is_the_prompt_branch():
    g = torch.Generator().manual_seed(72)
    m = torch.randn((2, 4, 3, 5), generator=g, dtype=torch.float64)
    assert float((R.guide(m, 1.0) - m[1]).abs().max()) < 1e-15      # neg + (prompt - neg): the prompt, to a rounding
    assert torch.equal(R.guide(m[1:], 7.5), m[1])                    # and the pipeline runs g <= 1 as one sample: no combination at all
    assert float((R.guide(m, 7.5) - (m[0] + 7.5 * (m[1] - m[0]))).abs().max()) == 0 and not torch.equal(R.guide(m, 7.5, "guidance_order_swapped"), R.guide(m, 7.5))


def test_noise_coefficients_are_the_low_res_table():
    low = R.low_res_alpha_bars()
    for level in (0, 5, 20, 350, 999):
        ab, co = S.noise_coefficients(level)
        assert ab == pytest.approx(low[level], rel=1e-12) and co[0] == np.float32(math.sqrt(low[level])) and co[1] == np.float32(math.sqrt(1 - low[level]))
    f = lambda s: math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2
    assert low[0] == pytest.approx(f(1 / 1000) / f(0), rel=1e-14)


def test_the_library_s_tables_are_the_restatement_s():
    abar = R.ddim_alpha_bars()
    for N in (1, 3, 20, 500):
        ts, ab, co = S.schedule(N)
        assert ts.tolist() == R.timesteps(N).tolist()
        for i, t in enumerate(ts):
            a, p = R.step_alphas(t, N, abar)
            assert ab[i, 0] == pytest.approx(a, rel=1e-12) and ab[i, 1] == pytest.approx(p, rel=1e-12)
            want = [math.sqrt(a), -math.sqrt(1 - a), math.sqrt(1 - a), math.sqrt(a), math.sqrt(p), math.sqrt(1 - p)]
            assert np.allclose(co[i], np.array(want, dtype=np.float32), rtol=2e-7, atol=0)
    _, ab, co = S.schedule(20, prediction_type="epsilon")
    assert np.allclose(co[:, 0], 1 / np.sqrt(ab[:, 0]), rtol=2e-7) and np.allclose(co[:, 1], -np.sqrt(1 - ab[:, 0]) / np.sqrt(ab[:, 0]), rtol=2e-7)
    assert bool((co[:, 2] == 0).all()) and bool((co[:, 3] == 1).all())
    lin = S.schedule(20, beta_schedule="linear")[1]
    assert np.allclose(lin[:, 0], R.ddim_alpha_bars(beta_schedule="linear")[R.timesteps(20)], rtol=1e-12)


@pytest.mark.parametrize("fields, steps, error, match", [
    (dict(prediction_type="sample"), 20, _lib.NesrUnsupportedError, "prediction_type"),
    (dict(beta_schedule="squaredcos_cap_v2"), 20, _lib.NesrUnsupportedError, "beta_schedule"),
    (dict(timestep_spacing="trailing"), 20, _lib.NesrUnsupportedError, "timestep_spacing"),
    (dict(steps_offset=2), 20, _lib.NesrUnsupportedError, "steps_offset"),
    (dict(beta_start=0.0), 20, _lib.NesrUnsupportedError, "beta_start"),
    (dict(), 0, _lib.NesrHipError, "steps must be 1 .. 1000"),
    (dict(), 1001, _lib.NesrHipError, "steps must be 1 .. 1000"),
    (dict(), 1000, _lib.NesrHipError, "past the table"),
])
def test_schedules_the_library_refuses(fields, steps, error, match):
    with pytest.raises(error, match=match):
        S.schedule(steps, **fields)


def test_noise_levels_the_library_refuses():
    with pytest.raises(_lib.NesrHipError, match="noise_level must be 0 .. 999"):
        S.noise_coefficients(1000)
    with pytest.raises(_lib.NesrUnsupportedError, match="beta_schedule"):
        S.noise_coefficients(20, beta_schedule="linear")


# ---------------------------------------------------------------------------------------------- the crafted pipeline
@pytest.mark.parametrize("guidance", [C.GUIDANCE, 1.0])
def test_thin_samples_stay_under_the_cap(guidance):
    lat64, y64, tol_lat, tol, y32 = C.reference(guidance)
    excluded, wrong, n = u8_check(VR.quantise(y32), y64, tol)
    clamped = float(((y64 <= 0) | (y64 >= 1)).double().mean())
    print(f"guidance {guidance}: latents tol {tol_lat:.3e}, frame tol {tol:.3e}, {excluded} of {n} samples thin ({100.0 * excluded / n:.2f} %), {wrong} wrong (f32 CPU), "
          f"{100 * clamped:.1f} % on the clamp, latents std {float(lat64.std()):.3f}")
    assert tuple(y64.shape) == (4 * C.H, 4 * C.W, 3) and n >= 1000 and excluded <= C.MAX_THIN * n and wrong == 0 and tol_lat > 0
    assert clamped < 0.5 and float(y64.std()) > 0.02      # an image, not a constant


@pytest.mark.parametrize("fault", R.FAULTS)
def test_fault_fails_the_crafted_loop(fault):
    lat64, _, tol, _, _ = C.reference()
    noise, latents = C.draws()
    m = C.models()
    from tests import clip_text_ref as TR
    with torch.no_grad():
        text = TR.forward(m["text"][0], C.ids(), torch.float32, **m["text"][1])
    got = R.loop(m["unet"], C.frame(), text, noise, latents, C.NOISE_LEVEL, C.STEPS, C.GUIDANCE, torch.float32, fault=fault)
    err = float((got.double() - lat64).abs().max())
    print(f"{fault}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.1f}")
    assert err >= 8 * tol


def test_the_loop_with_a_known_model_lands_on_the_closed_form():
    """The whole loop of the restatement (image input, guidance of two equal branches, 3 steps) around a model that returns the true v."""
    noise, latents = C.draws()
    abar = R.ddim_alpha_bars()
    ts = R.timesteps(C.STEPS)
    a0 = abar[ts[0]]
    x0 = torch.randn((4, C.H, C.W), generator=torch.Generator().manual_seed(73), dtype=torch.float64)
    eps = (latents.double() - math.sqrt(a0) * x0) / math.sqrt(1 - a0)          # so that the initial latents ARE x_t of (x0, eps)
    seen = []

    def model(sample, t, text, label):
        seen.append((tuple(sample.shape), t, label))
        a = abar[int(t)]
        return (math.sqrt(a) * eps - math.sqrt(1 - a) * x0)[None].expand(sample.shape[0], -1, -1, -1)

    got = R.loop(None, C.frame(), torch.zeros(2, 7, 32), noise, latents, C.NOISE_LEVEL, C.STEPS, C.GUIDANCE, model=model)
    final = abar[0]
    assert float((got[0] - (math.sqrt(final) * x0 + math.sqrt(1 - final) * eps)).abs().max()) < 1e-10
    assert seen == [((2, 7, C.H, C.W), float(t), C.NOISE_LEVEL) for t in ts]


# ---------------------------------------------------------------------------------------------- the Python class
def networks():
    m = C.models()
    nets = []
    for cls, key in ((ClipTextEncoder, "text"), (UNet2DCondition, "unet"), (VaeDecoder, "vae")):
        net = cls(**m[key][1])
        net.load_state_dict(m[key][0])
        nets.append(net)
    return nets


def test_the_class_checks_its_parts():
    text, unet, vae = networks()
    with pytest.raises(TypeError, match="unet must be a UNet2DCondition"):
        StableDiffusionX4Upscaler(text, vae, vae)
    with pytest.raises(_lib.NesrUnsupportedError, match="EulerDiscreteScheduler"):
        StableDiffusionX4Upscaler(text, unet, vae, scheduler=dict(_class_name="EulerDiscreteScheduler"))
    with pytest.raises(_lib.NesrUnsupportedError, match="low_res_scheduler"):
        StableDiffusionX4Upscaler(text, unet, vae, low_res_scheduler=dict(_class_name="DDIMScheduler"))
    with pytest.raises(_lib.NesrUnsupportedError, match="thresholding"):
        StableDiffusionX4Upscaler(text, unet, vae, scheduler=dict(_class_name="DDIMScheduler", thresholding=True))
    pipe = StableDiffusionX4Upscaler(text, unet, vae, scheduler=dict(_class_name="DDIMScheduler", steps_offset=0, trained_betas=None), max_noise_level=31)
    assert pipe.scheduler["steps_offset"] == 0 and pipe.scheduler["prediction_type"] == "v_prediction" and pipe.tokenizer is None
    with pytest.raises(RuntimeError, match="prompt_ids"):
        pipe(prompt="a photograph", image=C.frame().numpy())
    with pytest.raises(RuntimeError, match="not on the ROCm device"):
        pipe.upscale(C.frame(), prompt_ids=C.ids()[1], negative_ids=C.ids()[0])
    with pytest.raises(_lib.NesrUnsupportedError, match="eta 0"):
        pipe(prompt_ids=C.ids()[1], image=C.frame().numpy(), eta=0.5)
    with pytest.raises(_lib.NesrUnsupportedError, match="callback"):
        pipe(prompt_ids=C.ids()[1], image=C.frame().numpy(), callback=print)
    with pytest.raises(_lib.NesrUnsupportedError, match="65536"):
        pipe.upscale_frame(torch.zeros((257, 256, 3), dtype=torch.uint8), prompt_ids=C.ids()[1], negative_ids=C.ids()[0])


def test_from_pretrained_reads_a_local_directory(tmp_path):
    save_file = pytest.importorskip("safetensors.torch").save_file
    m = C.models()
    from tests import clip_text_ref as TR
    for folder, key, name, sd in (("text_encoder", "text", "model.safetensors", TR.old_generation(m["text"][0], 77)),
                                  ("unet", "unet", "diffusion_pytorch_model.safetensors", m["unet"][0]), ("vae", "vae", "diffusion_pytorch_model.safetensors", m["vae"][0])):
        (tmp_path / folder).mkdir()
        save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / folder / name))
        (tmp_path / folder / "config.json").write_text(json.dumps(m[key][1]))
    for folder, cfg in (("scheduler", dict(R.DDIM, _class_name="DDIMScheduler", _diffusers_version="0.0")), ("low_res_scheduler", dict(R.LOW_RES, _class_name="DDPMScheduler"))):
        (tmp_path / folder).mkdir()
        (tmp_path / folder / "scheduler_config.json").write_text(json.dumps(cfg))
    (tmp_path / "model_index.json").write_text(json.dumps(dict(_class_name="StableDiffusionUpscalePipeline", max_noise_level=31)))
    pipe = StableDiffusionX4Upscaler.from_pretrained(tmp_path)
    assert pipe.tokenizer is None and pipe.max_noise_level == 31 and pipe.scheduler == R.DDIM and pipe.low_res_scheduler == R.LOW_RES
    assert pipe.unet.config["block_out_channels"] == (32, 64) and pipe.text_encoder.config["hidden_size"] == 32 and pipe.vae.config["block_out_channels"] == (32, 32, 64)
    assert all(torch.equal(v, m["text"][0][k]) for k, v in pipe.text_encoder.state_dict().items())
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(_class_name="PNDMScheduler")))
    with pytest.raises(_lib.NesrUnsupportedError, match="PNDMScheduler"):
        StableDiffusionX4Upscaler.from_pretrained(tmp_path)
    with pytest.raises(FileNotFoundError, match="not fetched"):
        StableDiffusionX4Upscaler.from_pretrained("stabilityai/stable-diffusion-x4-upscaler")
