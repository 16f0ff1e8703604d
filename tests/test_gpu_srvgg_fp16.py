"""GPU: SRVGGNetCompact's fp16 compute form (compute_dtype="fp16", NESR_DTYPE_F16): bf16's kernels of srvgg_compact.hip on f16
elements (v_mfma_f32_16x16x32_f16, f16 storage rounded to nearest even, f32 accumulation) -- upstream's half=True numerics.

Two conditions carry the accuracy tests, both measured in the test itself on the same input:
  (a) PSNR against the float64 reference (tests/srvgg_ref.py) >= the bf16 form's + 12 dB: two of the three extra mantissa bits;
  (b) mean |kernel - emulation| < mean |emulation - float64 reference|, the emulation being tests/srvgg_fp16_emu.py: only the
      order of the f32 accumulation separates the kernel from it, so the kernel sits closer to its specification than the
      specification sits to the exact network.  An operand of another type, a store that does not round to nearest or a
      missing rounding moves the kernel away from the emulation by about the form's whole error.
Measured values (MI355X) are in DESIGN.md section 8.

(b) is one image-wide mean, which a correct kernel meets by a tenth at 16 to 32 layers and which a single layer's wrong
rounding passes at 2.  The per-value and the local checks of this form are in test_gpu_srvgg_pin.py (each layer kind pinned
to the rounded float64 value, from 1 x 1 to 289 tiles on resident weights; tests/srvgg_pin.py) and test_gpu_srvgg_emu16.py
(the same emulation with the maximum, per-band and mean conditions of rrdbnet_emu16.conditions)."""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import RealESRGANer, SRVGGNetCompact, _lib
from neural_enhanced_super_resolution_amd.realesrganer import normalize_u8_on_device
from neural_enhanced_super_resolution_amd.synth import synthetic_compact_state_dict, synthetic_frame
from oracle.realesrganer_ref import RealESRGANerRef
from tests.srvgg_fp16_emu import SRVGGEmu16
from tests.srvgg_ref import SRVGGRef

pytestmark = pytest.mark.gpu

X4V3 = dict(num_conv=32, upscale=4, act_type="prelu")           # realesr-general-x4v3
ANIME = dict(num_conv=16, upscale=4, act_type="prelu")          # realesr-animevideov3
RELU2 = dict(num_conv=16, upscale=2, act_type="relu")
SMALL = dict(num_conv=2, upscale=4, act_type="prelu")
TILE_H = 16                                                     # output rows of a workgroup's tile (32 columns), as bf16's

_cache = {}


def nets(cfg, seed=0, dtype="fp16"):
    key = (tuple(sorted(cfg.items())), seed, dtype)
    if key not in _cache:
        sd = synthetic_compact_state_dict(seed=seed, **cfg)
        ours = SRVGGNetCompact(**cfg, compute_dtype=dtype).to("cuda:0")
        ours.load_state_dict(sd)
        _cache[key] = ours
    return _cache[key]


def cpu_nets(cfg, seed=0):
    key = (tuple(sorted(cfg.items())), seed, "cpu")
    if key not in _cache:
        sd = synthetic_compact_state_dict(seed=seed, **cfg)
        ref, emu = SRVGGRef(**cfg), SRVGGEmu16(**cfg, store=torch.float16)
        ref.load_state_dict(sd)
        emu.load_state_dict(sd)
        _cache[key] = (ref, emu)
    return _cache[key]


def image_batch(n, h, w, seed=0):
    return torch.stack([torch.from_numpy(synthetic_frame(h, w, seed=seed + i)).permute(2, 0, 1).float() / 255 for i in range(n)])


def psnr(a, b):
    mse = float(((torch.as_tensor(a).double() - torch.as_tensor(b).double()) ** 2).mean())
    return 10 * np.log10(1.0 / max(mse, 1e-30))


def check_two_conditions(cfg, shape, seed, img_seed, tag):
    x = image_batch(*shape, seed=img_seed)
    f16, bf16 = nets(cfg, seed), nets(cfg, seed, "bf16")
    ref, emu = cpu_nets(cfg, seed)
    y16 = f16(x.to("cuda:0")).cpu().double()
    f16.check_range()
    ybf = bf16(x.to("cuda:0")).cpu().double()
    with torch.no_grad():
        want, spec = ref(x.double()), emu(x.double())
    p16, pbf = psnr(y16, want), psnr(ybf, want)
    to_spec, spec_err = float((y16 - spec).abs().mean()), float((spec - want).abs().mean())
    print(f"{tag} {cfg} {shape}: fp16 PSNR {p16:.2f} dB (mean abs {float((y16 - want).abs().mean()):.2e}), bf16 PSNR {pbf:.2f} dB, "
          f"mean |kernel - emulation| {to_spec:.2e}, mean |emulation - f64| {spec_err:.2e}, emulation PSNR {psnr(spec, want):.2f} dB")
    assert y16.shape == want.shape and bool(torch.isfinite(y16).all())
    assert p16 >= pbf + 12.0, (p16, pbf)
    assert to_spec < spec_err, (to_spec, spec_err)


# ------------------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("cfg,shape", [(X4V3, (2, 67, 93)), (ANIME, (2, 67, 93)), (RELU2, (2, 67, 93)), (X4V3, (1, 37, 53))])
def test_fp16_against_f64_reference_bf16_and_emulation(cfg, shape):
    """67 x 93: partial tiles in both directions (16 x 32 tiles), two images."""
    check_two_conditions(cfg, shape, 0, 3, "net")


# ------------------------------------------------------------------------------------------------------------ 2. tile loop
def tiles(n, h, w):
    return n * -(-h // TILE_H) * -(-w // 32)


def test_many_tiles_per_workgroup_meet_both_conditions():
    n, h, w = 1, 264, 528
    assert tiles(n, h, w) > torch.cuda.get_device_properties(0).multi_processor_count
    check_two_conditions(SMALL, (n, h, w), 4, 9, f"{tiles(n, h, w)} tiles")


def test_tile_loop_is_bitwise_one_tile_per_workgroup():
    """24 images of 64 x 96 in one batch (288 tiles: every workgroup walks several) against each image alone (12 tiles: one per
    workgroup): any state a workgroup carries from one tile into the next, the range accumulator included, shows as a bit."""
    n, h, w = 24, 64, 96
    assert tiles(n, h, w) > torch.cuda.get_device_properties(0).multi_processor_count > tiles(1, h, w)
    ours = nets(SMALL, seed=5)
    xs = image_batch(n, h, w, seed=30).to("cuda:0")
    batch = ours(xs)
    alone = torch.cat([ours(xs[i:i + 1].contiguous()) for i in range(n)])
    ours.check_range()
    assert torch.equal(batch, alone)
    assert not torch.equal(batch, nets(SMALL, seed=5, dtype="bf16")(xs))        # (and it is not the bf16 kernel that ran)


# ------------------------------------------------------------------------------------------------------------ 3. u8 output
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("rnd", [True, False])
def test_forward_u8_is_forward_then_the_torch_quantiser(flip, rnd):
    ours = nets(X4V3)
    img = torch.from_numpy(synthetic_frame(45, 71, seed=7)).to("cuda:0")
    y8 = ours.forward_u8(img, flip_rgb=flip, round_nearest=rnd)
    x = normalize_u8_on_device(img.permute(2, 0, 1))
    if flip:
        x = x.flip(0)
    y = ours(x[None].contiguous())[0]
    if flip:
        y = y.flip(0)
    q = y.clamp(0, 1).permute(1, 2, 0) * 255.0
    q = (q.round() if rnd else q).to(torch.uint8)
    ours.check_range()
    assert torch.equal(y8, q)


# ------------------------------------------------------------------------------------------------------------ 4. range
def test_weight_beyond_f16_is_refused_at_finalize():
    sd = synthetic_compact_state_dict(seed=2, **SMALL)
    sd["body.2.weight"][5, 7, 1, 2] = 7.0e4
    m = SRVGGNetCompact(**SMALL, compute_dtype="fp16").to("cuda:0")
    m.load_state_dict(sd)
    with pytest.raises(_lib.NesrRangeError, match=r"body\.2\.weight.*65504"):
        m(image_batch(1, 24, 24).to("cuda:0"))
    ok = SRVGGNetCompact(**SMALL, compute_dtype="bf16").to("cuda:0")          # bf16 has f32's range: the same weights load
    ok.load_state_dict(sd)
    ok(image_batch(1, 24, 24).to("cuda:0"))
    ok.check_status()


def _overflowing(where):
    """SMALL's weights with one layer scaled so that its stored activations leave +-65504 while every weight stays inside:
    "first": the first conv; "last": the last body layer, whose output only the tail reads."""
    sd = synthetic_compact_state_dict(seed=6, **SMALL)
    key = "body.0" if where == "first" else f"body.{2 * SMALL['num_conv']}"
    gain = 6.0e4 / float(sd[key + ".weight"].abs().max())
    sd[key + ".weight"] = sd[key + ".weight"] * gain
    sd[key + ".bias"] = sd[key + ".bias"] * gain
    return sd, (0 if where == "first" else SMALL["num_conv"])


@pytest.mark.parametrize("where", ["first", "last"])
def test_activation_beyond_f16_gives_nan_and_range_error_then_a_clean_forward(where):
    sd, layer = _overflowing(where)
    x = image_batch(1, 40, 72)
    ref = SRVGGRef(**SMALL)
    ref.load_state_dict(sd)
    pre = []
    with torch.no_grad():
        ref(x.double(), pre)
    tops = [float(p.max()) for p in pre]                      # positive values pass the activation unchanged
    assert tops[layer] > 2 * 65504 and all(t < 65504 / 4 for t in tops[:layer]), tops
    m = SRVGGNetCompact(**SMALL, compute_dtype="fp16").to("cuda:0")
    m.load_state_dict(sd)
    y = m(x.to("cuda:0"))
    assert bool(torch.isnan(y).all()), "an out-of-range forward must not return a plausible image"
    with pytest.raises(_lib.NesrRangeError, match="f16 path"):
        m.check_range()
    m.check_range()                                           # reported once
    m.load_state_dict(synthetic_compact_state_dict(seed=6, **SMALL))
    y = m(x.to("cuda:0"))
    m.check_range()
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -1.0e5])
def test_bad_input_is_caught_by_the_pack_kernel(bad):
    """The first conv reads the f16 image the pack kernel staged: the pack kernel is what checks it.  One bad pixel reaches few
    outputs through the convs, yet the whole output is NaN."""
    m = nets(SMALL, seed=6)
    x = image_batch(1, 40, 72)
    x[0, 1, 20, 30] = bad
    y = m(x.to("cuda:0"))
    assert bool(torch.isnan(y).all())
    with pytest.raises(_lib.NesrRangeError):
        m.check_range()
    y = m(image_batch(1, 40, 72).to("cuda:0"))
    m.check_range()
    assert bool(torch.isfinite(y).all())


def test_cabi_dtype_4_context(cuda_device):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.nesr_create_compact(ctypes.byref(h), 0, 3, 3, 64, 2, 4, _lib.ACT_PRELU, _lib.DTYPE_F16) == 0
    b = ctypes.c_void_p()
    assert lib.nesr_create_compact(ctypes.byref(b), 0, 3, 3, 64, 2, 4, _lib.ACT_PRELU, _lib.DTYPE_BF16) == 0
    try:
        assert lib.nesr_num_tensors(h) == 2 * 4 + 3
        assert lib.nesr_workspace_bytes(h, 2, 67, 93) == lib.nesr_workspace_bytes(b, 2, 67, 93) > 0       # the 16-bit layout
        assert lib.nesr_forward_flops(h, 2, 67, 93) == lib.nesr_forward_flops(b, 2, 67, 93) > 0
        assert lib.nesr_check_range(h, None) == 0
    finally:
        lib.nesr_destroy(h)
        lib.nesr_destroy(b)


# ------------------------------------------------------------------------------------------------------------ 5. wrapper
def frame(kind, h, w, seed=0):
    img = synthetic_frame(h, w, seed=seed)
    if kind == "bgra":
        return np.concatenate([img, synthetic_frame(h, w, seed=seed + 50)[:, :, :1]], axis=2)
    if kind == "u16":
        return img.astype(np.uint16) * 257 + np.uint16(seed)
    return img


def wrapper(sd, dtype=None, ref=False, **kw):
    if ref:
        return RealESRGANerRef(scale=4, model_path={"params": sd}, model=SRVGGRef(**X4V3), **kw)
    model = SRVGGNetCompact(**X4V3) if dtype is None else SRVGGNetCompact(**X4V3, compute_dtype=dtype)
    return RealESRGANer(scale=4, model_path={"params": {k: v.clone() for k, v in sd.items()}}, model=model, half=True, device="cuda:0", **kw)


WRAPPER = [("bgr", 0, 0, 96, 128), ("bgr", 64, 0, 96, 128), ("bgra", 0, 10, 40, 52), ("u16", 0, 10, 29, 39)]


@pytest.mark.parametrize("kind,tile,pre_pad,h,w", WRAPPER)
def test_wrapper_half_with_an_fp16_model_against_reference(kind, tile, pre_pad, h, w):
    """RealESRGANer(half=True) with an fp16 model against RealESRGANerRef, and beside it half=True with a default model (bf16).

    Condition (a) is asserted on the image the wrapper computes, enhance_float(), and on a 16-bit enhance() result, whose
    step (1.5e-5) is far below either form's error.  An 8-bit enhance() result differs from the reference's only where the
    error carries a value across a rounding boundary; the share of such values, and with it the mean square difference, is
    proportional to the error, not to its square, so the 12 dB of (a) are 6 dB there: that is what is asserted on 8 bits."""
    sd = synthetic_compact_state_dict(seed=1, **X4V3)
    kw = dict(tile=tile, tile_pad=10, pre_pad=pre_pad)
    img = frame(kind, h, w, seed=h)
    f16, bf16, ref = wrapper(sd, "fp16", **kw), wrapper(sd, **kw), wrapper(sd, ref=True, **kw)
    assert f16.model.compute_dtype == "fp16" and bf16.model.compute_dtype == "bf16"
    want, want_mode = ref.enhance(img)
    want_f, _, _ = ref.enhance_float(img)
    top = float(np.iinfo(img.dtype).max)
    p, pf = {}, {}
    for name, up in (("fp16", f16), ("bf16", bf16)):
        out, mode = up.enhance(img)
        out_f, _, _ = up.enhance_float(img)
        assert mode == want_mode and out.shape == want.shape and out.dtype == want.dtype and out_f.shape == want_f.shape
        p[name], pf[name] = psnr(out / top, want / top), psnr(out_f, want_f)
        assert up.model.calls > 0
    print(f"wrapper {kind} tile={tile} pre_pad={pre_pad} {h}x{w}: enhance_float fp16 {pf['fp16']:.2f} dB, bf16 {pf['bf16']:.2f} dB; "
          f"enhance ({img.dtype}) fp16 {p['fp16']:.2f} dB, bf16 {p['bf16']:.2f} dB")
    assert pf["fp16"] >= pf["bf16"] + 12.0, pf
    assert p["fp16"] >= p["bf16"] + (12.0 if img.dtype == np.uint16 else 6.0), p


def test_two_lanes_on_one_device_are_bitwise_the_single_lane():
    """devices=[0, 0]: a tiled frame's tiles over two lanes, and enhance_many's frames dealt to them (replicas get the fp16
    weights and their own range word from the pool)."""
    sd = synthetic_compact_state_dict(seed=1, **ANIME)

    def make(devices, tile):
        return RealESRGANer(scale=4, model_path={"params": {k: v.clone() for k, v in sd.items()}},
                            model=SRVGGNetCompact(**ANIME, compute_dtype="fp16"), tile=tile, tile_pad=10, pre_pad=0, half=True,
                            device="cuda:0", devices=devices)
    img = synthetic_frame(150, 210, seed=3)
    want, _ = make(None, 64).enhance(img)
    two = make([0, 0], 64)
    got, _ = two.enhance(img)
    assert two.model.compute_dtype == "fp16" and len(two.model._handles()) >= 2
    assert np.array_equal(got, want)
    frames = [synthetic_frame(96, 128, seed=10 + i) for i in range(4)]
    one = make(None, 0)
    many = make([0, 0], 0).enhance_many(frames, inflight=2)
    for (g, mode), f in zip(many, frames):
        assert mode == "RGB" and np.array_equal(g, one.enhance(f)[0])


def test_denoise_blend_with_an_fp16_model_is_loading_the_blended_dict():
    a = synthetic_compact_state_dict(seed=21, **ANIME)
    b = synthetic_compact_state_dict(seed=22, **ANIME)
    img = synthetic_frame(40, 52, seed=4)
    mk = lambda: SRVGGNetCompact(**ANIME, compute_dtype="fp16")      # noqa: E731
    up = RealESRGANer(scale=4, model_path=[{"params": {k: v.clone() for k, v in a.items()}}, {"params": b}], dni_weight=[0.5, 0.5],
                      model=mk(), tile=0, tile_pad=10, pre_pad=10, half=True, device="cuda:0")
    direct = RealESRGANer(scale=4, model_path={"params": {k: 0.5 * a[k] + 0.5 * b[k] for k in a}}, model=mk(), tile=0, tile_pad=10,
                          pre_pad=10, half=True, device="cuda:0")
    assert up.model.compute_dtype == "fp16"
    assert np.array_equal(up.enhance(img)[0], direct.enhance(img)[0])
