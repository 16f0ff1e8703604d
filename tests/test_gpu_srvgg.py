"""GPU: SRVGGNetCompact (srvgg_compact.hip) against a float64 torch-CPU restatement of upstream's network (tests/srvgg_ref.py),
alone and inside RealESRGANer against the unchanged oracle.realesrganer_ref.RealESRGANerRef.

The bf16 floors and ceilings below (BF16_NET, BF16_WRAPPER, BF16_LOOP) were measured on this kernel and stay as a guard against
drift.  What holds the bf16 form to a specification is elsewhere: test_gpu_srvgg_pin.py pins the first layer, a feature layer
and the tail per value to the rounded float64 value (tests/srvgg_pin.py), and test_gpu_srvgg_emu16.py judges whole networks
against the exact bf16 specification (tests/srvgg_fp16_emu.py with store=torch.bfloat16) with local conditions."""
import ctypes

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import RealESRGANer, SRVGGNetCompact, _lib
from neural_enhanced_super_resolution_amd.realesrganer import normalize_u8_on_device
from neural_enhanced_super_resolution_amd.synth import synthetic_compact_state_dict, synthetic_frame
from oracle.realesrganer_ref import RealESRGANerRef
from tests.srvgg_ref import SRVGGRef

pytestmark = pytest.mark.gpu

X4V3 = dict(num_conv=32, upscale=4, act_type="prelu")           # realesr-general-x4v3
ANIME = dict(num_conv=16, upscale=4, act_type="prelu")          # realesr-animevideov3
# bf16 against the f64 reference, measured on MI355X ("SRVGGNetCompact"); floors 1.5 dB below the measurement,
# mean-abs ceilings 1.25x above it (2 dB)
BF16_NET = {  # config -> (measured PSNR dB, measured mean abs), 2 x 67 x 93 frames
    (32, 4, "prelu"): (50.69, 2.28e-3),
    (16, 4, "prelu"): (54.89, 1.42e-3),
    (16, 2, "relu"): (58.86, 8.92e-4),
}
BF16_WRAPPER = (55.36, 7.43e-4)   # RealESRGANer(half=True) u8 output against RealESRGANerRef: the lowest PSNR / highest mean abs seen

_cache = {}


def nets(cfg, seed=0, dtype="f32"):
    key = (tuple(sorted(cfg.items())), seed, dtype)
    if key not in _cache:
        sd = synthetic_compact_state_dict(seed=seed, **cfg)
        ours = SRVGGNetCompact(**cfg, compute_dtype=dtype).to("cuda:0")
        ours.load_state_dict(sd)
        ref = SRVGGRef(**cfg)
        ref.load_state_dict(sd)
        _cache[key] = (ours, ref, sd)
    return _cache[key]


def image_batch(n, h, w, seed=0):
    return torch.stack([torch.from_numpy(synthetic_frame(h, w, seed=seed + i)).permute(2, 0, 1).float() / 255 for i in range(n)])


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10 * np.log10(1.0 / max(mse, 1e-30))


F32_CASES = [(X4V3, s) for s in [(1, 1, 1), (1, 3, 5), (1, 37, 53), (2, 64, 64), (1, 130, 257)]] + \
            [(ANIME, s) for s in [(1, 1, 1), (1, 37, 53), (2, 64, 64), (1, 130, 257)]] + \
            [(dict(num_conv=16, upscale=4, act_type="relu"), (1, 37, 53)),
             (dict(num_conv=16, upscale=4, act_type="leakyrelu"), (1, 37, 53)),
             (dict(num_conv=16, upscale=2, act_type="prelu"), (1, 37, 53)),
             (dict(num_conv=16, upscale=2, act_type="leakyrelu"), (2, 64, 64))]


@pytest.mark.parametrize("cfg,shape", F32_CASES)
def test_f32_matches_f64_reference(cfg, shape):
    ours, ref, _ = nets(cfg)
    x = image_batch(*shape)
    y = ours(x.to("cuda:0")).cpu()
    ours.check_range()
    with torch.no_grad():
        r = ref(x.double())
    err = float((y.double() - r).abs().max())
    print(f"f32 {cfg} {shape}: max abs {err:.2e}")
    assert y.shape == r.shape
    assert err <= 1e-5, err


@pytest.mark.parametrize("cfg", [X4V3, ANIME, dict(num_conv=16, upscale=2, act_type="relu")])
def test_bf16_against_f64_reference(cfg):
    ours, ref, _ = nets(cfg, dtype="bf16")
    x = image_batch(2, 67, 93, seed=3)
    y = ours(x.to("cuda:0")).cpu()
    with torch.no_grad():
        r = ref(x.double())
    p, mae = psnr(y, r), float((y.double() - r).abs().mean())
    print(f"bf16 {cfg}: PSNR {p:.2f} dB, mean abs {mae:.2e}")
    m_psnr, m_mae = BF16_NET[(cfg["num_conv"], cfg["upscale"], cfg["act_type"])]
    assert p >= m_psnr - 1.5 and mae <= 1.25 * m_mae, (p, mae)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("flip,rnd", [(True, True), (False, False)])
def test_forward_u8_is_forward_then_the_torch_quantiser(dtype, flip, rnd):
    ours, _, _ = nets(X4V3, dtype=dtype)
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


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_and_slot_independence(dtype):
    ours, _, _ = nets(ANIME, dtype=dtype)
    xs = image_batch(5, 50, 61, seed=11).to("cuda:0")
    alone = ours(xs[2:3].contiguous())
    batch = ours(xs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_slot = ours(xs[2:3].contiguous(), slot=2)
    torch.cuda.current_stream().wait_stream(side)
    ours.check_range()
    assert torch.equal(alone, batch[2:3])
    assert torch.equal(alone, on_slot)


def frame(kind, h, w, seed=0):
    img = synthetic_frame(h, w, seed=seed)
    if kind == "gray":
        return img[:, :, 1].copy()
    if kind == "bgra":
        a = synthetic_frame(h, w, seed=seed + 50)[:, :, :1]
        return np.concatenate([img, a], axis=2)
    if kind == "u16":
        return img.astype(np.uint16) * 257 + np.uint16(seed)
    return img


WRAPPER = [("bgr", 0, 0, 37, 53), ("bgr", 0, 10, 37, 53), ("bgr", 128, 10, 150, 301), ("bgr", 128, 0, 131, 140),
           ("gray", 0, 10, 33, 41), ("bgra", 128, 0, 140, 45), ("u16", 0, 10, 29, 39)]


def run_pair(kind, tile, pre_pad, h, w, half):
    sd = synthetic_compact_state_dict(seed=1, **X4V3)
    ours = RealESRGANer(scale=4, model_path={"params": sd}, model=SRVGGNetCompact(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=32,
                                                                                    upscale=4, act_type="prelu"),
                        tile=tile, tile_pad=10, pre_pad=pre_pad, half=half, device="cuda:0")
    ref = RealESRGANerRef(scale=4, model_path={"params": sd}, model=SRVGGRef(**X4V3), tile=tile, tile_pad=10, pre_pad=pre_pad)
    img = frame(kind, h, w, seed=h)
    out, mode = ours.enhance(img)
    exp, exp_mode = ref.enhance(img)
    assert mode == exp_mode and out.shape == exp.shape and out.dtype == exp.dtype
    return out.astype(np.int64), exp.astype(np.int64), ours


@pytest.mark.parametrize("kind,tile,pre_pad,h,w", WRAPPER)
def test_wrapper_f32_matches_reference(kind, tile, pre_pad, h, w):
    out, exp, ours = run_pair(kind, tile, pre_pad, h, w, half=False)
    d = np.abs(out - exp)
    # 16-bit output: one LSB is 1/65535, so the f32 path's ~1e-6 is 0.1 LSB and rounding ties are ~10x as frequent
    share = 1e-2 if kind == "u16" else 1e-3
    print(f"wrapper f32 {kind} tile={tile} pre_pad={pre_pad} {h}x{w}: max diff {d.max()}, share off {np.mean(d > 0):.2e}")
    assert d.max() <= 1 and np.mean(d > 0) <= share
    assert ours.model.calls > 0


@pytest.mark.parametrize("kind,tile,pre_pad,h,w", [WRAPPER[1], WRAPPER[2], WRAPPER[5]])
def test_wrapper_bf16_against_reference(kind, tile, pre_pad, h, w):
    out, exp, _ = run_pair(kind, tile, pre_pad, h, w, half=True)
    p = psnr(torch.from_numpy(out / 255.0), torch.from_numpy(exp / 255.0))
    mae = float(np.abs(out - exp).mean()) / 255.0
    print(f"wrapper bf16 {kind} tile={tile}: PSNR {p:.2f} dB, mean abs {mae:.2e}")
    assert p >= BF16_WRAPPER[0] - 1.5 and mae <= 1.25 * BF16_WRAPPER[1], (p, mae)


def test_denoise_strength_blend_is_loading_the_blended_dict():
    a = synthetic_compact_state_dict(seed=21, **X4V3)
    b = synthetic_compact_state_dict(seed=22, **X4V3)
    img = synthetic_frame(40, 52, seed=4)
    up = RealESRGANer(scale=4, model_path=[{"params": {k: v.clone() for k, v in a.items()}}, {"params": b}], dni_weight=[0.5, 0.5],
                      model=SRVGGNetCompact(num_conv=32), tile=0, tile_pad=10, pre_pad=10, half=False, device="cuda:0")
    blended = {k: 0.5 * a[k] + 0.5 * b[k] for k in a}
    direct = RealESRGANer(scale=4, model_path={"params": blended}, model=SRVGGNetCompact(num_conv=32), tile=0, tile_pad=10, pre_pad=10,
                          half=False, device="cuda:0")
    o1, _ = up.enhance(img)
    o2, _ = direct.enhance(img)
    assert np.array_equal(o1, o2)
    f1, _, _ = up.enhance_float(img)
    f2, _, _ = direct.enhance_float(img)
    assert np.array_equal(f1, f2)


def test_range_error_in_the_f16_pair_form():
    sd = synthetic_compact_state_dict(seed=2, **ANIME)
    sd["body.0.weight"] = sd["body.0.weight"] * 3000.0
    sd["body.2.weight"] = sd["body.2.weight"] * 3000.0
    up = RealESRGANer(scale=4, model_path={"params": sd}, model=SRVGGNetCompact(**ANIME), tile=0, tile_pad=10, pre_pad=0, device="cuda:0")
    with pytest.raises(_lib.NesrRangeError):
        up.enhance(synthetic_frame(24, 24))
    ok = synthetic_compact_state_dict(seed=2, **ANIME)
    up.model.load_state_dict(ok)
    out, _ = up.enhance(synthetic_frame(24, 24))          # a valid frame after the error: no stale flag
    assert out.shape == (96, 96, 3)


def test_cabi_errors_on_a_compact_context(cuda_device):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.nesr_create_compact(ctypes.byref(h), 0, 3, 3, 64, 2, 4, _lib.ACT_PRELU, _lib.DTYPE_BF16) == 0
    try:
        assert lib.nesr_num_tensors(h) == 2 * 4 + 3
        x = torch.zeros(1, 3, 8, 8, device=cuda_device)
        y = torch.zeros(1, 3, 32, 32, device=cuda_device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        assert lib.nesr_forward(h, p(x), 1, 3, 8, 8, p(y), None) == -3               # weights not finalized
        w = np.zeros((64, 3, 3, 3), np.float32)
        shp = (ctypes.c_int64 * 4)(64, 3, 3, 3)
        assert lib.nesr_load_weight(h, b"body.0.weight", w.ctypes.data_as(ctypes.c_void_p), shp, 4) == 0
        assert lib.nesr_load_weight(h, b"body.1.weight", w.ctypes.data_as(ctypes.c_void_p), shp, 4) == -1   # PReLU is [64]
        assert lib.nesr_load_weight(h, b"body.9.weight", w.ctypes.data_as(ctypes.c_void_p), shp, 4) == -1   # no such layer
        assert lib.nesr_load_weight(h, b"conv_first.weight", w.ctypes.data_as(ctypes.c_void_p), shp, 4) == -1
        assert lib.nesr_finalize_weights(h) == -3 and b"missing" in lib.nesr_last_error()
        hw = (ctypes.c_int * 2)(8, 8)
        assert lib.nesr_forward_ragged(h, p(x), 1, 3, 8, 8, hw, p(y), None) == -1
        assert lib.nesr_band_begin(h, p(x), 3, 8, 8, None) == -1
        assert lib.nesr_band_rdb(h, 0, None) == -1
        assert lib.nesr_band_tail(h, p(y), None) == -1
        assert lib.nesr_band_row_bytes(h) == 0
        assert lib.nesr_set_fused(h, 1) == -1
        assert lib.nesr_fused_state(h) == -1
        assert lib.nesr_debug_fault(h, 1) == -1
        assert lib.nesr_preferred_batch(h, 64, 64, 8) == -1
        assert lib.nesr_forward_sharded_u8(h, p(x), 8, 8, 512, 10, 0, p(y), None) == -1
        assert lib.nesr_comm_destroy(h) == -1
        assert b"RRDBNet contexts only" in lib.nesr_last_error()
        assert lib.nesr_set_size_independent(h, 1) == 0 and lib.nesr_set_concurrent(h, 1) == 0
    finally:
        lib.nesr_destroy(h)


# ---- the persistent tile loop: a grid of one workgroup per CU walks the tiles (srvgg_compact.hip, launch_one); the frames
# below have more tiles than the device has CUs, so workgroups carry LDS, weights and accumulators from one tile to the next
TILE_H = {"f32": 8, "bf16": 16}     # output rows of a workgroup's tile (32 columns)
SMALL = dict(num_conv=2, upscale=4, act_type="prelu")
BF16_LOOP = (65.19, 4.37e-4)        # measured PSNR / mean abs of the 264 x 528 case below


def tiles(dtype, n, h, w):
    return n * -(-h // TILE_H[dtype]) * -(-w // 32)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_many_tiles_per_workgroup_against_f64_reference(dtype):
    n, h, w = 1, 264, 528
    assert tiles(dtype, n, h, w) > torch.cuda.get_device_properties(0).multi_processor_count
    ours, ref, _ = nets(SMALL, seed=4, dtype=dtype)
    x = image_batch(n, h, w, seed=9)
    y = ours(x.to("cuda:0")).cpu()
    ours.check_range()
    with torch.no_grad():
        r = ref(x.double())
    err, p, mae = float((y.double() - r).abs().max()), psnr(y, r), float((y.double() - r).abs().mean())
    print(f"{dtype} {tiles(dtype, n, h, w)} tiles: max abs {err:.2e}, PSNR {p:.2f} dB, mean abs {mae:.2e}")
    if dtype == "f32":
        assert err <= 1e-5, err
    else:
        assert p >= BF16_LOOP[0] - 1.5 and mae <= 1.25 * BF16_LOOP[1], (p, mae)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tile_loop_is_bitwise_one_tile_per_workgroup(dtype):
    """24 images of 64 x 96 in one batch (288 | 576 tiles: every workgroup walks several) against each image alone (12 | 24 tiles:
    one per workgroup).  Pixels never depend on which workgroup computed them, so any state leaking from one tile into the
    next shows up as a differing bit."""
    n, h, w = 24, 64, 96
    assert tiles(dtype, n, h, w) > torch.cuda.get_device_properties(0).multi_processor_count
    assert tiles(dtype, 1, h, w) < torch.cuda.get_device_properties(0).multi_processor_count
    ours, _, _ = nets(SMALL, seed=5, dtype=dtype)
    xs = image_batch(n, h, w, seed=30).to("cuda:0")
    batch = ours(xs)
    alone = torch.cat([ours(xs[i:i + 1].contiguous()) for i in range(n)])
    ours.check_range()
    assert torch.equal(batch, alone)


def test_range_error_in_the_last_body_layer_poisons_the_whole_output():
    """Only the last body conv's output leaves the f16-pair range: the tail itself is what reads it, and still writes NaN."""
    sd = synthetic_compact_state_dict(seed=6, **SMALL)
    sd[f"body.{2 * SMALL['num_conv']}.bias"] = torch.full((64,), 1.0e5)
    m = SRVGGNetCompact(**SMALL).to("cuda:0")
    m.load_state_dict(sd)
    y = m(image_batch(1, 40, 72).to("cuda:0"))
    assert bool(torch.isnan(y).all())
    with pytest.raises(_lib.NesrRangeError):
        m.check_range()
    ok = synthetic_compact_state_dict(seed=6, **SMALL)
    m.load_state_dict(ok)
    y = m(image_batch(1, 40, 72).to("cuda:0"))
    m.check_range()
    assert bool(torch.isfinite(y).all())
