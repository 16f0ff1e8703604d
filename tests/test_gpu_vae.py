"""GPU: the VAE decoder's frame route and its edges.

  decode_latents_u8   on the frames of tests/vae_cases.py (at least 1000 samples each): the u8 result equals the float64 route's u8
                      wherever the float64 value x 255 lies farther than 255 tol from a rounding boundary, and is off by at most 1
                      elsewhere; no sample is wrong and at most 2 % are left out (tests/test_vae_cases_host.py holds that
                      condition on the CPU).  Guard bytes surround the frame.
  ties                a model whose every sample is a rounding tie (k + 0.5 exactly in float32): round half to even, sample for sample
  workspace           a small frame after a large one on one context gives the bits of a fresh context
  checkpoints         from_checkpoint through a temporary safetensors file, a vae/ directory with a config.json, legacy names
  refusals            shapes, capacities and the token limit: all rejected before any launch
"""
import ctypes
import json

import pytest
import torch

from neural_enhanced_super_resolution_amd import VaeDecoder, _lib
from tests import vae_cases as C
from tests import vae_ref as R
from tests.swin2sr_ref import u8_check
from tests.test_gpu_vae_cases import DEV, GUARD, model

pytestmark = pytest.mark.gpu


def guarded_frame(m, latents):
    _, ch, h, w = latents.shape
    oh, ow = m.output_size(h, w)
    n = oh * ow * 3
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    src = latents.to(DEV).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().nesr_vae_decode_latents_u8(m._context(src.device), ctypes.c_void_p(src.data_ptr()), 1, ch, h, w,
                                                      ctypes.c_void_p(buf.data_ptr() + GUARD), n, stream), "nesr_vae_decode_latents_u8")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n:] == 0xA5).all()), "the entry wrote outside the frame it reports"
    return buf[GUARD:GUARD + n].view(oh, ow, 3).cpu()


@pytest.mark.parametrize("name", C.FRAME_CASES)
def test_decode_latents_u8_against_the_float64_route(name):
    m = model(name)
    latents, y64, tol = C.frame_reference(name)
    got = guarded_frame(m, latents)
    excluded, wrong, total = u8_check(got, y64, tol)
    print(f"{name}: tol {tol:.3e}, {excluded} of {total} samples thin ({100.0 * excluded / total:.2f} %), {wrong} wrong")
    assert total >= 1000 and wrong == 0 and excluded <= C.MAX_THIN * total
    via_module = m.decode_latents_u8(latents.to(DEV))
    assert via_module.is_cuda and via_module.dtype == torch.uint8 and torch.equal(via_module.cpu(), got)


def test_u8_rounds_ties_to_even():
    """Exact: every sample of this model is k + 0.5 in float32 before the rounding; no sample is left out."""
    case = C.by_name("rounding_ties")
    got = guarded_frame(model("rounding_ties"), case.latents)
    want = C.ties_expected_frame(case)
    bad = (got != want).nonzero()
    assert got.shape == want.shape and bad.numel() == 0, (bad[:8].tolist(), got[0, 0].tolist(), want[0, 0].tolist())


def test_workspace_reuse_leaves_no_trace():
    """The workspace only grows, and a smaller frame carves its buffers from the same base: a read past a frame's extent would meet
    what the larger frame left there.  Bit-equal to a context that never saw the large frame, and the large frame to itself."""
    case = C.by_name("two_levels")
    used, fresh = VaeDecoder(**case.cfg).to(DEV), VaeDecoder(**case.cfg).to(DEV)
    used.load_state_dict(case.sd)
    fresh.load_state_dict(case.sd)
    big = (R.seeded_latents(19, 23, 71) / 0.08333).to(DEV)
    small = (R.seeded_latents(3, 5, 72) / 0.08333).to(DEV)
    y_big, y_small, y_again = used.decode(big).cpu(), used.decode(small).cpu(), used.decode(big).cpu()
    assert bool(torch.isfinite(y_big).all()) and torch.equal(y_big, y_again)
    assert torch.equal(y_small, fresh.decode(small).cpu())
    u_big, u_small = used.decode_latents_u8(big * 0.08333).cpu(), used.decode_latents_u8(small * 0.08333).cpu()
    assert torch.equal(u_small, fresh.decode_latents_u8(small * 0.08333).cpu())
    assert torch.equal(fresh.decode(big).cpu(), y_big) and torch.equal(fresh.decode_latents_u8(big * 0.08333).cpu(), u_big)
    assert used.workspace_bytes(19, 23) > used.workspace_bytes(3, 5) > 0


def test_checkpoint_round_trips(tmp_path):
    save_file = pytest.importorskip("safetensors.torch").save_file
    case = C.by_name("two_levels")
    z = C.reference("two_levels")[0].to(DEV)
    want = model("two_levels").decode(z).cpu()
    # a vae/ directory: the published file name, a config.json beside it, the encoder's keys in the file
    vae = tmp_path / "vae"
    vae.mkdir()
    full = dict(case.sd, **{"encoder.conv_in.weight": torch.zeros(16, 3, 3, 3), "quant_conv.weight": torch.zeros(8, 8, 1, 1), "quant_conv.bias": torch.zeros(8)})
    save_file({k: v.contiguous() for k, v in full.items()}, str(vae / "diffusion_pytorch_model.safetensors"))
    (vae / "config.json").write_text(json.dumps(dict(R.config(**case.cfg), _class_name="AutoencoderKL", sample_size=64)))
    m = VaeDecoder.from_checkpoint(vae).to(DEV)
    assert m.config["block_out_channels"] == (16, 32) and m.config["norm_num_groups"] == 4
    assert torch.equal(m.decode(z).cpu(), want)
    # the file itself, the configuration by argument, the attention's legacy names
    legacy = {k.replace(".to_q.", ".query.").replace(".to_k.", ".key.").replace(".to_v.", ".value.").replace(".to_out.0.", ".proj_attn."): v
              for k, v in case.sd.items()}
    assert set(legacy) != set(case.sd)
    path = tmp_path / "legacy.safetensors"
    save_file({k: v.contiguous() for k, v in legacy.items()}, str(path))
    m2 = VaeDecoder.from_checkpoint(path, **case.cfg).to(DEV)
    assert torch.equal(m2.decode(z).cpu(), want)
    torch.save(dict(case.sd), tmp_path / "diffusion_pytorch_model.bin")
    assert torch.equal(VaeDecoder.from_checkpoint(tmp_path / "diffusion_pytorch_model.bin", **case.cfg).to(DEV).decode(z).cpu(), want)


def test_shape_capacity_and_token_refusals():
    m = model("two_levels")
    with pytest.raises(_lib.NesrHipError, match=r"expected \[1, 4, h, w\]"):
        m.decode(torch.zeros(2, 4, 3, 3, device=DEV))
    with pytest.raises(_lib.NesrHipError, match=r"expected \[1, 4, h, w\]"):
        m.decode(torch.zeros(1, 3, 3, 3, device=DEV))
    with pytest.raises(_lib.NesrHipError, match="token limit"):
        m.decode(torch.zeros(1, 4, 257, 256, device=DEV))
    with pytest.raises(ValueError):
        m.decode(torch.zeros(1, 4, 3, 3, device=DEV, dtype=torch.float64))
    lib, h = _lib.load(), m._context(torch.device(DEV))
    z = torch.zeros(1, 4, 3, 3, device=DEV)
    out = torch.full((3 * 6 * 6,), -7.0, device=DEV)
    o8 = torch.full((6 * 6 * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    assert lib.nesr_vae_decode_f32(h, ctypes.c_void_p(z.data_ptr()), 1, 4, 3, 3, ctypes.c_void_p(out.data_ptr()), out.numel() - 1, None) == _lib.ERR_ARG
    assert "capacity" in lib.nesr_last_error().decode()
    assert lib.nesr_vae_decode_latents_u8(h, ctypes.c_void_p(z.data_ptr()), 1, 4, 3, 3, ctypes.c_void_p(o8.data_ptr()), o8.numel() - 1, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((o8 == 0xA5).all())      # refused before any launch
    gray = VaeDecoder(**dict(C.SMALL, out_channels=1)).to(DEV)
    gray.load_state_dict(R.seeded_state_dict(9, **dict(C.SMALL, out_channels=1)))
    assert tuple(gray.decode(z).shape) == (1, 1, 6, 6)
    with pytest.raises(_lib.NesrHipError, match="out_channels = 3"):
        gray.decode_latents_u8(z)


def test_kernel_timing_and_launch_count():
    m = model("two_levels")                                             # two levels, one layer a block
    z = C.reference("two_levels")[0].to(DEV)
    m.decode(z)
    m.kernel_time_ms()
    m.set_kernel_timing(True)
    m.decode(z)
    t = m.kernel_time_ms()
    m.set_kernel_timing(False)
    # latents, post_quant_conv, conv_in | a ResnetBlock: 2 x (2 statistics, conv), + 1 with a shortcut | attention: 2 statistics, q | k | v,
    # the stream, to_out | mid: 2 blocks | up 0: 2 blocks and the upsampler | up 1: 2 blocks, the first with a shortcut | 2 statistics, conv_out
    assert t["launches"] == 3 + 2 * 6 + 5 + (2 * 6 + 1) + (7 + 6) + 3
    assert list(t["groups"]) == ["conv", "norm", "attention", "projection", "upsample"] and all(v > 0 for v in t["groups"].values())
