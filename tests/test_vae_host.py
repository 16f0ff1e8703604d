"""The VAE decoder without a GPU: the restatement of tests/vae_ref.py pinned in float64 to a transcription built from torch's own
modules (nn.GroupNorm, nn.Conv2d, nn.Linear, F.scaled_dot_product_attention; diffusers is not a dependency), the key set for both
generations of attention names, the keys that are dropped, the strictness of the loader in Python and in the library, the
configuration checks of nesr_vae_create on a context without a device, and nesr_vae_output_size."""
import ctypes
import json

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from neural_enhanced_super_resolution_amd import VaeDecoder, _lib, vae_state_dict_spec
from neural_enhanced_super_resolution_amd.vae import DEFAULTS, decoder_state_dict
from tests import vae_cases as C
from tests import vae_ref as R

NO_DEVICE = -1      # NESR_VAE_NO_DEVICE


# ------------------------------------------------------------------------------------------------ the transcription
class Resnet(nn.Module):
    def __init__(self, cin, cout, groups):
        super().__init__()
        self.norm1, self.conv1 = nn.GroupNorm(groups, cin, eps=1e-6), nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2, self.conv2 = nn.GroupNorm(groups, cout, eps=1e-6), nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h)))
        return (self.conv_shortcut(x) if hasattr(self, "conv_shortcut") else x) + h


class Attention(nn.Module):
    def __init__(self, c, groups):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, c, eps=1e-6)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c)])

    def forward(self, x):
        n, c, h, w = x.shape
        t = self.group_norm(x).view(n, c, h * w).transpose(1, 2)
        q, k, v = (m(t).unsqueeze(1) for m in (self.to_q, self.to_k, self.to_v))      # one head of width c
        o = F.scaled_dot_product_attention(q, k, v).squeeze(1)
        return x + self.to_out[0](o).transpose(1, 2).reshape(n, c, h, w)


class Mid(nn.Module):
    def __init__(self, c, groups):
        super().__init__()
        self.resnets = nn.ModuleList([Resnet(c, c, groups), Resnet(c, c, groups)])
        self.attentions = nn.ModuleList([Attention(c, groups)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))


class Upsampler(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, padding=1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


class Up(nn.Module):
    def __init__(self, cin, cout, layers, groups, upsample):
        super().__init__()
        self.resnets = nn.ModuleList([Resnet(cin if j == 0 else cout, cout, groups) for j in range(layers + 1)])
        if upsample:
            self.upsamplers = nn.ModuleList([Upsampler(cout)])

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return self.upsamplers[0](x) if hasattr(self, "upsamplers") else x


class Decoder(nn.Module):
    def __init__(self, c):
        super().__init__()
        widths, groups = c["block_out_channels"], c["norm_num_groups"]
        self.conv_in = nn.Conv2d(c["latent_channels"], widths[-1], 3, padding=1)
        self.mid_block = Mid(widths[-1], groups)
        rev = list(reversed(widths))
        self.up_blocks = nn.ModuleList([Up(rev[max(i - 1, 0)], wd, c["layers_per_block"], groups, i < len(rev) - 1) for i, wd in enumerate(rev)])
        self.conv_norm_out, self.conv_out = nn.GroupNorm(groups, widths[0], eps=1e-6), nn.Conv2d(widths[0], c["out_channels"], 3, padding=1)

    def forward(self, x):
        x = self.mid_block(self.conv_in(x))
        for u in self.up_blocks:
            x = u(x)
        return self.conv_out(F.silu(self.conv_norm_out(x)))


class Transcription(nn.Module):
    def __init__(self, **cfg):
        super().__init__()
        c = R.config(**cfg)
        self.post_quant_conv = nn.Conv2d(c["latent_channels"], c["latent_channels"], 1)
        self.decoder = Decoder(c)

    def forward(self, z):
        return self.decoder(self.post_quant_conv(z))


HOST_CASES = [n for n in C.NAMES if n != "published_width"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_restatement_matches_the_module_transcription_f64(name):
    case = C.by_name(name)
    model = Transcription(**case.cfg).double().eval()
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == dict(R.spec(**case.cfg))      # the modules' own key set
    model.load_state_dict({k: v.double() for k, v in case.sd.items()})
    z = C.z_of(case)
    with torch.no_grad():
        want, got = model(z), R.decode(case.sd, z, **case.cfg)
    err, bound = float((got - want).abs().max()), 1e-9 * max(1.0, float(want.abs().max()))
    print(f"restatement vs modules f64, {name}: {tuple(want.shape)}, max |diff| = {err:.3e}, bound {bound:.3e}")
    assert got.shape == want.shape and err <= bound


def test_published_widths_at_2x3_latents():
    """The published configuration end to end: (128, 256, 512), 32 groups, two layers a block, x4."""
    sd = R.seeded_state_dict(31)
    model = Transcription().double().eval()
    model.load_state_dict({k: v.double() for k, v in sd.items()})
    z = torch.randn((1, 4, 2, 3), generator=torch.Generator().manual_seed(32), dtype=torch.float64)
    with torch.no_grad():
        want, got = model(z), R.decode(sd, z)
    assert tuple(got.shape) == (1, 3, 8, 12)
    assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))
    assert VaeDecoder().output_size(2, 3) == (8, 12)


@pytest.mark.parametrize("cfg", [{}, C.SMALL, dict(block_out_channels=(8, 16, 16, 32), norm_num_groups=4, layers_per_block=3, latent_channels=6, out_channels=1)],
                         ids=["published", "small", "four"])
def test_spec_for_both_generations_of_attention_names(cfg):
    current, legacy = R.spec(**cfg), R.spec("legacy", **cfg)
    assert list(vae_state_dict_spec(**cfg).items()) == list(current.items())
    assert list(vae_state_dict_spec("legacy", **cfg).items()) == list(legacy.items())
    assert len(current) == len(legacy) and list(current.values()) == list(legacy.values())
    a = R.ATTENTION
    assert {k for k in legacy if k not in current} == {f"{a}.{n}.{leaf}" for n in ("query", "key", "value", "proj_attn") for leaf in ("weight", "bias")}
    m = VaeDecoder(**cfg)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(current)      # the module tree groups a block's keys
    # the module takes either generation, and they are the same tensors
    sd_legacy = R.seeded_state_dict(5, "legacy", **cfg)
    m.load_state_dict(sd_legacy)
    assert torch.equal(m.state_dict()[a + ".to_out.0.weight"], sd_legacy[a + ".proj_attn.weight"])
    assert list(R.current_names(sd_legacy)) == list(current)


def test_encoder_and_quant_conv_keys_are_dropped():
    case = C.by_name("two_levels")
    extra = {"encoder.conv_in.weight": torch.zeros(16, 3, 3, 3), "encoder.mid_block.resnets.0.norm1.bias": torch.zeros(32),
             "quant_conv.weight": torch.zeros(8, 8, 1, 1), "quant_conv.bias": torch.zeros(8)}
    full = dict(case.sd, **extra)
    assert list(decoder_state_dict(full)) == list(case.sd)
    m = VaeDecoder(**case.cfg)
    m.load_state_dict(full)
    z = C.z_of(case)
    with torch.no_grad():
        assert torch.equal(R.decode(full, z, **case.cfg), R.decode(case.sd, z, **case.cfg))


def test_load_state_dict_is_strict():
    case = C.by_name("two_levels")
    m = VaeDecoder(**case.cfg)
    m.load_state_dict(case.sd)
    first = next(iter(case.sd))
    sd = dict(case.sd)
    del sd[first]
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict(dict(case.sd, **{"decoder.extra.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict(dict(case.sd, **{first: torch.zeros(5)}))
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        m.decode(torch.zeros(1, 4, 2, 2))
    with pytest.raises(FileNotFoundError):
        VaeDecoder.from_checkpoint("stabilityai/stable-diffusion-x4-upscaler")
    with pytest.raises(TypeError, match="unknown configuration"):
        VaeDecoder(sample_size=64)


def test_a_null_field_of_config_json_leaves_the_default(tmp_path):
    """from_checkpoint's config.json reader is _HFNet's: a field the file holds as null is left to the default, an argument overrides the file."""
    case = C.by_name("two_levels")
    torch.save(dict(case.sd), tmp_path / "diffusion_pytorch_model.bin")
    found = dict(R.config(**case.cfg), scaling_factor=None, layers_per_block=3, _class_name="AutoencoderKL")
    (tmp_path / "config.json").write_text(json.dumps({k: list(v) if isinstance(v, tuple) else v for k, v in found.items()}))
    m = VaeDecoder.from_checkpoint(tmp_path, layers_per_block=case.cfg["layers_per_block"])
    assert m.config["scaling_factor"] == DEFAULTS["scaling_factor"] and m.config["layers_per_block"] == case.cfg["layers_per_block"]
    assert m.config["block_out_channels"] == tuple(case.cfg["block_out_channels"])


def _load(lib, h, key, t):
    t = t.contiguous()
    shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
    return lib.nesr_vae_load_weight(h, key.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim())


def test_library_loading_is_strict_on_a_context_without_a_device():
    case = C.by_name("two_levels")
    lib = _lib.load()
    h = VaeDecoder(**case.cfg)._create(NO_DEVICE)
    try:
        assert lib.nesr_vae_num_tensors(h) == len(case.sd)
        keys = list(case.sd)
        for k in keys[:-1]:
            assert _load(lib, h, k, case.sd[k]) == 0
        assert lib.nesr_vae_finalize(h) == -3 and keys[-1] in lib.nesr_last_error().decode()      # NESR_ERR_STATE
        assert _load(lib, h, "decoder.nothing.weight", torch.zeros(3)) == _lib.ERR_ARG and "unexpected key" in lib.nesr_last_error().decode()
        assert _load(lib, h, "encoder.conv_in.weight", torch.zeros(3)) == _lib.ERR_ARG      # the caller drops these; the library is strict
        assert _load(lib, h, keys[-1], torch.zeros(2, 2)) == _lib.ERR_ARG and "size mismatch" in lib.nesr_last_error().decode()
        a = R.ATTENTION
        assert _load(lib, h, a + ".proj_attn.weight", case.sd[a + ".to_out.0.weight"]) == 0      # the legacy name of the same tensor
        assert _load(lib, h, a + ".query.bias", torch.zeros(3)) == _lib.ERR_ARG and "size mismatch" in lib.nesr_last_error().decode()
        assert _load(lib, h, keys[-1], case.sd[keys[-1]]) == 0
        assert lib.nesr_vae_finalize(h) == 0
        n = ctypes.c_size_t(0)
        assert lib.nesr_vae_workspace_bytes(h, 5, 7, ctypes.byref(n)) == 0 and n.value > 3 * 4 * 35 * 3 * 32
        assert lib.nesr_vae_workspace_bytes(h, 257, 256, ctypes.byref(n)) == _lib.ERR_ARG and "token limit" in lib.nesr_last_error().decode()
        z = torch.zeros(1, 4, 2, 2)
        out = torch.zeros(1, 3, 4, 4)
        assert lib.nesr_vae_decode_f32(h, ctypes.c_void_p(z.data_ptr()), 1, 4, 2, 2, ctypes.c_void_p(out.data_ptr()), out.numel(), None) == -3      # no device: no decode
    finally:
        lib.nesr_vae_destroy(h)


BASE = dict(C.SMALL)
UNSUPPORTED = [
    ("block_out_channels", dict(block_out_channels=(32,))),
    ("block_out_channels", dict(block_out_channels=(16, 16, 16, 16, 16))),
    ("block_out_channels", dict(block_out_channels=(16, 30))),
    ("block_out_channels", dict(block_out_channels=(16, 1024))),
    ("norm_num_groups", dict(norm_num_groups=0)),
    ("layers_per_block", dict(layers_per_block=0)),
    ("layers_per_block", dict(layers_per_block=5)),
    ("latent_channels", dict(latent_channels=0)),
    ("latent_channels", dict(latent_channels=9)),
    ("out_channels", dict(out_channels=0)),
    ("out_channels", dict(out_channels=5)),
    ("act_fn", dict(act_fn="gelu")),
    ("scaling_factor", dict(scaling_factor=0.0)),
]


@pytest.mark.parametrize("field,change", UNSUPPORTED, ids=[f"{f}-{i}" for i, (f, _) in enumerate(UNSUPPORTED)])
def test_unsupported_configurations_name_the_field_before_any_device(field, change):
    m = VaeDecoder(**dict(BASE, **change))
    with pytest.raises(_lib.NesrUnsupportedError, match=field):
        m._create(NO_DEVICE)


@pytest.mark.parametrize("widths,scale", [((16, 32), 2), ((128, 256, 512), 4), ((8, 16, 16, 32), 8)])
def test_output_size_for_two_three_and_four_levels(widths, scale):
    m = VaeDecoder(block_out_channels=widths, norm_num_groups=4)
    assert m.output_size(5, 7) == (5 * scale, 7 * scale) and m.output_size(1, 1) == (scale, scale)
    lib = _lib.load()
    oh, ow = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.nesr_vae_output_size(len(widths), 0, 7, ctypes.byref(oh), ctypes.byref(ow)) == _lib.ERR_ARG
    assert lib.nesr_vae_output_size(len(widths), 256, 257, ctypes.byref(oh), ctypes.byref(ow)) == _lib.ERR_ARG      # past the token limit
    assert lib.nesr_vae_output_size(1, 5, 7, ctypes.byref(oh), ctypes.byref(ow)) == _lib.ERR_ARG
    assert lib.nesr_vae_output_size(5, 5, 7, ctypes.byref(oh), ctypes.byref(ow)) == _lib.ERR_ARG
