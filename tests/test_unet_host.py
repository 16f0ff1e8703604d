"""The UNet without a GPU: the restatement of tests/unet_ref.py against a second, independent transcription built from torch's own
modules (nn.GroupNorm, nn.LayerNorm, nn.Conv2d(stride=2, padding=1), nn.Linear, nn.Embedding, F.scaled_dot_product_attention, F.gelu,
torch.cat, F.interpolate) under diffusers' module names, so that the restatement's state dict loads into it strictly; the spec's
keys, shapes and parameter count at the published configuration; the launch-count formula's inputs; checkpoint round trips."""
import json
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from neural_enhanced_super_resolution_amd import UNet2DCondition, unet_state_dict_spec
from neural_enhanced_super_resolution_amd import unet as U
from tests import unet_cases as C
from tests import unet_ref as R


class Resnet(nn.Module):
    def __init__(self, cin, cout, td, groups, eps):
        super().__init__()
        self.norm1, self.conv1 = nn.GroupNorm(groups, cin, eps=eps), nn.Conv2d(cin, cout, 3, padding=1)
        self.time_emb_proj = nn.Linear(td, cout)
        self.norm2, self.conv2 = nn.GroupNorm(groups, cout, eps=eps), nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x, emb):
        h = self.conv1(F.silu(self.norm1(x))) + self.time_emb_proj(F.silu(emb))[:, :, None, None]
        h = self.conv2(F.silu(self.norm2(h)))
        return (self.conv_shortcut(x) if hasattr(self, "conv_shortcut") else x) + h


class Attention(nn.Module):
    def __init__(self, dim, kv, heads):
        super().__init__()
        self.heads = heads
        self.to_q, self.to_k, self.to_v = nn.Linear(dim, dim, bias=False), nn.Linear(kv, dim, bias=False), nn.Linear(kv, dim, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(dim, dim)])

    def forward(self, x, ctx):
        n, t, dim = x.shape
        split = lambda v: v.view(n, v.shape[1], self.heads, dim // self.heads).transpose(1, 2)
        o = F.scaled_dot_product_attention(split(self.to_q(x)), split(self.to_k(ctx)), split(self.to_v(ctx)))
        return self.to_out[0](o.transpose(1, 2).reshape(n, t, dim))


class GEGLU(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Linear(dim, 8 * dim)

    def forward(self, x):
        value, gate = self.proj(x).chunk(2, dim=-1)
        return value * F.gelu(gate)


class Block(nn.Module):
    def __init__(self, dim, cross, heads, only_cross):
        super().__init__()
        self.only_cross = only_cross
        self.norm1, self.attn1 = nn.LayerNorm(dim), Attention(dim, cross if only_cross else dim, heads)
        self.norm2, self.attn2 = nn.LayerNorm(dim), Attention(dim, cross, heads)
        self.norm3 = nn.LayerNorm(dim)
        self.ff = nn.Module()
        self.ff.net = nn.ModuleList([GEGLU(dim), nn.Identity(), nn.Linear(4 * dim, dim)])

    def forward(self, x, text):
        y = self.norm1(x)
        x = x + self.attn1(y, text if self.only_cross else y)
        x = x + self.attn2(self.norm2(x), text)
        return x + self.ff.net[2](self.ff.net[0](self.norm3(x)))


class Transformer(nn.Module):
    def __init__(self, dim, cross, heads, groups, only_cross):
        super().__init__()
        self.norm, self.proj_in = nn.GroupNorm(groups, dim, eps=1e-6), nn.Linear(dim, dim)
        self.transformer_blocks = nn.ModuleList([Block(dim, cross, heads, only_cross)])
        self.proj_out = nn.Linear(dim, dim)

    def forward(self, x, text):
        n, c, h, w = x.shape
        t = self.proj_in(self.norm(x).flatten(2).transpose(1, 2))
        t = self.proj_out(self.transformer_blocks[0](t, text))
        return t.transpose(1, 2).reshape(n, c, h, w) + x


class Stage(nn.Module):
    """A down, mid or up block: resnets, attentions (or none), one resampling conv (or none)."""

    def __init__(self, resnets, attentions, sampler=None, name=None):
        super().__init__()
        self.resnets = nn.ModuleList(resnets)
        if attentions:
            self.attentions = nn.ModuleList(attentions)
        if sampler is not None:
            holder = nn.Module()
            holder.conv = sampler
            setattr(self, name, nn.ModuleList([holder]))


class Transcription(nn.Module):
    def __init__(self, **cfg):
        super().__init__()
        c = R.config(**cfg)
        self.c = c
        widths, layers, groups, eps = c["block_out_channels"], c["layers_per_block"], c["norm_num_groups"], c["norm_eps"]
        heads, cross, levels, td = c["attention_head_dim"], c["cross_attention_dim"], len(widths), 4 * widths[0]
        tf = lambda dim, oc: Transformer(dim, cross, heads, groups, oc)
        self.conv_in = nn.Conv2d(c["in_channels"], widths[0], 3, padding=1)
        self.time_embedding = nn.Module()
        self.time_embedding.linear_1, self.time_embedding.linear_2 = nn.Linear(widths[0], td), nn.Linear(td, td)
        self.class_embedding = nn.Embedding(c["num_class_embeds"], td)
        self.down_blocks, self.up_blocks = nn.ModuleList(), nn.ModuleList()
        prev = widths[0]
        for i, wd in enumerate(widths):
            has = c["down_block_types"][i] == "CrossAttnDownBlock2D"
            self.down_blocks.append(Stage([Resnet(prev if j == 0 else wd, wd, td, groups, eps) for j in range(layers)],
                                          [tf(wd, c["only_cross_attention"][i]) for _ in range(layers)] if has else [],
                                          nn.Conv2d(wd, wd, 3, stride=2, padding=1) if i < levels - 1 else None, "downsamplers"))
            prev = wd
        for i in range(levels):
            wd, level = widths[levels - 1 - i], levels - 1 - i
            has = c["up_block_types"][i] == "CrossAttnUpBlock2D"
            chans = [R.up_channels(widths, layers, i, j) for j in range(layers + 1)]
            self.up_blocks.append(Stage([Resnet(hd + sk, o, td, groups, eps) for hd, sk, o in chans],
                                        [tf(wd, c["only_cross_attention"][level]) for _ in range(layers + 1)] if has else [],
                                        nn.Conv2d(wd, wd, 3, padding=1) if i < levels - 1 else None, "upsamplers"))
        top = widths[-1]
        self.mid_block = Stage([Resnet(top, top, td, groups, eps), Resnet(top, top, td, groups, eps)], [tf(top, False)])
        self.conv_norm_out, self.conv_out = nn.GroupNorm(groups, widths[0], eps=eps), nn.Conv2d(widths[0], c["out_channels"], 3, padding=1)

    def forward(self, sample, timestep, text, label):
        half = self.c["block_out_channels"][0] // 2
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half) * float(timestep)
        emb = torch.cat([freqs.cos(), freqs.sin()])[None].to(sample.dtype)
        emb = self.time_embedding.linear_2(F.silu(self.time_embedding.linear_1(emb))) + self.class_embedding(torch.tensor([int(label)]))
        x = self.conv_in(sample)
        stack = [x]
        for b in self.down_blocks:
            for j, r in enumerate(b.resnets):
                x = r(x, emb)
                if hasattr(b, "attentions"):
                    x = b.attentions[j](x, text)
                stack.append(x)
            if hasattr(b, "downsamplers"):
                x = b.downsamplers[0].conv(x)
                stack.append(x)
        x = self.mid_block.resnets[1](self.mid_block.attentions[0](self.mid_block.resnets[0](x, emb), text), emb)
        for b in self.up_blocks:
            for j, r in enumerate(b.resnets):
                x = r(torch.cat([x, stack.pop()], dim=1), emb)
                if hasattr(b, "attentions"):
                    x = b.attentions[j](x, text)
            if hasattr(b, "upsamplers"):
                x = b.upsamplers[0].conv(F.interpolate(x, scale_factor=2, mode="nearest"))
        return self.conv_out(F.silu(self.conv_norm_out(x)))


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_agrees_with_the_transcription_in_float64(name):
    case = C.by_name(name)
    net = Transcription(**case.cfg).double().eval()
    net.load_state_dict({k: v.double() for k, v in case.sd.items()}, strict=True)      # the same keys and shapes
    y64, _ = C.reference(name)
    with torch.no_grad():
        got = net(case.sample.double(), case.timestep, case.text.double(), case.label)
    err = float((got - y64).abs().max())
    print(f"{name}: restatement vs transcription {err:.3e}")
    assert got.shape == y64.shape and err < 1e-9


def test_spec_of_the_published_configuration():
    spec = unet_state_dict_spec()
    assert spec == R.spec() and list(spec) == list(R.spec())
    assert spec["time_embedding.linear_1.weight"] == (1024, 256) and spec["class_embedding.weight"] == (1000, 1024)
    assert spec["conv_in.weight"] == (256, 7, 3, 3) and spec["conv_out.weight"] == (4, 256, 3, 3)
    assert spec["down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight"] == (512, 512)
    assert spec["down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_k.weight"] == (512, 1024)      # only_cross_attention: the text states
    assert spec["down_blocks.3.attentions.1.transformer_blocks.0.attn1.to_k.weight"] == (1024, 1024)     # the tokens themselves
    assert spec["down_blocks.3.attentions.1.transformer_blocks.0.ff.net.0.proj.weight"] == (8192, 1024)
    assert spec["down_blocks.3.attentions.1.transformer_blocks.0.ff.net.2.weight"] == (1024, 4096)
    assert spec["up_blocks.0.resnets.0.conv1.weight"] == (1024, 2048, 3, 3) and spec["up_blocks.0.upsamplers.0.conv.weight"] == (1024, 1024, 3, 3)
    assert spec["up_blocks.3.resnets.2.conv1.weight"] == (256, 512, 3, 3) and "up_blocks.3.attentions.0.norm.weight" not in spec
    assert "down_blocks.0.attentions.0.norm.weight" not in spec and "down_blocks.3.downsamplers.0.conv.weight" not in spec
    assert "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.bias" not in spec
    params = sum(math.prod(s) for s in spec.values())
    print(f"published configuration: {len(spec)} tensors, {params} parameters")
    assert len(spec) == 687 and 4.0e8 < params < 5.5e8
    assert U.launches_per_forward() == 438


def test_configuration_is_checked():
    with pytest.raises(TypeError, match="unknown configuration"):
        unet_state_dict_spec(sample_size=128)
    with pytest.raises(ValueError, match="down_block_types has 4 entries"):
        unet_state_dict_spec(block_out_channels=(16, 32))
    assert unet_state_dict_spec(**dict(C.SMALL, only_cross_attention=True)) == unet_state_dict_spec(**dict(C.SMALL, only_cross_attention=(True, True)))


def test_checkpoint_round_trips(tmp_path):
    save_file = pytest.importorskip("safetensors.torch").save_file
    case = C.by_name("thin")
    folder = tmp_path / "unet"
    folder.mkdir()
    save_file({k: v.contiguous() for k, v in case.sd.items()}, str(folder / "diffusion_pytorch_model.safetensors"))
    (folder / "config.json").write_text(json.dumps(dict(R.config(**case.cfg), _class_name="UNet2DConditionModel", sample_size=128, time_embedding_type=None)))
    m = UNet2DCondition.from_checkpoint(folder)
    assert m.config["block_out_channels"] == (16, 32) and m.config["cross_attention_dim"] == 40 and m.config["only_cross_attention"] == (True, False)
    assert all(torch.equal(v, case.sd[k]) for k, v in m.state_dict().items()) and list(m.state_dict()) == list(case.sd)
    torch.save(dict(case.sd), tmp_path / "diffusion_pytorch_model.bin")
    m2 = UNet2DCondition.from_checkpoint(tmp_path / "diffusion_pytorch_model.bin", **case.cfg)
    assert all(torch.equal(v, case.sd[k]) for k, v in m2.state_dict().items())
    with pytest.raises(FileNotFoundError, match="not fetched"):
        UNet2DCondition.from_checkpoint("stabilityai/stable-diffusion-x4-upscaler")
    with pytest.raises(RuntimeError):
        m2.load_state_dict({k: v for k, v in case.sd.items() if k != "conv_in.bias"})
    with pytest.raises(RuntimeError, match="inference only"):
        m2.train()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        m2(case.sample, case.timestep, case.text, case.label)
