"""``VaeDecoder``: the decoder half of diffusers' ``AutoencoderKL`` as ``StableDiffusionUpscalePipeline`` uses it
("stabilityai/stable-diffusion-x4-upscaler", nesr/nesr.py:243-283, 988-1031), as HIP kernels behind the C ABI (csrc/vae.hip,
csrc/vae_api.cpp).  It is the last network of the reference's diffusion stage: latents in, the finished RGB frame out.

The module owns ordinary torch Parameters under diffusers' names (``post_quant_conv.weight``, ``decoder.mid_block.attentions.0.
to_q.weight`` ...) and has no torch implementation of its forward.  ``decode(z)`` takes [1, latent_channels, h, w] float32 on the
device and gives the sample [1, out_channels, h s, w s], s = 2^(len(block_out_channels) - 1); ``decode_latents_u8(latents)`` does
what the pipeline does around the decoder (latents / scaling_factor, decode, / 2 + 0.5, clamp, x 255, round half to even) and
gives the uint8 RGB frame [h s, w s, 3] on the device, which is what ``nesr_ensemble_u8`` and the JPEG and PNG encoders take.
float32 throughout: diffusers itself upcasts this VAE, whose activations leave float16's range.

A state dict may carry the attention's legacy names (``query``, ``key``, ``value``, ``proj_attn``) and the keys of the encoder
half (``encoder.*``, ``quant_conv.*``): the former are renamed, the latter dropped; everything else is strict.

Supported: 2 to 4 entries of block_out_channels (each a multiple of norm_num_groups, at most 512), layers_per_block 1 to 4,
latent_channels 1 to 8, out_channels 1 to 4 (decode_latents_u8 needs 3), act_fn "silu", one image a call.  Anything else raises
NesrUnsupportedError when the context is created, and the message names the field.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch

from . import _lib
from ._contexts import _invoke
from ._hfnet import _HFNet, _merged_config
from ._tiling import sdx4_tile_plan

# the published x4 upscaler's values, recalled from memory: a config.json beside the weights, or the arguments, override them
DEFAULTS = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256, 512), layers_per_block=2, norm_num_groups=32,
                scaling_factor=0.08333, act_fn="silu")
KERNEL_GROUPS = ("conv", "norm", "attention", "projection", "upsample")      # NESR_VAE_GROUP_*
LEGACY_ATTENTION = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}
_ATTENTION = "decoder.mid_block.attentions.0."
_DROPPED = ("encoder.", "quant_conv.")


def _config(cfg):
    c = _merged_config("VaeDecoder", DEFAULTS, cfg)
    c["block_out_channels"] = tuple(int(v) for v in c["block_out_channels"])
    if not c["block_out_channels"]:
        raise ValueError("VaeDecoder: block_out_channels is empty")
    return c


def vae_state_dict_spec(attention_names="current", **cfg):
    """Ordered {key: shape} of the decoder half of an AutoencoderKL checkpoint (post_quant_conv and decoder.*).  Keyword arguments
    are the configuration's fields; attention_names "legacy" spells the attention's four projections query, key, value, proj_attn."""
    if attention_names not in ("current", "legacy"):
        raise ValueError(f"attention_names {attention_names!r}: 'current' or 'legacy'")
    c = _config(cfg)
    widths, lat, top = c["block_out_channels"], int(c["latent_channels"]), c["block_out_channels"][-1]
    spec = OrderedDict()

    def wb(name, wshape):
        spec[name + ".weight"] = tuple(wshape)
        spec[name + ".bias"] = (wshape[0],)

    def resnet(r, cin, cout):
        wb(r + ".norm1", (cin,))
        wb(r + ".conv1", (cout, cin, 3, 3))
        wb(r + ".norm2", (cout,))
        wb(r + ".conv2", (cout, cout, 3, 3))
        if cin != cout:
            wb(r + ".conv_shortcut", (cout, cin, 1, 1))

    wb("post_quant_conv", (lat, lat, 1, 1))
    wb("decoder.conv_in", (top, lat, 3, 3))
    resnet("decoder.mid_block.resnets.0", top, top)
    wb(_ATTENTION + "group_norm", (top,))
    for old, new in LEGACY_ATTENTION.items():
        wb(_ATTENTION + (old if attention_names == "legacy" else new), (top, top))
    resnet("decoder.mid_block.resnets.1", top, top)
    prev = top
    for i, wd in enumerate(reversed(widths)):
        for j in range(int(c["layers_per_block"]) + 1):
            resnet(f"decoder.up_blocks.{i}.resnets.{j}", prev if j == 0 else wd, wd)
        if i < len(widths) - 1:
            wb(f"decoder.up_blocks.{i}.upsamplers.0.conv", (wd, wd, 3, 3))
        prev = wd
    wb("decoder.conv_norm_out", (prev,))
    wb("decoder.conv_out", (int(c["out_channels"]), prev, 3, 3))
    return spec


def decoder_state_dict(state_dict):
    """The decoder's part of an AutoencoderKL state dict under the current names: encoder.* and quant_conv.* dropped, the
    attention's legacy names renamed.  Every other key passes as it is (and is refused later if it is not expected)."""
    out = OrderedDict()
    for key, value in state_dict.items():
        if key.startswith(_DROPPED):
            continue
        if key.startswith(_ATTENTION):
            head, _, leaf = key[len(_ATTENTION):].rpartition(".")
            key = _ATTENTION + LEGACY_ATTENTION.get(head, head) + "." + leaf
        out[key] = value
    return out


class VaeDecoder(_HFNet):
    """AutoencoderKL.decode in eval mode on the HIP path.  Keyword arguments are the configuration's fields."""

    PREFIX, NAME, KERNEL_GROUPS, DEFAULTS = "nesr_vae", "VaeDecoder", KERNEL_GROUPS, DEFAULTS
    TRAIN_ERROR = "VaeDecoder is inference only"
    _spec = staticmethod(vae_state_dict_spec)
    CHECKPOINT_FILES = ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin")

    def __init__(self, **cfg):
        super().__init__(_config(cfg))

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Strict about the decoder: a missing or an unexpected key raises.  encoder.* and quant_conv.* are dropped and the
        attention's legacy names renamed first (decoder_state_dict)."""
        return super().load_state_dict(decoder_state_dict(state_dict), strict=strict, **kw)

    def _create(self, index):
        """A context of this configuration without weights (NesrUnsupportedError names the field the kernels do not take)."""
        c = self.config
        widths = c["block_out_channels"]
        return self._create_handle("nesr_vae_create", index, int(c["latent_channels"]), int(c["out_channels"]), len(widths),
                                   (ctypes.c_int * len(widths))(*widths), int(c["layers_per_block"]), int(c["norm_num_groups"]),
                                   float(c["scaling_factor"]), str(c["act_fn"]).encode())

    # ------------------------------------------------------------------ decode
    def output_size(self, h, w):
        """(oh, ow) of the sample for h x w latents, as the library computes it.  Needs no device."""
        oh, ow = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().nesr_vae_output_size(len(self.config["block_out_channels"]), int(h), int(w), ctypes.byref(oh), ctypes.byref(ow)),
                   "nesr_vae_output_size")
        return oh.value, ow.value

    def workspace_bytes(self, h, w, device=None):
        """Bytes of workspace a decode of h x w latents allocates on the context of `device`."""
        return self._query_size("nesr_vae_workspace_bytes", device, int(h), int(w))

    def _latents(self, z, what):
        self._require_device(z, what)
        if z.dim() != 4 or z.dtype != torch.float32:
            raise ValueError(f"VaeDecoder.{what}: a [1, {self.config['latent_channels']}, h, w] float32 tensor, got {z.dtype} {tuple(z.shape)}")
        return z.contiguous()

    def decode(self, z):
        """z [1, latent_channels, h, w] float32 on the device -> the sample [1, out_channels, h s, w s]."""
        z = self._latents(z, "decode")
        n, ch, h, w = z.shape
        with torch.cuda.device(z.device):
            handle = self._context(z.device)
            out = torch.empty((1, int(self.config["out_channels"])) + self.output_size(h, w), dtype=torch.float32, device=z.device)
            _invoke("nesr_vae_decode_f32", z.device, handle, (z, n, ch, h, w, out, out.numel()))
        self.calls += 1
        return out

    forward = decode

    def decode_latents_u8(self, latents, tile=None, tile_overlap=0):
        """latents [1, latent_channels, h, w] float32 on the device, as the denoising loop leaves them -> the uint8 RGB frame
        [h s, w s, 3] on the device: / scaling_factor, decode, / 2 + 0.5, clamp, x 255, round half to even.
        `tile` (latent pixels): the decode runs over overlapping windows of min(tile, h) x min(tile, w) whose seams are blended on
        the device with ramps of `tile_overlap` (nesr_vae_decode_latents_tiled_u8), which lifts the limit of 65536 latents; h, w,
        tile and tile_overlap are even.  One window gives the untiled bytes.  `calls` rises by the number of windows."""
        z = self._latents(latents, "decode_latents_u8")
        n, ch, h, w = z.shape
        with torch.cuda.device(z.device):
            handle = self._context(z.device)
            if tile is None:
                out = torch.empty(self.output_size(h, w) + (3,), dtype=torch.uint8, device=z.device)
                _invoke("nesr_vae_decode_latents_u8", z.device, handle, (z, n, ch, h, w, out, out.numel()))
                self.calls += 1
                return out
            s = 2 ** (len(self.config["block_out_channels"]) - 1)
            out = torch.empty((h * s, w * s, 3), dtype=torch.uint8, device=z.device)
            _invoke("nesr_vae_decode_latents_tiled_u8", z.device, handle, (z, n, ch, h, w, int(tile), int(tile_overlap), out, out.numel()))
        (ky, kx), _, _ = sdx4_tile_plan(h, w, 2, int(tile), int(tile_overlap))
        self.calls += ky * kx
        return out
