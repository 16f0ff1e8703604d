"""``ClipTextEncoder``: transformers' ``CLIPTextModel`` as ``StableDiffusionUpscalePipeline`` uses it
("stabilityai/stable-diffusion-x4-upscaler", nesr/nesr.py:243-283, 988-1031), as HIP kernels behind the C ABI (csrc/clip_text.hip,
csrc/clip_text_api.cpp; every product and every LayerNorm inside a layer is a launcher of csrc/unet.hip as it is).  It runs once a
frame, on the prompt and the negative prompt, and its result is the UNet's ``encoder_hidden_states``.

The module owns ordinary torch Parameters under ``transformers``-5's names (``embeddings.token_embedding.weight``,
``encoder.layers.0.self_attn.k_proj.weight`` ..., ``final_layer_norm.bias``), takes a state dict of either key generation
(published ``text_encoder/`` files carry ``text_model.`` in front and an ``embeddings.position_ids`` buffer) and has no torch
implementation of its forward.  ``forward(input_ids)`` takes [n, tokens] integer ids, n = 1 or 2, on the host or on the device,
and gives ``last_hidden_state`` [n, tokens, hidden_size] float32 on the device: ``CLIPTextModel(input_ids)[0]``.  The attention
mask is causal only: the pipeline passes none, so a padding id is an ordinary token.  The pooled output and ``text_projection``
are not computed.

Supported: hidden_size up to 1024 that is a multiple of the heads, head widths 8 to 128 in steps of 8, intermediate_size up to
4096, any layer count, hidden_act "gelu" (erf) or "quick_gelu".  Anything else raises NesrUnsupportedError when the context is
created, and the message names the field.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch

from ._contexts import _invoke
from ._hfnet import _HFNet, _merged_config

# the published x4 upscaler's values, recalled from memory: a config.json beside the weights, or the arguments, override them
DEFAULTS = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16,
                max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="gelu")
KERNEL_GROUPS = ("embedding", "norm", "projection", "attention", "feedforward")      # NESR_CLIP_TEXT_GROUP_*
PREFIX = "text_model."
POSITION_IDS = "embeddings.position_ids"


def _config(cfg):
    c = _merged_config("ClipTextEncoder", DEFAULTS, cfg)
    for name in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings"):
        c[name] = int(c[name])
        if c[name] < 1:
            raise ValueError(f"ClipTextEncoder: {name} must be positive, got {c[name]}")
    return c


def clip_text_state_dict_spec(**cfg):
    """Ordered {key: shape} of a transformers-5 ``CLIPTextModel`` state dict.  Keyword arguments are the configuration's fields."""
    c = _config(cfg)
    h, inter = c["hidden_size"], c["intermediate_size"]
    spec = OrderedDict()

    def wb(name, wshape):
        spec[name + ".weight"] = tuple(wshape)
        spec[name + ".bias"] = (wshape[0],)

    spec["embeddings.token_embedding.weight"] = (c["vocab_size"], h)
    spec["embeddings.position_embedding.weight"] = (c["max_position_embeddings"], h)
    for i in range(c["num_hidden_layers"]):
        layer = f"encoder.layers.{i}"
        for part in ("k_proj", "v_proj", "q_proj", "out_proj"):
            wb(f"{layer}.self_attn.{part}", (h, h))
        wb(f"{layer}.layer_norm1", (h,))
        wb(f"{layer}.mlp.fc1", (inter, h))
        wb(f"{layer}.mlp.fc2", (h, inter))
        wb(f"{layer}.layer_norm2", (h,))
    wb("final_layer_norm", (h,))
    return spec


def new_key(key):
    """The transformers-5 name of a checkpoint key of either generation (a new name comes back as it is)."""
    return key[len(PREFIX):] if key.startswith(PREFIX) else key


def text_state_dict(state_dict):
    """A CLIPTextModel state dict under the current names: ``text_model.`` stripped and the ``embeddings.position_ids`` buffer
    (arange(max_position_embeddings)) dropped.  Every other key passes as it is (and is refused later if it is not expected)."""
    out = OrderedDict()
    for key, value in state_dict.items():
        key = new_key(key)
        if key != POSITION_IDS:
            out[key] = value
    return out


def launches_per_forward(**cfg):
    """Kernel launches of one forward, whatever n and tokens: the embedding gather; per layer the statistics
    of layer_norm1, q | k | v, the attention, out_proj, the statistics of layer_norm2, fc1, its activation, fc2; the statistics of
    final_layer_norm and its application."""
    return 1 + 8 * _config(cfg)["num_hidden_layers"] + 2


class ClipTextEncoder(_HFNet):
    """CLIPTextModel(input_ids)[0] in eval mode on the HIP path.  Keyword arguments are the configuration's fields."""

    PREFIX, NAME, KERNEL_GROUPS, DEFAULTS = "nesr_clip_text", "ClipTextEncoder", KERNEL_GROUPS, DEFAULTS
    TRAIN_ERROR = "ClipTextEncoder is inference only"
    _spec = staticmethod(clip_text_state_dict_spec)

    def __init__(self, **cfg):
        super().__init__(_config(cfg))

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Strict: a missing or an unexpected key raises.  ``text_model.`` is stripped and ``embeddings.position_ids`` dropped first
        (text_state_dict), so a published file and a transformers-5 state dict both load."""
        return super().load_state_dict(text_state_dict(state_dict), strict=strict, **kw)

    def _create(self, index):
        """A context of this configuration without weights (NesrUnsupportedError names the field the kernels do not take)."""
        c = self.config
        return self._create_handle("nesr_clip_text_create", index, int(c["vocab_size"]), int(c["hidden_size"]), int(c["intermediate_size"]),
                                   int(c["num_hidden_layers"]), int(c["num_attention_heads"]), int(c["max_position_embeddings"]),
                                   float(c["layer_norm_eps"]), str(c["hidden_act"]).encode())

    # ------------------------------------------------------------------ forward
    def workspace_bytes(self, n, tokens, device=None):
        """Bytes of workspace an encode of n samples of `tokens` ids allocates on the context of `device`."""
        return self._query_size("nesr_clip_text_workspace_bytes", device, int(n), int(tokens))

    def forward(self, input_ids, device=None):
        """input_ids [n, tokens] integers (a tensor anywhere, an array or nested lists: the entry reads them on the host) ->
        last_hidden_state [n, tokens, hidden_size] float32 on `device` (default: the ids' device if they are on one, else the
        parameters')."""
        if torch.is_tensor(input_ids):
            if input_ids.dtype.is_floating_point or input_ids.dtype == torch.bool:
                raise ValueError(f"ClipTextEncoder.forward: input_ids are integers, got {input_ids.dtype}")
            if device is None and input_ids.is_cuda:
                device = input_ids.device
            ids = input_ids.detach().to("cpu", torch.int64)
        else:
            ids = torch.as_tensor(input_ids, dtype=torch.int64)
        if ids.dim() != 2 or ids.numel() == 0:
            raise ValueError(f"ClipTextEncoder.forward: input_ids is [n, tokens], got {tuple(ids.shape)}")
        device = torch.device(next(self.parameters()).device if device is None else device)
        if device.type != "cuda":
            raise RuntimeError(f"ClipTextEncoder.forward: the module is on {device}; the forward runs on the ROCm device only "
                               "(there is no CPU or PyTorch fallback)")
        n, tokens = ids.shape
        if int(ids.min()) < -2 ** 31 or int(ids.max()) >= 2 ** 31:
            raise ValueError("ClipTextEncoder.forward: an id does not fit 32 bits")
        host = (ctypes.c_int32 * (n * tokens))(*ids.reshape(-1).tolist())
        with torch.cuda.device(device):
            handle = self._context(device)
            out = torch.empty((n, tokens, int(self.config["hidden_size"])), dtype=torch.float32, device=device)
            _invoke("nesr_clip_text_encode_f32", device, handle, (host, n, tokens, out, out.numel()))
        self.calls += 1
        return out
