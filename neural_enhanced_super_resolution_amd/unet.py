"""``UNet2DCondition``: diffusers' ``UNet2DConditionModel`` as ``StableDiffusionUpscalePipeline`` uses it
("stabilityai/stable-diffusion-x4-upscaler", nesr/nesr.py:243-283, 988-1031), as HIP kernels behind the C ABI (csrc/unet.hip,
csrc/unet_api.cpp).  It is the network the denoising loop calls twenty times a frame, on a batch of two (classifier-free guidance).

The module owns ordinary torch Parameters under diffusers' names (``time_embedding.linear_1.weight``, ``down_blocks.1.attentions.0.
transformer_blocks.0.attn1.to_q.weight`` ...) and has no torch implementation of its forward.  ``forward(sample, timestep,
encoder_hidden_states, class_labels)`` takes [n, in_channels, h, w] and [n, tokens, cross_attention_dim] float32 on the device,
n = 1 or 2, and gives [n, out_channels, h, w].  The samples share the timestep and the class label (the pipeline's noise level).

Supported: the configuration family of the published model.  2 to 4 levels of DownBlock2D / CrossAttnDownBlock2D and their
mirrors, the mid block UNetMidBlock2DCrossAttn, layers_per_block 1 to 3, widths up to 1024, head widths 8 to 128 in steps of 8
(``attention_head_dim`` is the NUMBER of heads in this family), cross_attention_dim up to 1024, use_linear_projection.  Anything
else raises NesrUnsupportedError when the context is created, and the message names the field.

``compute_dtype="fp16"`` selects the fp16 compute form: storage stays float32 in and out, both operands of
every 3x3 conv and row product are rounded to f16 and multiplied on the f16 matrix cores with f32 sums, and the device holds the f16
copy of those weights instead of their f32 form.  A weight of those products beyond +-65504 raises NesrRangeError when the context
is made, an activation beyond it raises NesrRangeError from ``forward``, which is synchronous in this form.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch

from . import _lib
from ._contexts import _invoke
from ._hfnet import _HFNet, _merged_config

# the published x4 upscaler's values, recalled from memory: a config.json beside the weights, or the arguments, override them
DEFAULTS = dict(in_channels=7, out_channels=4, block_out_channels=(256, 512, 512, 1024),
                down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", layers_per_block=2, attention_head_dim=8, cross_attention_dim=1024,
                only_cross_attention=(True, True, True, False), use_linear_projection=True, num_class_embeds=1000, norm_num_groups=32,
                norm_eps=1e-5, flip_sin_to_cos=True, freq_shift=0, downsample_padding=1, act_fn="silu", transformer_layers_per_block=1,
                dual_cross_attention=False)
KERNEL_GROUPS = ("conv", "norm", "attention", "projection", "feedforward", "embedding", "resample")      # NESR_UNET_GROUP_*
COMPUTE_DTYPES = {"f32": _lib.DTYPE_F32, "fp16": _lib.DTYPE_F16}
_TUPLES = ("block_out_channels", "down_block_types", "up_block_types", "only_cross_attention")


def _config(cfg):
    c = _merged_config("UNet2DCondition", DEFAULTS, cfg)
    if not c["block_out_channels"]:
        raise ValueError("UNet2DCondition: block_out_channels is empty")
    levels = len(c["block_out_channels"])
    if isinstance(c["only_cross_attention"], bool):
        c["only_cross_attention"] = (c["only_cross_attention"],) * levels
    for name in _TUPLES:
        c[name] = tuple(c[name])
        if len(c[name]) != levels:
            raise ValueError(f"UNet2DCondition: {name} has {len(c[name])} entries, block_out_channels has {levels}")
    c["block_out_channels"] = tuple(int(v) for v in c["block_out_channels"])
    c["only_cross_attention"] = tuple(bool(v) for v in c["only_cross_attention"])
    if not isinstance(c["attention_head_dim"], int):
        raise ValueError("UNet2DCondition: attention_head_dim is one integer, the number of heads of every block")
    return c


def unet_state_dict_spec(**cfg):
    """Ordered {key: shape} of a UNet2DConditionModel checkpoint of this configuration family.  Keyword arguments are the
    configuration's fields."""
    c = _config(cfg)
    widths, layers, cross = c["block_out_channels"], int(c["layers_per_block"]), int(c["cross_attention_dim"])
    levels, td = len(widths), 4 * widths[0]
    spec = OrderedDict()

    def wb(name, wshape, bias=True):
        spec[name + ".weight"] = tuple(wshape)
        if bias:
            spec[name + ".bias"] = (wshape[0],)

    def resnet(r, cin, cout):
        wb(r + ".norm1", (cin,))
        wb(r + ".conv1", (cout, cin, 3, 3))
        wb(r + ".time_emb_proj", (cout, td))
        wb(r + ".norm2", (cout,))
        wb(r + ".conv2", (cout, cout, 3, 3))
        if cin != cout:
            wb(r + ".conv_shortcut", (cout, cin, 1, 1))

    def transformer(a, dim, only_cross):
        wb(a + ".norm", (dim,))
        wb(a + ".proj_in", (dim, dim))
        b = a + ".transformer_blocks.0"
        for i in (1, 2):
            kv = cross if (i == 2 or only_cross) else dim
            wb(f"{b}.norm{i}", (dim,))
            wb(f"{b}.attn{i}.to_q", (dim, dim), bias=False)
            wb(f"{b}.attn{i}.to_k", (dim, kv), bias=False)
            wb(f"{b}.attn{i}.to_v", (dim, kv), bias=False)
            wb(f"{b}.attn{i}.to_out.0", (dim, dim))
        wb(b + ".norm3", (dim,))
        wb(b + ".ff.net.0.proj", (8 * dim, dim))
        wb(b + ".ff.net.2", (dim, 4 * dim))
        wb(a + ".proj_out", (dim, dim))

    wb("conv_in", (widths[0], int(c["in_channels"]), 3, 3))
    wb("time_embedding.linear_1", (td, widths[0]))
    wb("time_embedding.linear_2", (td, td))
    spec["class_embedding.weight"] = (int(c["num_class_embeds"]), td)
    prev = widths[0]
    for i, wd in enumerate(widths):
        if c["down_block_types"][i] == "CrossAttnDownBlock2D":
            for j in range(layers):
                transformer(f"down_blocks.{i}.attentions.{j}", wd, c["only_cross_attention"][i])
        for j in range(layers):
            resnet(f"down_blocks.{i}.resnets.{j}", prev if j == 0 else wd, wd)
        if i < levels - 1:
            wb(f"down_blocks.{i}.downsamplers.0.conv", (wd, wd, 3, 3))
        prev = wd
    rev = widths[::-1]
    for i, wd in enumerate(rev):
        before, in_ch = rev[max(i - 1, 0)], rev[min(i + 1, levels - 1)]
        if c["up_block_types"][i] == "CrossAttnUpBlock2D":
            for j in range(layers + 1):
                transformer(f"up_blocks.{i}.attentions.{j}", wd, c["only_cross_attention"][levels - 1 - i])
        for j in range(layers + 1):
            resnet(f"up_blocks.{i}.resnets.{j}", (before if j == 0 else wd) + (in_ch if j == layers else wd), wd)
        if i < levels - 1:
            wb(f"up_blocks.{i}.upsamplers.0.conv", (wd, wd, 3, 3))
    transformer("mid_block.attentions.0", widths[-1], False)
    resnet("mid_block.resnets.0", widths[-1], widths[-1])
    resnet("mid_block.resnets.1", widths[-1], widths[-1])
    wb("conv_norm_out", (widths[0],))
    wb("conv_out", (int(c["out_channels"]), widths[0], 3, 3))
    return spec


def launches_per_forward(**cfg):
    """Kernel launches of one forward, whatever the frame and n: 5 at the head (sample and text states as
    rows, the embedding, every ResnetBlock's conv1 bias, conv_in), 6 a ResnetBlock + 1 for its shortcut, + 1 for the second
    source's statistics over a concatenation, 17 a Transformer whose attn1 reads the text states and 16 where it reads the tokens,
    1 a resampling conv, 3 at the tail."""
    c = _config(cfg)
    widths, layers, levels = c["block_out_channels"], int(c["layers_per_block"]), len(c["block_out_channels"])
    total, prev = 5 + 3, widths[0]
    for i, wd in enumerate(widths):
        tf = (17 if c["only_cross_attention"][i] else 16) if c["down_block_types"][i] == "CrossAttnDownBlock2D" else 0
        for j in range(layers):
            total += 6 + (1 if (prev if j == 0 else wd) != wd else 0) + tf
        total += 1 if i < levels - 1 else 0
        prev = wd
    total += 6 + 16 + 6                                        # the mid block
    for i in range(levels):
        level = levels - 1 - i
        tf = (17 if c["only_cross_attention"][level] else 16) if c["up_block_types"][i] == "CrossAttnUpBlock2D" else 0
        total += (layers + 1) * (8 + tf) + (1 if i < levels - 1 else 0)
    return total


class UNet2DCondition(_HFNet):
    """UNet2DConditionModel.forward in eval mode on the HIP path.  Keyword arguments are the configuration's fields."""

    PREFIX, NAME, KERNEL_GROUPS, DEFAULTS = "nesr_unet", "UNet2DCondition", KERNEL_GROUPS, DEFAULTS
    TRAIN_ERROR = "UNet2DCondition is inference only"
    _spec = staticmethod(unet_state_dict_spec)
    CHECKPOINT_FILES = ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin")

    def __init__(self, compute_dtype="f32", **cfg):
        if compute_dtype not in COMPUTE_DTYPES:
            raise ValueError(f"UNet2DCondition: compute_dtype {compute_dtype!r}: expected 'f32' or 'fp16'")
        super().__init__(_config(cfg))
        self.compute_dtype = compute_dtype

    @classmethod
    def from_checkpoint(cls, path, compute_dtype="f32", **cfg):
        """A UNet with the weights of a local ``diffusion_pytorch_model.safetensors`` / ``.bin`` (or of the ``unet/`` directory
        that holds one).  A ``config.json`` beside the weights supplies the configuration's fields; arguments override it.  Nothing
        is ever fetched."""
        return super().from_checkpoint(path, compute_dtype=compute_dtype, **cfg)

    def _create(self, index):
        """A context of this configuration without weights (NesrUnsupportedError names the field the kernels do not take)."""
        lib = _lib.load()
        c = self.config
        widths = c["block_out_channels"]
        n = len(widths)
        strings = lambda names: (ctypes.c_char_p * n)(*[str(v).encode() for v in names])
        handle = _HFNet._create_handle(      # not through self: the refusal tests call _create with a bare configuration holder
            "nesr_unet_create", index, int(c["in_channels"]), int(c["out_channels"]), n, (ctypes.c_int * n)(*widths),
            strings(c["down_block_types"]), strings(c["up_block_types"]), str(c["mid_block_type"]).encode(),
            (ctypes.c_int * n)(*[int(v) for v in c["only_cross_attention"]]), int(c["layers_per_block"]),
            int(c["attention_head_dim"]), int(c["cross_attention_dim"]), int(c["transformer_layers_per_block"]),
            int(bool(c["use_linear_projection"])), int(bool(c["dual_cross_attention"])), int(c["num_class_embeds"] or 0),
            int(c["norm_num_groups"]), float(c["norm_eps"]), int(bool(c["flip_sin_to_cos"])), float(c["freq_shift"]),
            int(c["downsample_padding"]), str(c["act_fn"]).encode())
        try:
            _lib.check(lib.nesr_unet_set_dtype(handle, COMPUTE_DTYPES[getattr(self, "compute_dtype", "f32")]), "nesr_unet_set_dtype")
        except Exception:
            lib.nesr_unet_destroy(handle)
            raise
        return handle

    def weight_bytes(self, device=None):
        """Bytes of weights the context of `device` holds on it: in the fp16 form the f16 copy of the GEMM weights and the f32 rest."""
        return self._query_size("nesr_unet_weight_bytes", device)

    # ------------------------------------------------------------------ forward
    def workspace_bytes(self, n, h, w, tokens, device=None):
        """Bytes of workspace a forward of n samples of h x w latents with `tokens` text states allocates on the context of `device`."""
        return self._query_size("nesr_unet_workspace_bytes", device, int(n), int(h), int(w), int(tokens))

    def forward(self, sample, timestep, encoder_hidden_states, class_labels):
        """sample [n, in_channels, h, w] and encoder_hidden_states [n, tokens, cross_attention_dim], float32 on the device; timestep
        a number (or a one-element tensor); class_labels an integer (or a tensor whose elements are all that integer) -> the
        predicted noise [n, out_channels, h, w]."""
        self._require_device(sample, "forward")
        self._require_device(encoder_hidden_states, "forward")
        if sample.dim() != 4 or sample.dtype != torch.float32:
            raise ValueError(f"UNet2DCondition.forward: sample is [n, {self.config['in_channels']}, h, w] float32, got {sample.dtype} {tuple(sample.shape)}")
        text = encoder_hidden_states
        if text.dim() != 3 or text.dtype != torch.float32 or text.shape[0] != sample.shape[0] or text.shape[2] != int(self.config["cross_attention_dim"]):
            raise ValueError(f"UNet2DCondition.forward: encoder_hidden_states is [{sample.shape[0]}, tokens, {self.config['cross_attention_dim']}] float32, "
                             f"got {text.dtype} {tuple(text.shape)}")
        if torch.is_tensor(timestep):
            if timestep.numel() != 1:
                raise ValueError("UNet2DCondition.forward: one timestep for the batch")
            timestep = timestep.item()
        if torch.is_tensor(class_labels):
            labels = class_labels.reshape(-1).tolist()
            if not labels or any(v != labels[0] for v in labels):
                raise ValueError("UNet2DCondition.forward: one class label for the batch")
            class_labels = labels[0]
        sample, text = sample.contiguous(), text.contiguous()
        n, ch, h, w = sample.shape
        with torch.cuda.device(sample.device):
            handle = self._context(sample.device)
            out = torch.empty((n, int(self.config["out_channels"]), h, w), dtype=torch.float32, device=sample.device)
            _invoke("nesr_unet_forward_f32", sample.device, handle,
                    (sample, n, ch, h, w, ctypes.c_double(float(timestep)), int(class_labels), text, int(text.shape[1]), out, out.numel()))
        self.calls += 1
        return out
