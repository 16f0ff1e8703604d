"""``Swin2SR``: transformers' ``Swin2SRForImageSuperResolution`` (the SwinV2 window-attention super-resolution transformer) as HIP
kernels behind the C ABI (csrc/swin2sr.hip, csrc/swin2sr_api.cpp): a second upscaler for the slot the reference's ensemble step
averages over (nesr/nesr.py:1033-1054) and its first-generation pipeline leaves a stub (standalone/superres_project.py:80-88).

The module owns ordinary torch Parameters under ``transformers``-5's names (``swin2sr.encoder.stages.{i}.layers.{j}.attention.self.
query.weight`` ...; there is one key generation, transformers' conversion mapping renames nothing for Swin2SR) and has no torch
implementation of its forward.  ``forward(pixel_values)`` gives the reconstruction [1, C_out, H s, W s] of a [1, C, H, W] float32
tensor whose H and W are multiples of the window (transformers itself fails on anything else); ``upscale(frame)`` takes an
[H, W, 3] uint8 RGB frame of any size and returns the uint8 frame [H s, W s, 3], doing what ``Swin2SRImageProcessor`` and the
documented post-processing do (/ 255, symmetric padding to (n // 8 + 1) * 8, the model, the crop, clamp, x 255, round).  Both run
on the ROCm device; calling the object with a uint8 HWC frame is ``upscale``.  ``upscale(frame, tile=T, tile_pad=P)`` cuts a large
frame into windows of one shape that run as a batch (``tile_plan``), and ``forward_batch`` takes [N, C, H, W].
``upscale(frame, tile=T, tile_overlap=O)`` is the Swin2SR authors' tiling instead: overlapped windows of the frame padded once to the
window, their float outputs averaged where they overlap (``overlap_plan``).

Supported: upsampler pixelshuffle (x2^n, x3), pixelshuffledirect, nearest+conv (x4); resi_connection "1conv"; patch_size 1;
qkv_bias True; image_size > window_size; the same number of heads in every stage.  Anything else raises NesrUnsupportedError
when the context is created, and the message names the field.

``Swin2SR(compute_dtype="fp16", **cfg)`` (``SRVGGNetCompact``'s name for it) selects the fp16 compute form: storage stays float32,
every GEMM takes both operands rounded to f16 with f32 sums on the f16 matrix cores (include/nesr_hip.h lists them).  The default
``"f32"`` is the path above.  ``.half()`` does not select it.  f16 carries |x| <= 65504: a weight beyond that raises
``NesrRangeError`` when the context is made, an activation beyond it when the forward returns (the fp16 form's calls wait for the
stream).  ``part(part, stage, layer, tokens)`` runs one launch of the model (an attention block, an MLP block or a stage's 3x3
conv) on given tokens, in the model's form.
"""
from __future__ import annotations

import ctypes
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._contexts import _invoke
from ._hfnet import _HFNet, _merged_config

DEFAULTS = dict(image_size=64, patch_size=1, num_channels=3, num_channels_out=None, embed_dim=180, depths=(6, 6, 6, 6, 6, 6),
                num_heads=(6, 6, 6, 6, 6, 6), window_size=8, mlp_ratio=2.0, qkv_bias=True, use_absolute_embeddings=False,
                layer_norm_eps=1e-5, upscale=2, img_range=1.0, resi_connection="1conv", upsampler="pixelshuffle")
NUM_FEATURES = 64                     # the width of the pixelshuffle and nearest+conv heads
KERNEL_GROUPS = ("conv", "projection", "attention", "mlp", "upsample")      # NESR_S2_GROUP_*
_IGNORED = ("relative_position_index", "relative_coords_table", "attn_mask")      # buffers older checkpoints carry
COMPUTE_DTYPES = {"f32": _lib.DTYPE_F32, "fp16": _lib.DTYPE_F16}
PARTS = {"attention": 0, "mlp": 1, "stage_conv": 2}      # NESR_S2_PART_*


def _config(cfg):
    c = _merged_config("Swin2SR", DEFAULTS, cfg)
    c["depths"], c["num_heads"] = tuple(int(v) for v in c["depths"]), tuple(int(v) for v in c["num_heads"])
    if len(c["depths"]) != len(c["num_heads"]) or not c["depths"]:
        raise ValueError(f"Swin2SR: depths and num_heads must have the same, positive number of entries, got {c['depths']} and {c['num_heads']}")
    if c["num_channels_out"] is None:
        c["num_channels_out"] = c["num_channels"]
    return c


def swin2sr_state_dict_spec(**cfg):
    """Ordered {key: shape} of a Swin2SRForImageSuperResolution checkpoint under transformers-5's names.  Keyword arguments are
    Swin2SRConfig's fields; the defaults are the configuration class's own (classical x2: embed 180, six stages of six layers)."""
    c = _config(cfg)
    C, hid, nf = int(c["embed_dim"]), int(c["mlp_ratio"] * c["embed_dim"]), NUM_FEATURES
    spec = OrderedDict()

    def wb(name, wshape, bias=True):
        spec[name + ".weight"] = tuple(wshape)
        if bias:
            spec[name + ".bias"] = (wshape[0],)

    wb("swin2sr.first_convolution", (C, c["num_channels"], 3, 3))
    wb("swin2sr.embeddings.patch_embeddings.projection", (C, C, 1, 1))
    wb("swin2sr.embeddings.patch_embeddings.layernorm", (C,))
    for i, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
        s = f"swin2sr.encoder.stages.{i}"
        for j in range(depth):
            layer, a = f"{s}.layers.{j}", f"{s}.layers.{j}.attention.self"
            spec[a + ".logit_scale"] = (heads, 1, 1)
            wb(a + ".continuous_position_bias_mlp.0", (512, 2))
            wb(a + ".continuous_position_bias_mlp.2", (heads, 512), bias=False)
            wb(a + ".query", (C, C), bias=bool(c["qkv_bias"]))
            wb(a + ".key", (C, C), bias=False)
            wb(a + ".value", (C, C), bias=bool(c["qkv_bias"]))
            wb(layer + ".attention.output.dense", (C, C))
            wb(layer + ".layernorm_before", (C,))
            wb(layer + ".intermediate.dense", (hid, C))
            wb(layer + ".output.dense", (C, hid))
            wb(layer + ".layernorm_after", (C,))
        wb(s + ".conv", (C, C, 3, 3))
        wb(s + ".patch_embed.projection", (C, C, 1, 1))
    wb("swin2sr.layernorm", (C,))
    wb("swin2sr.conv_after_body", (C, C, 3, 3))
    up, scale, cout = c["upsampler"], int(c["upscale"]), c["num_channels_out"]
    if up == "pixelshuffledirect":
        wb("upsample.conv", (scale * scale * cout, C, 3, 3))
    elif up in ("pixelshuffle", "nearest+conv"):
        wb("upsample.conv_before_upsample", (nf, C, 3, 3))
        if up == "nearest+conv":
            for name in ("conv_up1", "conv_up2", "conv_hr"):
                wb("upsample." + name, (nf, nf, 3, 3))
        elif scale == 3:
            wb("upsample.upsample.convolution", (9 * nf, nf, 3, 3))
        else:
            for i in range(int(math.log2(max(scale, 1)))):
                wb(f"upsample.upsample.convolution_{i}", (4 * nf, nf, 3, 3))
        wb("upsample.final_convolution", (cout, nf, 3, 3))
    # any other head has no supported weight set: the context's creation names the field
    return spec


class Swin2SR(_HFNet):
    """Swin2SRForImageSuperResolution in eval mode on the HIP path.  Keyword arguments are Swin2SRConfig's fields."""

    PREFIX, NAME, KERNEL_GROUPS = "nesr_swin2sr", "Swin2SR", KERNEL_GROUPS
    TRAIN_ERROR = "Swin2SR is inference only (eval mode: no dropout, no stochastic depth)"
    _spec = staticmethod(swin2sr_state_dict_spec)

    def __init__(self, compute_dtype="f32", **cfg):
        if compute_dtype not in COMPUTE_DTYPES:
            raise ValueError(f"Swin2SR: compute_dtype {compute_dtype!r}: expected 'f32' or 'fp16' (bf16 is not a form of this network: its 8 "
                             "significand bits cost 0.2 to 0.4 in the logits of cosine attention)")
        super().__init__(_config(cfg))
        self.compute_dtype = compute_dtype

    def _register_leaf(self, mod, leaf, shape, init=None):
        super()._register_leaf(mod, leaf, shape, torch.full(shape, math.log(10.0)) if leaf == "logit_scale" else init)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Strict: a missing or an unexpected key raises.  The buffers older checkpoints carry (relative_position_index,
        relative_coords_table, attn_mask) are dropped: they follow from the configuration."""
        sd = OrderedDict((k, v) for k, v in state_dict.items() if not k.endswith(_IGNORED))
        return super().load_state_dict(sd, strict=strict, **kw)

    def _create(self, index):
        """A context of this configuration without weights (NesrUnsupportedError names the field the kernels do not take)."""
        lib = _lib.load()
        c = self.config
        n = len(c["depths"])
        handle = self._create_handle(
            "nesr_swin2sr_create", index, int(c["image_size"]), int(c["patch_size"]), int(c["num_channels"]),
            int(c["num_channels_out"]), int(c["embed_dim"]), n, (ctypes.c_int * n)(*c["depths"]),
            (ctypes.c_int * n)(*c["num_heads"]), int(c["window_size"]), float(c["mlp_ratio"]), int(bool(c["qkv_bias"])),
            int(bool(c["use_absolute_embeddings"])), float(c["layer_norm_eps"]), int(c["upscale"]), float(c["img_range"]),
            str(c["resi_connection"]).encode(), str(c["upsampler"]).encode())
        try:
            _lib.check(lib.nesr_swin2sr_set_dtype(handle, COMPUTE_DTYPES[self.compute_dtype]), "nesr_swin2sr_set_dtype")
        except Exception:
            lib.nesr_swin2sr_destroy(handle)
            raise
        return handle

    # ------------------------------------------------------------------ forward
    def output_size(self, h, w):
        """(oh, ow) of the result for an h x w input or frame: h s x w s, as the library computes it.  Needs no device."""
        oh, ow = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().nesr_swin2sr_output_size(int(self.config["upscale"]), int(h), int(w), ctypes.byref(oh), ctypes.byref(ow)),
                   "nesr_swin2sr_output_size")
        return oh.value, ow.value

    def forward(self, pixel_values):
        """pixel_values [1, C, H, W] float32 on the device (H, W multiples of window_size) -> reconstruction [1, C_out, H s, W s]."""
        if pixel_values.dtype == torch.uint8 and pixel_values.dim() == 3:
            return self.upscale(pixel_values)
        x = self._pixel_values(pixel_values)
        n, ch, h, w = x.shape
        with torch.cuda.device(x.device):
            handle = self._context(x.device)
            out = torch.empty((1, self.config["num_channels_out"]) + self.output_size(h, w), dtype=torch.float32, device=x.device)
            _invoke("nesr_swin2sr_forward_f32", x.device, handle, (x, n, ch, h, w, out, out.numel()))
        self.calls += 1
        return out

    def forward_batch(self, pixel_values):
        """pixel_values [N, C, H, W] float32 on the device (N >= 1; H, W multiples of window_size) -> [N, C_out, H s, W s].  The N
        images go through every launch together; each gets the bits `forward` gives it alone."""
        x = self._pixel_values(pixel_values)
        n, ch, h, w = x.shape
        with torch.cuda.device(x.device):
            handle = self._context(x.device)
            out = torch.empty((n, self.config["num_channels_out"]) + self.output_size(h, w), dtype=torch.float32, device=x.device)
            _invoke("nesr_swin2sr_forward_batch_f32", x.device, handle, (x, n, ch, h, w, out, out.numel()))
        self.calls += 1
        return out

    def part(self, part, stage, layer, tokens):
        """One launch of the model, in its compute form, on `tokens` [N, H, W, C] float32 on the device (C = embed_dim; H, W
        multiples of window_size) -> the same shape.  part "attention": the attention block of layer `layer` of stage `stage`
        (shifted when `layer` is odd), tokens + LayerNorm(output.dense(attention)); "mlp": its MLP block, tokens +
        LayerNorm(fc2(GELU(fc1(tokens)))); "stage_conv": the stage's 3x3 convolution (`layer` is ignored)."""
        if part not in PARTS:
            raise ValueError(f"Swin2SR.part: part {part!r}: expected one of {sorted(PARTS)}")
        self._require_device(tokens, "part")
        if tokens.dim() != 4 or tokens.dtype != torch.float32 or tokens.shape[3] != self.config["embed_dim"]:
            raise ValueError(f"Swin2SR.part: an [N, H, W, {self.config['embed_dim']}] float32 tensor, got {tokens.dtype} {tuple(tokens.shape)}")
        x = tokens.contiguous()
        n, h, w, _ = x.shape
        with torch.cuda.device(x.device):
            handle = self._context(x.device)
            out = torch.empty_like(x)
            _invoke("nesr_swin2sr_part_f32", x.device, handle, (PARTS[part], int(stage), int(layer), x, n, h, w, out, out.numel()))
        return out

    def tile_plan(self, h, w, tile, tile_pad=16):
        """The plan `upscale(tile=, tile_pad=)` follows on an h x w frame, as the library computes it (needs no device):
        {"tiles": (tiles_y, tiles_x), "window": (win_h, win_w), "plan": int32 array [tiles, 8]}, a row (win_y, win_x, crop_y, crop_x,
        crop_h, crop_w, out_y, out_x) per tile in row-major order: the window's origin in the frame, then the core inside the
        window's output and its place in the result, in output pixels.  Every window has one shape: at the edge it slides inward."""
        lib, args = _lib.load(), (int(self.config["upscale"]), int(h), int(w), int(tile), int(tile_pad))
        ty, tx, wh, ww = (ctypes.c_int(0) for _ in range(4))
        counts = (ctypes.byref(ty), ctypes.byref(tx), ctypes.byref(wh), ctypes.byref(ww))
        _lib.check(lib.nesr_swin2sr_tile_plan(*args, *counts, None, 0), "nesr_swin2sr_tile_plan")
        plan = np.zeros((ty.value * tx.value, 8), np.int32)
        _lib.check(lib.nesr_swin2sr_tile_plan(*args, *counts, plan.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), plan.size), "nesr_swin2sr_tile_plan")
        return {"tiles": (ty.value, tx.value), "window": (wh.value, ww.value), "plan": plan}

    def workspace_bytes(self, win_h, win_w, batch=1, device=None):
        """Bytes of workspace a forward of `batch` frames (or windows) of win_h x win_w allocates on the context of `device`."""
        return self._query_size("nesr_swin2sr_workspace_bytes", device, int(win_h), int(win_w), int(batch))

    def overlap_plan(self, h, w, tile, tile_overlap):
        """The plan `upscale(tile=, tile_overlap=)` follows on an h x w frame, as the library computes it (needs no device):
        {"tiles": (tiles_y, tiles_x), "tile": t, "padded": (hp, wp), "plan": int32 array [windows, 4]}, a row (win_y, win_x, out_y,
        out_x) per t x t window in row-major order: its origin in the frame padded to hp x wp (multiples of the window), in input
        and in output pixels.  t = min(tile, hp, wp); the last window of an axis ends at the padded frame's edge."""
        lib = _lib.load()
        args = (int(self.config["upscale"]), int(self.config["window_size"]), int(h), int(w), int(tile), int(tile_overlap))
        ty, tx, t, hp, wp = (ctypes.c_int(0) for _ in range(5))
        counts = tuple(ctypes.byref(v) for v in (ty, tx, t, hp, wp))
        _lib.check(lib.nesr_swin2sr_overlap_plan(*args, *counts, None, 0), "nesr_swin2sr_overlap_plan")
        plan = np.zeros((ty.value * tx.value, 4), np.int32)
        _lib.check(lib.nesr_swin2sr_overlap_plan(*args, *counts, plan.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), plan.size), "nesr_swin2sr_overlap_plan")
        return {"tiles": (ty.value, tx.value), "tile": t.value, "padded": (hp.value, wp.value), "plan": plan}

    def overlap_workspace_bytes(self, h, w, tile, tile_overlap, batch=1, device=None):
        """Bytes `upscale(tile=, tile_overlap=)` allocates on the context of `device` for an h x w frame with `batch` windows a
        launch: the network's workspace of the windows, their float32 outputs, and the accumulator of the padded output."""
        return self._query_size("nesr_swin2sr_overlap_workspace_bytes", device, int(h), int(w), int(tile), int(tile_overlap), int(batch))

    def upscale(self, frame, device=None, tile=0, tile_pad=16, max_batch=None, tile_overlap=None):
        """[H, W, 3] uint8 RGB frame -> the uint8 frame [H s, W s, 3] on the device.  `frame` is a tensor on the device, or an
        ndarray, which is copied up once (to `device`, default the current ROCm device).

        tile = 0: the whole frame at once; the workspace grows with it.  tile = T > 0: the frame is cut into cores of T x T input
        pixels, each run inside a window of T + 2 tile_pad (see tile_plan), treated exactly as a frame of its own; windows share
        launches, `max_batch` at a time (None: as many as fit the library's workspace budget).  The result does not depend on
        max_batch; a frame no larger than T + 2 tile_pad is one window and gives the bits of tile = 0.

        tile_overlap = O (an integer; None, the default, is the route above) with tile = T > 0 selects the Swin2SR authors' tiling
        instead (see overlap_plan): the frame is padded once to the window, T x T windows step by T - O, the last one of an axis
        ends at the edge, every window's float output is added up and each pixel divided by the number of windows that covered
        it.  No window is padded; tile_pad has no meaning there and must be left alone."""
        if tile_overlap is not None and (int(tile) == 0 or tile_pad != 16):
            raise ValueError(f"Swin2SR.upscale: tile_overlap={tile_overlap!r} selects the overlapped route, which needs tile > 0 and takes no "
                             f"tile_pad (got tile={tile!r}, tile_pad={tile_pad!r}); leave tile_overlap=None for cores with a tile_pad of context")
        if isinstance(frame, np.ndarray):
            frame = torch.from_numpy(np.ascontiguousarray(frame)).to(torch.device("cuda") if device is None else torch.device(device))
        frame = self._frame_u8(frame, "upscale", "frame")
        h, w = frame.shape[:2]
        tile = int(tile)
        with torch.cuda.device(frame.device):
            handle = self._context(frame.device)
            if tile_overlap is not None:
                s = int(self.config["upscale"])
                out = torch.empty((h * s, w * s, 3), dtype=torch.uint8, device=frame.device)
                _invoke("nesr_swin2sr_upscale_overlapped_u8", frame.device, handle,
                        (frame, h, w, tile, int(tile_overlap), 0 if max_batch is None else int(max_batch), out, out.numel()))
            elif tile == 0:
                out = torch.empty(self.output_size(h, w) + (3,), dtype=torch.uint8, device=frame.device)
                _invoke("nesr_swin2sr_upscale_u8", frame.device, handle, (frame, h, w, out, out.numel()))
            else:
                s = int(self.config["upscale"])
                out = torch.empty((h * s, w * s, 3), dtype=torch.uint8, device=frame.device)
                _invoke("nesr_swin2sr_upscale_tiled_u8", frame.device, handle,
                        (frame, h, w, tile, int(tile_pad), 0 if max_batch is None else int(max_batch), out, out.numel()))
        self.calls += 1
        return out
