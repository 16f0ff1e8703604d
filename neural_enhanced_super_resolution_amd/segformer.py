"""``SegFormer``: the pipeline's segmenter, ``nvidia/segformer-b0-finetuned-ade-512-512`` of the reference's default
configuration (``segment_enhancement`` True, nesr/nesr.py:40; loaded at :285-301, run on every iteration at :691-724), as HIP
kernels behind the C ABI (csrc/segformer.hip, csrc/segformer_pre.hip, csrc/segformer_api.cpp).

The module owns ordinary torch Parameters and buffers under ``transformers``-5's names
(``segformer.stages.{i}.blocks.{j}.attention.q_proj.weight`` ...), takes a state dict of either key generation (the published
checkpoint carries the transformers-4 names) and has no torch implementation of its forward: ``forward(pixel_values)`` gives the
logits [1, num_labels, oh, ow] at the first stage's token grid (H/4 x W/4 at B0; ``output_size(H, W)``) and ``segment(frame)``
the class map of an [H, W, 3] uint8 RGB frame, both on the ROCm device; a tensor anywhere else raises.  ``segment`` restates the reference's pre-processing (a PIL LANCZOS resize when the longer side
exceeds 1024, the extractor's PIL BILINEAR resize to 512 x 512, its normalisation) and takes the argmax at the logits' own size,
as the reference does (nesr/nesr.py:716); the logits never reach memory there.  Calling the object with a uint8 HWC frame is
``segment``, so it goes straight into ``enhance_iterations(segmenter=...)``.
"""
from __future__ import annotations

import ctypes
import os
import re
from collections import OrderedDict

import torch
from torch import nn

from . import _lib

PIL_LANCZOS, PIL_BILINEAR = 1, 2      # PIL.Image's filter numbers: the `filter` of nesr_pil_resize_u8
MODEL_SIZE = 512                      # the side of the image the extractor makes of a frame (segment, pixel_values)

B0 = dict(num_channels=3, num_encoder_blocks=4, depths=(2, 2, 2, 2), sr_ratios=(8, 4, 2, 1), hidden_sizes=(32, 64, 160, 256),
          patch_sizes=(7, 3, 3, 3), strides=(4, 2, 2, 2), num_attention_heads=(1, 2, 5, 8), mlp_ratios=(4, 4, 4, 4),
          decoder_hidden_size=256, num_labels=150)


def _config(cfg):
    unknown = sorted(set(cfg) - set(B0))
    if unknown:
        raise TypeError(f"SegFormer: unknown configuration field(s) {unknown}; expected some of {sorted(B0)}")
    c = dict(B0)
    c.update(cfg)
    n = int(c["num_encoder_blocks"])
    for name in ("depths", "sr_ratios", "hidden_sizes", "patch_sizes", "strides", "num_attention_heads", "mlp_ratios"):
        c[name] = tuple(int(v) for v in c[name])
        if len(c[name]) != n:
            raise ValueError(f"SegFormer: {name} must have num_encoder_blocks = {n} entries, got {c[name]}")
    return c


def segformer_state_dict_spec(**cfg):
    """Ordered {key: shape} of a SegformerForSemanticSegmentation checkpoint under transformers-5's names (B0 with 150 labels:
    208 tensors, 3,752,694 parameters).  Keyword arguments are SegformerConfig's fields; the defaults are B0's."""
    c = _config(cfg)
    spec = OrderedDict()

    def wb(name, wshape):
        spec[name + ".weight"] = tuple(wshape)
        spec[name + ".bias"] = (wshape[0],)

    cin = c["num_channels"]
    for i in range(c["num_encoder_blocks"]):
        s = f"segformer.stages.{i}"
        ch, k, sr = c["hidden_sizes"][i], c["patch_sizes"][i], c["sr_ratios"][i]
        hid = ch * c["mlp_ratios"][i]
        wb(s + ".patch_embeddings.proj", (ch, cin, k, k))
        wb(s + ".patch_embeddings.layer_norm", (ch,))
        for j in range(c["depths"][i]):
            b = f"{s}.blocks.{j}"
            wb(b + ".layernorm_before", (ch,))
            for proj in ("q_proj", "k_proj", "v_proj", "o_proj"):
                wb(f"{b}.attention.{proj}", (ch, ch))
            if sr > 1:
                wb(b + ".attention.sequence_reduction.sequence_reduction", (ch, ch, sr, sr))
                wb(b + ".attention.sequence_reduction.layer_norm", (ch,))
            wb(b + ".layernorm_after", (ch,))
            wb(b + ".mlp.fc1", (hid, ch))
            wb(b + ".mlp.dwconv.dwconv", (hid, 1, 3, 3))
            wb(b + ".mlp.fc2", (ch, hid))
        wb(s + ".layer_norm", (ch,))
        cin = ch
    d = c["decoder_hidden_size"]
    for i in range(c["num_encoder_blocks"]):
        wb(f"decode_head.linear_projections.{i}.proj", (d, c["hidden_sizes"][i]))
    spec["decode_head.linear_fuse.weight"] = (d, d * c["num_encoder_blocks"], 1, 1)
    wb("decode_head.batch_norm", (d,))
    spec["decode_head.batch_norm.running_mean"] = (d,)
    spec["decode_head.batch_norm.running_var"] = (d,)
    spec["decode_head.batch_norm.num_batches_tracked"] = ()
    wb("decode_head.classifier", (c["num_labels"], d, 1, 1))
    return spec


# transformers-4 checkpoint names -> transformers-5 names (transformers/conversion_mapping.py, "SegformerModel" and
# "SegformerForSemanticSegmentation")
_OLD_TO_NEW = [
    (re.compile(r"encoder\.patch_embeddings\.(\d+)\."), r"stages.\1.patch_embeddings."),
    (re.compile(r"encoder\.block\.(\d+)\."), r"stages.\1.blocks."),
    (re.compile(r"encoder\.layer_norm\.(\d+)\."), r"stages.\1.layer_norm."),
    (re.compile(r"attention\.self\.query\."), "attention.q_proj."),
    (re.compile(r"attention\.self\.key\."), "attention.k_proj."),
    (re.compile(r"attention\.self\.value\."), "attention.v_proj."),
    (re.compile(r"attention\.self\.sr\."), "attention.sequence_reduction.sequence_reduction."),
    (re.compile(r"attention\.self\.layer_norm\."), "attention.sequence_reduction.layer_norm."),
    (re.compile(r"attention\.output\.dense\."), "attention.o_proj."),
    (re.compile(r"mlp\.dense1\."), "mlp.fc1."),
    (re.compile(r"mlp\.dense2\."), "mlp.fc2."),
    (re.compile(r"\.layer_norm_1\."), ".layernorm_before."),
    (re.compile(r"\.layer_norm_2\."), ".layernorm_after."),
    (re.compile(r"decode_head\.linear_c\."), "decode_head.linear_projections."),
]


def new_key(key):
    """The transformers-5 name of a checkpoint key of either generation (a new name comes back as it is)."""
    for pat, rep in _OLD_TO_NEW:
        key = pat.sub(rep, key)
    return key


class _Holder(nn.Module):
    """One level of the parameter tree.  Not callable."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("SegFormer's sub-modules hold weights only; SegFormer.forward runs in libnesr_hip.so")


class SegFormer(nn.Module):
    """SegformerForSemanticSegmentation in eval mode on the HIP path.  Keyword arguments are SegformerConfig's fields
    (num_channels, num_encoder_blocks, depths, sr_ratios, hidden_sizes, patch_sizes, strides, num_attention_heads, mlp_ratios,
    decoder_hidden_size, num_labels) with B0's values and 150 labels as defaults.  The kernels need a head dimension of 32 in
    every stage (B0; B1-B5 have 64), hidden sizes that are multiples of 32 and at most 256, N = 1 and H, W multiples of 32:
    anything else raises when the context is created or at the forward."""

    def __init__(self, **cfg):
        super().__init__()
        self.config = _config(cfg)
        for key, shape in segformer_state_dict_spec(**self.config).items():
            *path, leaf = key.split(".")
            mod = self
            for name in path:
                if name not in mod._modules:
                    mod.add_module(name, _Holder())
                mod = mod._modules[name]
            if leaf == "num_batches_tracked":
                mod.register_buffer(leaf, torch.tensor(0, dtype=torch.int64))
            elif leaf in ("running_mean", "running_var"):
                mod.register_buffer(leaf, torch.zeros(shape) if leaf == "running_mean" else torch.ones(shape))
            else:
                init = torch.ones(shape) if (leaf == "weight" and len(shape) == 1) else torch.zeros(shape)
                mod.register_parameter(leaf, nn.Parameter(init, requires_grad=False))
        self.calls = 0            # forwards so far (a caller can assert that the network really ran)
        self._handles = {}        # device index -> context with the current weights
        self._timing = False
        self.eval()

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict=True, **kw):
        """Takes transformers-5 names or the published checkpoint's transformers-4 names.  Strict: a missing or an unexpected
        key raises; batch_norm.num_batches_tracked may be left out (it is not used)."""
        sd = OrderedDict()
        for k, v in state_dict.items():
            nk = new_key(k)
            if nk in sd:
                raise RuntimeError(f"SegFormer.load_state_dict: {k!r} names the same tensor as another key ({nk!r})")
            sd[nk] = v
        sd.setdefault("decode_head.batch_norm.num_batches_tracked", torch.tensor(0, dtype=torch.int64))
        out = super().load_state_dict(sd, strict=strict, **kw)
        self._release()
        return out

    @classmethod
    def from_checkpoint(cls, path, **cfg):
        """A model with the weights of a local ``model.safetensors`` or ``pytorch_model.bin`` (or of the directory that holds
        one).  Anything that is not an existing local path raises: nothing is ever fetched (the reference's
        from_pretrained(hub id), nesr/nesr.py:291-296, is a network download)."""
        path = os.fspath(path)
        if os.path.isdir(path):
            for name in ("model.safetensors", "pytorch_model.bin"):
                if os.path.isfile(os.path.join(path, name)):
                    path = os.path.join(path, name)
                    break
        if not os.path.isfile(path):
            raise FileNotFoundError(f"SegFormer.from_checkpoint: {path!r} is not a local checkpoint file (a hub id is not fetched: "
                                    "pass the path of a downloaded model.safetensors or pytorch_model.bin)")
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path, device="cpu")
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        model = cls(**cfg)
        model.load_state_dict(sd)
        return model

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._release()
        return out

    def train(self, mode=True):
        if mode:
            raise RuntimeError("SegFormer is inference only (eval mode: BatchNorm with its running statistics, no dropout)")
        return super().train(False)

    # ------------------------------------------------------------------ contexts
    def _release(self):
        handles, self._handles = getattr(self, "_handles", {}), {}
        for h in handles.values():
            _lib.load().nesr_segformer_destroy(h)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _context(self, device):
        index = device.index if device.index is not None else torch.cuda.current_device()
        if index in self._handles:
            return self._handles[index]
        lib = _lib.load()
        c = self.config
        n = c["num_encoder_blocks"]

        def arr(name):
            return (ctypes.c_int * n)(*c[name])

        handle = ctypes.c_void_p()
        _lib.check(lib.nesr_segformer_create(ctypes.byref(handle), index, c["num_channels"], n, arr("depths"), arr("sr_ratios"),
                                             arr("hidden_sizes"), arr("patch_sizes"), arr("strides"), arr("num_attention_heads"),
                                             arr("mlp_ratios"), c["decoder_hidden_size"], c["num_labels"]), "nesr_segformer_create")
        try:
            for key, t in self.state_dict().items():
                if key.endswith("num_batches_tracked"):
                    continue
                t = t.detach().to("cpu", torch.float32).contiguous()
                shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
                _lib.check(lib.nesr_segformer_load_weight(handle, key.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()),
                           "nesr_segformer_load_weight")
            _lib.check(lib.nesr_segformer_finalize(handle), "nesr_segformer_finalize")
            _lib.check(lib.nesr_segformer_set_timing(handle, 1 if self._timing else 0), "nesr_segformer_set_timing")
        except Exception:
            lib.nesr_segformer_destroy(handle)
            raise
        self._handles[index] = handle
        return handle

    @staticmethod
    def _require_device(t, what):
        if not t.is_cuda:
            raise RuntimeError(f"SegFormer.{what}: the tensor is on {t.device}; the forward runs on the ROCm device only "
                               "(there is no CPU or PyTorch fallback)")

    # ------------------------------------------------------------------ forward
    def output_size(self, h, w):
        """(oh, ow) of the logits of an h x w input: the first stage's token grid, as the library computes it
        (nesr_segformer_output_size; H/4 x W/4 at B0).  Needs no device."""
        c = self.config
        n = c["num_encoder_blocks"]
        oh, ow = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().nesr_segformer_output_size(n, (ctypes.c_int * n)(*c["patch_sizes"]), (ctypes.c_int * n)(*c["strides"]), int(h), int(w),
                                                          ctypes.byref(oh), ctypes.byref(ow)), "nesr_segformer_output_size")
        return oh.value, ow.value

    def forward(self, pixel_values):
        """pixel_values [1, 3, H, W] float32 on the device (H, W multiples of 32) -> logits [1, num_labels, oh, ow],
        (oh, ow) = output_size(H, W)."""
        if pixel_values.dtype == torch.uint8 and pixel_values.dim() == 3:
            return self.segment(pixel_values)
        x = pixel_values
        self._require_device(x, "forward")
        if x.dim() != 4 or x.dtype != torch.float32:
            raise ValueError(f"SegFormer.forward: a [1, {self.config['num_channels']}, H, W] float32 tensor, got {x.dtype} {tuple(x.shape)}")
        x = x.contiguous()
        n, ch, h, w = x.shape
        with torch.cuda.device(x.device):
            handle = self._context(x.device)
            out = torch.empty((1, self.config["num_labels"]) + self.output_size(h, w), dtype=torch.float32, device=x.device)
            stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
            _lib.check(_lib.load().nesr_segformer_forward_f32(handle, ctypes.c_void_p(x.data_ptr()), n, ch, h, w,
                                                              ctypes.c_void_p(out.data_ptr()), stream), "nesr_segformer_forward_f32")
        self.calls += 1
        return out

    def segment(self, frame):
        """[H, W, 3] uint8 RGB tensor on the device -> the class map, uint8 [oh, ow] = output_size(512, 512) on the device
        (128 x 128 at B0; the argmax of the logits of the 512 x 512 image the reference's extractor makes of the frame; ties
        take the lowest class)."""
        self._require_device(frame, "segment")
        if frame.dim() != 3 or frame.shape[2] != 3 or frame.dtype != torch.uint8 or frame.numel() == 0:
            raise ValueError(f"SegFormer.segment: an [H, W, 3] uint8 tensor, got {frame.dtype} {tuple(frame.shape)}")
        frame = frame.contiguous()
        h, w = frame.shape[:2]
        with torch.cuda.device(frame.device):
            handle = self._context(frame.device)
            out = torch.empty(self.output_size(MODEL_SIZE, MODEL_SIZE), dtype=torch.uint8, device=frame.device)
            oh, ow = ctypes.c_int(0), ctypes.c_int(0)
            stream = ctypes.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)
            _lib.check(_lib.load().nesr_segformer_segment_u8(handle, ctypes.c_void_p(frame.data_ptr()), h, w, ctypes.c_void_p(out.data_ptr()),
                                                             out.numel(), ctypes.byref(oh), ctypes.byref(ow), stream), "nesr_segformer_segment_u8")
        self.calls += 1
        if (oh.value, ow.value) != tuple(out.shape):
            raise _lib.NesrHipError(f"nesr_segformer_segment_u8 reported a {oh.value} x {ow.value} map")
        return out

    def pixel_values(self, frame):
        """The network input `segment` makes of an [H, W, 3] uint8 RGB frame: [1, 3, 512, 512] float32 on the device."""
        self._require_device(frame, "pixel_values")
        if frame.dim() != 3 or frame.shape[2] != 3 or frame.dtype != torch.uint8 or frame.numel() == 0:
            raise ValueError(f"SegFormer.pixel_values: an [H, W, 3] uint8 tensor, got {frame.dtype} {tuple(frame.shape)}")
        frame = frame.contiguous()
        with torch.cuda.device(frame.device):
            handle = self._context(frame.device)
            out = torch.empty((1, 3, MODEL_SIZE, MODEL_SIZE), dtype=torch.float32, device=frame.device)
            stream = ctypes.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)
            _lib.check(_lib.load().nesr_segformer_preprocess_u8(handle, ctypes.c_void_p(frame.data_ptr()), frame.shape[0], frame.shape[1],
                                                                ctypes.c_void_p(out.data_ptr()), stream), "nesr_segformer_preprocess_u8")
        return out

    # ------------------------------------------------------------------ timing
    def set_kernel_timing(self, enable=True):
        """Switches the launch counter and the per-group event timing of every context (kernel_time_ms reads them)."""
        self._timing = bool(enable)
        for h in self._handles.values():
            _lib.check(_lib.load().nesr_segformer_set_timing(h, 1 if enable else 0), "nesr_segformer_set_timing")

    def kernel_time_ms(self, device=None):
        """{"launches": kernel launches, "groups": {name: ms}} since the last call, summed over the forwards in between."""
        handles = list(self._handles.items())
        if device is not None:
            handles = [(i, h) for i, h in handles if i == torch.device(device).index]
        launches, groups = 0, OrderedDict()
        for index, h in handles:
            ms = (ctypes.c_double * len(KERNEL_GROUPS))()
            n = ctypes.c_int64(0)
            with torch.cuda.device(index):
                _lib.check(_lib.load().nesr_segformer_kernel_time_ms(h, ms, len(KERNEL_GROUPS), ctypes.byref(n)), "nesr_segformer_kernel_time_ms")
            launches += n.value
            for name, v in zip(KERNEL_GROUPS, ms):
                groups[name] = groups.get(name, 0.0) + v
        return {"launches": launches, "groups": groups}


KERNEL_GROUPS = ("preprocess", "patch_embed", "ln_proj", "seq_reduction", "attention", "mix_ffn", "decode_head")   # NESR_SEG_GROUP_*


def pil_resize_u8(img, oh, ow, filter=PIL_BILINEAR):
    """PIL's Image.resize((ow, oh), filter) of an [h, w, c] uint8 tensor on the device (filter: PIL_BILINEAR or PIL_LANCZOS),
    bit for bit: nesr_pil_resize_u8."""
    if img.dim() != 3 or img.dtype != torch.uint8 or not img.is_cuda or img.numel() == 0:
        raise ValueError(f"pil_resize_u8: an [h, w, c] uint8 tensor on the ROCm device, got {img.dtype} {tuple(img.shape)} on {img.device}")
    img = img.contiguous()
    h, w, c = img.shape
    out = torch.empty((oh, ow, c), dtype=torch.uint8, device=img.device)
    index = img.device.index if img.device.index is not None else torch.cuda.current_device()
    with torch.cuda.device(img.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(img.device).cuda_stream)
        _lib.check(_lib.load().nesr_pil_resize_u8(index, ctypes.c_void_p(img.data_ptr()), h, w, c, ctypes.c_void_p(out.data_ptr()), oh, ow,
                                                  int(filter), stream), "nesr_pil_resize_u8")
    return out
