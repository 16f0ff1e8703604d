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
import re
from collections import OrderedDict

import torch

from . import _lib
from ._contexts import _invoke, current_stream_ptr, device_call
from ._hfnet import _HFNet, _merged_config

PIL_LANCZOS, PIL_BILINEAR = 1, 2      # PIL.Image's filter numbers: the `filter` of nesr_pil_resize_u8
MODEL_SIZE = 512                      # the side of the image the extractor makes of a frame (segment, pixel_values)

B0 = dict(num_channels=3, num_encoder_blocks=4, depths=(2, 2, 2, 2), sr_ratios=(8, 4, 2, 1), hidden_sizes=(32, 64, 160, 256),
          patch_sizes=(7, 3, 3, 3), strides=(4, 2, 2, 2), num_attention_heads=(1, 2, 5, 8), mlp_ratios=(4, 4, 4, 4),
          decoder_hidden_size=256, num_labels=150)


def _config(cfg):
    c = _merged_config("SegFormer", B0, cfg)
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


KERNEL_GROUPS = ("preprocess", "patch_embed", "ln_proj", "seq_reduction", "attention", "mix_ffn", "decode_head")   # NESR_SEG_GROUP_*


class SegFormer(_HFNet):
    """SegformerForSemanticSegmentation in eval mode on the HIP path.  Keyword arguments are SegformerConfig's fields
    (num_channels, num_encoder_blocks, depths, sr_ratios, hidden_sizes, patch_sizes, strides, num_attention_heads, mlp_ratios,
    decoder_hidden_size, num_labels) with B0's values and 150 labels as defaults.  The kernels need a head dimension of 32 in
    every stage (B0; B1-B5 have 64), hidden sizes that are multiples of 32 and at most 256, N = 1 and H, W multiples of 32:
    anything else raises when the context is created or at the forward."""

    PREFIX, NAME, KERNEL_GROUPS = "nesr_segformer", "SegFormer", KERNEL_GROUPS
    TRAIN_ERROR = "SegFormer is inference only (eval mode: BatchNorm with its running statistics, no dropout)"
    _spec = staticmethod(segformer_state_dict_spec)

    def __init__(self, **cfg):
        super().__init__(_config(cfg))

    def _register_leaf(self, mod, leaf, shape, init=None):
        if leaf == "num_batches_tracked":
            mod.register_buffer(leaf, torch.tensor(0, dtype=torch.int64))
        elif leaf in ("running_mean", "running_var"):
            mod.register_buffer(leaf, torch.zeros(shape) if leaf == "running_mean" else torch.ones(shape))
        else:
            super()._register_leaf(mod, leaf, shape, init)

    def _skip_upload(self, key):
        return key.endswith("num_batches_tracked")

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
        return super().load_state_dict(sd, strict=strict, **kw)

    def _create(self, index):
        c = self.config
        n = c["num_encoder_blocks"]

        def arr(name):
            return (ctypes.c_int * n)(*c[name])

        return self._create_handle("nesr_segformer_create", index, c["num_channels"], n, arr("depths"), arr("sr_ratios"), arr("hidden_sizes"),
                                   arr("patch_sizes"), arr("strides"), arr("num_attention_heads"), arr("mlp_ratios"), c["decoder_hidden_size"],
                                   c["num_labels"])

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
        x = self._pixel_values(pixel_values)
        n, ch, h, w = x.shape
        with torch.cuda.device(x.device):
            handle = self._context(x.device)
            out = torch.empty((1, self.config["num_labels"]) + self.output_size(h, w), dtype=torch.float32, device=x.device)
            _invoke("nesr_segformer_forward_f32", x.device, handle, (x, n, ch, h, w, out))
        self.calls += 1
        return out

    def segment(self, frame):
        """[H, W, 3] uint8 RGB tensor on the device -> the class map, uint8 [oh, ow] = output_size(512, 512) on the device
        (128 x 128 at B0; the argmax of the logits of the 512 x 512 image the reference's extractor makes of the frame; ties
        take the lowest class)."""
        frame = self._frame_u8(frame, "segment")
        h, w = frame.shape[:2]
        with torch.cuda.device(frame.device):
            handle = self._context(frame.device)
            out = torch.empty(self.output_size(MODEL_SIZE, MODEL_SIZE), dtype=torch.uint8, device=frame.device)
            oh, ow = ctypes.c_int(0), ctypes.c_int(0)
            _lib.check(_lib.load().nesr_segformer_segment_u8(handle, ctypes.c_void_p(frame.data_ptr()), h, w, ctypes.c_void_p(out.data_ptr()),
                                                             out.numel(), ctypes.byref(oh), ctypes.byref(ow), current_stream_ptr(frame.device)),
                       "nesr_segformer_segment_u8")
        self.calls += 1
        if (oh.value, ow.value) != tuple(out.shape):
            raise _lib.NesrHipError(f"nesr_segformer_segment_u8 reported a {oh.value} x {ow.value} map")
        return out

    def pixel_values(self, frame):
        """The network input `segment` makes of an [H, W, 3] uint8 RGB frame: [1, 3, 512, 512] float32 on the device."""
        frame = self._frame_u8(frame, "pixel_values")
        with torch.cuda.device(frame.device):
            handle = self._context(frame.device)
            out = torch.empty((1, 3, MODEL_SIZE, MODEL_SIZE), dtype=torch.float32, device=frame.device)
            _invoke("nesr_segformer_preprocess_u8", frame.device, handle, (frame, frame.shape[0], frame.shape[1], out))
        return out


def pil_resize_u8(img, oh, ow, filter=PIL_BILINEAR):
    """PIL's Image.resize((ow, oh), filter) of an [h, w, c] uint8 tensor on the device (filter: PIL_BILINEAR or PIL_LANCZOS),
    bit for bit: nesr_pil_resize_u8."""
    if img.dim() != 3 or img.dtype != torch.uint8 or not img.is_cuda or img.numel() == 0:
        raise ValueError(f"pil_resize_u8: an [h, w, c] uint8 tensor on the ROCm device, got {img.dtype} {tuple(img.shape)} on {img.device}")
    img = img.contiguous()
    h, w, c = img.shape
    out = torch.empty((oh, ow, c), dtype=torch.uint8, device=img.device)
    device_call("nesr_pil_resize_u8", img.device, img, h, w, c, out, oh, ow, int(filter))
    return out
