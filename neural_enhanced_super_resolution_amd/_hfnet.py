"""``_HFNet``: what ``SegFormer``, ``Swin2SR``, ``VaeDecoder``, ``UNet2DCondition`` and ``ClipTextEncoder`` share, the models that
take a ``transformers`` or ``diffusers`` checkpoint and run as a chain of launches behind their own entries of the C ABI
(``nesr_segformer_*``, ``nesr_swin2sr_*``, ``nesr_vae_*``, ``nesr_unet_*``, ``nesr_clip_text_*``; their C side shares
csrc/net_context.h in the same way).

The base owns the parameter tree built from the subclass's spec, the checkpoint reader, one context per device with the current
weights (strictly loaded: the library refuses a key or a shape it does not expect), the argument checks of the forwards, the size
queries and the per-group kernel timing.  A subclass declares ``PREFIX`` (its entries' prefix), ``NAME`` (in messages),
``KERNEL_GROUPS``, ``TRAIN_ERROR`` and ``_spec`` (its state-dict spec function) and gives ``_create(index)``, usually through
``_create_handle``; it may declare ``DEFAULTS`` (then ``from_checkpoint`` reads a ``config.json`` beside the weights) and override
``_register_leaf`` (how a leaf of the spec becomes a Parameter or a buffer) and ``_skip_upload`` (keys of the state dict the
library does not take).  Calls go through ``_contexts._invoke``: tensors as pointers, torch's current stream appended.
"""
from __future__ import annotations

import ctypes
import json
import os
from collections import OrderedDict

import torch
from torch import nn

from . import _lib
from ._contexts import _invoke


class _Holder(nn.Module):
    """One level of the parameter tree.  Not callable."""

    def __init__(self, owner):
        super().__init__()
        self._owner = owner

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(f"{self._owner}'s sub-modules hold weights only; {self._owner}.forward runs in libnesr_hip.so")


def _merged_config(name, defaults, cfg):
    """`defaults` overridden by `cfg`; a field that is not one of the defaults' is a TypeError.  The model's own normalisation follows."""
    unknown = sorted(set(cfg) - set(defaults))
    if unknown:
        raise TypeError(f"{name}: unknown configuration field(s) {unknown}; expected some of {sorted(defaults)}")
    return dict(defaults, **cfg)


class _HFNet(nn.Module):
    PREFIX = NAME = TRAIN_ERROR = _spec = None
    DEFAULTS = None           # the configuration's fields with their defaults, where a config.json beside the weights supplies them
    KERNEL_GROUPS = ()
    CHECKPOINT_FILES = ("model.safetensors", "pytorch_model.bin")      # what from_checkpoint looks for in a directory

    def __init__(self, config):
        super().__init__()
        self.config = config
        for key, shape in self._spec(**config).items():
            *path, leaf = key.split(".")
            mod = self
            for name in path:
                if name not in mod._modules:
                    mod.add_module(name, _Holder(self.NAME))
                mod = mod._modules[name]
            self._register_leaf(mod, leaf, shape)
        self.calls = 0            # forwards so far (a caller can assert that the network really ran)
        self._handles = {}        # device index -> context with the current weights
        self._timing = False
        self.eval()

    def _register_leaf(self, mod, leaf, shape, init=None):
        if init is None:
            init = torch.ones(shape) if (leaf == "weight" and len(shape) == 1) else torch.zeros(shape)
        mod.register_parameter(leaf, nn.Parameter(init, requires_grad=False))

    def _skip_upload(self, key):
        return False

    def _create(self, index):
        """A context of this configuration on device `index`, without weights."""
        raise NotImplementedError

    @staticmethod
    def _create_handle(entry, *args):
        """The handle `entry`(&handle, *args) makes; NesrUnsupportedError names the field the kernels do not take."""
        lib = _lib.load()
        handle = ctypes.c_void_p()
        rc = getattr(lib, entry)(ctypes.byref(handle), *args)
        if rc == _lib.ERR_UNSUPPORTED:
            msg = lib.nesr_last_error()
            raise _lib.NesrUnsupportedError(f"{entry} failed ({rc}): {msg.decode() if msg else '?'}")
        _lib.check(rc, entry)
        return handle

    @classmethod
    def _entry(cls, name):
        return f"{cls.PREFIX}_{name}"

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._release()
        return out

    @classmethod
    def from_checkpoint(cls, path, **cfg):
        """A model with the weights of a local ``model.safetensors`` or ``pytorch_model.bin`` (or of the directory that holds
        one; a subclass names its files in CHECKPOINT_FILES).  Where the subclass declares DEFAULTS, a ``config.json`` beside the
        weights supplies the configuration's fields; arguments override it.  Anything that is not an existing local path raises:
        nothing is ever fetched (the reference's from_pretrained(hub id), nesr/nesr.py:291-296, is a network download)."""
        path = os.fspath(path)
        config = os.path.join(path if os.path.isdir(path) else os.path.dirname(path), "config.json")
        if cls.DEFAULTS is not None and os.path.isfile(config):
            with open(config) as f:
                found = json.load(f)
            cfg = dict({k: found[k] for k in cls.DEFAULTS if found.get(k) is not None}, **cfg)
        if os.path.isdir(path):
            for name in cls.CHECKPOINT_FILES:
                if os.path.isfile(os.path.join(path, name)):
                    path = os.path.join(path, name)
                    break
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{cls.NAME}.from_checkpoint: {path!r} is not a local checkpoint file (a hub id is not fetched: "
                                    "pass the path of a downloaded " + " or ".join(cls.CHECKPOINT_FILES) + ")")
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
            raise RuntimeError(self.TRAIN_ERROR)
        return super().train(False)

    # ------------------------------------------------------------------ contexts
    def _release(self):
        handles, self._handles = getattr(self, "_handles", {}), {}
        for h in handles.values():
            getattr(_lib.load(), self._entry("destroy"))(h)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _context(self, device):
        """The handle of `device`'s context, created and given the module's weights if need be."""
        index = device.index if device.index is not None else torch.cuda.current_device()
        if index in self._handles:
            return self._handles[index]
        handle = self._create(index)
        try:
            for key, t in self.state_dict().items():
                if self._skip_upload(key):
                    continue
                t = t.detach().to("cpu", torch.float32).contiguous()
                shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
                _invoke(self._entry("load_weight"), None, handle, (key.encode(), t, shape, t.dim()))
            _invoke(self._entry("finalize"), None, handle, ())
            _invoke(self._entry("set_timing"), None, handle, (1 if self._timing else 0,))
        except Exception:
            getattr(_lib.load(), self._entry("destroy"))(handle)
            raise
        self._handles[index] = handle
        return handle

    def _query_size(self, entry, device, *args):
        """The size_t that `entry`(context of `device`, *args, &size) reports: a workspace's or the weights' bytes."""
        device = torch.device("cuda" if device is None else device)
        size = ctypes.c_size_t(0)
        with torch.cuda.device(device):
            _invoke(entry, None, self._context(device), (*args, ctypes.byref(size)))
        return size.value

    # ------------------------------------------------------------------ the forwards' arguments
    def _require_device(self, t, what):
        if not t.is_cuda:
            raise RuntimeError(f"{self.NAME}.{what}: the tensor is on {t.device}; the forward runs on the ROCm device only "
                               "(there is no CPU or PyTorch fallback)")

    def _pixel_values(self, x):
        """The checked, contiguous [1, C, H, W] float32 input of `forward`."""
        self._require_device(x, "forward")
        if x.dim() != 4 or x.dtype != torch.float32:
            raise ValueError(f"{self.NAME}.forward: a [1, {self.config['num_channels']}, H, W] float32 tensor, got {x.dtype} {tuple(x.shape)}")
        return x.contiguous()

    def _frame_u8(self, frame, what, noun="tensor"):
        """The checked, contiguous [H, W, 3] uint8 frame of method `what`."""
        self._require_device(frame, what)
        if frame.dim() != 3 or frame.shape[2] != 3 or frame.dtype != torch.uint8 or frame.numel() == 0:
            raise ValueError(f"{self.NAME}.{what}: an [H, W, 3] uint8 {noun}, got {frame.dtype} {tuple(frame.shape)}")
        return frame.contiguous()

    # ------------------------------------------------------------------ timing
    def set_kernel_timing(self, enable=True):
        """Switches the per-group event timing of every context (kernel_time_ms reads it; the launch counter always runs)."""
        self._timing = bool(enable)
        for h in self._handles.values():
            _invoke(self._entry("set_timing"), None, h, (1 if enable else 0,))

    def kernel_time_ms(self, device=None):
        """{"launches": kernel launches, "groups": {name: ms}} since the last call, summed over the forwards in between; every
        group of KERNEL_GROUPS is there, at 0.0 where nothing ran."""
        handles = list(self._handles.items())
        if device is not None:
            handles = [(i, h) for i, h in handles if i == torch.device(device).index]
        launches, groups = 0, OrderedDict((name, 0.0) for name in self.KERNEL_GROUPS)
        for index, h in handles:
            ms = (ctypes.c_double * len(groups))()
            n = ctypes.c_int64(0)
            with torch.cuda.device(index):
                _invoke(self._entry("kernel_time_ms"), None, h, (ms, len(groups), ctypes.byref(n)))
            launches += n.value
            for name, v in zip(groups, ms):
                groups[name] += v
        return {"launches": launches, "groups": groups}
