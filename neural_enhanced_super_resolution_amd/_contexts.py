"""The contexts of one model in libnesr_hip.so, and the part of the two networks that reaches the library through them.

``ContextPool`` owns every context handle of a model: which (device, slot) has one, when weights are uploaded again, which
switches a new context starts with.  ``_HipNet`` is the ``nn.Module`` base of ``RRDBNet`` and ``SRVGGNetCompact``: the only
place that knows the pool, and the one way a model's method calls the C ABI (``_call``).  ``device_call`` is its sibling for
the entries that take a device index instead of a context.
"""
from __future__ import annotations

import ctypes
import weakref
from collections import OrderedDict

import torch
from torch import nn

from . import _lib


def _device_guard(index):
    return torch.cuda.device(index)


class ContextPool:
    """{(device index, slot): handle} of one model.

    Slot 0 of the first device asked for is the model's own context and that device its `home`; further slots are replicas
    (own packed weights and workspace) so independent forwards can run beside each other on different streams; a request on
    another device gets that device's own contexts and leaves the home's in place.  All live contexts share one dtype `code`:
    a request with another releases everything.  Changed weights (mark_dirty) are uploaded again into home slot 0, in place,
    at the next request; every other context is destroyed then and re-created when it is next asked for.  A context that the
    pool creates gets every switch in `settings` directly after its upload, so replicas, other devices and contexts re-created
    after a release all run as the model was told to.

    create(index, code) -> handle and upload(handle) are the model's; `lib` (default: the loaded library) is what the
    setters and nesr_destroy are called on."""

    def __init__(self, create, upload, lib=None):
        self._create, self._upload, self._lib = create, upload, lib
        self.contexts = OrderedDict()
        self.home = None          # device index of home slot 0
        self.code = None          # dtype code the live contexts were created with
        self.dirty = True         # parameters changed since the last upload
        self.settings = {}        # setter name -> int, replayed on every new context

    @property
    def lib(self):
        return self._lib if self._lib is not None else _lib.load()

    def _switch(self, name, handle, value):
        _lib.check(getattr(self.lib, name)(handle, value), name)

    def _new(self, index, code):
        handle = self._create(index, code)
        try:
            self._upload(handle)
            for name, value in self.settings.items():
                self._switch(name, handle, value)
        except Exception:
            self.lib.nesr_destroy(handle)     # refused weights: nothing half-made stays behind
            raise
        return handle

    def _settle(self, index, code):
        """Home slot 0 exists and holds the model's current weights; contexts with older ones are gone."""
        key = (index, 0)
        if key not in self.contexts:
            self.contexts[key] = self._new(index, code)
            self.home, self.code = index, code
        elif self.dirty:
            for k in [k for k in self.contexts if k != key]:
                self.lib.nesr_destroy(self.contexts.pop(k))
            self._upload(self.contexts[key])
        self.dirty = False

    def get(self, index, slot, code):
        """The handle of context (device `index`, `slot`), created and given the weights if need be."""
        if self.home is not None and code != self.code:
            self.release()
        if self.home is None or index == self.home:
            self._settle(index, code)
        else:
            with _device_guard(self.home):
                self._settle(self.home, code)
        key = (index, slot)
        if key not in self.contexts:
            self.contexts[key] = self._new(index, code)
            same = self.handles(index)
            if len(same) > 1:                 # they exist to run beside each other: tell every context of the device
                for h in same:
                    self._switch("nesr_set_concurrent", h, 1)
        return self.contexts[key]

    def handle(self, index, slot):
        return self.contexts.get((index, slot))

    def handles(self, device=None):
        """Home slot 0, the home's replicas, then the other devices' contexts, each in creation order (`device`: only its)."""
        if device is not None:
            return [h for k, h in self.contexts.items() if k[0] == device]
        items = self.contexts.items()
        return [h for k, h in items if k[0] == self.home] + [h for k, h in items if k[0] != self.home]

    def devices(self):
        """Device indices with a context, the home first."""
        return list(OrderedDict.fromkeys(k[0] for k in self.contexts))

    def set(self, name, value):
        """Switch `name` (a nesr_set_* entry taking one int) for every live context and every later one."""
        self.settings[name] = int(value)
        for h in self.handles():
            self._switch(name, h, int(value))

    def set_concurrent(self, on):
        """The kernel-selection hint `get` sets when contexts share a device; not kept for later contexts."""
        for h in self.handles():
            self._switch("nesr_set_concurrent", h, 1 if on else 0)

    def mark_dirty(self):
        self.dirty = True

    def release(self):
        while self.contexts:
            self.lib.nesr_destroy(self.contexts.popitem(last=False)[1])
        self.home = None
        self.dirty = True


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def current_stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _invoke(name, device, first, args):
    """libnesr_hip.so entry `name`(first, *args[, device's current stream]): tensors (None: a null pointer) go as pointers, the
    stream is appended where the signature has one parameter more than was given, a negative status raises.  The caller
    holds the device guard."""
    argv = [first] + [_ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    argtypes = _lib.SIGNATURES[name][1]
    if len(argv) == len(argtypes) - 1 and argtypes[-1] is ctypes.c_void_p:
        argv.append(current_stream_ptr(device))
    _lib.check(getattr(_lib.load(), name)(*argv), name)


def device_call(name, device, *args):
    """Entry `name`(device index, *args[, stream]) under the device's guard, on its current stream."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    with torch.cuda.device(device):
        _invoke(name, device, index, args)


class _HipNet(nn.Module):
    """What RRDBNet and SRVGGNetCompact share: contexts, upload, the forward calls both have, status and timing.
    A subclass gives its parameters, _dtype_code(), _create(index, code), out_scale() and, if it has one, _check_input(h, w)."""

    def __init__(self):
        super().__init__()
        self.calls = 0            # forward evaluations so far (callers assert on it: the reference's exception ladders
                                  # turn a dead backend into a silent bicubic resize, nesr/nesr.py:815-843)
        me = weakref.ref(self)    # (no cycle: the contexts go when the last reference to the model does)
        self._pool = ContextPool(lambda index, code: me()._create(index, code), lambda handle: me()._upload(handle))

    # ------------------------------------------------------------------ parameters changed
    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._pool.mark_dirty()
        return out

    def _to_bf16(self):
        """.half() / a 16-bit parameter dtype: upstream's fp16 switch selects the bf16 MFMA kernels here."""
        self.compute_dtype = "bf16"

    def half(self):
        """Upstream's fp16 switch (RealESRGANer(half=True) calls model.half()).  Here it selects the bf16 MFMA
        kernels; the parameters stay float32, so the bf16 weights are rounded once from the checkpoint's values
        (not float32 -> fp16 -> bf16)."""
        self._to_bf16()
        self._pool.mark_dirty()
        return self

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._pool.mark_dirty()
        if next(self.parameters()).dtype in (torch.float16, torch.bfloat16):
            self._to_bf16()
        return out

    # ------------------------------------------------------------------ HIP contexts
    def _release(self):
        self._pool.release()

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _upload(self, handle):
        lib = _lib.load()
        for key, t in self.state_dict().items():
            arr = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
            shape = (ctypes.c_int64 * arr.dim())(*arr.shape)
            _lib.check(lib.nesr_load_weight(handle, key.encode(), ctypes.c_void_p(arr.data_ptr()), shape, arr.dim()),
                       f"nesr_load_weight({key})")
        _lib.check(lib.nesr_finalize_weights(handle), "nesr_finalize_weights")

    def _context(self, device: torch.device, slot: int = 0):
        """Handle of the context of (device, `slot`), see ContextPool: slot 0 is the model's own, further slots are replicas
        for concurrent streams, and one model can run on several devices at once."""
        index = device.index if device.index is not None else torch.cuda.current_device()
        return self._pool.get(index, slot, self._dtype_code())

    def _handle(self, index, slot=0):
        """Handle of context (device `index`, `slot`), or None if it does not exist."""
        return self._pool.handle(index, slot)

    def _handles(self):
        """Every context of the model: home slot 0, the home's replicas, then the other devices' contexts."""
        return self._pool.handles()

    def _call(self, name, device, slot, *args):
        """libnesr_hip.so entry `name`(context of (device, slot), *args[, stream]) on the device's current stream."""
        device = torch.device(device)
        with torch.cuda.device(device):
            _invoke(name, device, self._context(device, slot), args)

    def reserve(self, device, n, h, w, slot=0):
        """Creates context (device, `slot`) if needed and grows its workspace for a batch of n images of h x w input now
        (nesr_reserve): a forward that has to grow it synchronises the device, which would serialise work enqueued on several."""
        self._call("nesr_reserve", device, slot, int(n), int(h), int(w))

    # ------------------------------------------------------------------ forward
    def _require_cuda(self, x):
        if x.device.type != "cuda":
            raise RuntimeError(
                f"{type(self).__name__}.forward runs only on an AMD GPU through libnesr_hip.so; got a tensor on "
                f"{x.device}. There is no CPU/PyTorch fallback for this path.")

    def _check_input(self, h, w):
        pass

    @torch.no_grad()
    def forward(self, x, slot: int = 0):
        """x: [N, num_in_ch, H, W] float on a ROCm device -> [N, num_out_ch, H*s, W*s].
        `slot` selects a context replica (see _context); work is enqueued on torch's current stream."""
        self._require_cuda(x)
        if x.dim() != 4:
            raise ValueError(f"expected NCHW input, got shape {tuple(x.shape)}")
        in_dtype = x.dtype
        xf = x.to(torch.float32).contiguous()
        n, c, h, w = xf.shape
        self._check_input(h, w)
        s = self.out_scale()
        self.calls += 1
        y = torch.empty((n, self.num_out_ch, h * s, w * s), dtype=torch.float32, device=xf.device)
        self._call("nesr_forward", xf.device, slot, xf, n, c, h, w, y)
        return y if in_dtype == torch.float32 else y.to(in_dtype)

    @torch.no_grad()
    def forward_u8(self, img_hwc_u8, flip_rgb=True, round_nearest=True, slot: int = 0):
        """Fused image path: u8 HWC [H,W,3] device tensor -> u8 HWC [H*s,W*s,3] (`slot`: context replica, see forward).

        flip_rgb/round_nearest = (True, True) reproduces RealESRGANer.enhance's /255, BGR<->RGB,
        clamp, x255, round; (False, False) reproduces nesr/nesr.py:851-857,894-898 (truncation)."""
        self._require_cuda(img_hwc_u8)
        if img_hwc_u8.dtype != torch.uint8 or img_hwc_u8.dim() != 3 or img_hwc_u8.shape[2] != 3:
            raise ValueError("expected a uint8 [H, W, 3] tensor")
        x = img_hwc_u8.contiguous()
        h, w, _ = x.shape
        s = self.out_scale()
        self.calls += 1
        y = torch.empty((h * s, w * s, 3), dtype=torch.uint8, device=x.device)
        self._call("nesr_forward_u8", x.device, slot, x, h, w, y, 1 if flip_rgb else 0,
                   _lib.ROUND_NEAREST if round_nearest else _lib.ROUND_TRUNC)
        return y

    # ------------------------------------------------------------------ status and measurement
    def set_kernel_timing(self, device, enable=True):
        self._context(torch.device(device))
        self._pool.set("nesr_set_kernel_timing", bool(enable))

    def set_concurrent(self, concurrent: bool):
        """Hint for kernel selection: forwards of this model's contexts run beside each other on several streams
        (set automatically when a context replica is created; clear it to time one forward alone)."""
        self._pool.set_concurrent(concurrent)

    def check_status(self):
        """Synchronises every device the model has a context on and raises if asynchronous work of this model failed."""
        for index in self._pool.devices():
            _lib.check(_lib.load().nesr_check_status(self._pool.handles(index)[0]), "nesr_check_status")
        self.check_range()

    def check_range(self, slot=None, device=None):
        """Raises NesrRangeError if a forward enqueued so far (on torch's current stream) met an input or activation
        the f16-pair fp32 form or the f16 form cannot carry (non-finite or beyond +-65504): its float output is NaN and an 8-bit
        output is invalid.  Waits for the current stream only; a no-op for the other compute dtypes.  The wrappers
        call it after every device-to-host copy (the reference would have returned NaN pixels, nesr/nesr.py:891-898).
        Covers every context of every device, the home device's `slot`, or with `device` that device's contexts (all, or
        `slot`).  Every covered context is checked and cleared before the first failure is raised (a range error before a
        persistent launch that gave up), so the next forward starts clean on all of them."""
        pool = self._pool
        if pool.home is None or pool.code not in (_lib.DTYPE_F32_SPLIT, _lib.DTYPE_BF16, _lib.DTYPE_F16):
            return                        # only these forms have a range word or persistent launches
        if device is not None:
            indices = [torch.device(device).index]
        else:
            indices = pool.devices() if slot is None else [pool.home]
        first = None
        for index in indices:
            dev = torch.device("cuda", index)
            for h in pool.handles(index) if slot is None else [pool.handle(index, slot)]:
                if h is None:
                    continue
                with torch.cuda.device(dev):
                    try:
                        _invoke("nesr_check_range", dev, h, ())
                    except _lib.NesrHipError as e:
                        if first is None or (isinstance(e, _lib.NesrRangeError) and not isinstance(first, _lib.NesrRangeError)):
                            first = e
        if first is not None:
            raise first

    def kernel_time(self):
        """(total ms, launches, algorithmic flops) of the convs the contexts time (RRDBNet: the dense blocks) since the last call."""
        tot_ms, tot_n, tot_fl = 0.0, 0, 0.0
        # replicas run on concurrent streams: their brackets overlap in wall time, so the sum of the
        # bracketed times is an upper bound of the busy time (the derived TFLOP/s a lower bound)
        for h in self._pool.handles():
            ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
            _lib.check(_lib.load().nesr_kernel_time_ms(h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)),
                       "nesr_kernel_time_ms")
            tot_ms, tot_n, tot_fl = tot_ms + ms.value, tot_n + n.value, tot_fl + fl.value
        return tot_ms, tot_n, tot_fl
