"""``RRDBNet`` drop-in: same constructor, state_dict key names and call signature as
``basicsr.archs.rrdbnet_arch.RRDBNet`` (basicsr>=1.4.2, requirements.txt:10), which the
reference builds at nesr/nesr.py:216, standalone/direct_esrgan.py:104 and
standalone/superres_project.py:69 and calls at nesr/nesr.py:891,935 (``model(img_12ch)``).

The module owns ordinary torch Parameters under upstream's names (so ``load_state_dict(strict=True)``,
``.parameters()``, ``.to()``, ``.eval()`` behave as the reference expects, nesr/nesr.py:888,962-973),
but its ``forward`` is the hand-written HIP path in libnesr_hip.so, reached through the C ABI.
There is no torch/CPU implementation of forward here: a non-CUDA input raises.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch
from torch import nn

from . import _lib
from ._contexts import _HipNet, current_stream_ptr, device_call


def conv_first_in_ch(num_in_ch: int, scale: int) -> int:
    """basicsr RRDBNet.__init__: scale 2 -> x4 channels (pixel_unshuffle 2), scale 1 -> x16."""
    return num_in_ch * {2: 4, 1: 16}.get(scale, 1)


def rrdbnet_state_dict_spec(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32):
    """Ordered {key: shape} of the 702 (for 23 blocks) tensors of an RRDBNet checkpoint."""
    spec = OrderedDict()

    def conv(name, cin, cout):
        spec[name + ".weight"] = (cout, cin, 3, 3)
        spec[name + ".bias"] = (cout,)

    conv("conv_first", conv_first_in_ch(num_in_ch, scale), num_feat)
    for b in range(num_block):
        for r in (1, 2, 3):
            for k in (1, 2, 3, 4):
                conv(f"body.{b}.rdb{r}.conv{k}", num_feat + (k - 1) * num_grow_ch, num_grow_ch)
            conv(f"body.{b}.rdb{r}.conv5", num_feat + 4 * num_grow_ch, num_feat)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(name, num_feat, num_feat)
    conv("conv_last", num_feat, num_out_ch)
    return spec


class _ConvParams(nn.Module):
    """Parameter holder for one 3x3 conv (weight OIHW + bias).  Not callable: the arithmetic
    happens in the HIP library, never in torch."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, 3, 3), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("_ConvParams holds weights only; RRDBNet.forward runs in libnesr_hip.so")


class _RDBParams(nn.Module):
    def __init__(self, nf, gc):
        super().__init__()
        for k in range(1, 5):
            setattr(self, f"conv{k}", _ConvParams(nf + (k - 1) * gc, gc))
        self.conv5 = _ConvParams(nf + 4 * gc, nf)


class _RRDBParams(nn.Module):
    def __init__(self, nf, gc):
        super().__init__()
        self.rdb1 = _RDBParams(nf, gc)
        self.rdb2 = _RDBParams(nf, gc)
        self.rdb3 = _RDBParams(nf, gc)


# compute_dtype strings of the f16 form (opt-in: .half() and torch.float16 keep selecting bf16), and the 16-bit forms whose tiles run
# as ragged batches through the LDS-resident strip kernel
F16_FORMS = ("f16", "fp16")
RAGGED_FORMS = ("bf16",) + F16_FORMS


class RRDBNet(_HipNet):
    """Networks consisting of Residual in Residual Dense Blocks (ESRGAN / Real-ESRGAN generator).

    Args mirror upstream: num_in_ch, num_out_ch, scale=4, num_feat=64, num_block=23, num_grow_ch=32.
    Extra keyword ``compute_dtype``:
      "f32" (default; the reference's half=False)  f32 in / out / accumulation; every conv operand is carried
                      as a pair of halves (x = hi + lo 2^-11) and each product is three f16 MFMAs (conv3x3_f16x2.hip);
                      whole-network max abs error vs an f64 evaluation 3e-6 (torch CPU f32: 1e-6).  Values beyond
                      +-65504 or non-finite do not fit: weights are refused at upload, activations turn the output
                      into NaN and raise NesrRangeError at the next check_range()/check_status()
      "f32-winograd"  f32 matrix cores, Winograd F(2x2,3x3) for the feature-map convs (error 2e-6)
      "f32-direct"    f32 matrix cores, direct implicit GEMM: bitwise a k-ordered fmaf chain
      "bf16"          bf16 storage and MFMA, f32 accumulation (what .half() / half=True select here)
      "f16" ("fp16")  f16 storage and MFMA, f32 accumulation: upstream's half=True numerics.  Opt-in: an "f16" model
                      stays f16 through .half(); the range contract of "f32" holds (|x| <= 65504: weights refused at
                      upload, an activation beyond it makes the output NaN and raises NesrRangeError at check_range())
    """

    def __init__(self, num_in_ch, num_out_ch, scale=4, num_feat=64, num_block=23, num_grow_ch=32,
                 compute_dtype="f32"):
        super().__init__()
        self.num_in_ch = num_in_ch
        self.num_out_ch = num_out_ch
        self.scale = scale
        self.num_feat = num_feat
        self.num_block = num_block
        self.num_grow_ch = num_grow_ch
        self.compute_dtype = "f16" if compute_dtype == "fp16" else compute_dtype
        self._build_params()
        self._band = None         # {(device index, slot): (internal height, internal width)} of the band images band_begin started

    # ------------------------------------------------------------------ parameters
    def _build_params(self):
        cin0 = conv_first_in_ch(self.num_in_ch, self.scale)
        self.conv_first = _ConvParams(cin0, self.num_feat)
        self.body = nn.Sequential(*[_RRDBParams(self.num_feat, self.num_grow_ch) for _ in range(self.num_block)])
        self.conv_body = _ConvParams(self.num_feat, self.num_feat)
        self.conv_up1 = _ConvParams(self.num_feat, self.num_feat)
        self.conv_up2 = _ConvParams(self.num_feat, self.num_feat)
        self.conv_hr = _ConvParams(self.num_feat, self.num_feat)
        self.conv_last = _ConvParams(self.num_feat, self.num_out_ch)

    def set_scale(self, scale):
        """Re-declares the network for another upstream ``scale`` (changes conv_first's input
        channels); used by RealESRGANer to accept genuine x2plus weights for a model that was
        declared without ``scale=2`` (the reference does that: SURVEY.md Appendix A)."""
        if scale == self.scale:
            return
        self.scale = scale
        dev = self.conv_body.weight.device
        self.conv_first = _ConvParams(conv_first_in_ch(self.num_in_ch, scale), self.num_feat).to(dev)
        self._release()

    def _to_bf16(self):
        """As _HipNet's, but a model built with compute_dtype="f16" stays f16 (upstream's fp16 run)."""
        if self.compute_dtype not in F16_FORMS:
            self.compute_dtype = "bf16"

    # ------------------------------------------------------------------ HIP context
    def _dtype_code(self):
        if self.compute_dtype in ("f32", "fp32", torch.float32, "f32-split", "f32-f16x2", "split"):
            return _lib.DTYPE_F32_SPLIT         # default f32 algorithm: operands as (hi, lo) half pairs on the f16 matrix cores
        if self.compute_dtype in ("f32-winograd", "f32w", "winograd"):
            return _lib.DTYPE_F32_WINOGRAD      # f32 matrix cores, Winograd F(2x2,3x3) for the feature-map convs
        if self.compute_dtype in ("f32-direct", "direct"):
            return _lib.DTYPE_F32               # direct implicit GEMM everywhere (bitwise a k-ordered fmaf chain)
        if self.compute_dtype in ("bf16", torch.bfloat16, "half", torch.float16):
            return _lib.DTYPE_BF16
        if self.compute_dtype in F16_FORMS:
            return _lib.DTYPE_F16               # f16 operands on the f16 matrix cores, range-checked (|x| <= 65504)
        raise ValueError(f"compute_dtype {self.compute_dtype!r}: expected 'f32', 'bf16' or 'f16'")

    def _create(self, index, code):
        handle = ctypes.c_void_p()
        _lib.check(_lib.load().nesr_create(ctypes.byref(handle), index, conv_first_in_ch(self.num_in_ch, self.scale),
                                           self.unshuffle, self.num_feat, self.num_block, self.num_grow_ch, self.num_out_ch, code),
                   "nesr_create")
        return handle

    RAGGED_MAX = 64          # images per forward_ragged call (nesr::RAG_MAX)

    @property
    def size_independent(self):
        """True: kernels are chosen by arithmetic only, never by image size, so an image has the same bits alone, in an
        equal-shape batch and in a ragged batch (include/nesr_hip.h: nesr_set_size_independent)."""
        return bool(self._pool.settings.get("nesr_set_size_independent"))

    @size_independent.setter
    def size_independent(self, on):
        self._pool.set("nesr_set_size_independent", bool(on))

    def strip_kernel_active(self):
        """True when bf16 / f16 dense blocks of a size-independent model run as the LDS-resident strip kernel (rdb_bf16_strip.hip;
        NESR_STRIP=0 turns it off): the tiling wrapper then hands all tiles of a frame over as one ragged batch."""
        import os
        return (self.compute_dtype in RAGGED_FORMS and self.size_independent and self.num_feat == 64 and self.num_grow_ch == 32
                and self.num_block > 0 and os.environ.get("NESR_STRIP", "-1") != "0")

    # ------------------------------------------------------------------ forward
    @property
    def unshuffle(self):
        """Input rows per internal (trunk) row: 2 for scale=2, 4 for scale=1, else 1."""
        return {2: 2, 1: 4}.get(self.scale, 1)

    def out_scale(self):
        """Output size / input size of forward(): 4 / unshuffle factor."""
        return 4 // self.unshuffle

    def _check_input(self, h, w):
        u = self.unshuffle
        if h % u or w % u:
            raise AssertionError(f"hh({h}) and hw({w}) must be divisible by {u}")  # upstream pixel_unshuffle asserts

    @torch.no_grad()
    def forward_ragged(self, x, sizes, slot: int = 0):
        """Images of different sizes in one batch (the tiles of a frame: realesrgan's tile_process as
        standalone/direct_esrgan.py:118-127 configures it cuts interior tiles of 532 x 532 and smaller edge tiles).
        x: [N, num_in_ch, H, W] float on a ROCm device, image i in the top-left sizes[i] = (h_i, w_i) pixels of slot i
        (the rest of a slot is ignored); returns [N, num_out_ch, H*s, W*s] whose slot i holds image i's output in its
        top-left h_i*s x w_i*s pixels (the rest is unspecified).  Every image gets the values forward() gives it alone
        on a model with size_independent = True.  compute_dtype "bf16" or "f16" only; N <= RAGGED_MAX."""
        self._require_cuda(x)
        if x.dim() != 4 or len(sizes) != x.shape[0]:
            raise ValueError(f"expected NCHW input and one (h, w) per image, got {tuple(x.shape)} and {len(sizes)} sizes")
        in_dtype = x.dtype
        xf = x.to(torch.float32).contiguous()
        n, c, h, w = xf.shape
        hw = (ctypes.c_int * (2 * n))(*[int(v) for pair in sizes for v in pair])
        s = self.out_scale()
        self.calls += 1
        y = torch.empty((n, self.num_out_ch, h * s, w * s), dtype=torch.float32, device=xf.device)
        self._call("nesr_forward_ragged", xf.device, slot, xf, n, c, h, w, hw, y)
        return y if in_dtype == torch.float32 else y.to(in_dtype)

    @torch.no_grad()
    def forward_nesr_u8(self, img_u8, mode, out=None, slot: int = 0):
        """The NESR pipeline's call of its 12-channel network, u8 in, u8 out (nesr_forward_nesr_u8): RGB u8 HWC [H, W, 3] device
        tensor -> RGB u8 HWC [4H, 4W, 3].  mode "12ch" | _lib.INPUT_12CH: _apply_esrgan_12channel (nesr/nesr.py:845-903), the
        synthesis [t, clamp(1.1 t), clamp(0.9 t), GaussianBlur3x3 / 255] of the BGR image, the network, the truncating quantiser,
        BGR -> RGB; "3ch" | _lib.INPUT_3CH_X4: _apply_esrgan_3channel (nesr/nesr.py:905-945), the image four times.  Bit for bit
        nesr_adapter.apply_esrgan_12channel / _3channel(use_hip=False).  `img_u8` may be a window of a frame (frame[y0:y1, x0:x1]:
        the blur reflects at the window's edges) and `out` a [4H, 4W, 3] window of a canvas; both need contiguous pixels in a row.
        A model with 12 input channels, scale 4 and 3 output channels; H, W >= 2."""
        self._require_cuda(img_u8)
        if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
            raise ValueError("expected a uint8 [H, W, 3] tensor")
        code = {"12ch": _lib.INPUT_12CH, "3ch": _lib.INPUT_3CH_X4}.get(mode, mode)
        rows = lambda t: t.stride(2) == 1 and t.stride(1) == 3 and t.stride(0) >= 3 * t.shape[1]      # noqa: E731
        x = img_u8 if rows(img_u8) else img_u8.contiguous()
        h, w, _ = x.shape
        if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (4 * h, 4 * w, 3) or out.device != x.device or not rows(out)):
            raise ValueError(f"out must be a uint8 [{4 * h}, {4 * w}, 3] tensor on {x.device} with contiguous pixels in a row")
        self.calls += 1
        y = torch.empty((4 * h, 4 * w, 3), dtype=torch.uint8, device=x.device) if out is None else out
        self._call("nesr_forward_nesr_u8", x.device, slot, x, x.stride(0), h, w, int(code), y, y.stride(0))
        return y

    # ------------------------------------------------------------------ sharded frames through the C ABI (RCCL below Python)
    def comm_init(self, device, rank, nranks, unique_id: bytes):
        """ncclCommInitRank for this model's context on `device` (include/nesr_hip.h: nesr_comm_init); `unique_id` = the 128 bytes
        rank 0 got from comm_unique_id(), distributed by the caller."""
        self._call("nesr_comm_init", device, 0, int(rank), int(nranks), ctypes.create_string_buffer(bytes(unique_id), 128))

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.load().nesr_comm_unique_id(buf), "nesr_comm_unique_id")
        return buf.raw

    @torch.no_grad()
    def forward_sharded_u8(self, band_u8, frame_hw, tile, tile_pad, through_fp16=False, rank=0):
        """This rank's rows of a uint8 HWC BGR frame -> (rank 0) the whole upscaled uint8 frame on the device, the tiles of
        upstream's grid dealt to the ranks of the communicator (nesr_forward_sharded_u8).  Without comm_init: the one-rank case."""
        self._require_cuda(band_u8)
        b = band_u8.contiguous()
        H, W = int(frame_hw[0]), int(frame_hw[1])
        s = self.out_scale()
        self.calls += 1
        out = torch.empty((H * s, W * s, 3), dtype=torch.uint8, device=b.device) if rank == 0 else None
        self._call("nesr_forward_sharded_u8", b.device, 0, b, H, W, int(tile), int(tile_pad), 1 if through_fp16 else 0, out)
        return out

    # ------------------------------------------------------------------ measurement helpers
    def forward_flops(self, n, h, w):
        """Algorithmic FLOPs of one forward on [n, *, h, w]."""
        macs = 0
        u = self.unshuffle
        px = n * (h // u) * (w // u)
        nf, gc = self.num_feat, self.num_grow_ch
        rdb = sum(9 * (nf + k * gc) * gc for k in range(4)) + 9 * (nf + 4 * gc) * nf
        macs += 9 * conv_first_in_ch(self.num_in_ch, self.scale) * nf + self.num_block * 3 * rdb + 9 * nf * nf
        macs += 4 * 9 * nf * nf + 16 * 9 * nf * nf * 2 + 16 * 9 * nf * self.num_out_ch
        return 2.0 * macs * px

    # ---- banded evaluation (banded.py: one row band of the frame per rank, SURVEY.md section 8(e) mode 2) ----
    @property
    def num_rdb(self):
        return 3 * self.num_block

    @torch.no_grad()
    def band_begin(self, x, slot: int = 0):
        """pixel_unshuffle + conv_first on this rank's rows (band + apron): x [1, num_in_ch, H, W] float32 on a ROCm device.
        `slot`: the context replica of x's device that holds the band (several bands of one process: see band_link)."""
        self._require_cuda(x)
        if x.dim() != 4 or x.shape[0] != 1:
            raise ValueError(f"expected [1, C, H, W], got {tuple(x.shape)}")
        xf = x.to(torch.float32).contiguous()
        _, c, h, w = xf.shape
        self._call("nesr_band_begin", xf.device, slot, xf, c, h, w)
        index = xf.device.index if xf.device.index is not None else torch.cuda.current_device()
        if self._band is None:
            self._band = {}
        self._band[(index, int(slot))] = (h // self.unshuffle, w // self.unshuffle)
        self._band_last = (index, int(slot))

    def _band_at(self, slot=None, device=None):
        """(device, slot, internal height, internal width) of the band image of context (device, slot); None = where band_begin
        ran last (`slot` alone: that slot of the last device)."""
        last = getattr(self, "_band_last", None)
        if device is not None:
            index = torch.device(device).index
            index = torch.cuda.current_device() if index is None else index
        else:
            index = last[0] if last else None
        slot = (last[1] if last else None) if slot is None and device is None else int(slot or 0)
        if self._band is None or (index, slot) not in self._band or self._handle(index, slot) is None:
            raise RuntimeError("band_begin has not run")
        return (torch.device("cuda", index), slot) + self._band[(index, slot)]

    def _band_call(self, name, slot, device, *args):
        dev, slot, _, _ = self._band_at(slot, device)
        self._call(name, dev, slot, *args)

    @torch.no_grad()
    def band_rdb(self, index, slot=None, device=None):
        """The five convs of RDB `index` (0 .. num_rdb-1) on the band image."""
        self._band_call("nesr_band_rdb", slot, device, int(index))

    @torch.no_grad()
    def band_rdb_phase(self, index, phase, top, bottom, edge_rows, slot=None, device=None):
        """Phase 0: conv1..conv4 of RDB `index` and conv5 on the `edge_rows` band rows next to each apron (what the
        neighbours wait for); phase 1: conv5 on the rows in between.  Same values as band_rdb."""
        self._band_call("nesr_band_rdb_phase", slot, device, int(index), int(phase), int(top), int(bottom), int(edge_rows))

    def band_row_bytes(self, slot=None, device=None):
        dev, slot, _, _ = self._band_at(slot, device)
        return int(_lib.load().nesr_band_row_bytes(self._handle(dev.index, slot)))

    @torch.no_grad()
    def band_pack_edges(self, buffer, top, bottom, nrows, top_dst, bottom_dst, slot=None, device=None):
        """The first / last `nrows` BAND rows (the rows the neighbours need) of `buffer` -> two preallocated uint8 tensors
        (either may be None), in one C-ABI call."""
        self._band_call("nesr_band_pack_edges", slot, device, int(buffer), int(top), int(bottom), int(nrows), top_dst, bottom_dst)

    @torch.no_grad()
    def band_unpack_aprons(self, buffer, top, bottom, nrows, top_src, bottom_src, slot=None, device=None):
        """The neighbours' rows -> the `nrows` apron rows next to the band on each side (either source may be None)."""
        self._band_call("nesr_band_unpack_aprons", slot, device, int(buffer), int(top), int(bottom), int(nrows), top_src, bottom_src)

    @torch.no_grad()
    def band_tail(self, slot=None, device=None):
        """conv_body .. conv_last -> [1, num_out_ch, 4 h, 4 w] float32 (h, w = internal size of the band image)."""
        dev, slot, h, w = self._band_at(slot, device)
        y = torch.empty((1, self.num_out_ch, 4 * h, 4 * w), dtype=torch.float32, device=dev)
        self._call("nesr_band_tail", dev, slot, y)
        return y

    @torch.no_grad()
    def band_rows(self, buffer, row0, nrows, slot=None, device=None):
        """Internal rows [row0, row0+nrows) of the num_feat-channel slice of `buffer` (0..2 dense-block buffers,
        3 = conv_first output) as an opaque uint8 tensor (the context's own element layout)."""
        dev, slot, _, _ = self._band_at(slot, device)
        out = torch.empty(int(nrows) * self.band_row_bytes(slot, dev), dtype=torch.uint8, device=dev)
        self._call("nesr_band_rows", dev, slot, int(buffer), int(row0), int(nrows), out, 0)
        return out

    @torch.no_grad()
    def band_set_rows(self, buffer, row0, rows, slot=None, device=None):
        """Inverse of band_rows: overwrites the rows with another rank's band_rows() bytes."""
        dev, slot, _, _ = self._band_at(slot, device)
        rb = self.band_row_bytes(slot, dev)
        if rb == 0:
            raise RuntimeError("band_set_rows: no banded evaluation is active (band_begin has not run, or a whole-frame forward reused the workspace)")
        rows = rows.to(dev).contiguous()
        if rows.dtype != torch.uint8 or rows.numel() % rb:
            raise ValueError("rows must be the uint8 tensor band_rows() returned on the sending rank")
        self._call("nesr_band_rows", dev, slot, int(buffer), int(row0), rows.numel() // rb, rows, 1)

    # ---- row bands inside one process (include/nesr_hip.h: nesr_band_link ...) ----
    def _lane_handles(self, lanes):
        """[(device, slot, handle)] of `lanes` = [(device, slot, ...)], contexts created where they are missing."""
        out = []
        for lane in lanes:
            dev = torch.device(lane[0])
            dev = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
            out.append((dev, int(lane[1]), self._context(dev, int(lane[1]))))
        return out

    def band_link(self, lanes):
        """Makes the contexts of `lanes` = [(device, slot)], top band first, neighbours of one another (nesr_band_link): their
        band_push_edges calls then write into each other's memory.  Returns band_link_state() of every lane."""
        hs = self._lane_handles(lanes)
        for j, (dev, _, h) in enumerate(hs):
            with torch.cuda.device(dev):
                _lib.check(_lib.load().nesr_band_link(h, hs[j - 1][2] if j else None, hs[j + 1][2] if j + 1 < len(hs) else None), "nesr_band_link")
        return [self.band_link_state(slot, dev) for dev, slot, _ in hs]

    def band_unlink(self, slot=0, device=None):
        h = self._existing(slot, device)
        if h is not None:
            _lib.check(_lib.load().nesr_band_unlink(h), "nesr_band_unlink")

    def band_link_state(self, slot=0, device=None):
        """{"up" | "down": None (no neighbour) | "local" (same device, the plain pointer) | "peer" (another device, written through
        the peer mapping) | "staged" (packed, then a device-to-device copy)} of a context."""
        h = self._existing(slot, device)
        v = int(_lib.load().nesr_band_link_state(h)) if h is not None else 0
        _lib.check(min(v, 0), "nesr_band_link_state")
        kind = lambda side: None if not v >> side & 1 else ("staged" if not v >> (2 + side) & 1 else ("peer" if v >> (4 + side) & 1 else "local"))   # noqa: E731
        return {"up": kind(0), "down": kind(1)}

    def band_set_staged(self, on, slot=0, device=None):
        """Every link of the context as a staged copy, whatever the devices allow (nesr_band_set_staged): A/B runs and tests."""
        _lib.check(_lib.load().nesr_band_set_staged(self._existing(slot, device), 1 if on else 0), "nesr_band_set_staged")

    @torch.no_grad()
    def band_push_edges(self, buffer, top, bottom, edge_rows, parity, slot=None, device=None):
        """This band's first / last `edge_rows` band rows of `buffer` -> the linked neighbours' landing buffers of `parity`, one
        launch on the current stream.  Ordering against the neighbours' streams is the caller's (events)."""
        self._band_call("nesr_band_push_edges", slot, device, int(buffer), int(top), int(bottom), int(edge_rows), int(parity))

    @torch.no_grad()
    def band_land_aprons(self, buffer, top, bottom, edge_rows, parity, also=(), slot=None, device=None):
        """The landing buffers of `parity` -> the apron rows of `buffer` (and of the buffers in `also`) next to the band."""
        mask = sum(1 << int(b) for b in also)
        self._band_call("nesr_band_land_aprons", slot, device, int(buffer), mask, int(top), int(bottom), int(edge_rows), int(parity))

    def _banded(self, entry, src, lanes, out, *args):
        """nesr_forward_banded / _u8 over `lanes` = [(device, slot[, stream])], top band first; lane 0 is on src's device and runs on
        its current stream, every other lane on its own stream (given, or kept by the model).  The streams first wait for what
        their devices' current streams hold (the contexts may still be in use there) and those wait for them afterwards, so the
        call is ordered like any other forward."""
        hs = self._lane_handles(lanes)
        if hs[0][0] != src.device:
            raise ValueError(f"the first lane is on {hs[0][0]}, the input on {src.device}")
        if not hasattr(self, "_band_streams"):
            self._band_streams = {}
        streams = []
        for j, (dev, slot, _) in enumerate(hs):
            cur = torch.cuda.current_stream(dev)
            if j == 0:
                st = cur
            elif len(lanes[j]) > 2 and lanes[j][2] is not None:
                st = lanes[j][2]
            else:
                st = self._band_streams.get((dev.index, slot))
                if st is None:
                    st = self._band_streams[(dev.index, slot)] = torch.cuda.Stream(device=dev)
            if st != cur:
                st.wait_stream(cur)
            streams.append(st)
        n = len(hs)
        ctxs = (ctypes.c_void_p * n)(*[h.value if isinstance(h, ctypes.c_void_p) else h for _, _, h in hs])
        sts = (ctypes.c_void_p * n)(*[st.cuda_stream for st in streams])
        self.calls += 1
        with torch.cuda.device(src.device):
            _lib.check(getattr(_lib.load(), entry)(ctxs, n, ctypes.c_void_p(src.data_ptr()), *args, ctypes.c_void_p(out.data_ptr()), sts), entry)
        for (dev, _, _), st in zip(hs, streams):
            cur = torch.cuda.current_stream(dev)
            if st != cur:
                cur.wait_stream(st)
        return out

    @torch.no_grad()
    def forward_banded(self, x, lanes):
        """forward() of ONE image as row bands, one per lane, inside this process (nesr_forward_banded): x [1, num_in_ch, H, W] float
        on the first lane's device -> [1, num_out_ch, H*s, W*s] there, for the f32 forms bit for bit forward(x).  `lanes`: see
        _banded; len(lanes) bands of banded.band_split.  check_range() afterwards covers every lane's context."""
        self._require_cuda(x)
        if x.dim() != 4 or x.shape[0] != 1:
            raise ValueError(f"expected [1, C, H, W], got {tuple(x.shape)}")
        in_dtype = x.dtype
        xf = x.to(torch.float32).contiguous()
        _, c, h, w = xf.shape
        self._check_input(h, w)
        s = self.out_scale()
        y = torch.empty((1, self.num_out_ch, h * s, w * s), dtype=torch.float32, device=xf.device)
        self._banded("nesr_forward_banded", xf, lanes, y, c, h, w)
        return y if in_dtype == torch.float32 else y.to(in_dtype)

    @torch.no_grad()
    def forward_banded_u8(self, img_hwc_u8, lanes, flip_rgb=True, round_nearest=True):
        """forward_u8() of one frame as row bands (nesr_forward_banded_u8): byte for byte forward_u8's result for the f32 forms."""
        self._require_cuda(img_hwc_u8)
        if img_hwc_u8.dtype != torch.uint8 or img_hwc_u8.dim() != 3 or img_hwc_u8.shape[2] != 3:
            raise ValueError("expected a uint8 [H, W, 3] tensor")
        x = img_hwc_u8.contiguous()
        h, w, _ = x.shape
        self._check_input(h, w)
        s = self.out_scale()
        y = torch.empty((h * s, w * s, 3), dtype=torch.uint8, device=x.device)
        # (the output goes last in _banded's argument list: the two switches stand before it in the C signature)
        return self._banded("nesr_forward_banded_u8", x, lanes, y, h, w, 1 if flip_rgb else 0, _lib.ROUND_NEAREST if round_nearest else _lib.ROUND_TRUNC)

    # ------------------------------------------------------------------ switches (ContextPool.settings: every context, now and later)
    def set_fused(self, on: bool):
        """Persistent (fused) dense-block launches on / off for every context of this model (include/nesr_hip.h: nesr_set_fused).
        They switch themselves off after a forward that gave up waiting (NesrHipError at check_range / check_status).
        Contexts the model creates later start with the same setting."""
        self._pool.set("nesr_set_fused", bool(on))

    def set_upconv(self, mode: str):
        """"2x2" (default) | "3x3": how compute_dtype "f32" runs conv_up1 / conv_up2 (include/nesr_hip.h: nesr_set_upconv), for
        every context of this model; contexts created later start with the same setting."""
        self._pool.set("nesr_set_upconv", {"3x3": _lib.UPCONV_3X3, "2x2": _lib.UPCONV_2X2}[mode])

    def set_conv_last(self, mode: str):
        """"narrow" (default) | "general": the launch geometry of compute_dtype "f32"'s conv_last (include/nesr_hip.h:
        nesr_set_conv_last); the image is bit-identical either way."""
        self._pool.set("nesr_set_conv_last", {"general": _lib.CONV_LAST_GENERAL, "narrow": _lib.CONV_LAST_NARROW}[mode])

    def _existing(self, slot, device):
        """Handle of context `slot` of `device` (None = the home device), or None."""
        return self._handle(self._pool.home if device is None else torch.device(device).index, slot)

    def upconv_state(self, slot=0, device=None):
        """"2x2" | "3x3": the form a context's conv_up1 / conv_up2 run in (None if it does not exist; `device`: None = the home device)."""
        h = self._existing(slot, device)
        if h is None:
            return None
        v = int(_lib.load().nesr_upconv_state(h))
        _lib.check(min(v, 0), "nesr_upconv_state")
        return "2x2" if v == _lib.UPCONV_2X2 else "3x3"

    def fused_state(self, slot=0, device=None):
        """(persistent launches enabled, forwards that gave up so far) of a context (`device`: None = the home device)."""
        h = self._existing(slot, device)
        if h is None:
            return False, 0
        v = int(_lib.load().nesr_fused_state(h))
        return bool(v & 1), v >> 1

    def chain_state(self, slot=0, device=None):
        """(kernel launches, dense blocks) that the context's last forward sent through the fused f32 dense-block kernels
        (nesr_rdb_chain_state): (1, 3 num_block) chained, equal numbers with one launch per block, (0, 0) with per-layer
        launches or if the context does not exist."""
        h = self._existing(slot, device)
        if h is None:
            return 0, 0
        launches, blocks = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().nesr_rdb_chain_state(h, ctypes.byref(launches), ctypes.byref(blocks)), "nesr_rdb_chain_state")
        return launches.value, blocks.value

    def debug_fault(self, drop_workgroups=1, slot=0):
        """TEST HOOK: the next persistent launch of the context leaves out its last workgroups (nesr_debug_fault)."""
        _lib.check(_lib.load().nesr_debug_fault(self._existing(slot, None), int(drop_workgroups)), "nesr_debug_fault")

    def preferred_batch(self, device, h, w, max_batch):
        """Tiles of h x w input per forward call that fill the GPU's CUs most evenly (<= max_batch)."""
        ctx = self._context(torch.device(device))
        return max(1, int(_lib.load().nesr_preferred_batch(ctx, h, w, max_batch)))


def cut_tiles_u8(frame_u8, windows, slot_hw, flip_rgb=True, through_fp16=False):
    """All tiles of a frame in one launch: u8 HWC [H, W, 3] device tensor -> float32 [n, 3, Hs, Ws], tile i =
    frame[y0:y0+h, x0:x0+w] / 255 (BGR -> RGB if flip_rgb) in the top-left of slot i, zeros elsewhere -- what
    RealESRGANer.enhance + tile_process feed the network (include/nesr_hip.h: nesr_cut_tiles_u8).  windows: [(y0, x0, h, w)]."""
    if frame_u8.device.type != "cuda" or frame_u8.dtype != torch.uint8 or frame_u8.dim() != 3 or frame_u8.shape[2] != 3:
        raise ValueError("cut_tiles_u8: a uint8 [H, W, 3] tensor on the ROCm device")
    f = frame_u8.contiguous()
    n = len(windows)
    hs, ws = int(slot_hw[0]), int(slot_hw[1])
    x = torch.empty((n, 3, hs, ws), dtype=torch.float32, device=f.device)
    arr = (ctypes.c_int * (4 * n))(*[int(v) for win in windows for v in win])
    device_call("nesr_cut_tiles_u8", f.device, f, f.shape[0], f.shape[1], 1 if flip_rgb else 0, 1 if through_fp16 else 0, arr, n, hs, ws, x)
    return x


def paste_tiles_u8(tiles, descs, dst_u8, flip_rgb=True, round_nearest=True, through_fp16=False):
    """The un-padded centres of all tiles in one launch: tiles float32 [n, 3, Hs, Ws] (network outputs in their slots) ->
    clamp(0, 1), RGB -> BGR, x255, round, into the uint8 device tensor dst_u8 (a frame's output canvas [H, W, 3], or any flat
    buffer).  descs: [(crop_y, crop_x, h, w, dst_byte_offset, dst_row_pitch_bytes)] (nesr_paste_tiles_u8)."""
    if tiles.device.type != "cuda" or tiles.dtype != torch.float32 or tiles.dim() != 4 or tiles.shape[1] != 3 or not tiles.is_contiguous():
        raise ValueError("paste_tiles_u8: a contiguous float32 [n, 3, Hs, Ws] tensor on the ROCm device")
    if dst_u8.dtype != torch.uint8 or not dst_u8.is_contiguous() or dst_u8.device != tiles.device:
        raise ValueError("paste_tiles_u8: a contiguous uint8 destination on the same device")
    n = tiles.shape[0]
    arr = (ctypes.c_int64 * (6 * n))(*[int(v) for d in descs for v in d])
    device_call("nesr_paste_tiles_u8", tiles.device, tiles, n, tiles.shape[2], tiles.shape[3], arr, dst_u8, dst_u8.numel(), 1 if flip_rgb else 0,
                _lib.ROUND_NEAREST if round_nearest else _lib.ROUND_TRUNC, 1 if through_fp16 else 0)


def fold_upconv_weights(weight):
    """OIHW float32 [cout, cin, 3, 3] -> [2, 2, 2, 2, cout, cin] = W[py][px][a][b]: the folded 2x2 taps of
    conv3x3(nearest_x2(x)) as libnesr_hip.so builds them (nesr_fold_upconv_weights; host only, no GPU)."""
    wt = weight.detach().to("cpu", torch.float32).contiguous()
    cout, cin = wt.shape[0], wt.shape[1]
    out = torch.empty((2, 2, 2, 2, cout, cin), dtype=torch.float32)
    _lib.check(_lib.load().nesr_fold_upconv_weights(ctypes.c_void_p(wt.data_ptr()), cout, cin, ctypes.c_void_p(out.data_ptr())),
               "nesr_fold_upconv_weights")
    return out


def conv3x3(x, weight, bias, lrelu=False, upsample=False, dtype="f32", upconv=None):
    """Single fused layer through the C ABI (test hook): conv3x3(pad 1) + bias [+ LeakyReLU(0.2)],
    optionally on the nearest-x2 upsample of x.  x NCHW float32 on a ROCm device.  upconv: None (the default form) | "3x3" |
    "2x2" for an upsampled f32 layer (nesr_conv3x3_up)."""
    if x.device.type != "cuda":
        raise RuntimeError("conv3x3 runs only on an AMD GPU through libnesr_hip.so (no CPU fallback)")
    x = x.to(torch.float32).contiguous()
    n, cin, h, w = x.shape
    wt = weight.detach().to("cpu", torch.float32).contiguous()
    bs = bias.detach().to("cpu", torch.float32).contiguous()
    cout = wt.shape[0]
    up = 1 if upsample else 0
    y = torch.empty((n, cout, h << up, w << up), dtype=torch.float32, device=x.device)
    # "f32" is what RRDBNet(compute_dtype="f32") runs: the f16-pair kernel
    code = {"bf16": _lib.DTYPE_BF16, "f32-winograd": _lib.DTYPE_F32_WINOGRAD, "f32": _lib.DTYPE_F32_SPLIT, "f32-split": _lib.DTYPE_F32_SPLIT,
            "f32-direct": _lib.DTYPE_F32, "f16": _lib.DTYPE_F16, "fp16": _lib.DTYPE_F16}[dtype]
    args = (code, x, n, cin, h, w, wt, bs, cout, 1 if lrelu else 0, up, y)
    if upconv is None:
        device_call("nesr_conv3x3", x.device, *args)
    else:   # (the stream is not this entry's last parameter: it is given here)
        device_call("nesr_conv3x3_up", x.device, *args, current_stream_ptr(x.device), {"3x3": _lib.UPCONV_3X3, "2x2": _lib.UPCONV_2X2}[upconv])
    return y


def last_conv_kernel():
    """The kernel family that the last conv3x3() call on this thread launched, as its launcher noted it at the point of
    dispatch (nesr_debug_last_conv_kernel): "generic" | "xl" | "winograd" | "f16-pair" | "upconv2x2", None before any call."""
    return _lib.CONV_KERNEL_NAMES[_lib.load().nesr_debug_last_conv_kernel()]
