"""``RealESRGANer`` drop-in: same constructor keywords, attributes and methods as
``realesrgan.RealESRGANer`` (realesrgan>=0.3.0, requirements.txt:9), as the reference uses it:

  nesr/nesr.py:220-229                   RealESRGANer(scale=int(upscale_factor), model_path=..., model=model,
                                         tile=0, tile_pad=0, pre_pad=0, half=False, device=self.device);
                                         afterwards only ``.model`` is used (nesr/nesr.py:887-891,930-935)
  standalone/direct_esrgan.py:118-127    RealESRGANer(scale, model_path, model, tile=512, tile_pad=10,
                                         pre_pad=0, half=False, device) ; ``.enhance(img)`` at :148
  standalone/superres_project.py:70-75   ctor defaults ; ``.enhance(bgr)`` at :282

Host logic only (padding, tile grid, cropping, colour order, quantisation); every network
evaluation goes through ``self.model``, which for this package is the HIP-backed
:class:`RRDBNet`.  cv2 is not needed: the colour conversions are plain numpy, and ``outscale != scale`` /
``alpha_upsampler != 'realesrgan'`` use imgproc.py's device-side restatement of cv2.resize (parity unpinned).

The routes of a frame, in the order ``_enhance_once`` tries them (planning: _tiling.py; ``devices=`` lanes: _lanes.py):

  _fused_u8_ok                      one forward_u8 call, inline in _enhance_once (enhance_many: _forward_u8_to_host)
  _u8_on_device_ok                  _enhance_u8_on_device: _pad_on_device + _run(), quantised on the device
    .. and _u8_tiles_fused_ok       _enhance_u8_tiles_fused (several devices: _enhance_u8_tiles_fused_devices)
  _device_frame_ok                  _enhance_frame_on_device (enhance_many, _frame_inflight_ok: _frame_in_flight)
  otherwise                         enhance_float on the host, then enhance's numpy quantiser
"""
from __future__ import annotations

import functools
import math
import types
import warnings

import numpy as np
import torch
from torch.nn import functional as F

from . import _lanes, _tiling
from ._lanes import parse_devices
from ._lib import NesrHipError, NesrRangeError
from .rrdbnet import RAGGED_FORMS, RRDBNet
from .srvgg import SRVGGNetCompact

# enhance(outscale=...) and the plain alpha upsampler run imgproc's HIP resize kernels (8-bit frames and the float32 alpha plane;
# 16-bit frames keep the torch chain, see _resize_on_host_route), on the 8-bit device routes before the frame's one
# device-to-host copy.  False: the frame goes to the host first and the resize is imgproc's torch chain (use_hip=False).
HIP_RESIZE = True

# Gray, BGRA and 16-bit frames (everything enhance() takes besides 8-bit BGR) stay on the device from the upload of the uint8 / uint16
# frame to the one copy home of the quantised result (_enhance_frame_on_device: _frame_through's frame_io.pack_frame / unpack_frame
# around the same _pad_on_device and _run()).  False: enhance_float's host route -- numpy preparation, float32 upload, float32 canvas download, numpy
# clamp / flip / gray / quantiser; the two give the same bits.
DEVICE_FRAMES = True


# Integrity pins of the published checkpoints: the only ones the reference holds (nesr/utils/downloader.py:25-26, 33-34).
KNOWN_CHECKPOINTS = {
    "5db904e3e9f0dbf5c64b7ae665527e62": "RealESRGAN_x2plus.pth (v0.2.5.0 release, 67,010,191 bytes)",
    "94df4e7c584b55e2e9a5d2b8f161860e": "RealESRGAN_x4plus.pth (v0.1.0 release)",
}


def checkpoint_provenance(path):
    """md5 of a checkpoint file against the reference's table -> ("verified"|"unverified", description).
    A file NAMED like a published checkpoint whose digest differs is reported with a warning (it may be a fine-tune;
    it is not the file the reference downloads)."""
    import hashlib
    import os
    h = hashlib.md5()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    digest, size = h.hexdigest(), os.path.getsize(path)
    if digest in KNOWN_CHECKPOINTS:
        return "verified", f"{KNOWN_CHECKPOINTS[digest]}: md5 {digest} matches nesr/utils/downloader.py"
    base = os.path.basename(str(path))
    if base in ("RealESRGAN_x2plus.pth", "RealESRGAN_x4plus.pth"):
        warnings.warn(f"{path}: named like a published Real-ESRGAN checkpoint but md5 {digest} ({size} bytes) is not the "
                      "digest recorded in the reference (nesr/utils/downloader.py:25-26,33-34)")
    return "unverified", f"{base}: md5 {digest}, {size} bytes (not a digest the reference records)"


def _bgr2gray(img):
    # cv2.COLOR_BGR2GRAY on float32
    return (img[..., 0] * np.float32(0.114) + img[..., 1] * np.float32(0.587) + img[..., 2] * np.float32(0.299)).astype(np.float32)


_U8_LUT = np.arange(256, dtype=np.float32) / 255     # exactly enhance()'s `img.astype(float32) / 255`


def normalize_u8_on_device(x):
    """uint8 tensor -> float32 in [0,1] with numpy's correctly rounded division.  (torch divides by a
    Python scalar on the GPU by multiplying with its reciprocal, which is 1 ulp off for some of the 256
    values -- enough to flip a rounding tie 351 layers later.)"""
    lut = torch.from_numpy(_U8_LUT).to(x.device)
    return lut[x.long()]


def _gray2rgb(img):
    return np.repeat(img[:, :, None], 3, axis=2)


def _is_gave_up(e):
    """A persistent dense-block launch gave up waiting for its workgroups (not a range error): the frame can be evaluated again."""
    return not isinstance(e, NesrRangeError) and "gave up waiting" in str(e)


class _InFlight:
    """enhance_many's frames in flight, oldest first: ``add(*entry)`` behind a frame's last enqueued work, on its stream;
    ``collect(leave)`` waits for the oldest and calls ``finish(*entry)`` (context check, result) until `leave` are pending.
    Errors are the caller's, and the two callers differ (as they always have; kept, not decided): enhance_many on one device lets
    every error through -- no retry after a launch that gave up, the frames in flight not waited for; _enhance_many_devices does both."""

    def __init__(self, finish):
        self.finish, self.pending = finish, []     # pending: [(event, *entry)]

    def add(self, *entry):
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((ev,) + entry)

    def collect(self, leave=0):
        while len(self.pending) > leave:
            ev, *entry = self.pending.pop(0)
            ev.synchronize()
            self.finish(*entry)


class RealESRGANer:
    """A helper class for upsampling images with RealESRGAN (MI355X/HIP backend).

    Args:
        scale (int): Upsampling scale factor used in the networks. It is usually 2 or 4.
        model_path (str | list[str] | dict): checkpoint path(s) ({'params_ema'|'params': state_dict}),
            or an already loaded checkpoint dict.
        dni_weight (list[float]): deep-network-interpolation weights when model_path is a list of two.
        model (nn.Module): the network (RRDBNet).
        tile (int): tile size; 0 = no tiling.
        tile_pad (int): pad size of each tile.  pre_pad (int): reflect pad before the network.
        half (bool): upstream's fp16 switch; here it selects the bf16 MFMA kernels, or keeps a model built with
            RRDBNet(..., compute_dtype="f16") or SRVGGNetCompact(..., compute_dtype="fp16") in f16 (upstream's fp16 numerics).
        device: 'cuda' (= the ROCm GPU), torch.device or None (-> cuda if available).
        devices (list[int] | None): not upstream's: CUDA device indices one wrapper spreads its work over from this process
            (repeats put several contexts on one device).  None reads NESR_DEVICES (see parse_devices); with neither set the
            wrapper runs on `device` alone, as upstream's does.  With two or more entries a tiled frame's tiles are split over
            them (sharded.plan_tiles) and enhance_many deals whole frames to them; the result is bitwise the one-device result.
            An image that is ONE network evaluation (tile=0, or a frame no larger than the tile) is split into row bands, one
            per entry, when the model is an RRDBNet in an f32 form (see _band_plan; `band_devices = False` switches that off, and
            then, as for every other model, such a frame runs on the first entry).  The first entry is also where the output is
            assembled and `device` points.
    """

    # Row bands of an untiled frame over `devices` (class attributes: an instance that never sets them has upstream's state)
    band_devices = True       # None | False: untiled frames run on the first entry
    BAND_MIN_ROWS = 48        # banded.BAND_MIN_ROWS: internal rows a lane gets at least (fewer lanes below that, down to one)
    last_bands = None         # [(lo, hi)] internal rows per lane of the last frame's (last) network evaluation; None: it was not banded

    def __init__(self, scale, model_path, dni_weight=None, model=None, tile=0, tile_pad=10, pre_pad=10,
                 half=False, device=None, gpu_id=None, devices=None):
        self.scale = scale
        self.tile_size = tile
        self.tile_pad = tile_pad
        self.pre_pad = pre_pad
        self.mod_scale = None
        self.half = half
        self.tile_batch = 24  # upper bound on equal-shaped tiles per forward call (1 = upstream's serial loop)
        self.tile_streams = 3 # HIP streams (context replicas) the shape groups of one frame are spread over
        self.ragged_tiles = None  # bf16: all tiles of a frame, whatever their shapes, in ragged batches (see _run_tiles_ragged).  None = when the
                                  # model's dense blocks run as the LDS-resident strip kernel (rdb_bf16_strip.hip), whose schedule packs the
                                  # strips of ALL tiles onto the compute units; with the per-layer kernels ragged batches measured no faster
        self.ragged_batch = 64    # tiles per ragged batch
        self.small_job_tiles = 12   # a call with at most this many tiles (a rank's share of a sharded frame) ...
        self.small_job_streams = 5  # ... is spread over this many streams, its batches split until every stream has one

        if gpu_id:
            self.device = torch.device(f"cuda:{gpu_id}" if torch.cuda.is_available() else "cpu") if device is None else device
        else:
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu") if device is None else device
        self.device = torch.device(self.device)
        self.devices = parse_devices(devices, torch.cuda.device_count())
        if self.devices is not None:
            self.device = torch.device("cuda", self.devices[0])

        # where the weights came from: "verified" only for a file whose md5 is one the reference records
        self.weights_provenance = ("unverified", "in-memory state_dict (tests and benches use seeded synthetic weights: "
                                                 "no checkpoint ships with the reference)")
        if isinstance(model_path, list):
            assert len(model_path) == len(dni_weight), "model_path and dni_weight should have the save length."
            loadnet = self.dni(model_path[0], model_path[1], dni_weight)
            self.weights_provenance = ("unverified", "deep network interpolation of two checkpoints")
        elif isinstance(model_path, dict):
            loadnet = model_path
        else:
            if str(model_path).startswith("https://"):
                raise RuntimeError(f"{model_path}: downloading checkpoints is not supported (offline build); "
                                   "pass a local path to RealESRGAN_x2plus.pth / RealESRGAN_x4plus.pth")
            loadnet = torch.load(model_path, map_location=torch.device("cpu"), weights_only=True)
            self.weights_provenance = checkpoint_provenance(model_path)

        keyname = "params_ema" if "params_ema" in loadnet else "params"
        state = loadnet[keyname]
        self._adapt_declared_scale(model, state)
        model.load_state_dict(state, strict=True)
        model.eval()
        self.model = model.to(self.device)
        if self.half:
            self.model = self.model.half()
        if isinstance(self.model, RRDBNet) and self.tile_size > 0 and self.model.compute_dtype in RAGGED_FORMS:
            # a tiling wrapper batches tiles of different shapes (ragged batches): a tile's values must not depend on how it
            # was batched, nor on whether model(tile) was called directly -- kernels are chosen by arithmetic only
            self.model.size_independent = True
        if self._multi() and not self._hip_model():
            raise ValueError("devices=: only the HIP networks (RRDBNet, SRVGGNetCompact) run on several devices at once")

    @staticmethod
    def _adapt_declared_scale(model, state):
        """The reference declares RRDBNet(num_in_ch=3, ...) without scale=2 and then loads
        RealESRGAN_x2plus weights, whose conv_first has 12 input channels
        (standalone/direct_esrgan.py:104, standalone/download-x3-model.py:2-4 documents the
        resulting 'channel mismatch').  A genuine x2plus checkpoint is recognised by
        conv_first.weight having 4x the declared input channels and the model is switched to
        upstream's scale=2 form (pixel_unshuffle + 12-channel conv_first) instead of failing."""
        if not isinstance(model, RRDBNet) or "conv_first.weight" not in state:
            return
        cin = state["conv_first.weight"].shape[1]
        if model.scale == 4 and cin == model.num_in_ch * 4:
            warnings.warn("RRDBNet was declared without scale=2 but the checkpoint's conv_first takes "
                          f"{cin} channels: treating it as the scale=2 (pixel_unshuffle) network")
            model.set_scale(2)
        elif model.scale == 4 and cin == model.num_in_ch * 16:
            model.set_scale(1)

    def dni(self, net_a, net_b, dni_weight, key="params", loc="cpu"):
        """Deep network interpolation: weighted sum of two checkpoints' tensors."""
        if not isinstance(net_a, dict):
            net_a = torch.load(net_a, map_location=torch.device(loc), weights_only=True)
        if not isinstance(net_b, dict):
            net_b = torch.load(net_b, map_location=torch.device(loc), weights_only=True)
        for k, v_a in net_a[key].items():
            net_a[key][k] = dni_weight[0] * v_a + dni_weight[1] * net_b[key][k]
        return net_a

    # ------------------------------------------------------------------ pre / process / post
    def pre_process(self, img):
        """HWC float32 RGB [0,1] -> self.img [1,3,H,W] on device; reflect pre-pad; pad to mod_scale."""
        img = torch.from_numpy(np.transpose(img, (2, 0, 1))).float()
        self._pad_on_device(img.unsqueeze(0).to(self.device))

    def _pad_on_device(self, x):
        """The device-side half of upstream's pre_process: x is [1,3,H,W] float on self.device."""
        self.img = x
        if self.half:
            self.img = self.img.half()
        if self.pre_pad != 0:
            self.img = F.pad(self.img, (0, self.pre_pad, 0, self.pre_pad), "reflect")
        if self.scale == 2:
            self.mod_scale = 2
        elif self.scale == 1:
            self.mod_scale = 4
        if self.mod_scale is not None:
            self.mod_pad_h, self.mod_pad_w = 0, 0
            _, _, h, w = self.img.size()
            if h % self.mod_scale != 0:
                self.mod_pad_h = self.mod_scale - h % self.mod_scale
            if w % self.mod_scale != 0:
                self.mod_pad_w = self.mod_scale - w % self.mod_scale
            self.img = F.pad(self.img, (0, self.mod_pad_w, 0, self.mod_pad_h), "reflect")

    def process(self):
        plan = self._band_plan(self.img) if self.img.shape[0] == 1 else None
        if plan is None:
            self.output = self.model(self.img)
            return
        self.output = self.model.forward_banded(self.img, plan[0])
        self.last_bands = plan[1]

    def _band_plan(self, img):
        """(lanes, bands) when `img`, the image the network sees ([1, 3, H, W] after pre-pad and mod-pad, or the uint8 [H, W, 3]
        frame of the fused route), is evaluated as row bands over `devices`, else None: two or more entries, banding not switched
        off, an RRDBNet in one of the f32 forms (their bands are bit for bit the whole frame; bf16 / f16 pick kernels by image
        size), and at least BAND_MIN_ROWS internal rows for two lanes.  Lanes: the first len(bands) entries of `devices`."""
        from . import _lib, banded
        if not (self._multi() and self.band_devices and isinstance(self.model, RRDBNet) and self.device.type == "cuda"
                and self.model._dtype_code() in (_lib.DTYPE_F32_SPLIT, _lib.DTYPE_F32_WINOGRAD, _lib.DTYPE_F32)):
            return None
        h, w = (img.shape[0], img.shape[1]) if img.dim() == 3 else (img.shape[2], img.shape[3])
        u = self.model.unshuffle
        if h % u or w % u:
            return None
        bands = banded.band_lanes(h // u, len(self.devices), self.BAND_MIN_ROWS)
        if len(bands) < 2:
            return None
        lanes, _ = _lanes.lanes(self.devices, self._streams, self.device)
        return lanes[:len(bands)], bands

    def tile_grid(self, height, width):
        """The tile windows upstream's tile_process visits, in its order.  Each entry:
        (padded input window y0,y1,x0,x1 ; output window y0,y1,x0,x1 ; crop inside the tile's output y0,y1,x0,x1)."""
        tiles_x = math.ceil(width / self.tile_size)
        tiles_y = math.ceil(height / self.tile_size)
        s = self.scale
        grid = []
        for y in range(tiles_y):
            for x in range(tiles_x):
                ix0, iy0 = x * self.tile_size, y * self.tile_size
                ix1, iy1 = min(ix0 + self.tile_size, width), min(iy0 + self.tile_size, height)
                px0, px1 = max(ix0 - self.tile_pad, 0), min(ix1 + self.tile_pad, width)
                py0, py1 = max(iy0 - self.tile_pad, 0), min(iy1 + self.tile_pad, height)
                tw, th = ix1 - ix0, iy1 - iy0
                cx0, cy0 = (ix0 - px0) * s, (iy0 - py0) * s
                grid.append(((py0, py1, px0, px1), (iy0 * s, iy1 * s, ix0 * s, ix1 * s), (cy0, cy0 + th * s, cx0, cx0 + tw * s)))
        return grid

    def batch_for(self, th, tw, ntiles):
        """Tiles of th x tw input evaluated per forward call: at most ``tile_batch``, and on the HIP
        backend the count whose workgroups fill the CUs most evenly (values do not depend on it)."""
        nb = max(1, min(int(self.tile_batch), ntiles))
        if nb > 1 and isinstance(self.model, RRDBNet) and self.device.type == "cuda":
            nb = self.model.preferred_batch(self.device, th, tw, nb)
        return nb

    def run_tiles(self, img, tiles, sink, slot_base=0):
        """Evaluates the network on windows of `img` ([1,C,H,W] on a device).  `tiles` is a list of
        (y0, y1, x0, x1, payload); `sink(payload, out)` receives each window's output [1,C,h*s,w*s] (a view
        valid on the current stream).  Equal-shaped windows are batched (batch_for); on the HIP backend
        the shape groups are spread over `tile_streams` streams with their own context replicas, so the
        small edge-tile groups -- whose 351 launches are latency-bound -- overlap the large ones.
        Values do not depend on batching or stream assignment.  `slot_base`: the first context replica used (a lane of a
        multi-device frame, see _tile_process_devices, takes slots slot_base, slot_base + 1, ...)."""
        hip = self._hip_model() and img.device.type == "cuda"
        if hip and isinstance(self.model, RRDBNet) and img.shape[0] == 1 and self.model.compute_dtype in RAGGED_FORMS:
            ragged = self.model.strip_kernel_active() if self.ragged_tiles is None else bool(self.ragged_tiles)
            if ragged and (len({(t[1] - t[0], t[3] - t[2]) for t in tiles}) > 1 or self.ragged_tiles is None):
                return self._run_tiles_ragged(img, tiles, sink, single_stream=self.ragged_tiles is None, slot_base=slot_base)
        plan = _tiling.shape_group_plan(tiles, self.batch_for if img.shape[0] == 1 else lambda *_: 1, self.tile_streams,
                                        self.small_job_tiles, self.small_job_streams, multi=hip and len(tiles) > 1)

        def run_batch(chunk, slot):
            if len(chunk) == 1:
                inp = img[:, :, chunk[0][0]:chunk[0][1], chunk[0][2]:chunk[0][3]]
            else:
                inp = torch.cat([img[:, :, t[0]:t[1], t[2]:t[3]] for t in chunk], 0)
            with torch.no_grad():
                out = self.model(inp, slot=slot) if hip else self.model(inp)
            for j, t in enumerate(chunk):
                sink(t[4], out[j:j + 1] if len(chunk) > 1 else out)

        self._fan_out(img.device, slot_base, plan, run_batch)

    @functools.cached_property
    def _streams(self):
        """Streams kept across frames: side[(device index, slot_base)] _fan_out's, lane[entry of `devices`], gather (_lanes.py)."""
        return types.SimpleNamespace(side={}, lane={}, gather=None)

    def _fan_out(self, device, slot_base, plan, run_batch):
        """Runs a _tiling plan: stream k's batches in order as ``run_batch(batch, slot_base + k)``, stream 0 being the current one;
        the side streams first wait for it (the image and the output canvas were produced there) and it for them at the end."""
        if len(plan) == 1:
            for b in plan[0]:
                run_batch(b, slot_base)
            return
        main = torch.cuda.current_stream(device)
        side = self._streams.side.setdefault((device.index, slot_base), [])
        while len(side) < len(plan) - 1:
            side.append(torch.cuda.Stream(device=device))
        streams = [main] + side[:len(plan) - 1]
        for st in streams[1:]:
            st.wait_stream(main)
        for k, st in enumerate(streams):
            with torch.cuda.stream(st):
                for b in plan[k]:
                    run_batch(b, slot_base + k)
        for st in streams[1:]:
            main.wait_stream(st)

    def _ragged_cap(self):
        return max(1, min(self.model.RAGGED_MAX, int(self.ragged_batch)))   # tiles per ragged batch: what forward_ragged takes at most

    def _run_tiles_ragged(self, img, tiles, sink, single_stream=False, slot_base=0):
        """All windows of a frame, whatever their shapes, in `tile_streams` ragged batches that run side by side: every
        window lies in the top-left corner of an equal-sized slot and the kernels take each image's own size from the
        call (nesr_forward_ragged).  Against one batch per tile shape: the small edge-tile groups were latency-bound
        launches of a few workgroups -- and with the tiles sharded over ranks every group shrinks further -- while
        batches of mixed sizes keep every launch large; several batches on their own streams (context replicas) fill
        each other's prologues and epilogues as the shape groups did.  bf16 only; the model is size_independent, so a
        window's values are the ones model(window) gives it alone."""
        if not self.model.size_independent:
            self.model.size_independent = True
        # (strip kernel: one batch after the other on one stream -- a persistent launch holds the whole device)
        nstreams = 1 if single_stream else max(1, min(int(self.tile_streams), len(tiles)))
        plan = _tiling.ragged_plan(tiles, nstreams, self._ragged_cap())

        def run_batch(chunk, slot):
            H = max(t[1] - t[0] for t in chunk)
            W = max(t[3] - t[2] for t in chunk)
            x = img.new_zeros((len(chunk), img.shape[1], H, W))
            for j, t in enumerate(chunk):
                x[j, :, :t[1] - t[0], :t[3] - t[2]] = img[0, :, t[0]:t[1], t[2]:t[3]]
            with torch.no_grad():
                out = self.model.forward_ragged(x, [(t[1] - t[0], t[3] - t[2]) for t in chunk], slot=slot)
            s = out.shape[2] // H
            for j, t in enumerate(chunk):
                sink(t[4], out[j:j + 1, :, :(t[1] - t[0]) * s, :(t[3] - t[2]) * s])

        self._fan_out(img.device, slot_base, plan, run_batch)

    def tile_process(self):
        """Runs the network on overlapping tiles and pastes the un-padded centres (upstream
        semantics, tile for tile); see run_tiles for the batching / stream spreading."""
        if self._multi():
            return self._tile_process_devices()
        batch, channel, height, width = self.img.shape
        s = self.scale
        self.output = self.img.new_zeros((batch, channel, height * s, width * s))
        tiles = [(py0, py1, px0, px1, (o, c)) for ((py0, py1, px0, px1), o, c) in self.tile_grid(height, width)]

        def paste(payload, out):
            (oy0, oy1, ox0, ox1), (cy0, cy1, cx0, cx1) = payload
            self.output[:, :, oy0:oy1, ox0:ox1] = out[:, :, cy0:cy1, cx0:cx1]

        self.run_tiles(self.img, tiles, paste)

    # ------------------------------------------------------------------ several devices (devices=[...])
    def _multi(self):
        """Two or more entries in `devices`: tiles and frames are spread over them."""
        return getattr(self, "devices", None) is not None and len(self.devices) > 1

    def device_shares(self, height, width):
        """(tiles, shares): upstream's tile grid of a height x width frame (the padded image the network sees) as
        sharded.Tile records, and per entry of `devices` the indices of the tiles it computes -- sharded.plan_tiles with
        world = len(devices): contiguous runs in row-major order, balanced by padded input area."""
        from .sharded import plan_tiles
        tiles, owner = plan_tiles(self, height, width, len(self.devices))
        return tiles, [[i for i, o in enumerate(owner) if o == j] for j in range(len(self.devices))]

    @torch.no_grad()
    def _tile_process_devices(self):
        """tile_process with the tiles split over `devices`: every device gets the padded image (one copy from the first
        device), runs its share through run_tiles on its lane's stream and replicas, and the un-padded centres come back to
        self.output on the first device.  The first device's lanes paste straight into self.output."""
        _, channel, height, width = self.img.shape
        dev0 = self.img.device
        self.output = self.img.new_zeros((1, channel, height * self.scale, width * self.scale))
        tiles, shares = self.device_shares(height, width)
        lanes, gather = _lanes.lanes(self.devices, self._streams, self.device)
        stride = max(1, int(self.tile_streams), int(self.small_job_streams))   # replicas one lane's run_tiles may use

        def copy(dev, st):
            with torch.cuda.stream(gather), torch.cuda.stream(st):
                return self.img.to(dev, non_blocking=True)         # copied on `gather`; `st` waits for it (and so does its event)
        def run_share(dev, o, st, share, img):
            if img is not self.img:
                img.record_stream(st)                   # read here after this call has returned: not freed before
            pieces = []
            def sink(t, out):
                p = out[:, :, t.crop[0]:t.crop[1], t.crop[2]:t.crop[3]]
                if dev.index == dev0.index:
                    self.output[:, :, t.out[0]:t.out[1], t.out[2]:t.out[3]] = p
                else:
                    pieces.append((t, p.contiguous()))       # made on one of run_tiles' streams ...
                    pieces[-1][1].record_stream(st)          # ... read on the lane's
            self.run_tiles(img, [(t.inp[0], t.inp[1], t.inp[2], t.inp[3], t) for t in (tiles[i] for i in share)], sink,
                           slot_base=o * stride)
            items, off = [], 0
            for t, p in pieces:
                items.append((off, tuple(p.shape), (slice(None), slice(None), slice(t.out[0], t.out[1]), slice(t.out[2], t.out[3]))))
                off += p.numel()
            return (torch.cat([p.reshape(-1) for _, p in pieces]), items) if pieces else None

        _lanes.run_shares(lanes, shares, gather, self.output, {dev0.index: (self.img, None)}, copy, run_share)

    @torch.no_grad()
    def _enhance_u8_tiles_fused_devices(self, img):
        """_enhance_u8_tiles_fused with the tiles split over `devices`: the 8-bit frame goes to every device, each cuts, runs
        and pastes its share (tiles_u8_on_device on its lane's stream and replica), the first device's lanes into the output
        canvas, the others into a packed buffer that one device-to-device copy brings to the first device.  All devices are
        enqueued before the frame is waited for; workspaces are reserved first, since growing one synchronises."""
        h, w = img.shape[:2]
        s = self.scale
        dev0 = self.device
        tiles, shares = self.device_shares(h, w)
        lanes, gather = _lanes.lanes(self.devices, self._streams, self.device)
        cap = self._ragged_cap()
        for (dev, o, _), share in zip(lanes, shares):
            for i in range(0, len(share), cap):
                part = [tiles[k] for k in share[i:i + cap]]
                self.model.reserve(dev, len(part), max(t.inp[1] - t.inp[0] for t in part), max(t.inp[3] - t.inp[2] for t in part), slot=o)
        main = torch.cuda.current_stream(dev0)
        pinned = torch.from_numpy(np.ascontiguousarray(img)).pin_memory()
        canvas = torch.empty((h * s, w * s, 3), dtype=torch.uint8, device=dev0)

        def copy(dev, st):
            with torch.cuda.device(dev), torch.cuda.stream(st):
                return pinned.to(dev, non_blocking=True)   # H2D: uint8 HWC BGR
        def run_share(dev, o, st, share, frame):
            mine = [tiles[i] for i in share]
            if dev.index == dev0.index:
                self.tiles_u8_on_device(frame, _tiling.windows(mine), _tiling.canvas_pastes(mine, w * s), canvas, slot=o)
                return None
            pastes, offs = _tiling.packed_pastes(mine)
            packed = torch.empty((offs[-1],), dtype=torch.uint8, device=dev)
            self.tiles_u8_on_device(frame, _tiling.windows(mine), pastes, packed, slot=o)
            return packed, [(offs[i], (t.out[1] - t.out[0], t.out[3] - t.out[2], 3), (slice(t.out[0], t.out[1]), slice(t.out[2], t.out[3])))
                            for i, t in enumerate(mine)]

        frames = {}                                     # device index -> (the frame there, the event behind its copy)
        _lanes.run_shares(lanes, shares, gather, canvas, frames, copy, run_share)
        host = torch.empty(canvas.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(canvas, non_blocking=True)
        main.synchronize()                              # every lane and copy is behind it (run_shares' join)
        del frames                                      # (read by every lane of their device: freed only now)
        self._check_range()
        return host.numpy()

    def post_process(self):
        if self.mod_scale is not None:
            _, _, h, w = self.output.size()
            self.output = self.output[:, :, 0:h - self.mod_pad_h * self.scale, 0:w - self.mod_pad_w * self.scale]
        if self.pre_pad != 0:
            _, _, h, w = self.output.size()
            self.output = self.output[:, :, 0:h - self.pre_pad * self.scale, 0:w - self.pre_pad * self.scale]
        return self.output

    def _run(self):
        one_tile = self.tile_size > 0 and self.img.shape[2] <= self.tile_size and self.img.shape[3] <= self.tile_size
        if self.tile_size > 0 and not (one_tile and self.img.shape[0] == 1 and self._band_plan(self.img) is not None):
            self.tile_process()
        else:
            self.process()
        return self.post_process()

    # ------------------------------------------------------------------ enhance
    def _hip_model(self):
        """The network runs in libnesr_hip.so (RRDBNet or SRVGGNetCompact): the fused 8-bit, on-device and replica paths apply.
        The RRDB-only paths (ragged batches, the strip kernel, preferred batch sizes, the declared-scale fix) test RRDBNet."""
        return isinstance(self.model, (RRDBNet, SRVGGNetCompact))

    def _one_evaluation(self, h, w, tiled=False):
        """A h x w frame is a single network evaluation: no tiling, pre_pad or mod-pad (`tiled`: one per tile, it may need tiling)."""
        ms = {2: 2, 1: 4}.get(self.scale, 1)        # _pad_on_device's mod-pad: 2 for scale 2, 4 for scale 1
        fits = not (self.tile_size > 0 and (h > self.tile_size or w > self.tile_size))
        return (tiled or fits) and self.pre_pad == 0 and h % ms == 0 and w % ms == 0

    def _three_channel_hip(self):
        """A HIP model on cuda of three channels in and out whose output is `scale` times its input."""
        return (self._hip_model() and self.device.type == "cuda" and self.model.num_in_ch == 3 and self.model.num_out_ch == 3
                and self.model.out_scale() == self.scale)

    def _fused_u8_ok(self, img):
        """The fused u8 kernel path applies when the call reduces to one network evaluation of a
        plain 8-bit BGR frame: no tiling needed, no pre_pad / mod_pad, HIP-backed model."""
        return self._u8_on_device_ok(img) and self._one_evaluation(*img.shape[:2]) and self._three_channel_hip()

    def _u8_on_device_ok(self, img):
        """8-bit BGR frames on the HIP backend (any tiling / padding): the uint8 frame is uploaded
        (4x fewer bytes than float), normalised, padded, tiled, clamped and quantised on the GPU with
        the same float32 operations enhance() performs in numpy, and only uint8 comes back."""
        return (self._hip_model() and self.device.type == "cuda" and (img.dtype == torch.uint8 if isinstance(img, torch.Tensor) else img.dtype == np.uint8)
                and img.ndim == 3 and img.shape[2] == 3)

    def _u8_tiles_fused_ok(self, h, w):
        """8-bit frames larger than a tile whose tiles run as ragged batches (bf16, strip kernel): cut and paste are one launch
        each and the float canvas of the frame never exists.  Frames that need the reflect pre-pad / mod-pad keep the general path."""
        return (self.tile_size > 0 and self._one_evaluation(h, w, tiled=True) and isinstance(self.model, RRDBNet)
                and self.model.compute_dtype in RAGGED_FORMS and self.model.strip_kernel_active() and self.ragged_tiles is None
                and self.model.out_scale() == self.scale)

    @torch.no_grad()
    def tiles_u8_on_device(self, frame_u8, windows, pastes, dst_u8, slot=0):
        """frame_u8 [H, W, 3] uint8 on the device; windows [(y0, x0, h, w)] of the padded tiles; pastes [(crop_y, crop_x, h, w, dst byte
        offset, dst row pitch)] -> the tiles' quantised centres in dst_u8 (uint8, on the device).  Ragged batches of at most
        RAGGED_MAX tiles: cut (nesr_cut_tiles_u8), forward_ragged on context replica `slot`, paste (nesr_paste_tiles_u8)."""
        from .rrdbnet import cut_tiles_u8, paste_tiles_u8
        cap = self._ragged_cap()
        for i in range(0, len(windows), cap):
            win, pst = windows[i:i + cap], pastes[i:i + cap]
            hs, ws = max(v[2] for v in win), max(v[3] for v in win)
            x = cut_tiles_u8(frame_u8, win, (hs, ws), flip_rgb=True, through_fp16=bool(self.half))
            out = self.model.forward_ragged(x, [(v[2], v[3]) for v in win], slot=slot)
            paste_tiles_u8(out, pst, dst_u8, flip_rgb=True, round_nearest=True, through_fp16=bool(self.half))

    @torch.no_grad()
    def _enhance_u8_tiles_fused(self, img, resize_to=None, keep=False):
        if self._multi():
            out = self._enhance_u8_tiles_fused_devices(img)
            return out if resize_to is None else self._resize_on_host_route(out, resize_to)
        h, w = img.shape[:2]
        s = self.scale
        frame = self._upload_u8(img)                                                 # H2D: uint8 HWC BGR
        canvas = torch.empty((h * s, w * s, 3), dtype=torch.uint8, device=self.device)
        tiles = [_tiling.Tile(i, *g) for i, g in enumerate(self.tile_grid(h, w))]
        self.tiles_u8_on_device(frame, _tiling.windows(tiles), _tiling.canvas_pastes(tiles, w * s), canvas)
        if resize_to is not None:
            canvas = self._resize_u8_on_device(canvas, resize_to)
        if keep:
            return canvas
        host = torch.empty(canvas.shape, dtype=torch.uint8, pin_memory=True)          # (the caching host allocator recycles these)
        self._frame_to_host(canvas, host)
        torch.cuda.current_stream(self.device).synchronize()
        self._check_range()
        return host.numpy()

    @torch.no_grad()
    def _enhance_u8_on_device(self, img, resize_to=None, keep=False):
        """resize_to = (out_h, out_w): enhance(outscale=...)'s Lanczos resize, on the device before the one device-to-host copy.
        keep: the quantised frame stays on the device and is returned as a tensor (_enhance_once)."""
        if self._u8_tiles_fused_ok(img.shape[0], img.shape[1]) and (img.shape[0] > self.tile_size or img.shape[1] > self.tile_size):
            return self._enhance_u8_tiles_fused(img, resize_to, keep)
        x = self._upload_u8(img)                                                   # H2D: uint8 HWC BGR
        x = normalize_u8_on_device(x.permute(2, 0, 1).flip(0)).unsqueeze(0)          # BGR->RGB, /255 (f32), HWC->NCHW
        self._pad_on_device(x)
        out = self._run()                                                            # [1,3,H*s,W*s] RGB
        out = out.data.squeeze(0).float().clamp_(0, 1)
        q = (out.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8)           # RGB->BGR, CHW->HWC, x255, round
        q = q.contiguous()
        if resize_to is not None:
            q = self._resize_u8_on_device(q, resize_to)
        if keep:
            return q
        host = self._frame_to_host(q).numpy()
        self._check_range()
        return host

    def _upload_u8(self, img):
        """The upload at the head of the 8-bit routes.  A frame that was born on the device (enhance_file: decoded there from the
        file's bytes) is a uint8 tensor already and passes through."""
        if isinstance(img, torch.Tensor):
            return img.contiguous()
        return torch.from_numpy(np.ascontiguousarray(img)).to(self.device)

    @staticmethod
    def _frame_to_host(t, host=None):
        """The device-to-host copy of a finished 8-bit frame on the enhance() routes (one per call; the tests count them here)."""
        if host is None:
            return t.cpu()
        host.copy_(t, non_blocking=True)
        return host

    @staticmethod
    def _resize_u8_on_device(frame, size):
        from . import imgproc
        return imgproc.lanczos4_resize(frame, size[0], size[1])

    def _resize_on_host_route(self, output, size):
        """enhance(outscale=...) for a frame that is on the host already (the float route: 16 bit, gray, alpha; several devices):
        upload, imgproc.lanczos4_resize, download.  8-bit frames take the HIP kernel, which is bit for bit the torch chain.  16-bit
        frames keep the torch chain: the uint16 kernel sums in oracle/cv2_ref.py's order (k ascending) and the chain in torch's, so
        the kernel would move enhance()'s 16-bit results by one LSB where a sum lands next to a half."""
        from . import imgproc
        is8 = output.dtype == np.uint8
        t = torch.from_numpy(np.ascontiguousarray(output if is8 else output.astype(np.int32))).to(self.device)
        t = t[:, :, None] if t.dim() == 2 else t
        r = imgproc.lanczos4_resize(t, size[0], size[1], use_hip=None if HIP_RESIZE and is8 else False).cpu().numpy().astype(output.dtype)
        return r[:, :, 0] if output.ndim == 2 else r

    def _check_range(self, slot=None):
        """After a device-to-host copy: an out-of-range forward of the f16-pair fp32 form raises here."""
        if self._hip_model():
            self.model.check_range(slot)

    def _forward_u8_to_host(self, img, device, slot):
        """A frame in flight: an 8-bit BGR frame through forward_u8 on `device`'s context replica `slot`, enqueued on the current
        stream -- pinned upload, network, copy into the pinned host tensor that is returned."""
        x = torch.from_numpy(np.ascontiguousarray(img)).pin_memory().to(device, non_blocking=True)
        y = self.model.forward_u8(x, flip_rgb=True, round_nearest=True, slot=slot)
        host = torch.empty(y.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(y, non_blocking=True)
        return host

    @torch.no_grad()
    def enhance_many(self, imgs, inflight=4):
        """``[self.enhance(img) for img in imgs]`` with up to `inflight` frames on the GPU at once.

        Not part of upstream's API: a frame whose network layers are only a few hundred workgroups (512x512:
        256-512 per layer in one round, all in the same phase) leaves the GPU idle a third of the time; a second frame on its own HIP
        stream and context replica fills it (bench.py's default `value`: 134 -> 160 / 167 / 170 MP/s with 2 / 3 / 4 frames
        in flight, no more beyond).  Gray, BGRA and 16-bit frames that need no tiling or padding join the frames in flight
        (_frame_in_flight), in any mix; a list with a frame that needs tiling or padding is processed one frame at a time.
        The results are identical to enhance()'s.  Errors: see _InFlight."""
        from .frame_io import frame_to_numpy
        imgs = list(imgs)
        if self._multi() and imgs and all(self._fused_u8_ok(i) for i in imgs):
            return self._enhance_many_devices(imgs, max(1, int(inflight)))
        if inflight <= 1 or not imgs or not all(self._fused_u8_ok(i) or self._frame_inflight_ok(i) for i in imgs):
            return [self.enhance(i) for i in imgs]
        streams = [torch.cuda.Stream(self.device) for _ in range(inflight)]
        caller = torch.cuda.current_stream(self.device)
        for st in streams:
            st.wait_stream(caller)     # the context workspaces (slot 0 is the caller's own) may still be in use there
        results = [None] * len(imgs)

        def finish(idx, host, mode):
            with torch.cuda.stream(streams[idx % inflight]):
                self._check_range(idx % inflight)
            results[idx] = (frame_to_numpy(host).copy(), mode)

        queue = _InFlight(finish)
        for i, img in enumerate(imgs):
            queue.collect(leave=inflight - 1)
            k = i % inflight
            with torch.cuda.stream(streams[k]):
                if self._fused_u8_ok(img):
                    host, mode = self._forward_u8_to_host(img, self.device, k), "RGB"
                else:
                    host, mode = self._frame_in_flight(img, "realesrgan", k)
                queue.add(i, host, mode)
        queue.collect()
        for st in streams:
            caller.wait_stream(st)
        return results

    @torch.no_grad()
    def _enhance_many_devices(self, imgs, inflight):
        """enhance_many over `devices`: frame i to entry i % n, up to `inflight` frames in flight per entry, each on a stream of
        its own and context replica occurrence * inflight + k of its device (k = the frame's place among the entry's in
        flight).  Results in input order.  A frame whose persistent launch gave up is evaluated again by enhance(); after a
        range error the frames still in flight are waited for and their contexts cleared before it is raised."""
        n = len(self.devices)
        lanes = []
        for dev, o in _lanes.lane_slots(self.devices):
            caller = torch.cuda.current_stream(dev)
            sts = [torch.cuda.Stream(dev) for _ in range(inflight)]
            for st in sts:
                st.wait_stream(caller)     # the context workspaces may still be in use there
            lanes.append((dev, o, sts))
        results = [None] * len(imgs)

        def check(dev, slot, st):
            with torch.cuda.device(dev), torch.cuda.stream(st):
                self.model.check_range(slot, device=dev)

        def finish(idx, host, *where):
            try:
                check(*where)
            except NesrHipError as e:
                if not _is_gave_up(e):
                    raise
                warnings.warn(f"{e}; evaluating the frame again")
                for ev, *_ in queue.pending:   # enhance() takes the first device's slot 0, which a frame in flight may hold
                    ev.synchronize()
                results[idx] = self.enhance(imgs[idx])
                return
            results[idx] = (host.numpy().copy(), "RGB")

        queue = _InFlight(finish)
        try:
            for i, img in enumerate(imgs):
                queue.collect(leave=inflight * n - 1)
                dev, o, sts = lanes[i % n]
                k = (i // n) % inflight
                st, slot = sts[k], o * inflight + k
                with torch.cuda.device(dev), torch.cuda.stream(st):
                    queue.add(i, self._forward_u8_to_host(img, dev, slot), dev, slot, st)
            queue.collect()
        except NesrHipError:
            for ev, _, _, *where in queue.pending:   # the next frame starts clean on every device
                ev.synchronize()
                try:
                    check(*where)
                except NesrHipError:
                    pass
            raise
        finally:
            for dev, _, sts in lanes:
                for st in sts:
                    torch.cuda.current_stream(dev).wait_stream(st)
        return results

    # ------------------------------------------------------------------ gray, BGRA and 16-bit frames on the device
    def _device_frame_ok(self, img):
        """A frame enhance_float would take (gray, BGRA, 16 bit; 8-bit BGR has routes of its own) on a HIP model of three channels
        in and out whose output is `scale` times its input: the frame stays on the device (_enhance_frame_on_device)."""
        if isinstance(img, torch.Tensor):       # enhance_file's / enhance_image_file's frame, on the device: uint8, or int16 carrying uint16
            return (DEVICE_FRAMES and self._three_channel_hip() and img.dtype in (torch.uint8, torch.int16) and img.numel() != 0
                    and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (3, 4))))
        return (DEVICE_FRAMES and self._three_channel_hip() and isinstance(img, np.ndarray) and img.dtype in (np.uint8, np.uint16)
                and img.size != 0 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (3, 4))))

    @staticmethod
    def _frame_kind(img):
        """(max_range, img_mode) as enhance_float decides them on the host: a frame whose maximum is at most 256 counts as 8-bit
        range whatever its dtype (a uint16 frame that dark comes back as uint8), the mode follows the shape."""
        if isinstance(img, torch.Tensor):       # a frame decoded on the device: the maximum is a device reduction, 4 bytes come home
            max_range = 65535 if img.dtype == torch.int16 and int((img.to(torch.int32) & 0xFFFF).max().item()) > 256 else 255
        else:
            max_range = 65535 if np.max(img) > 256 else 255
        return max_range, "L" if img.ndim == 2 else ("RGBA" if img.shape[2] == 4 else "RGB")

    def _frame_inflight_ok(self, img):
        """enhance_many: a frame of _device_frame_ok's kinds that is one network evaluation per plane set (no tiling, pre_pad or
        mod-pad), so it can run on a stream and context replica of its own."""
        return (not self._multi() and self._device_frame_ok(img) and not self._u8_on_device_ok(img)
                and self._one_evaluation(*img.shape[:2]))

    def _frame_through(self, img, frame, alpha_upsampler, net):
        """`frame` (img's own bytes on the device) -> (the quantised result on the device, img_mode): frame_io.pack_frame normalises,
        replicates or flips it, `net` ([1,3,H,W] -> float32 [1,3,H*s,W*s]) evaluates the colour planes and then the alpha plane (a
        plain alpha upsampler: imgproc.linear_resize_f32 to the colour output's size, which is img's times `scale`, _device_frame_ok
        having out_scale() == scale), frame_io.unpack_frame clamps, flips, takes the gray value and quantises: enhance_float's bits."""
        from . import frame_io, imgproc
        max_range, img_mode = self._frame_kind(img)
        plain = img_mode == "RGBA" and alpha_upsampler != "realesrgan"
        x, a = frame_io.pack_frame(frame, max_range, alpha="linear" if plain else "network", through_fp16=bool(self.half))
        out = net(x)
        if a is not None:   # upstream's plain upsampler: cv2.resize(alpha, (w * scale, h * scale), interpolation=cv2.INTER_LINEAR)
            a = imgproc.linear_resize_f32(a, out.shape[2], out.shape[3], use_hip=None if HIP_RESIZE else False) if plain else net(a)
        q = frame_io.unpack_frame(out, {"L": 1, "RGB": 3, "RGBA": 4}[img_mode], max_range, alpha=a, through_fp16=bool(self.half))
        return q, img_mode

    @torch.no_grad()
    def _frame_in_flight(self, img, alpha_upsampler, slot):
        """enhance() of a _frame_inflight_ok frame, enqueued on the current stream with context replica `slot`: returns (the pinned
        host tensor the result is being copied into, img_mode).  The caller waits for the stream and calls _check_range(slot)."""
        from . import frame_io
        frame = frame_io.frame_to_tensor(img).pin_memory().to(self.device, non_blocking=True)
        q, img_mode = self._frame_through(img, frame, alpha_upsampler,
                                          lambda t: self.model(t.half() if self.half else t, slot=slot).float())
        host = torch.empty(q.shape, dtype=q.dtype, pin_memory=True)
        host.copy_(q, non_blocking=True)
        return host, img_mode

    @torch.no_grad()
    def _enhance_frame_on_device(self, img, resize_to=None, alpha_upsampler="realesrgan", keep=False):
        """enhance() for the frames enhance_float takes, without its host passes: the uint8 / uint16 frame is uploaded as it is
        and goes through _frame_through, where _pad_on_device and _run() evaluate it as they do for every frame (padding, tiles,
        ragged batches, devices= lanes; a second time for the alpha plane); outscale's resize follows (resize_to), and one copy
        brings the finished frame home."""
        from . import frame_io, imgproc

        def net(t):
            self._pad_on_device(t)
            return self._run().float()                                                  # [1,3,H*s,W*s] RGB (fp16 upstream when half)

        frame = img.contiguous() if isinstance(img, torch.Tensor) else frame_io.frame_to_tensor(img, self.device)   # H2D: the frame's own bytes
        q, img_mode = self._frame_through(img, frame, alpha_upsampler, net)
        if resize_to is not None:
            q3 = q[:, :, None] if q.dim() == 2 else q
            if q.dtype == torch.uint8:
                q3 = self._resize_u8_on_device(q3, resize_to) if HIP_RESIZE else imgproc.lanczos4_resize(q3, resize_to[0], resize_to[1], use_hip=False)
            else:       # 16 bit keeps the torch chain, for the reason given at _resize_on_host_route
                q3 = imgproc.lanczos4_resize(q3.to(torch.int32) & 0xFFFF, resize_to[0], resize_to[1], use_hip=False).to(torch.int16)
            q = q3[:, :, 0] if q.dim() == 2 else q3
        if keep:
            return q, img_mode
        host = frame_io.frame_to_numpy(self._frame_to_host(q.contiguous()))
        self._check_range()
        return host, img_mode

    @torch.no_grad()
    def enhance_float(self, img, alpha_upsampler="realesrgan"):
        """Everything of enhance() up to (not including) quantisation: returns (HWC float32 in
        [0,1] in BGR(A)/gray order, img_mode, max_range)."""
        img = img.astype(np.float32)
        if np.max(img) > 256:  # 16-bit image
            max_range = 65535
        else:
            max_range = 255
        img = img / max_range
        if len(img.shape) == 2:  # gray image
            img_mode = "L"
            img = _gray2rgb(img)
        elif img.shape[2] == 4:  # RGBA image with alpha channel
            img_mode = "RGBA"
            alpha = img[:, :, 3]
            img = img[:, :, 0:3][:, :, ::-1]
            if alpha_upsampler == "realesrgan":
                alpha = _gray2rgb(alpha)
        else:
            img_mode = "RGB"
            img = img[:, :, ::-1]

        def through_network(planes):        # HWC float32 RGB -> the network's output as HWC float32 BGR in [0,1], on the host
            self.pre_process(np.ascontiguousarray(planes))
            out = self._run().data.squeeze().float().cpu().clamp_(0, 1).numpy()
            self._check_range()
            return np.transpose(out[[2, 1, 0], :, :], (1, 2, 0))

        output_img = through_network(img)
        if img_mode == "L":
            output_img = _bgr2gray(output_img)

        if img_mode == "RGBA":
            if alpha_upsampler == "realesrgan":
                output_alpha = _bgr2gray(through_network(alpha))
            else:   # upstream: cv2.resize(alpha, (w * scale, h * scale), interpolation=cv2.INTER_LINEAR)
                from . import imgproc
                h, w = alpha.shape[0:2]
                a = torch.from_numpy(np.ascontiguousarray(alpha)).to(self.device)
                output_alpha = imgproc.linear_resize_f32(a, h * self.scale, w * self.scale, use_hip=None if HIP_RESIZE else False).cpu().numpy()
            output_img = np.concatenate([output_img, output_alpha[:, :, None]], axis=2)
        return output_img, img_mode, max_range

    @torch.no_grad()
    def enhance(self, img, outscale=None, alpha_upsampler="realesrgan"):
        """img: HWC uint8/uint16 BGR | BGRA | gray ndarray -> (ndarray of the same kind, upscaled; img_mode).

        A forward whose persistent dense-block launch gave up waiting (another process's kernels kept its workgroups off the
        device: NesrHipError from the status check, never a silently wrong image) is evaluated once more: the context has
        switched to per-layer launches by then (include/nesr_hip.h, nesr_set_fused)."""
        return self._again_if_gave_up(lambda: self._enhance_once(img, outscale, alpha_upsampler))

    @staticmethod
    def _again_if_gave_up(evaluate):
        try:
            return evaluate()
        except NesrHipError as e:
            if not _is_gave_up(e):
                raise
            warnings.warn(f"{e}; evaluating the frame again with per-layer launches")
            return evaluate()

    @torch.no_grad()
    def enhance_jpeg(self, img, quality=95, outscale=None, alpha_upsampler="realesrgan", *, sampling="4:2:0", optimize=False, restart_interval=0):
        """enhance() followed by cv2.imwrite(path.jpg, output) (standalone/direct_esrgan.py:163-169), the file as bytes:
        (bytes, img_mode).  The quantised frame of enhance()'s route stays on the device and is encoded there
        (imgproc.encode_jpeg_u8: csrc/jpeg.hip); only the file comes home.  The bytes are those of the JPEG file of enhance(img)'s
        frame.  8-bit BGR and gray frames; a BGRA or 16-bit frame raises ValueError (cv2.imwrite would drop the alpha plane or the
        depth without a word).  sampling, optimize, restart_interval: imgproc.encode_jpeg_u8's (cv2's IMWRITE_JPEG_SAMPLING_FACTOR,
        IMWRITE_JPEG_OPTIMIZE, IMWRITE_JPEG_RST_INTERVAL)."""
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
            kind = f"{getattr(img, 'dtype', type(img).__name__)} {tuple(getattr(img, 'shape', ()))}"
            raise ValueError(f"enhance_jpeg: an 8-bit BGR [H, W, 3] or gray [H, W] frame, got {kind} (a JPEG file holds neither alpha nor 16 bits)")
        return self._enhance_to_jpeg(img, quality, outscale, alpha_upsampler, sampling=sampling, optimize=optimize, restart_interval=restart_interval)

    def _enhance_to_jpeg(self, img, quality, outscale, alpha_upsampler, **options):
        from . import imgproc

        def evaluate():
            q, img_mode = self._enhance_once(img, outscale, alpha_upsampler, keep=True)
            if not isinstance(q, torch.Tensor):          # a route that assembles its frame on the host (several devices, no HIP model)
                q = torch.from_numpy(np.ascontiguousarray(q)).to(self.device)
            data = imgproc.encode_jpeg_u8(q, quality, order="bgr", **options)
            self._check_range()                          # after the copy that waited for the stream, as enhance() does
            return data, img_mode

        return self._again_if_gave_up(evaluate)

    @torch.no_grad()
    def enhance_png(self, img, outscale=None, alpha_upsampler="realesrgan"):
        """enhance() followed by cv2.imwrite(path.png, output) (standalone/superres_project.py:203-206; standalone/direct_esrgan.py:169
        for a PNG input), the file as bytes: (bytes, img_mode).  Every frame kind enhance() takes -- gray, BGR, BGRA, 8 and 16 bit: the
        ones enhance_jpeg has to refuse.  The quantised frame of enhance()'s route stays on the device and is encoded there
        (imgproc.encode_png: csrc/png.hip); only the file comes home.  The file is lossless: it decodes to exactly enhance(img)'s
        frame (in R G B (A) order, as every PNG file holds it)."""
        if not isinstance(img, (np.ndarray, torch.Tensor)) or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (3, 4))):
            kind = f"{getattr(img, 'dtype', type(img).__name__)} {tuple(getattr(img, 'shape', ()))}"
            raise ValueError(f"enhance_png: a gray [H, W], BGR [H, W, 3] or BGRA [H, W, 4] frame, got {kind}")
        return self._enhance_to_png(img, outscale, alpha_upsampler)

    def _enhance_to_png(self, img, outscale, alpha_upsampler):
        from . import frame_io, imgproc

        def evaluate():
            q, img_mode = self._enhance_once(img, outscale, alpha_upsampler, keep=True)
            if not isinstance(q, torch.Tensor):          # a route that assembles its frame on the host (several devices, no HIP model)
                q = frame_io.frame_to_tensor(np.ascontiguousarray(q), self.device)
            data = imgproc.encode_png(q, order="bgr")
            self._check_range()                          # after the copy that waited for the stream, as enhance() does
            return data, img_mode

        return self._again_if_gave_up(evaluate)

    def _read_jpeg(self, data_or_path, who):
        """The head of enhance_file: the file's bytes (or the file at a path) -> the BGR (or gray) uint8 frame, decoded on the wrapper's
        device (imgproc.decode_jpeg_u8: csrc/jpeg_decode.hip) and left there for the routes that start with an upload; the routes that
        assemble their frame on the host (devices=[...], a model that is not a HIP one, a CPU device) get it copied home once."""
        from . import imgproc
        if isinstance(data_or_path, (bytes, bytearray, memoryview)):
            data = bytes(data_or_path)
        else:
            with open(data_or_path, "rb") as f:
                data = f.read()
        if data[:2] != b"\xff\xd8":
            raise ValueError(f"{who}: not a JPEG file (it does not start with SOI); no other format is decoded on the device")
        frame = imgproc.decode_jpeg_u8(data, order="bgr", device=self.device)
        if self._multi() or not (self._u8_on_device_ok(frame) or self._device_frame_ok(frame)):
            return frame.cpu().numpy()
        return frame

    def _read_image(self, data_or_path, who):
        """_read_jpeg for a JPEG or a PNG file, told apart by signature -> (frame, "jpeg" | "png").  A PNG file gives IMREAD_UNCHANGED's
        frame (imgproc.decode_png: csrc/png_decode.hip): gray stays [H, W], alpha is kept, 16 bit stays 16 bit -- on the device as uint8
        or as int16 carrying the uint16 pattern, on the host (the routes that assemble there) as uint8 / uint16."""
        from . import frame_io, imgproc
        if isinstance(data_or_path, (bytes, bytearray, memoryview)):
            data = bytes(data_or_path)
        else:
            with open(data_or_path, "rb") as f:
                data = f.read()
        if data[:2] == b"\xff\xd8":
            return self._read_jpeg(data, who), "jpeg"
        if data[:8] != b"\x89PNG\r\n\x1a\n":
            raise ValueError(f"{who}: neither a JPEG file (SOI) nor a PNG file (signature)")
        frame = imgproc.decode_png(data, order="bgr", device=self.device)
        if self._multi() or not (self._u8_on_device_ok(frame) or self._device_frame_ok(frame)):
            return frame_io.frame_to_numpy(frame.cpu()), "png"
        return frame, "png"

    @torch.no_grad()
    def enhance_image_file(self, data_or_path, outscale=None, alpha_upsampler="realesrgan"):
        """enhance(cv2.imread(path, cv2.IMREAD_UNCHANGED)) for a JPEG or a PNG file given as bytes or as a path
        (standalone/direct_esrgan.py:130): (ndarray, img_mode), bit for bit enhance() of the host-decoded frame.  The file's bytes go
        up (a PNG of one deflate stream: its inflated stream), the frame is born on the device and handed to enhance()'s routes as a
        device tensor.  enhance_file* stay JPEG-only."""
        img, _ = self._read_image(data_or_path, "enhance_image_file")
        return self._again_if_gave_up(lambda: self._enhance_once(img, outscale, alpha_upsampler))

    @torch.no_grad()
    def enhance_image_file_to(self, data_or_path, fmt=None, quality=95, outscale=None, alpha_upsampler="realesrgan", *, sampling="4:2:0", optimize=False,
                              restart_interval=0):
        """enhance_image_file followed by cv2.imwrite, the file as bytes: (bytes, img_mode).  fmt=None writes the input's own format
        (standalone/direct_esrgan.py:130,169: read unchanged, write with the input's extension); "png" or "jpeg" force one.  A JPEG
        file of an alpha or 16-bit frame is enhance_jpeg's ValueError.  sampling, optimize, restart_interval: enhance_jpeg's, for a
        JPEG file (a PNG file has none of them)."""
        if fmt not in (None, "png", "jpeg"):
            raise ValueError(f"enhance_image_file_to: fmt must be None, 'png' or 'jpeg', got {fmt!r}")
        img, kind = self._read_image(data_or_path, "enhance_image_file_to")
        if (fmt or kind) == "png":
            return self._enhance_to_png(img, outscale, alpha_upsampler)
        if img.dtype not in (np.uint8, torch.uint8) or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
            raise ValueError(f"enhance_image_file_to: a JPEG file holds neither alpha nor 16 bits, the frame is {img.dtype} {tuple(img.shape)}")
        return self._enhance_to_jpeg(img, quality, outscale, alpha_upsampler, sampling=sampling, optimize=optimize, restart_interval=restart_interval)

    @torch.no_grad()
    def enhance_file(self, data_or_path, outscale=None, alpha_upsampler="realesrgan"):
        """enhance(cv2.imread(path, cv2.IMREAD_UNCHANGED)) for a JPEG file given as bytes or as a path (the reference reads with
        cv2.imread, standalone/direct_esrgan.py:130): (ndarray, img_mode).  The file's bytes go up, the frame is decoded on the device
        and handed to enhance()'s routes as a device tensor: the decoded frame never crosses the bus.  EXIF orientation is not
        applied and a gray file stays gray (IMREAD_UNCHANGED; cv2.imread's default flag would rotate and give three channels).
        Anything but a JPEG file raises ValueError."""
        img = self._read_jpeg(data_or_path, "enhance_file")
        return self._again_if_gave_up(lambda: self._enhance_once(img, outscale, alpha_upsampler))

    @torch.no_grad()
    def enhance_file_jpeg(self, data_or_path, quality=95, outscale=None, alpha_upsampler="realesrgan", *, sampling="4:2:0", optimize=False, restart_interval=0):
        """enhance_file followed by cv2.imwrite(path.jpg, output), the file as bytes: (bytes, img_mode).  File bytes in, file bytes out;
        nothing else crosses the bus.  sampling, optimize, restart_interval: enhance_jpeg's."""
        return self._enhance_to_jpeg(self._read_jpeg(data_or_path, "enhance_file_jpeg"), quality, outscale, alpha_upsampler, sampling=sampling,
                                     optimize=optimize, restart_interval=restart_interval)

    @torch.no_grad()
    def enhance_file_png(self, data_or_path, outscale=None, alpha_upsampler="realesrgan"):
        """enhance_file followed by cv2.imwrite(path.png, output), the file as bytes: (bytes, img_mode).  A JPEG file's bytes in, a
        lossless PNG file's bytes out (standalone/superres_project.py:203-206 names its result .png whatever it read); nothing else
        crosses the bus."""
        return self._enhance_to_png(self._read_jpeg(data_or_path, "enhance_file_png"), outscale, alpha_upsampler)

    def _enhance_once(self, img, outscale=None, alpha_upsampler="realesrgan", keep=False):
        """keep: the routes that hold the finished frame on the device return it there (a uint8 tensor, not yet range-checked)
        instead of copying it home; the others return their ndarray as always."""
        if self.last_bands is not None:
            self.last_bands = None
        h_input, w_input = img.shape[0:2]
        plain_alpha = alpha_upsampler != "realesrgan" and img.ndim == 3 and img.shape[2] == 4
        # upstream: cv2.resize(output, (int(w_input * outscale), int(h_input * outscale)), interpolation=cv2.INTER_LANCZOS4);
        # here OpenCV's algorithm restated on the device (imgproc.lanczos4_resize: PARITY UNPINNED, cv2 is not installed)
        resize_to = None
        if outscale is not None and outscale != float(self.scale):
            resize_to = (int(h_input * outscale), int(w_input * outscale))
        on_device = resize_to if HIP_RESIZE else None     # the 8-bit routes resize before their one device-to-host copy
        kept = {"keep": True} if keep else {}            # (left out otherwise: the routes are called as they always were)

        if self._fused_u8_ok(img) and not plain_alpha:
            # /255, BGR->RGB, network, clamp, RGB->BGR, x255, round -- all inside the HIP path
            x = self._upload_u8(img)
            plan = self._band_plan(x)
            if plan is None:
                y = self.model.forward_u8(x, flip_rgb=True, round_nearest=True)
            else:           # row bands over `devices`: byte for byte forward_u8's frame
                y = self.model.forward_banded_u8(x, plan[0], flip_rgb=True, round_nearest=True)
                self.last_bands = plan[1]
            if on_device is not None:
                y = self._resize_u8_on_device(y, on_device)
            if keep:
                output = y
            else:
                output = self._frame_to_host(y).numpy()
                self._check_range(0 if plan is None else None)     # (banded: every lane's context before the frame is used)
            img_mode = "RGB"
            done = on_device is not None
        elif self._u8_on_device_ok(img):
            output = self._enhance_u8_on_device(img, on_device, **kept)
            img_mode = "RGB"
            done = on_device is not None
        elif self._device_frame_ok(img):
            output, img_mode = self._enhance_frame_on_device(img, resize_to, alpha_upsampler, **kept)
            done = resize_to is not None
        else:
            output_img, img_mode, max_range = self.enhance_float(img, alpha_upsampler)
            if max_range == 65535:  # 16-bit image
                output = (output_img * 65535.0).round().astype(np.uint16)
            else:
                output = (output_img * 255.0).round().astype(np.uint8)
            done = False

        if resize_to is not None and not done:
            if isinstance(output, torch.Tensor):
                output = output.cpu().numpy()
            output = self._resize_on_host_route(output, resize_to)
        return output, img_mode
