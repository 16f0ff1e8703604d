"""GPU versions of the NESR pipeline's ESRGAN call sites (SURVEY.md section 8(a) rows a16-a19,
section 8(f) row 2): everything between "HWC uint8 RGB ndarray in" and "HWC uint8 RGB ndarray out"
runs on the device -- 12-channel synthesis, the network (``upscaler.model``, the reference's own way of
calling it), the truncating quantiser, and the NESR tiler with its Lanczos resize.

Reference (all in nesr/nesr.py):
  _apply_esrgan                 :754-843   dispatch by megapixels / device, 12-ch vs 3-ch, tiling
  _apply_esrgan_12channel       :845-903   [img, clamp(1.1 img), clamp(0.9 img), GaussianBlur3x3(img)] -> model
  _apply_esrgan_3channel        :905-945   img repeated 4x -> model
  _process_with_tiling          :311-475   ceil grid, +-padding windows, crop, Lanczos resize to the canvas
  enhance_image's loop          :516-633   pre-filter, mask stage, the upscalers, ensemble or bicubic step, post-filter (enhance_iterations)

Differences, on purpose: no exception ladder (nesr.py:815-843, 448-473 turn any backend failure into a
bicubic result -- here failures raise), no MPS branches, no probe tile (nesr.py:349-357 runs the
processor on a 256x256 corner and discards the result).

On a ROCm device with the HIP RRDBNet(num_in_ch=12) the stage is one call of the C ABI, u8 frame in, u8 frame out
(`use_hip=None`, the default: nesr_forward_nesr_u8 for one window, nesr_apply_esrgan_u8 for a frame with its tiler; csrc/nesr12.hip,
csrc/nesr_stage_api.cpp) -- no [1,12,H,W] float input, no float output, no Python tile loop.  `use_hip=False` keeps the torch
chains below, which are the specification, the CPU-side statement, and what the C entries equal bit for bit.

cv2 is not available offline, so its two non-trivial image ops are restated, PARITY UNPINNED:
  * cv2.GaussianBlur(u8, (3,3), 0): kernel [1 2 1]/4 separable, BORDER_REFLECT_101, fixed-point with
    round-half-up -> (S + 8) >> 4 on the 16-weight integer sum.
  * cv2.resize(..., INTER_LANCZOS4): cv2's coefficient formula (interpolateLanczos4), sampling geometry and 8-bit
    fixed point (coefficients x2048 as shorts, integer passes, (v + 2^21) >> 22): imgproc.lanczos4_resize.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch
from torch.nn import functional as F

from . import _lib
from .realesrganer import normalize_u8_on_device


# ----------------------------------------------------------------------------- 12-channel builder
def gaussian_blur3x3_u8(img):
    """img: uint8 [H, W, C] tensor -> uint8, cv2.GaussianBlur(img, (3, 3), 0) restated (see module doc)."""
    x = img.permute(2, 0, 1).unsqueeze(0).to(torch.int32)
    h, w = x.shape[-2:]
    if h > 1 and w > 1:
        xp = F.pad(x.float(), (1, 1, 1, 1), mode="reflect").to(torch.int32)     # BORDER_REFLECT_101
    else:
        xp = F.pad(x.float(), (1, 1, 1, 1), mode="replicate").to(torch.int32)
    hs = xp[..., :, 0:-2] + 2 * xp[..., :, 1:-1] + xp[..., :, 2:]
    s = hs[..., 0:-2, :] + 2 * hs[..., 1:-1, :] + hs[..., 2:, :]
    return ((s + 8) >> 4).clamp_(0, 255).to(torch.uint8).squeeze(0).permute(1, 2, 0)


def _u8_on(image_rgb, device):
    """HWC uint8 ndarray or tensor -> tensor on `device` (a tensor already there is used as it is: the
    iteration loop keeps its frames on the GPU)."""
    if isinstance(image_rgb, torch.Tensor):
        return image_rgb.to(device)
    return torch.as_tensor(np.ascontiguousarray(image_rgb)).to(device)


def build_12channel(image_rgb, device):
    """nesr.py:851-882: RGB u8 -> [1, 12, H, W] float32 on device
    = [bgr/255, clamp(1.1 bgr/255), clamp(0.9 bgr/255), GaussianBlur3x3(bgr)/255]."""
    bgr = _u8_on(image_rgb, device).flip(2)                                                # cv2.COLOR_RGB2BGR
    t = normalize_u8_on_device(bgr.permute(2, 0, 1))                                       # /255.0
    blurred = normalize_u8_on_device(gaussian_blur3x3_u8(bgr).permute(2, 0, 1))
    return torch.cat([t, torch.clamp(t * 1.1, 0, 1), torch.clamp(t * 0.9, 0, 1), blurred], 0).unsqueeze(0)


def build_3channel_x4(image_rgb, device):
    """nesr.py:915-927: RGB u8 -> [1, 12, H, W] = the BGR/255 image repeated 4 times."""
    bgr = _u8_on(image_rgb, device).flip(2)
    t = normalize_u8_on_device(bgr.permute(2, 0, 1))
    return torch.cat([t, t, t, t], 0).unsqueeze(0)


def quantize_trunc_to_rgb(output):
    """nesr.py:894-901: [1,3,H,W] float -> HWC uint8 RGB: x*255, clip(0,255), truncating astype, BGR->RGB."""
    out = output.squeeze(0).float()
    q = (out.permute(1, 2, 0) * 255.0).clamp_(0, 255).to(torch.uint8)
    return q.flip(2)


def _to_host(upscaler, t):
    """Device-to-host copy + the range check of the f16-pair fp32 form (a NaN image is an error here; the
    reference's np.clip(...).astype(uint8) would turn NaN pixels into garbage silently, nesr.py:897-898)."""
    host = t.cpu().numpy()
    check = getattr(upscaler.model, "check_range", None)
    if check is not None:
        check()
    return host


NET_SCALE = 4            # output / input size of RRDBNet(num_in_ch=12, scale=4), nesr.py:216
TILE_PADDING = 16        # nesr.py:797: what _apply_esrgan passes to _process_with_tiling


def _hip_stage_refusal(upscaler, image_rgb, windows):
    """Why the C entries of the stage cannot take this frame (None: they can): they want a uint8 [H, W, 3] frame bound for a ROCm
    device, the HIP RRDBNet with 12 input channels (scale 4, 3 output channels), and windows (h, w) of at least 2 x 2."""
    from .rrdbnet import RRDBNet
    m = upscaler.model
    if torch.device(upscaler.device).type != "cuda":
        return f"the upscaler's device is {upscaler.device}, not a ROCm device"
    if not (isinstance(m, RRDBNet) and m.num_in_ch == 12 and m.num_out_ch == 3 and m.scale not in (1, 2)):
        return "upscaler.model is not the HIP RRDBNet(num_in_ch=12, num_out_ch=3, scale=4)"
    dtype = image_rgb.dtype
    if dtype not in (torch.uint8, np.uint8) or len(image_rgb.shape) != 3 or image_rgb.shape[2] != 3:
        return f"the frame is {dtype} {tuple(image_rgb.shape)}, not uint8 [H, W, 3]"
    if any(h < 2 or w < 2 for h, w in windows):
        return "a window has a one-pixel side (the torch chain pads such a blur by replication)"
    return None


def _takes_hip(use_hip, upscaler, image_rgb, windows):
    if use_hip is False:
        return False
    why = _hip_stage_refusal(upscaler, image_rgb, windows)
    if use_hip and why:
        raise ValueError(f"use_hip=True: {why}")
    return why is None


def _apply_one(upscaler, image_rgb, mode, as_numpy, use_hip):
    model = upscaler.model
    model.eval()
    if _takes_hip(use_hip, upscaler, image_rgb, [image_rgb.shape[:2]]):
        q = model.forward_nesr_u8(_u8_on(image_rgb, upscaler.device), mode)
    else:
        build = build_12channel if mode == _lib.INPUT_12CH else build_3channel_x4
        q = quantize_trunc_to_rgb(model(build(image_rgb, upscaler.device)))
    return _to_host(upscaler, q) if as_numpy else q


@torch.no_grad()
def apply_esrgan_12channel(upscaler, image_rgb, as_numpy=True, use_hip=None):
    """_apply_esrgan_12channel (nesr.py:845-903) with every step on the GPU: one call of RRDBNet.forward_nesr_u8 where that
    applies (module doc), else (and with use_hip=False) build_12channel, the model, quantize_trunc_to_rgb -- the same bits."""
    return _apply_one(upscaler, image_rgb, _lib.INPUT_12CH, as_numpy, use_hip)


@torch.no_grad()
def apply_esrgan_3channel(upscaler, image_rgb, as_numpy=True, use_hip=None):
    """_apply_esrgan_3channel (nesr.py:905-945); routes as apply_esrgan_12channel."""
    return _apply_one(upscaler, image_rgb, _lib.INPUT_3CH_X4, as_numpy, use_hip)


# ----------------------------------------------------------------------------- Lanczos-4 resize
from .imgproc import lanczos4_resize as lanczos4_resize_u8   # noqa: E402  cv2.resize(INTER_LANCZOS4), OpenCV's 8-bit fixed point


# ----------------------------------------------------------------------------- NESR tiler + dispatcher
def _tile_windows(h, w, tile_size, padding, upscale_factor):
    """Per tile of _process_with_tiling's ceil grid (nesr.py:335-336), row-major: the source window y0, y1, x0, x1 (the tile grown
    by `padding`, clipped to the frame: nesr.py:370-373) and its canvas rectangle oy0, oy1, ox0, ox1 (nesr.py:400-412)."""
    nth, ntw = math.ceil(h / tile_size), math.ceil(w / tile_size)
    for i in range(nth):
        for j in range(ntw):
            y0, y1 = max(0, i * tile_size - padding), min(h, (i + 1) * tile_size + padding)
            x0, x1 = max(0, j * tile_size - padding), min(w, (j + 1) * tile_size + padding)
            oy0, oy1 = int(y0 * upscale_factor), int(y1 * upscale_factor)
            ox0, ox1 = int(x0 * upscale_factor), int(x1 * upscale_factor)
            if padding > 0:
                pu = int(padding * upscale_factor)
                if y0 > 0:
                    oy0 += pu
                if y1 < h:
                    oy1 -= pu
                if x0 > 0:
                    ox0 += pu
                if x1 < w:
                    ox1 -= pu
            yield y0, y1, x0, x1, oy0, oy1, ox0, ox1


def _tile_crop(th, tw, padding, y0, y1, x0, x1, h, w):
    """The part ty0, ty1, tx0, tx1 of a window's th x tw network output that belongs to the tile (nesr.py:414-426)."""
    sy, sx = th / (y1 - y0), tw / (x1 - x0)
    ty0 = 0 if y0 == 0 else int(padding * sy)
    ty1 = th if y1 == h else int(th - padding * sy)
    tx0 = 0 if x0 == 0 else int(padding * sx)
    tx1 = tw if x1 == w else int(tw - padding * sx)
    ty0 = max(0, min(ty0, th - 1))
    ty1 = max(ty0 + 1, min(ty1, th))
    tx0 = max(0, min(tx0, tw - 1))
    tx1 = max(tx0 + 1, min(tx1, tw))
    return ty0, ty1, tx0, tx1


def tile_plan(h, w, tile_size, padding, upscale_factor, net_scale=NET_SCALE):
    """The rectangles of process_with_tiling for a processor whose output is `net_scale` times its input, one tuple of 13 ints per
    tile: (y0, y1, x0, x1 source window | ty0, ty1, tx0, tx1 crop inside the processor's output | oy0, oy1, ox0, ox1 canvas rectangle |
    skip: 1 when the rectangle is empty).  A frame that fits one tile is one tile whose rectangle is the processor's whole output.
    nesr_stage_tile_plan (include/nesr_hip.h) returns the same table."""
    if h <= tile_size and w <= tile_size:
        return [(0, h, 0, w, 0, net_scale * h, 0, net_scale * w, 0, net_scale * h, 0, net_scale * w, 0)]
    rows = []
    for y0, y1, x0, x1, oy0, oy1, ox0, ox1 in _tile_windows(h, w, tile_size, padding, upscale_factor):
        crop = _tile_crop(net_scale * (y1 - y0), net_scale * (x1 - x0), padding, y0, y1, x0, x1, h, w)
        rows.append((y0, y1, x0, x1) + crop + (oy0, oy1, ox0, ox1, int(oy1 - oy0 <= 0 or ox1 - ox0 <= 0)))
    return rows


@torch.no_grad()
def process_with_tiling(processor, image_rgb, tile_size, padding, upscale_factor, device, as_numpy=True, use_hip=None):
    """_process_with_tiling (nesr.py:311-475): `processor(tile_rgb_u8 ndarray|tensor) -> uint8 tensor`.
    Returns an HWC uint8 RGB image of size int(h*uf) x int(w*uf) (ndarray, or the device tensor).
    A tile's region whose size differs from its place in the canvas is resized by imgproc.lanczos4_resize: on a ROCm device the
    HIP kernel reads the region inside the tile and writes the canvas rectangle in one launch (crop, resize and paste);
    use_hip=False keeps slice, torch chain and copy -- the two agree bit for bit."""
    h, w, c = image_rgb.shape
    if h <= tile_size and w <= tile_size:
        out = processor(image_rgb)
        return out.cpu().numpy() if as_numpy else out
    out_h, out_w = int(h * upscale_factor), int(w * upscale_factor)
    canvas = torch.zeros((out_h, out_w, c), dtype=torch.uint8, device=device)
    for y0, y1, x0, x1, oy0, oy1, ox0, ox1 in _tile_windows(h, w, tile_size, padding, upscale_factor):
        tile = image_rgb[y0:y1, x0:x1]
        pt = processor(tile)
        ty0, ty1, tx0, tx1 = _tile_crop(pt.shape[0], pt.shape[1], padding, y0, y1, x0, x1, h, w)
        oh, ow = oy1 - oy0, ox1 - ox0
        if oh <= 0 or ow <= 0:
            continue
        region = pt[ty0:ty1, tx0:tx1]
        if region.shape[0] != oh or region.shape[1] != ow:   # cv2.resize(..., INTER_LANCZOS4), nesr.py:438-443
            hip = use_hip if use_hip is not None else (region.device.type == "cuda" and region.dtype == torch.uint8 and c in (1, 3, 4)
                                                       and region.device == canvas.device)
            if hip:
                lanczos4_resize_u8(region, oh, ow, use_hip=True, out=canvas[oy0:oy1, ox0:ox1])
                continue
            region = lanczos4_resize_u8(region, oh, ow, use_hip=False)
        canvas[oy0:oy1, ox0:ox1] = region
    return canvas.cpu().numpy() if as_numpy else canvas


LARGE_IMAGE_MP = 16      # nesr.py:787: above this many "megapixels" (px / 1024^2) tiling and 3-channel mode are forced


def stage_route(h, w, cfg, device_kind="cuda", large_mp=LARGE_IMAGE_MP):
    """The dispatch of _apply_esrgan (nesr.py:761-793) -> (use_tiling, use_3ch); nesr_stage_route (include/nesr_hip.h) is the same."""
    megapixels = (h * w) / (1024 * 1024)
    use_tiling = False
    if cfg.get("enable_tiling", True):
        thr = {"cpu": cfg.get("cpu_megapixel_threshold", 2), "mps": cfg.get("mps_megapixel_threshold", 4)}.get(
            device_kind, cfg.get("cuda_megapixel_threshold", 8))
        use_tiling = megapixels > thr
    use_3ch = cfg.get("force_3channel", False)
    if megapixels > large_mp:
        use_tiling, use_3ch = True, True
    return use_tiling, use_3ch


def _apply_esrgan_hip(upscaler, image_rgb, mode, tiled, tile_size, upscale_factor):
    """nesr_apply_esrgan_u8 on torch's current stream: the frame's tiles, their crops and pastes in one call of the C ABI."""
    dev = torch.device(upscaler.device)
    x = _u8_on(image_rgb, dev).contiguous()
    h, w, _ = x.shape
    one = not tiled or (h <= tile_size and w <= tile_size)
    shape = (NET_SCALE * h, NET_SCALE * w, 3) if one else (int(h * upscale_factor), int(w * upscale_factor), 3)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        ctx = upscaler.model._context(x.device, 0)
        need = lib.nesr_apply_esrgan_scratch_bytes(ctx, h, w, int(tiled), int(tile_size), TILE_PADDING)
        if not need:
            _lib.check(_lib.ERR_ARG, "nesr_apply_esrgan_scratch_bytes")
        scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(lib.nesr_apply_esrgan_u8(ctx, ctypes.c_void_p(x.data_ptr()), h, w, mode, int(tiled), int(tile_size), TILE_PADDING, float(upscale_factor),
                                            ctypes.c_void_p(scratch.data_ptr()), need, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)),
                   "nesr_apply_esrgan_u8")
    return out


def apply_esrgan(upscaler, image_rgb, config=None, device_kind="cuda", as_numpy=True, trace=None, large_mp=LARGE_IMAGE_MP, use_hip=None):
    """_apply_esrgan (nesr.py:754-813): the reference's dispatch, minus its fallback ladder.
    config keys as the reference's: enable_tiling, force_3channel, max_tile_size, upscale_factor,
    cuda_megapixel_threshold (the reference's literal default for cuda is 8).  `large_mp` is the reference's
    literal 16 (a parameter only so that tests can reach that branch with small frames); `trace`, if a list,
    receives one dict describing the route taken.  use_hip=None: the whole stage as one call of the C ABI (nesr_apply_esrgan_u8)
    where it applies (module doc); use_hip=False: the torch chains and the Python tile loop; the same frame and trace either way."""
    cfg = {"enable_tiling": True, "force_3channel": False, "max_tile_size": 512, "upscale_factor": 2.0}
    cfg.update(config or {})
    h, w, _ = image_rgb.shape
    use_tiling, use_3ch = stage_route(h, w, cfg, device_kind, large_mp)
    model = upscaler.model
    calls0 = getattr(model, "calls", None)
    net_px = [0]
    # the windows the network sees (the C tiler evaluates every tile of the plan, as the loop below does)
    plan = tile_plan(h, w, cfg["max_tile_size"], TILE_PADDING, cfg["upscale_factor"]) if use_tiling else [(0, h, 0, w)]
    windows = [(r[1] - r[0], r[3] - r[2]) for r in plan]
    canvas_ok = len(plan) == 1 or (int(h * cfg["upscale_factor"]) >= 1 and int(w * cfg["upscale_factor"]) >= 1)

    def one(t):
        net_px[0] += int(t.shape[0]) * int(t.shape[1])
        return (apply_esrgan_3channel if use_3ch else apply_esrgan_12channel)(upscaler, t, as_numpy=False, use_hip=False)

    if canvas_ok and _takes_hip(use_hip, upscaler, image_rgb, windows):
        model.eval()
        out = _apply_esrgan_hip(upscaler, image_rgb, _lib.INPUT_3CH_X4 if use_3ch else _lib.INPUT_12CH, use_tiling, cfg["max_tile_size"], cfg["upscale_factor"])
        model.calls += len(plan)
        net_px[0] = sum(wh * ww for wh, ww in windows)
    elif use_tiling:
        out = process_with_tiling(one, image_rgb, cfg["max_tile_size"], TILE_PADDING, cfg["upscale_factor"], upscaler.device, as_numpy=False)
    else:
        out = one(image_rgb)
    if trace is not None:
        trace.append({"in_shape": (h, w), "out_shape": tuple(out.shape[:2]), "tiled": bool(use_tiling), "three_channel": bool(use_3ch),
                      "model_calls": None if calls0 is None else model.calls - calls0, "net_input_px": net_px[0]})
    if as_numpy:
        return _to_host(upscaler, out)
    return out


def realesrganer_stage(up):
    """A RealESRGANer (around an SRVGGNetCompact, say) as an `extra_upscalers` entry of enhance_iterations: RGB u8 frame -> upscaled RGB
    u8 frame, kept on the device.  It is `up.enhance(frame[:, :, ::-1])[0][:, :, ::-1]` without the trip home: enhance()'s BGR -> RGB
    flip and the caller's RGB -> BGR cancel, so the frame goes in as it is; /255, padding, tiles, clamp, x255, round are enhance()'s."""
    def stage(frame_rgb):
        up._pad_on_device(normalize_u8_on_device(_u8_on(frame_rgb, up.device).permute(2, 0, 1)).unsqueeze(0))
        return (up._run().data.squeeze(0).float().clamp_(0, 1).permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous()
    stage.check_range = up._check_range
    return stage


def swin2sr_stage(model, device=None, tile=0, tile_pad=16, max_batch=None, tile_overlap=None):
    """A swin2sr.Swin2SR as an `extra_upscalers` entry of enhance_iterations: RGB u8 frame -> upscaled RGB u8 frame, kept on the
    device (model.upscale: the image processor's padding, the network, the crop and the quantiser in one chain of HIP launches).
    The slot the reference's ensemble (nesr.py:1033-1054) leaves to a second upscaler.  `device`: where a host frame goes
    (default: the current ROCm device); a device frame stays where it is.  `tile`, `tile_pad`, `max_batch` are model.upscale's:
    with tile > 0 the workspace is bounded by the window, not by the frame, so the stage runs at every iteration's size.
    `tile_overlap` (None: off) is model.upscale's as well: the authors' overlapped tiles with averaged seams."""
    def stage(frame_rgb):
        if not (isinstance(frame_rgb, torch.Tensor) and frame_rgb.is_cuda):
            frame_rgb = _u8_on(frame_rgb, torch.device("cuda") if device is None else torch.device(device))
        return model.upscale(frame_rgb, tile=tile, tile_pad=tile_pad, max_batch=max_batch, tile_overlap=tile_overlap)
    return stage


def diffusion_stage(pipe, prompt="a high resolution, detailed photograph", noise_level=20, num_inference_steps=20, guidance_scale=7.5, seed=None,
                    prompt_ids=None, negative_ids=None, device=None, tile=None, tile_overlap=0, vae_tile=None, vae_overlap=None):
    """A sdx4.StableDiffusionX4Upscaler as an `extra_upscalers` entry of enhance_iterations: RGB u8 frame -> the x4 RGB u8 frame,
    kept on the device.  It is the reference's _apply_diffusion (nesr.py:988-1031) with its CUDA settings as defaults: the slot its
    ensemble (nesr.py:570-584) gives the diffusion result.  `prompt` needs the pipeline's tokenizer; `prompt_ids` / `negative_ids`
    replace it.  `seed`: every frame draws from a generator seeded with it (None: torch's global generator of the device).  A frame
    over the VAE's limit of 65536 low-res pixels raises NesrUnsupportedError naming the limit unless `tile` is given: then the loop and
    the decode run over overlapping windows (upscale_frame's tile, tile_overlap, vae_tile, vae_overlap)."""
    def stage(frame_rgb):
        if not (isinstance(frame_rgb, torch.Tensor) and frame_rgb.is_cuda):
            frame_rgb = _u8_on(frame_rgb, torch.device("cuda") if device is None else torch.device(device))
        generator = None if seed is None else torch.Generator(device=frame_rgb.device).manual_seed(int(seed))
        return pipe.upscale_frame(frame_rgb, prompt=prompt, noise_level=noise_level, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                  generator=generator, prompt_ids=prompt_ids, negative_ids=negative_ids, tile=tile, tile_overlap=tile_overlap, vae_tile=vae_tile,
                                  vae_overlap=vae_overlap)
    return stage


def enhance_iterations(upscaler, image_rgb, config=None, device_kind="cuda", preprocess=None, postprocess=None,
                       trace=None, large_mp=LARGE_IMAGE_MP, filters=False, segmenter=None, extra_upscalers=(), device=None, use_hip=None,
                       encode=None, png=False, intermediates=None):
    """The iteration loop of SuperResolutionPipeline.enhance_image (nesr.py:516-633):

        for iteration in range(config['iterations']):           nesr.py:516
            current = _preprocess_image(current)                 nesr.py:537   -> `preprocess` (NL-means + CLAHE; None = off)
            current = _segment_and_enhance(current)              nesr.py:549   -> `segmenter` + imgproc.segment_enhance (None = off)
            esrgan_result = _apply_esrgan(current)               nesr.py:566   -> apply_esrgan above (`upscaler`; None = use_esrgan off)
            further results, Nones dropped                       nesr.py:582-584 -> `extra_upscalers`
            current = _ensemble_results(results)                 nesr.py:596   -> imgproc.ensemble_results (one result: the identity)
              or, with no result, cv2.resize(INTER_CUBIC)        nesr.py:597-605 -> imgproc.resize_u8
            current = _postprocess_image(current)                nesr.py:616   -> `postprocess` (adaptive unsharp; None = off)

    `segmenter` is a callable, RGB u8 frame -> class map (any integer dtype, host or device).  The reference's is SegFormer-B0:
    segformer.SegFormer.from_checkpoint(local path) runs it as HIP kernels and goes in as it is, the frame never leaves the device
    (the reference fetches the weights from the hub; here the caller passes a local checkpoint); `extra_upscalers` a sequence of callables, frame -> upscaled RGB u8 frame or None
    (the reference's second model is a remote diffusion pipeline; realesrganer_stage wraps a RealESRGANer around the other network
    family).  `upscaler=None` with no extra result is the reference's no-model configuration (use_esrgan=False, use_diffusion=False)
    and takes its bicubic step to (int(w f), int(h f)); it is reached through that explicit configuration only, never from an
    exception.  `filters=True` runs the reference's cv2 pre / post filters too (NL-means + CLAHE, adaptive unsharp:
    imgproc.py, OpenCV's algorithms restated -- parity unpinned).  Frames stay on the GPU between iterations (`device`: where, when
    there is no upscaler to say; default the frame's own device, else the ROCm device if there is one); the final frame is returned
    as an HWC uint8 RGB ndarray.  A backend failure raises (the reference would hand back a bicubic resize, nesr.py:835-843); `trace`
    receives one dict per iteration with the route and the number of network evaluations, so a caller can assert
    that the network really ran -- and, when a segmenter, an extra upscaler or upscaler=None is in use, "segmented" and
    "ensemble_n" (the results that were combined; 0: the bicubic step).  With those arguments left out the loop, its result and
    its trace are what they were without them.  use_hip goes to every stage (None: the HIP kernels where they apply; False: the
    torch chains, the same bits).  encode="jpeg" or ("jpeg", quality): what enhance_image writes in the end (cv2.imwrite,
    nesr.py:639-646) -- the bytes of the final RGB frame's JPEG file (quality 95 unless given) instead of the ndarray, encoded on the
    device the frame is on (imgproc.encode_jpeg_u8), so only the file comes home; ("jpeg", quality, {"sampling": ..., "optimize": ...,
    "restart_interval": ...}) passes that call's options.  image_rgb may be a JPEG or an 8-bit PNG file's bytes:
    they are decoded on the device first (imgproc.decode_jpeg_u8 / decode_png), so only files cross the bus.  png=True: the final RGB frame's lossless PNG
    file instead (what standalone/superres_project.py:203-206 always writes), encoded on the device (imgproc.encode_png); together
    with `encode` it raises ValueError, and encode="png" stays an error.  intermediates=<list>: with config["intermediate_saves"]
    true it receives each iteration's frame as PNG bytes, the reference's intermediate_iter{n}.png (nesr.py:619-625), encoded where
    the frame is."""
    if png and encode is not None:
        raise ValueError("enhance_iterations: png=True and encode are two different files; give one")
    if encode is not None:
        kind, quality, jpeg_options = (encode, 95, {}) if isinstance(encode, str) else (tuple(encode) + ({},))[:3]
        if kind != "jpeg" or (not isinstance(encode, str) and len(encode) not in (2, 3)) or not isinstance(jpeg_options, dict):
            raise ValueError(f"enhance_iterations: encode must be None, 'jpeg', ('jpeg', quality) or ('jpeg', quality, {{options}}), got {encode!r}")
    cfg = {"iterations": 3, "upscale_factor": 2.0, "denoise_level": 0.5, "adaptive_sharpening": True}
    cfg.update(config or {})
    staged = segmenter is not None or len(extra_upscalers) > 0 or upscaler is None
    if upscaler is not None:
        device = upscaler.device
    elif device is None:
        device = image_rgb.device if isinstance(image_rgb, torch.Tensor) else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if filters:      # the reference's own pre / post filters (nesr.py:668-689, 1056-1084), on the device: imgproc.py (cv2 restated)
        from . import imgproc
        fkw = {} if use_hip is None else {"use_hip": use_hip}
        preprocess = preprocess or (lambda im: imgproc.preprocess_image(_u8_on(im, device), cfg["denoise_level"], **fkw))
        postprocess = postprocess or (lambda im: imgproc.postprocess_image(_u8_on(im, device), cfg["adaptive_sharpening"], **fkw))
    if isinstance(image_rgb, (bytes, bytearray, memoryview)):
        # enhance_image's cv2.imread + cvtColor(BGR2RGB) (nesr.py:661-666) for a JPEG file's bytes: decoded on `device`, RGB order
        from . import imgproc
        if bytes(image_rgb[:8]) == b"\x89PNG\r\n\x1a\n":
            # a PNG file under cv2.imread's default flag: three 8-bit channels, gray expanded, alpha dropped.  cv2's 16 -> 8 bit
            # conversion is not restated here: a 16-bit file is an error
            image_rgb = imgproc.decode_png(bytes(image_rgb), order="rgb", device=device)
            if image_rgb.dtype != torch.uint8:
                raise ValueError("enhance_iterations: a 16-bit PNG file (cv2.imread's default flag would reduce it to 8 bits; decode it yourself)")
            if image_rgb.dim() == 3:
                image_rgb = image_rgb[:, :, :3].contiguous()
        else:
            image_rgb = imgproc.decode_jpeg_u8(bytes(image_rgb), order="rgb", device=device)
        if image_rgb.dim() == 2:                                # (cv2.imread's default flag gives three channels for a gray file)
            image_rgb = image_rgb[:, :, None].expand(-1, -1, 3).contiguous()
    current = image_rgb
    for iteration in range(int(cfg["iterations"])):
        if preprocess is not None:
            current = preprocess(current)
        if staged:
            from . import imgproc
            current = _u8_on(current, device)
        if segmenter is not None:                                # nesr.py:540-549
            current = imgproc.segment_enhance(current, segmenter(current), use_hip=use_hip)
        source = current
        results = []
        if upscaler is not None:
            current = apply_esrgan(upscaler, current, cfg, device_kind, as_numpy=False, trace=trace, large_mp=large_mp,
                                   **({} if use_hip is None else {"use_hip": use_hip}))
            results.append(current)
        elif trace is not None:                                  # no network ran: nothing of apply_esrgan's route to report
            trace.append({"in_shape": tuple(source.shape[:2]), "model_calls": 0, "net_input_px": 0})
        if trace is not None:
            trace[-1]["iteration"] = iteration
        if staged:
            for extra in extra_upscalers:                        # nesr.py:582-584: a model that gave nothing is dropped
                r = extra(source)
                if r is not None:
                    results.append(_u8_on(r, device))
            if results:
                current = imgproc.ensemble_results(results, use_hip=use_hip)                    # nesr.py:595-596
            else:                                                # nesr.py:597-605: the configured no-model step
                h, w = source.shape[:2]
                f = cfg["upscale_factor"]
                current = imgproc.resize_u8(source, int(h * f), int(w * f), imgproc.INTER_CUBIC, use_hip=use_hip)
            if trace is not None:
                trace[-1].update({"segmented": segmenter is not None, "ensemble_n": len(results), "out_shape": tuple(current.shape[:2])})
        if postprocess is not None:
            current = postprocess(current)
        if intermediates is not None and cfg.get("intermediate_saves"):        # nesr.py:619-625: intermediate_iter{n}.png
            from . import imgproc
            intermediates.append(imgproc.encode_png(current, order="rgb"))
    for extra in extra_upscalers:
        check = getattr(extra, "check_range", None)
        if check is not None:
            check()
    if encode is not None or png:
        from . import imgproc
        data = imgproc.encode_png(current, order="rgb") if png else imgproc.encode_jpeg_u8(current, quality, order="rgb", **jpeg_options)
        check = getattr(getattr(upscaler, "model", None), "check_range", None)
        if check is not None and isinstance(current, torch.Tensor):
            check()
        return data
    if not isinstance(current, torch.Tensor):
        return current
    if upscaler is None:
        return current.cpu().numpy()
    return _to_host(upscaler, current)
