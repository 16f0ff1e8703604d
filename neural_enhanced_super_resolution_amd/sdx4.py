"""``StableDiffusionX4Upscaler``: diffusers' ``StableDiffusionUpscalePipeline("stabilityai/stable-diffusion-x4-upscaler")``, the
reference's second upscaler (nesr/nesr.py:243-283 loads it, :988-1031 calls it, :570-584 puts its result into the ensemble), as one
C call: ``nesr_sdx4_upscale_u8`` (csrc/sdx4_api.cpp) chains ``ClipTextEncoder``, ``UNet2DCondition`` and ``VaeDecoder`` with the two
kernels of csrc/sdx4_step.hip, which are the schedulers and the guidance.  A prompt's ids and a u8 frame in, the x4 u8 frame out,
with no host round trip inside the denoising loop.  With ``tile=`` the loop and the decode run over overlapping windows of one
shape, blended on the device (``nesr_sdx4_upscale_tiled_u8``, csrc/sdx4_tiled.hip): that is how a frame above the VAE's limit runs.

diffusers is not a dependency and nothing is fetched: the schedulers and the loop are written from memory of the library, and
DESIGN section 20 says "recalled" about each such value.  Departures on purpose: frames whose sides are no multiple of 8 are padded
up by edge replication and the x4 result is cropped (diffusers resizes, as recalled); random numbers come from this process's
torch generator on the ROCm device, so a CUDA run's draws are not reproduced; eta is 0, one image a prompt, no callbacks, no
watermarker, no fp16 form, and a frame above 65536 low-res pixels is refused unless ``tile`` is given.  The tiling is this project's
own specification (one shared latent frame, ramped seams: DESIGN section 22); how diffusers tiles is recalled, not checked.
"""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import torch

from . import _lib
from ._contexts import _invoke
from ._tiling import sdx4_tile_plan
from .clip_text import ClipTextEncoder
from .unet import UNet2DCondition
from .vae import VaeDecoder

# the published pipeline's scheduler configurations, recalled from memory: the files under scheduler/ and low_res_scheduler/, or the
# arguments, override them
DDIM_DEFAULTS = dict(num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="scaled_linear", prediction_type="v_prediction",
                     clip_sample=False, set_alpha_to_one=False, steps_offset=1, timestep_spacing="leading")
LOW_RES_DEFAULTS = dict(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
SCHEDULER_CLASS, LOW_RES_CLASS = "DDIMScheduler", "DDPMScheduler"
MAX_NOISE_LEVEL = 350
KERNEL_GROUPS = ("prepare", "step", "window_gather", "accumulate", "tiled_step", "blend_add", "blend_finish")      # NESR_SDX4_GROUP_*
FRAME_MULTIPLE = 8                       # __call__ pads to it: 2^(levels - 1) of the published UNet
MAX_LOW_RES_PIXELS = 1 << 16             # NESR_VAE_MAX_TOKENS


def _fields(given, defaults, what):
    given = dict(given or {})
    given.pop("_class_name", None), given.pop("_diffusers_version", None)
    out = dict(defaults)
    out.update({k: v for k, v in given.items() if k in defaults})
    extra = {k: v for k, v in given.items() if k not in defaults}
    # fields the kernels have one answer for: anything else is refused here, by name
    for key, only in (("thresholding", False), ("rescale_betas_zero_snr", False), ("trained_betas", None)):
        if extra.get(key) not in (only, None):
            raise _lib.NesrUnsupportedError(f"StableDiffusionX4Upscaler: {what} field {key} = {extra[key]!r} is not supported")
    return out


def schedule(steps, **fields):
    """(timesteps [steps] int, alpha_bars [steps, 2] float64, coefficients [steps, 6] float32) of a DDIM scheduler of `fields`, as
    the library computes them.  Needs no device."""
    c = _fields(fields, DDIM_DEFAULTS, "scheduler")
    steps = int(steps)
    cap = max(steps, 1)
    ts, ab, co = (ctypes.c_int * cap)(), (ctypes.c_double * (2 * cap))(), (ctypes.c_float * (6 * cap))()
    rc = _lib.load().nesr_sdx4_schedule(int(c["num_train_timesteps"]), float(c["beta_start"]), float(c["beta_end"]), str(c["beta_schedule"]).encode(),
                                        str(c["prediction_type"]).encode(), int(bool(c["set_alpha_to_one"])), int(c["steps_offset"]),
                                        str(c["timestep_spacing"]).encode(), steps, ts, ab, co)
    _check(rc, "nesr_sdx4_schedule")
    return (np.array(ts[:steps], dtype=np.int64), np.array(ab[:2 * steps], dtype=np.float64).reshape(steps, 2),
            np.array(co[:6 * steps], dtype=np.float32).reshape(steps, 6))


def noise_coefficients(noise_level, **fields):
    """(alpha-bar at the noise level, float64; [sqrt(abar), sqrt(1 - abar)] float32) of a low-res scheduler of `fields`."""
    c = _fields(fields, LOW_RES_DEFAULTS, "low_res_scheduler")
    ab, co = ctypes.c_double(0), (ctypes.c_float * 2)()
    _check(_lib.load().nesr_sdx4_noise_coefficients(int(c["num_train_timesteps"]), str(c["beta_schedule"]).encode(), int(noise_level), ctypes.byref(ab), co),
           "nesr_sdx4_noise_coefficients")
    return ab.value, np.array(co[:], dtype=np.float32)


def _check(rc, what):
    if rc == _lib.ERR_UNSUPPORTED:
        msg = _lib.load().nesr_last_error()
        raise _lib.NesrUnsupportedError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
    _lib.check(rc, what)


class UpscaleOutput:
    """What the reference reads of diffusers' ImagePipelineOutput: ``.images[0]``, here the host uint8 [H, W, 3] array (np.array of it
    is itself, nesr/nesr.py:1028)."""

    def __init__(self, images):
        self.images = images


class StableDiffusionX4Upscaler:
    """The three networks and the two schedulers as the x4 pipeline.  Not a Module: the networks are, and own their weights."""

    def __init__(self, text_encoder, unet, vae, scheduler=None, low_res_scheduler=None, tokenizer=None, max_noise_level=MAX_NOISE_LEVEL):
        for obj, cls, name in ((text_encoder, ClipTextEncoder, "text_encoder"), (unet, UNet2DCondition, "unet"), (vae, VaeDecoder, "vae")):
            if not isinstance(obj, cls):
                raise TypeError(f"StableDiffusionX4Upscaler: {name} must be a {cls.__name__}, got {type(obj).__name__}")
        for given, cls, what in ((scheduler, SCHEDULER_CLASS, "scheduler"), (low_res_scheduler, LOW_RES_CLASS, "low_res_scheduler")):
            name = (given or {}).get("_class_name", cls)
            if name != cls:
                raise _lib.NesrUnsupportedError(f"StableDiffusionX4Upscaler: {what} _class_name {name!r} is not supported ({cls} only)")
        self.text_encoder, self.unet, self.vae, self.tokenizer = text_encoder, unet, vae, tokenizer
        self.scheduler = _fields(scheduler, DDIM_DEFAULTS, "scheduler")
        self.low_res_scheduler = _fields(low_res_scheduler, LOW_RES_DEFAULTS, "low_res_scheduler")
        self.max_noise_level = int(max_noise_level)
        self.calls = 0
        self._timing = False
        self._pipes = {}          # device index -> (handle, the three contexts it was made of)

    @classmethod
    def from_pretrained(cls, path, unet_compute_dtype="f32", **kw):
        """The pipeline of a local directory in diffusers' layout: text_encoder/, unet/, vae/, scheduler/scheduler_config.json,
        low_res_scheduler/scheduler_config.json and, if transformers can read it, tokenizer/.  A hub id raises: nothing is fetched.
        unet_compute_dtype "fp16" loads the UNet in its fp16 compute form (UNet2DCondition(compute_dtype=)); the pipeline takes a
        UNet of either form, and with an fp16 one `upscale` waits once behind its last launch and may raise NesrRangeError."""
        path = os.fspath(path)
        if not os.path.isdir(path):
            raise FileNotFoundError(f"StableDiffusionX4Upscaler.from_pretrained: {path!r} is not a local directory (a hub id is not fetched: "
                                    "pass the path of a downloaded snapshot)")

        def config(*parts):
            with open(os.path.join(path, *parts)) as f:
                return json.load(f)

        scheduler, low_res = config("scheduler", "scheduler_config.json"), config("low_res_scheduler", "scheduler_config.json")
        index = os.path.join(path, "model_index.json")
        if os.path.isfile(index) and "max_noise_level" not in kw:
            found = config("model_index.json").get("max_noise_level")
            if found is not None:
                kw["max_noise_level"] = found
        tokenizer = None
        try:
            from transformers import CLIPTokenizer
            tokenizer = CLIPTokenizer.from_pretrained(os.path.join(path, "tokenizer"), local_files_only=True)
        except Exception:
            tokenizer = None      # upscale(prompt_ids=...) still works; a string prompt will say so
        return cls(ClipTextEncoder.from_checkpoint(os.path.join(path, "text_encoder")), UNet2DCondition.from_checkpoint(os.path.join(path, "unet"), compute_dtype=unet_compute_dtype),
                   VaeDecoder.from_checkpoint(os.path.join(path, "vae")), scheduler=scheduler, low_res_scheduler=low_res, tokenizer=tokenizer, **kw)

    def to(self, device):
        for m in (self.text_encoder, self.unet, self.vae):
            m.to(device)
        return self

    # ------------------------------------------------------------------ the context
    def _release(self):
        pipes, self._pipes = getattr(self, "_pipes", {}), {}
        for handle, _ in pipes.values():
            _lib.load().nesr_sdx4_destroy(handle)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _pipeline(self, device):
        """The nesr_sdx4 handle of `device`, made anew when one of the three contexts was (changed weights)."""
        index = device.index if device.index is not None else torch.cuda.current_device()
        parts = tuple(m._context(device) for m in (self.text_encoder, self.unet, self.vae))
        key = tuple(p.value for p in parts)
        if index in self._pipes and self._pipes[index][1] == key:
            return self._pipes[index][0]
        if index in self._pipes:
            _lib.load().nesr_sdx4_destroy(self._pipes.pop(index)[0])
        s, low = self.scheduler, self.low_res_scheduler
        handle = ctypes.c_void_p()
        rc = _lib.load().nesr_sdx4_create(ctypes.byref(handle), *parts, int(s["num_train_timesteps"]), float(s["beta_start"]), float(s["beta_end"]),
                                          str(s["beta_schedule"]).encode(), str(s["prediction_type"]).encode(), int(bool(s["clip_sample"])),
                                          int(bool(s["set_alpha_to_one"])), int(s["steps_offset"]), str(s["timestep_spacing"]).encode(), 0.0,
                                          int(low["num_train_timesteps"]), str(low["beta_schedule"]).encode(), self.max_noise_level)
        _check(rc, "nesr_sdx4_create")
        _invoke("nesr_sdx4_set_timing", None, handle, (1 if self._timing else 0,))
        self._pipes[index] = (handle, key)
        return handle

    def set_kernel_timing(self, enable=True):
        """Switches the event timing of the pipeline's own two kernels and of the three networks."""
        self._timing = bool(enable)
        for handle, _ in self._pipes.values():
            _invoke("nesr_sdx4_set_timing", None, handle, (1 if enable else 0,))
        for m in (self.text_encoder, self.unet, self.vae):
            m.set_kernel_timing(enable)

    def kernel_time_ms(self):
        """{"launches", "groups": {name of KERNEL_GROUPS: ms}} of the pipeline's own kernels since the last call."""
        launches, groups = 0, dict.fromkeys(KERNEL_GROUPS, 0.0)
        for index, (handle, _) in self._pipes.items():
            ms, n = (ctypes.c_double * len(KERNEL_GROUPS))(), ctypes.c_int64(0)
            with torch.cuda.device(index):
                _invoke("nesr_sdx4_kernel_time_ms", None, handle, (ms, len(KERNEL_GROUPS), ctypes.byref(n)))
            launches += n.value
            for name, v in zip(KERNEL_GROUPS, ms):
                groups[name] += v
        return {"launches": launches, "groups": groups}

    def last_launches(self, device=None):
        """Kernel launches of the last upscale on `device`: text + 1 + steps (UNet + 1) + VAE; of a tiled one: text + 1 + steps
        (windows (1 + UNet + 1) + 1) + vae_windows (1 + VAE + 1) + 1."""
        device = torch.device("cuda" if device is None else device)
        n = ctypes.c_int64(0)
        with torch.cuda.device(device):
            _invoke("nesr_sdx4_launches", None, self._pipeline(device), (ctypes.byref(n),))
        return n.value

    def frame_multiple(self):
        """2^(levels - 1) of this UNet: what a frame's sides, `tile` and `tile_overlap` are multiples of."""
        return 2 ** (len(self.unet.config["block_out_channels"]) - 1)

    def tile_plan(self, h, w, tile, tile_overlap=0):
        """((tiles_y, tiles_x), (ty, tx), [(y, x)]) of an h x w low-res frame as the library computes it (nesr_sdx4_tile_plan): the
        windows of `upscale(tile=, tile_overlap=)` in the order they run.  Needs no device."""
        counts = [ctypes.c_int(0) for _ in range(4)]
        args = (int(h), int(w), self.frame_multiple(), int(tile), int(tile_overlap))
        lib = _lib.load()
        _check(lib.nesr_sdx4_tile_plan(*args, *counts, None, 0), "nesr_sdx4_tile_plan")
        ky, kx, ty, tx = (c.value for c in counts)
        plan = (ctypes.c_int32 * (2 * ky * kx))()
        _check(lib.nesr_sdx4_tile_plan(*args, *counts, plan, len(plan)), "nesr_sdx4_tile_plan")
        return (ky, kx), (ty, tx), [(plan[2 * i], plan[2 * i + 1]) for i in range(ky * kx)]

    def workspace_bytes(self, n, h, w, tokens, device=None, tile=None, tile_overlap=0, vae_tile=None, vae_overlap=None):
        """Bytes the pipeline itself allocates for n samples of an h x w frame (the networks report their own); with `tile`, of the
        tiled call (no device needed)."""
        if tile is not None:
            size = ctypes.c_size_t(0)
            _check(_lib.load().nesr_sdx4_tiled_workspace_bytes(int(n), int(self.vae.config["latent_channels"]), int(self.text_encoder.config["hidden_size"]),
                                                               2 ** (len(self.vae.config["block_out_channels"]) - 1), int(h), int(w), int(tokens), self.frame_multiple(),
                                                               int(tile), int(tile_overlap), 0 if vae_tile is None else int(vae_tile),
                                                               -1 if vae_overlap is None else int(vae_overlap), ctypes.byref(size)), "nesr_sdx4_tiled_workspace_bytes")
            return size.value
        device = torch.device("cuda" if device is None else device)
        size = ctypes.c_size_t(0)
        with torch.cuda.device(device):
            _invoke("nesr_sdx4_workspace_bytes", None, self._pipeline(device), (int(n), int(h), int(w), int(tokens), ctypes.byref(size)))
        return size.value

    # ------------------------------------------------------------------ the call on ids
    @staticmethod
    def _ids(ids, what):
        ids = torch.as_tensor(ids).detach().to("cpu", torch.int64).reshape(-1)
        if ids.numel() == 0:
            raise ValueError(f"StableDiffusionX4Upscaler.upscale: {what} is empty")
        return ids

    def upscale(self, frame, prompt_ids=None, negative_ids=None, noise_level=20, num_inference_steps=20, guidance_scale=7.5, generator=None, noise=None,
                latents=None, return_latents=False, tile=None, tile_overlap=0, vae_tile=None, vae_overlap=None):
        """frame [h, w, 3] uint8 RGB on the device -> the x4 frame [4h, 4w, 3] uint8 on the device (and, return_latents, the final
        float32 latents [1, 4, h, w]).  prompt_ids / negative_ids: one row of token ids each, of the same length (negative_ids is
        needed when guidance_scale > 1).  noise [3, h, w] and latents [4, h, w]: unit normal float32 on the device; what is not given
        is drawn with torch.randn(generator=generator) on the frame's device, the low-res noise first, then the latents.
        tile (low-res pixels; None: the untiled call, unchanged): the denoising loop runs over overlapping windows of min(tile, h) x
        min(tile, w) on one shared latent frame, seams ramped over tile_overlap pixels, and the VAE decodes over windows of vae_tile
        / vae_overlap (None: tile / tile_overlap); tile_plan() gives the windows.  noise and latents stay full-frame draws."""
        if not (torch.is_tensor(frame) and frame.is_cuda):
            raise RuntimeError("StableDiffusionX4Upscaler.upscale: the frame is not on the ROCm device (there is no CPU or PyTorch fallback)")
        if frame.dim() != 3 or frame.shape[2] != 3 or frame.dtype != torch.uint8 or frame.numel() == 0:
            raise ValueError(f"StableDiffusionX4Upscaler.upscale: an [h, w, 3] uint8 tensor, got {frame.dtype} {tuple(frame.shape)}")
        if prompt_ids is None:
            raise ValueError("StableDiffusionX4Upscaler.upscale: prompt_ids is required (a tokenizer's input_ids of the prompt)")
        if tile is None and (tile_overlap or vae_tile is not None or vae_overlap is not None):
            raise ValueError("StableDiffusionX4Upscaler.upscale: tile_overlap, vae_tile and vae_overlap need tile")
        if vae_tile is not None and int(vae_tile) < 1:      # the C entry reads 0 as "tile" and a negative overlap as "tile_overlap": None says that here
            raise ValueError(f"StableDiffusionX4Upscaler.upscale: vae_tile must be positive (None: tile), got {vae_tile}")
        if vae_overlap is not None and int(vae_overlap) < 0:
            raise ValueError(f"StableDiffusionX4Upscaler.upscale: vae_overlap must not be negative (None: tile_overlap), got {vae_overlap}")
        frame = frame.contiguous()
        h, w = int(frame.shape[0]), int(frame.shape[1])
        device = frame.device
        lc = int(self.vae.config["latent_channels"])
        rows = [self._ids(prompt_ids, "prompt_ids")]
        if float(guidance_scale) > 1.0:
            if negative_ids is None:
                raise ValueError("StableDiffusionX4Upscaler.upscale: guidance_scale > 1 needs negative_ids (the ids of the negative prompt, \"\" by default)")
            rows.insert(0, self._ids(negative_ids, "negative_ids"))      # batch order [negative, prompt]
            if rows[0].numel() != rows[1].numel():
                raise ValueError(f"StableDiffusionX4Upscaler.upscale: negative_ids has {rows[0].numel()} ids, prompt_ids {rows[1].numel()}; pad both to one length")
        tokens = rows[0].numel()
        flat = torch.cat(rows)
        if int(flat.min()) < -2 ** 31 or int(flat.max()) >= 2 ** 31:
            raise ValueError("StableDiffusionX4Upscaler.upscale: an id does not fit 32 bits")
        host = (ctypes.c_int32 * flat.numel())(*flat.tolist())

        def given(t, shape, what):
            if t is None:
                return torch.randn(shape, generator=generator, device=device, dtype=torch.float32)
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape):
                raise ValueError(f"StableDiffusionX4Upscaler.upscale: {what} is a float32 tensor {shape} on the device")
            return t.contiguous()

        noise = given(noise, (3, h, w), "noise")                      # the pipeline's order, as recalled: the image's noise first
        latents = given(latents, (lc, h, w), "latents")
        with torch.cuda.device(device):
            handle = self._pipeline(device)
            scale = 2 ** (len(self.vae.config["block_out_channels"]) - 1)
            out = torch.empty((h * scale, w * scale, 3), dtype=torch.uint8, device=device)
            final = torch.empty((1, lc, h, w), dtype=torch.float32, device=device) if return_latents else None
            if tile is None:
                _invoke("nesr_sdx4_upscale_u8", device, handle, (frame, h, w, host, tokens, noise, latents, int(noise_level), int(num_inference_steps),
                                                                ctypes.c_double(float(guidance_scale)), out, out.numel(), final))
                windows = vae_windows = 1
            else:
                vt, vo = (0 if vae_tile is None else int(vae_tile)), (-1 if vae_overlap is None else int(vae_overlap))
                _invoke("nesr_sdx4_upscale_tiled_u8", device, handle, (frame, h, w, host, tokens, noise, latents, int(noise_level), int(num_inference_steps),
                                                                      ctypes.c_double(float(guidance_scale)), int(tile), int(tile_overlap), vt, vo, out, out.numel(), final))
                m = self.frame_multiple()
                (ky, kx), _, _ = sdx4_tile_plan(h, w, m, int(tile), int(tile_overlap))
                (vy, vx), _, _ = sdx4_tile_plan(h, w, m, int(tile) if vae_tile is None else int(vae_tile), int(tile_overlap) if vae_overlap is None else int(vae_overlap))
                windows, vae_windows = ky * kx, vy * vx
        self.calls += 1
        for m, count in ((self.text_encoder, 1), (self.unet, int(num_inference_steps) * windows), (self.vae, vae_windows)):
            m.calls += count
        return (out, final) if return_latents else out

    # ------------------------------------------------------------------ the reference's call
    def tokenize(self, prompt):
        """The prompt's ids, padded and truncated to max_position_embeddings, as the pipeline asks its tokenizer for them."""
        if self.tokenizer is None:
            raise RuntimeError("StableDiffusionX4Upscaler: no tokenizer is loaded (a BPE tokenizer of our own is out of scope), so a string prompt cannot be "
                               "encoded; pass prompt_ids= (and negative_ids=) to upscale(), or construct with tokenizer=")
        length = int(self.text_encoder.config["max_position_embeddings"])
        return list(self.tokenizer(prompt, padding="max_length", max_length=length, truncation=True)["input_ids"])

    def upscale_frame(self, image, prompt=None, noise_level=20, num_inference_steps=20, guidance_scale=7.5, negative_prompt=None, generator=None,
                      prompt_ids=None, negative_ids=None, device=None, tile=None, tile_overlap=0, vae_tile=None, vae_overlap=None):
        """`__call__` without the trip home: image (a PIL image, an [H, W, 3] uint8 ndarray or a device tensor) -> the device uint8
        [4H, 4W, 3] frame.  Sides that are no multiple of 8 are padded up by edge replication and the result is cropped (diffusers
        resizes instead, as recalled).  A frame above the VAE's limit raises NesrUnsupportedError naming it, unless `tile` is given:
        then it runs over windows (upscale's tile, tile_overlap, vae_tile, vae_overlap)."""
        if image is None:
            raise ValueError("StableDiffusionX4Upscaler: image is required")
        if prompt_ids is None:
            if not isinstance(prompt, str):
                raise ValueError("StableDiffusionX4Upscaler: prompt is one string (or pass prompt_ids)")
            prompt_ids = self.tokenize(prompt)
            if negative_ids is None and float(guidance_scale) > 1.0:
                negative_ids = self.tokenize("" if negative_prompt is None else negative_prompt)
        frame = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(np.asarray(image)))
        if frame.dim() != 3 or frame.shape[2] != 3 or frame.dtype != torch.uint8 or frame.numel() == 0:
            raise ValueError(f"StableDiffusionX4Upscaler: image is RGB uint8 [H, W, 3], got {frame.dtype} {tuple(frame.shape)}")
        H, W = int(frame.shape[0]), int(frame.shape[1])
        ph, pw = -H % FRAME_MULTIPLE, -W % FRAME_MULTIPLE
        if tile is None and (H + ph) * (W + pw) > MAX_LOW_RES_PIXELS:
            raise _lib.NesrUnsupportedError(f"StableDiffusionX4Upscaler: a frame of {H} x {W} exceeds the VAE's limit of {MAX_LOW_RES_PIXELS} low-res pixels "
                                            "(NESR_VAE_MAX_TOKENS; tiling is out of scope)")
        if not frame.is_cuda:
            frame = frame.to(torch.device("cuda" if device is None else device))
        if ph or pw:      # edge replication on the bottom and the right
            rows = torch.cat([torch.arange(H), torch.full((ph,), H - 1, dtype=torch.int64)]).to(frame.device)
            cols = torch.cat([torch.arange(W), torch.full((pw,), W - 1, dtype=torch.int64)]).to(frame.device)
            frame = frame[rows][:, cols]
        out = self.upscale(frame, prompt_ids=prompt_ids, negative_ids=negative_ids, noise_level=noise_level, num_inference_steps=num_inference_steps,
                           guidance_scale=guidance_scale, generator=generator, tile=tile, tile_overlap=tile_overlap, vae_tile=vae_tile, vae_overlap=vae_overlap)
        scale = out.shape[0] // frame.shape[0]
        return out[:H * scale, :W * scale].contiguous() if (ph or pw) else out

    def __call__(self, prompt=None, image=None, noise_level=20, num_inference_steps=20, guidance_scale=7.5, negative_prompt=None, generator=None,
                 prompt_ids=None, negative_ids=None, eta=0.0, num_images_per_prompt=1, device=None, tile=None, tile_overlap=0, vae_tile=None, vae_overlap=None,
                 **unsupported):
        """The reference's call (nesr/nesr.py:1001-1025): returns an object whose .images[0] is the host uint8 [4H, 4W, 3] array."""
        if unsupported:
            raise _lib.NesrUnsupportedError(f"StableDiffusionX4Upscaler: argument(s) {sorted(unsupported)} are not supported")
        if eta != 0.0 or num_images_per_prompt != 1:
            raise _lib.NesrUnsupportedError("StableDiffusionX4Upscaler: eta 0 and num_images_per_prompt 1 only")
        out = self.upscale_frame(image, prompt=prompt, noise_level=noise_level, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                 negative_prompt=negative_prompt, generator=generator, prompt_ids=prompt_ids, negative_ids=negative_ids, device=device,
                                 tile=tile, tile_overlap=tile_overlap, vae_tile=vae_tile, vae_overlap=vae_overlap)
        return UpscaleOutput([out.cpu().numpy()])
