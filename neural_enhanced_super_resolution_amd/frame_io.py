"""Gray, BGRA and 16-bit frames at the edges of ``RealESRGANer.enhance`` on the device (csrc/frame_io.hip through
nesr_pack_frame / nesr_unpack_frame, include/nesr_hip.h):

  pack_frame    enhance_float's host preparation: ``img.astype(float32) / max_range``, gray -> three planes, BGR -> RGB, HWC -> CHW,
                and for BGRA the alpha samples, as three planes (the network route) or as one (the linear-resize route)
  unpack_frame  what enhance() does with the network's output: clamp(0, 1), ``[[2, 1, 0]]``, BGR2GRAY for gray frames and for a
                network-upsampled alpha, ``(x * max_range).round().astype(uint8 | uint16)``

Both take ``use_hip=None|True|False`` like imgproc.py: False is a torch chain that runs on any device, the CPU included, and is bit
for bit the numpy arithmetic of enhance_float and enhance's quantiser; True calls the kernel; the two agree bit for bit.  None
takes the kernel on a ROCm device.

A 16-bit frame is held as an int16 tensor carrying the uint16 bit pattern (torch has few uint16 operations): frame_to_tensor and
frame_to_numpy convert at the ends, and a torch.uint16 tensor is accepted where the build has the dtype.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._contexts import device_call

_U16 = getattr(torch, "uint16", None)
_LUTS = {}


def frame_to_tensor(img, device=None, non_blocking=False):
    """numpy uint8 / uint16 frame -> uint8 / int16 (bit pattern) tensor, on `device` when given."""
    img = np.ascontiguousarray(img)
    if img.dtype == np.uint16:
        img = img.view(np.int16)
    elif img.dtype != np.uint8:
        raise ValueError(f"a uint8 or uint16 frame, got {img.dtype}")
    t = torch.from_numpy(img)
    return t if device is None else t.to(device, non_blocking=non_blocking)


def frame_to_numpy(t):
    """The inverse of frame_to_tensor for a tensor on the host."""
    a = t.numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _bits(frame):
    if frame.dtype == torch.uint8:
        return 8
    if frame.dtype == torch.int16 or (_U16 is not None and frame.dtype == _U16):
        return 16
    raise ValueError(f"a uint8 or int16-held uint16 frame, got {frame.dtype}")


def _check_kind(frame, max_range):
    bits = _bits(frame)
    if frame.dim() not in (2, 3) or (frame.dim() == 3 and frame.shape[2] not in (3, 4)) or frame.numel() == 0:
        raise ValueError(f"a frame is [H, W], [H, W, 3] or [H, W, 4], got {tuple(frame.shape)}")
    if max_range not in (255, 65535) or (max_range == 65535 and bits == 8):
        raise ValueError(f"max_range {max_range} for a {bits}-bit frame (255, or 65535 with 16 bits)")
    return bits


def _lut(bits, max_range, device):
    """sample -> float32(sample) / max_range as numpy divides (correctly rounded): torch divides by a scalar on the GPU by
    multiplying with its reciprocal, which is one ulp off for some samples (see realesrganer.normalize_u8_on_device)."""
    key = (bits, max_range, str(device))
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(np.arange(1 << bits, dtype=np.float32) / max_range).to(device)
    return _LUTS[key]


def _rows_contiguous(t, inner):
    """The last `inner` dimensions are dense (a row of samples, or of floats, is contiguous); outer pitches are free."""
    want = 1
    for d in range(t.dim() - 1, t.dim() - 1 - inner, -1):
        if t.shape[d] != 1 and t.stride(d) != want:
            return False
        want *= t.shape[d]
    return all(t.shape[d] == 1 or t.stride(d) >= want for d in range(t.dim() - inner))


def pack_frame(frame, max_range, alpha=None, through_fp16=False, use_hip=None):
    """frame: uint8 or 16-bit [H, W] | [H, W, 3] | [H, W, 4] tensor -> (image, alpha_out).

    image is float32 [1, 3, H, W] = frame / max_range, gray replicated, colour flipped BGR -> RGB.  alpha (BGRA frames): "network" ->
    alpha_out float32 [1, 3, H, W], the alpha samples replicated (upstream's cvtColor(alpha, GRAY2RGB)); "linear" -> float32 [H, W];
    None -> no alpha_out.  through_fp16 rounds image and a "network" alpha through fp16 (RealESRGANer(half=True): self.img.half());
    a "linear" alpha does not pass the network and is never rounded."""
    bits = _check_kind(frame, max_range)
    if alpha not in (None, "network", "linear"):
        raise ValueError(f"alpha {alpha!r}: None, 'network' or 'linear'")
    channels = 1 if frame.dim() == 2 else frame.shape[2]
    if channels != 4:
        alpha = None
    h, w = frame.shape[:2]
    if use_hip is None:
        use_hip = frame.device.type == "cuda"
    if use_hip:
        if frame.device.type != "cuda":
            raise ValueError(f"pack_frame: the HIP kernel takes a tensor on the ROCm device, got one on {frame.device}")
        src = frame if _rows_contiguous(frame, frame.dim() - 1) else frame.contiguous()
        image = torch.empty((1, 3, h, w), dtype=torch.float32, device=frame.device)
        out = None
        if alpha is not None:
            out = torch.empty((1, 3, h, w) if alpha == "network" else (h, w), dtype=torch.float32, device=frame.device)
        pitch = (src.stride(0) if h > 1 else w * channels) * src.element_size()
        device_call("nesr_pack_frame", src.device, src, h, w, channels, bits, pitch, int(max_range), 1 if through_fp16 else 0, image,
                    _lib.ALPHA_LINEAR if alpha == "linear" else _lib.ALPHA_NETWORK, out)
        return image, out
    idx = frame.to(torch.int64)
    if bits == 16:
        idx = idx & 0xFFFF
    v = _lut(bits, max_range, frame.device)[idx]

    def through(t):
        return t.half().float() if through_fp16 else t

    if channels == 1:
        image = v[None].expand(3, h, w)
    else:
        image = v[:, :, 0:3].permute(2, 0, 1).flip(0)
    image = through(image).contiguous()[None]
    out = None
    if alpha == "network":
        out = through(v[:, :, 3])[None].expand(3, h, w).contiguous()[None]
    elif alpha == "linear":
        out = v[:, :, 3].contiguous()
    return image, out


def _gray(bgr):
    """cv2.COLOR_BGR2GRAY on float32 [..., 3] as enhance() restates it: every product and sum a float32 operation of its own."""
    return bgr[..., 0] * 0.114 + bgr[..., 1] * 0.587 + bgr[..., 2] * 0.299


def unpack_frame(output, channels, max_range, alpha=None, through_fp16=False, use_hip=None):
    """The network's output -> the finished frame.

    output: float32 [1, 3, Ho, Wo] or [3, Ho, Wo] with contiguous rows (post_process's cropped view goes to the kernel as it is).
    channels 1: gray [Ho, Wo]; 3: BGR [Ho, Wo, 3]; 4: BGRA, with alpha either the alpha pass's output (three planes, shaped like
    `output`: its gray value is taken) or a float32 [Ho, Wo] plane (the linear resize's result).  max_range 255 -> uint8, 65535 ->
    16 bit (int16-held).  through_fp16 rounds the network outputs through fp16 before the clamp (upstream's half=True hands back
    fp16); a [Ho, Wo] alpha plane is only clamped."""
    if channels not in (1, 3, 4) or max_range not in (255, 65535):
        raise ValueError(f"unpack_frame: channels {channels} (1, 3 or 4), max_range {max_range} (255 or 65535)")
    x = output[0] if output.dim() == 4 else output
    if x.dim() != 3 or x.shape[0] != 3 or x.dtype != torch.float32:
        raise ValueError(f"unpack_frame: a float32 [1, 3, Ho, Wo] network output, got {output.dtype} {tuple(output.shape)}")
    ho, wo = x.shape[1:]
    plane = None
    if channels == 4:
        if alpha is None:
            raise ValueError("unpack_frame: a BGRA frame needs alpha")
        a = alpha[0] if alpha.dim() == 4 else alpha
        plane = a.dim() == 2
        if a.dtype != torch.float32 or a.device != x.device or tuple(a.shape) != ((ho, wo) if plane else (3, ho, wo)):
            raise ValueError(f"unpack_frame: alpha must be float32 [Ho, Wo] or shaped like the output, got {alpha.dtype} {tuple(alpha.shape)}")
    else:
        a = None
    bits = 16 if max_range == 65535 else 8
    if use_hip is None:
        use_hip = x.device.type == "cuda"
    if use_hip:
        if x.device.type != "cuda":
            raise ValueError(f"unpack_frame: the HIP kernel takes a tensor on the ROCm device, got one on {x.device}")
        x = x if _rows_contiguous(x, 1) else x.contiguous()
        if a is not None:
            a = a if _rows_contiguous(a, 1) else a.contiguous()
        shape = (ho, wo) if channels == 1 else (ho, wo, channels)
        dst = torch.empty(shape, dtype=torch.uint8 if bits == 8 else torch.int16, device=x.device)
        ap, ar = (0, 0) if a is None else ((0, a.stride(0)) if plane else (a.stride(0), a.stride(1)))
        device_call("nesr_unpack_frame", x.device, x, ho, wo, x.stride(0), x.stride(1), 1 if through_fp16 else 0,
                    _lib.ALPHA_LINEAR if plane else _lib.ALPHA_NETWORK, a, ap, ar, channels, bits, int(max_range), dst,
                    wo * channels * (bits // 8))
        return dst

    def unit(t, net=True):
        if through_fp16 and net:
            t = t.half().float()
        return t.clamp(0, 1)

    bgr = unit(x).flip(0).permute(1, 2, 0)                        # [[2, 1, 0]], CHW -> HWC
    if channels == 1:
        res = _gray(bgr)
    elif channels == 3:
        res = bgr
    else:
        av = unit(a, False) if plane else _gray(unit(a).flip(0).permute(1, 2, 0))
        res = torch.cat([bgr, av[:, :, None]], 2)
    q = (res * float(max_range)).round()
    if bits == 8:
        return q.to(torch.uint8).contiguous()
    return q.to(torch.int32).to(torch.int16).contiguous()          # the low 16 bits: the uint16 value's pattern
