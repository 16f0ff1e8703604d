"""The OpenCV image operations the reference wraps around its ESRGAN stage, as device-side torch code
(SURVEY.md section 8(f) rows 3 and 4):

  RealESRGANer.enhance(outscale=...)        cv2.resize(INTER_LANCZOS4)                      [UPSTREAM realesrgan utils.py]
  RealESRGANer.enhance(alpha_upsampler=..)  cv2.resize(alpha, INTER_LINEAR)                 [UPSTREAM]
  SuperResolutionPipeline._preprocess_image cv2.fastNlMeansDenoisingColored + CLAHE on L    nesr/nesr.py:668-689
  SuperResolutionPipeline._postprocess_image variance-masked unsharp                        nesr/nesr.py:1056-1084
  SuperResolutionPipeline._segment_and_enhance, image half: mask resize, dilate, unsharp    nesr/nesr.py:726-747
  SuperResolutionPipeline._ensemble_results  Lanczos alignment, float32 mean, truncation    nesr/nesr.py:1033-1054
  enhance_image's no-model step              cv2.resize(INTER_CUBIC)                         nesr/nesr.py:597-605
  enhance_image's last call                  cv2.imwrite(path.jpg): baseline JPEG (PINNED)   nesr/nesr.py:639-646
  the iterations' and projects' .png files   cv2.imwrite(path.png): lossless (pixels PINNED) nesr/nesr.py:619-625
  a .png input (gray, alpha, 16 bit)         cv2.imread(path.png, IMREAD_UNCHANGED) (PINNED) standalone/direct_esrgan.py:130
  (_process_with_tiling's Lanczos paste and the 12-channel builder's 3x3 blur use the same functions: nesr_adapter.py)

PARITY UNPINNED, all of it but the JPEG file (encode_jpeg_u8: libjpeg's integer pipeline, byte for byte): cv2 is not installed here or on the GPU box and the reference holds no output of any of
these calls, so each function restates OpenCV's documented algorithm (8-bit paths in OpenCV's fixed point: 11-bit
resize coefficients, 8-bit Gaussian kernels, integer non-local-means weights; Lab conversions in float with rounding
where OpenCV uses lookup tables -- expect +-1 LSB there).  oracle/cv2_ref.py restates them again, independently, in numpy:
the tests compare two restatements, not this code with OpenCV.

Everything takes and returns HWC uint8 tensors on the caller's device (the frames of the iteration loop stay on the
GPU: a 16384x16384 frame through cv2's CPU non-local means would take minutes).
"""
from __future__ import annotations

import math

import torch
from torch.nn import functional as F


def _hip_default(x):
    """use_hip=None: the HIP kernels for a uint8 tensor on the ROCm device."""
    return x.device.type == "cuda" and x.dtype == torch.uint8


def _hip_require(x, layout_ok, what, layout):
    """use_hip=True on a tensor the kernel cannot take: an error, never a launch on a wrong buffer."""
    if x.device.type != "cuda" or x.dtype != torch.uint8 or not layout_ok:
        raise ValueError(f"{what}: the HIP kernel takes a uint8 {layout} tensor on the ROCm device, got {x.dtype} "
                         f"{tuple(x.shape)} on {x.device}")


def _hip_call(x, name, *args):
    """libnesr_hip.so entry `name`(device, *args, stream) on x's device and current stream; raises on failure."""
    from ._contexts import device_call
    device_call(name, x.device, *args)


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------------------------- resize
def _lanczos4_coeffs(frac):
    """cv2 interpolateLanczos4 for a float32 tensor of fractional offsets -> [..., 8] float32 weights."""
    s45 = 0.70710678118654752440084436210485
    cs = torch.tensor([[1, 0], [-s45, -s45], [0, 1], [s45, -s45], [-1, 0], [s45, s45], [0, -1], [-s45, s45]],
                      dtype=torch.float64, device=frac.device)
    x = frac.to(torch.float64)
    y0 = -(x + 3) * (math.pi * 0.25)
    s0, c0 = torch.sin(y0), torch.cos(y0)
    i = torch.arange(8, device=frac.device, dtype=torch.float64)
    y = -(x[..., None] + 3 - i) * (math.pi * 0.25)
    co = ((cs[:, 0] * s0[..., None] + cs[:, 1] * c0[..., None]) / (y * y)).to(torch.float32)
    co = co * (1.0 / co.sum(-1, keepdim=True))
    exact = (frac < 1.1920929e-07)[..., None]
    delta = torch.zeros(8, device=frac.device)
    delta[3] = 1.0
    return torch.where(exact, delta.expand_as(co), co)


def _axis_taps(n_in, n_out, device, taps, first):
    """Source indices [n_out, taps] (clamped: cv2 replicates the border) and fractional offsets [n_out] of cv2.resize."""
    scale = n_in / n_out
    pos = (torch.arange(n_out, device=device, dtype=torch.float64) + 0.5) * scale - 0.5
    pos = pos.to(torch.float32)
    i0 = torch.floor(pos)
    frac = pos - i0
    idx = (i0.long()[:, None] + torch.arange(first, first + taps, device=device)).clamp_(0, n_in - 1)
    return idx, frac, i0.long()


def _rows_ok(t, channels):
    """[H, W, C] with the pixels of a row contiguous (any row stride that holds a row): what the resize kernels address as
    base pointer + row stride, so frame[y0:y1, x0:x1] goes to them as it is."""
    return (t.dim() == 3 and t.shape[2] in channels and min(t.shape) > 0 and (t.shape[2] == 1 or t.stride(2) == 1)
            and (t.shape[1] == 1 or t.stride(1) == t.shape[2]) and (t.shape[0] == 1 or t.stride(0) >= t.shape[1] * t.shape[2]))


def _row_bytes(t):
    return (t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2]) * t.element_size()


_U16 = getattr(torch, "uint16", None)


def _lanczos4_hip(img, out_h, out_w, out):
    """nesr_resize_u8 / nesr_resize_u16 (csrc/resize.hip) on an [H, W, C] device tensor; int32-held uint16 is narrowed once."""
    from . import _lib
    h, w, c = img.shape
    if img.dtype == torch.uint8:
        src = img if _rows_ok(img, (1, 3, 4)) else img.contiguous()
        dst = out if out is not None else torch.empty((out_h, out_w, c), dtype=torch.uint8, device=img.device)
        _hip_call(src, "nesr_resize_u8", _ptr(src), h, w, c, _row_bytes(src), _ptr(dst), out_h, out_w, _row_bytes(dst), _lib.INTER_LANCZOS4)
        return dst
    held = img.dtype == torch.int32
    # int32-held: the low 16 bits as little-endian byte pairs, which is the uint16 image in memory
    src = torch.stack([img & 255, (img >> 8) & 255], -1).to(torch.uint8) if held else (img if _rows_ok(img, (1, 3, 4)) else img.contiguous())
    dst = out if out is not None and not held else torch.empty((out_h, out_w, c, 2), dtype=torch.uint8, device=img.device)
    sb = w * c * 2 if held else _row_bytes(src)
    db = out_w * c * 2 if dst.dtype == torch.uint8 else _row_bytes(dst)
    _hip_call(src, "nesr_resize_u16", _ptr(src), h, w, c, sb, _ptr(dst), out_h, out_w, db, _lib.INTER_LANCZOS4)
    if held:
        r = dst.view(torch.int16).reshape(out_h, out_w, c).to(torch.int32) & 0xFFFF
        if out is not None:
            out.copy_(r)
            return out
        return r
    return dst if out is not None else dst.view(_U16).reshape(out_h, out_w, c)


def lanczos4_resize(img, out_h, out_w, use_hip=None, out=None):
    """cv2.resize(img, (out_w, out_h), interpolation=cv2.INTER_LANCZOS4) for HWC uint8 or uint16 (int32-held, or a real uint16
    tensor on the HIP route) tensors.
    uint8: OpenCV's fixed point -- coefficients rounded to 11 bits (x2048, short), integer horizontal pass, integer vertical
    pass, (v + 2^21) >> 22, saturate.  uint16: float32 coefficients and sums, round to nearest even, saturate.

    On a ROCm device one HIP kernel (csrc/resize.hip, nesr_resize_u8 / nesr_resize_u16: 1, 3 or 4 channels, both passes in one
    launch, nothing between them in device memory) unless use_hip=False selects the torch chain below.  uint8: the two agree bit
    for bit; uint16: the kernel sums in oracle/cv2_ref.py's order (k ascending), the chain in torch's: +-1.  A row-strided view
    (frame[y0:y1, x0:x1]) goes to the kernel as it is, and `out` may be such a view of a canvas ([out_h, out_w, C], img's
    dtype): crop, resize and paste are then one launch that writes nothing outside the rectangle."""
    if img.dim() != 3:
        raise ValueError(f"lanczos4_resize: an [H, W, C] tensor, got {tuple(img.shape)}")
    h, w, c = img.shape
    kinds = (torch.uint8, torch.int32) + ((_U16,) if _U16 is not None else ())
    fits = img.device.type == "cuda" and img.dtype in kinds and c in (1, 3, 4) and h > 0 and w > 0 and out_h > 0 and out_w > 0
    if out is not None:
        if tuple(out.shape) != (out_h, out_w, c) or out.dtype != img.dtype or out.device != img.device:
            raise ValueError(f"lanczos4_resize: out must be a {img.dtype} [{out_h}, {out_w}, {c}] tensor on {img.device}, got {out.dtype} "
                             f"{tuple(out.shape)} on {out.device}")
        fits = fits and (_rows_ok(out, (1, 3, 4)) or img.dtype == torch.int32)
    if use_hip is None:
        use_hip = fits
    if use_hip:
        if not fits:
            raise ValueError(f"lanczos4_resize: the HIP kernel takes a uint8 or uint16 (or int32-held) [H, W, 1 | 3 | 4] tensor on the ROCm "
                             f"device (out: rows of contiguous pixels), got {img.dtype} {tuple(img.shape)} on {img.device}")
        return _lanczos4_hip(img, out_h, out_w, out)
    if out is not None:
        out.copy_(_lanczos4_chain(img, out_h, out_w))
        return out
    return _lanczos4_chain(img, out_h, out_w)


def _lanczos4_chain(img, out_h, out_w):
    """lanczos4_resize as torch operations on any device (use_hip=False)."""
    h, w, c = img.shape
    is8 = img.dtype == torch.uint8
    ix, fx, _ = _axis_taps(w, out_w, img.device, 8, -3)
    iy, fy, _ = _axis_taps(h, out_h, img.device, 8, -3)
    wx, wy = _lanczos4_coeffs(fx), _lanczos4_coeffs(fy)
    if is8:
        ax = torch.round(wx * 2048.0).clamp_(-32768, 32767).to(torch.int64)     # saturate_cast<short>(c * INTER_RESIZE_COEF_SCALE)
        ay = torch.round(wy * 2048.0).clamp_(-32768, 32767).to(torch.int64)
        x = img.permute(2, 0, 1).to(torch.int64)                                  # [C, H, W]
        rows = (x[:, :, ix] * ax).sum(-1)                                         # [C, H, out_w]
        out = (rows[:, iy, :] * ay[None, :, :, None]).sum(2)                      # [C, out_h, out_w]
        out = (out + (1 << 21)) >> 22
        return out.clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    x = img.permute(2, 0, 1).float()
    rows = (x[:, :, ix] * wx).sum(-1)
    out = (rows[:, iy, :] * wy[None, :, :, None]).sum(2)
    return torch.round(out).clamp_(0, 65535).to(torch.int32).permute(1, 2, 0).contiguous()


def linear_resize_f32(img, out_h, out_w, use_hip=None):
    """cv2.resize(img, (out_w, out_h), interpolation=cv2.INTER_LINEAR) for float32 HW or HWC tensors.  On a ROCm device one HIP
    kernel (csrc/resize.hip, nesr_resize_f32: 1 to 4 channels) unless use_hip=False selects the torch chain below -- the two agree
    bit for bit (the kernel rounds every product and sum by itself, as the chain's separate operations do)."""
    squeeze = img.dim() == 2
    fits = (img.device.type == "cuda" and img.dtype == torch.float32 and (squeeze or (img.dim() == 3 and 1 <= img.shape[2] <= 4))
            and img.numel() > 0 and out_h > 0 and out_w > 0)
    if use_hip is None:
        use_hip = fits
    if use_hip:
        if not fits:
            raise ValueError(f"linear_resize_f32: the HIP kernel takes a float32 [H, W] or [H, W, 1..4] tensor on the ROCm device, got "
                             f"{img.dtype} {tuple(img.shape)} on {img.device}")
        from . import _lib
        src = img[:, :, None] if squeeze else img
        src = src if _rows_ok(src, (1, 2, 3, 4)) else src.contiguous()
        h, w, c = src.shape
        dst = torch.empty((out_h, out_w, c), dtype=torch.float32, device=img.device)
        _hip_call(src, "nesr_resize_f32", _ptr(src), h, w, c, _row_bytes(src), _ptr(dst), out_h, out_w, _row_bytes(dst), _lib.INTER_LINEAR)
        return dst[:, :, 0] if squeeze else dst
    x = (img[:, :, None] if squeeze else img).permute(2, 0, 1).float()
    h, w = x.shape[1:]

    def axis(n_in, n_out):
        scale = n_in / n_out
        pos = ((torch.arange(n_out, device=img.device, dtype=torch.float64) + 0.5) * scale - 0.5).to(torch.float32)
        i0 = torch.floor(pos)
        f = pos - i0
        i0 = i0.long()
        lo = i0 < 0
        hi = i0 >= n_in - 1
        f = torch.where(lo | hi, torch.zeros_like(f), f)
        i0 = torch.where(lo, torch.zeros_like(i0), torch.where(hi, torch.full_like(i0, n_in - 1), i0))
        return i0, (i0 + 1).clamp_(max=n_in - 1), f

    x0, x1, fx = axis(w, out_w)
    y0, y1, fy = axis(h, out_h)
    rows = x[:, :, x0] * (1.0 - fx) + x[:, :, x1] * fx
    out = rows[:, y0, :] * (1.0 - fy)[None, :, None] + rows[:, y1, :] * fy[None, :, None]
    out = out.permute(1, 2, 0)
    return out[:, :, 0].contiguous() if squeeze else out.contiguous()


# ----------------------------------------------------------------------------------------------- 8-bit resize, cv2's other interpolations
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_LANCZOS4 = 0, 1, 2, 4      # cv2's values


def _cubic_coeffs(frac):
    """cv2 interpolateCubic (A = -0.75) for a float32 tensor of fractional offsets -> [..., 4] float32 weights, every operation in
    float32 and in OpenCV's order (left to right)."""
    A = -0.75
    x = frac
    x1 = x + 1.0
    y = 1.0 - x
    w0 = ((A * x1 - 5.0 * A) * x1 + 8.0 * A) * x1 - 4.0 * A
    w1 = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    w2 = ((A + 2.0) * y - (A + 3.0)) * y * y + 1.0
    w3 = 1.0 - w0 - w1 - w2
    return torch.stack([w0, w1, w2, w3], -1)


def _fixed11(w):
    """saturate_cast<short>(w * INTER_RESIZE_COEF_SCALE): rint(w 2048) as int64."""
    return torch.round(w * 2048.0).clamp_(-32768, 32767).to(torch.int64)


def resize_u8_tables(n_in, n_out, interp):
    """(first index [n_out], integer coefficients [n_out, 1 | 2 | 4 | 8]) of one axis of resize_u8, on the CPU: the tables
    nesr_resize_cv_taps returns.  The position is cv2's, (d + 0.5) n_in / n_out - 0.5 in double, cast to float32, floor + fraction.
      NEAREST  first = min(floor(d n_in / n_out), n_in - 1); one coefficient, 1
      LINEAR   first = s, f = 0 and s clamped when s < 0 or s >= n_in - 1; rint((1 - f) 2048), rint(f 2048)
      CUBIC    first = s - 1, not clamped; the Keys weights (A = -0.75, float32) x 2048, rounded
      LANCZOS4 first = s - 3, not clamped; lanczos4_resize's 11-bit coefficients"""
    cpu = torch.device("cpu")
    if interp == INTER_NEAREST:
        idx = torch.floor(torch.arange(n_out, dtype=torch.float64) * (n_in / n_out)).long().clamp_(max=n_in - 1)
        return idx, torch.ones((n_out, 1), dtype=torch.int64)
    _, frac, i0 = _axis_taps(n_in, n_out, cpu, 1, 0)
    if interp == INTER_LINEAR:
        lo, hi = i0 < 0, i0 >= n_in - 1
        f = torch.where(lo | hi, torch.zeros_like(frac), frac)
        i0 = torch.where(lo, torch.zeros_like(i0), torch.where(hi, torch.full_like(i0, n_in - 1), i0))
        return i0, torch.stack([_fixed11(1.0 - f), _fixed11(f)], -1)
    if interp == INTER_CUBIC:
        return i0 - 1, _fixed11(_cubic_coeffs(frac))
    if interp == INTER_LANCZOS4:
        return i0 - 3, _fixed11(_lanczos4_coeffs(frac))
    raise ValueError(f"resize_u8: interpolation {interp} (INTER_NEAREST 0, INTER_LINEAR 1, INTER_CUBIC 2 or INTER_LANCZOS4 4)")


def _resize_u8_chain(img, out_h, out_w, interp):
    """resize_u8 as torch operations on any device (use_hip=False): integer arithmetic on tables built on the CPU."""
    h, w, c = img.shape
    dev = img.device
    x = img.permute(2, 0, 1).to(torch.int64)                                      # [C, H, W]
    if interp == INTER_LINEAR and w == 2 * out_w and h == 2 * out_h:                # cv2: INTER_LINEAR becomes INTER_AREA at exactly 1/2 x 1/2
        out = (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2] + 2) >> 2
        return out.to(torch.uint8).permute(1, 2, 0).contiguous()
    fx, ax = (t.to(dev) for t in resize_u8_tables(w, out_w, interp))
    fy, ay = (t.to(dev) for t in resize_u8_tables(h, out_h, interp))
    if interp == INTER_NEAREST:
        return img[fy][:, fx].contiguous()
    taps = ax.shape[1]
    ix = (fx[:, None] + torch.arange(taps, device=dev)).clamp_(0, w - 1)            # BORDER_REPLICATE
    iy = (fy[:, None] + torch.arange(taps, device=dev)).clamp_(0, h - 1)
    rows = (x[:, :, ix] * ax).sum(-1)                                               # [C, H, out_w]
    if interp == INTER_LINEAR:                                                      # OpenCV's 8-bit VResizeLinear
        t = rows[:, iy, :] >> 4                                                     # [C, out_h, 2, out_w]
        out = (((ay[None, :, 0, None] * t[:, :, 0]) >> 16) + ((ay[None, :, 1, None] * t[:, :, 1]) >> 16) + 2) >> 2
    else:
        out = ((rows[:, iy, :] * ay[None, :, :, None]).sum(2) + (1 << 21)) >> 22
    return out.clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def resize_u8(img, out_h, out_w, interp, use_hip=None, out=None):
    """cv2.resize(img, (out_w, out_h), interpolation=interp) for an HWC uint8 tensor and cv2's INTER_NEAREST (0), INTER_LINEAR (1),
    INTER_CUBIC (2) or INTER_LANCZOS4 (4) -- the reference's no-model step (nesr/nesr.py:597-605: INTER_CUBIC), the object mask's
    default resize (:732: linear) and the class map's (:720-724: nearest).  OpenCV 4.x's 8-bit arithmetic (resize_u8_tables; the
    linear form's vertical pass is (((b0 (t0 >> 4)) >> 16) + ((b1 (t1 >> 4)) >> 16) + 2) >> 2, and at exactly half size in both
    axes cv2 takes its area filter, (a + b + c + d + 2) >> 2); PARITY UNPINNED like the rest of this module.

    On a ROCm device one HIP kernel (csrc/resize.hip, nesr_resize_cv_u8: 1, 3 or 4 channels, both passes in one launch) unless
    use_hip=False selects the torch chain, which is the specification and runs on CPU tensors too -- the two agree bit for bit.
    Row-strided views and `out` as a view of a canvas work as in lanczos4_resize."""
    if img.dim() != 3:
        raise ValueError(f"resize_u8: an [H, W, C] tensor, got {tuple(img.shape)}")
    if interp not in (INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_LANCZOS4):
        raise ValueError(f"resize_u8: interpolation {interp} (INTER_NEAREST 0, INTER_LINEAR 1, INTER_CUBIC 2 or INTER_LANCZOS4 4)")
    if img.dtype != torch.uint8:
        raise ValueError(f"resize_u8: a uint8 tensor, got {img.dtype}")
    h, w, c = img.shape
    fits = img.device.type == "cuda" and c in (1, 3, 4) and h > 0 and w > 0 and out_h > 0 and out_w > 0
    if out is not None:
        if tuple(out.shape) != (out_h, out_w, c) or out.dtype != img.dtype or out.device != img.device:
            raise ValueError(f"resize_u8: out must be a {img.dtype} [{out_h}, {out_w}, {c}] tensor on {img.device}, got {out.dtype} "
                             f"{tuple(out.shape)} on {out.device}")
        fits = fits and _rows_ok(out, (1, 3, 4))
    if use_hip is None:
        use_hip = fits
    if use_hip:
        if not fits:
            raise ValueError(f"resize_u8: the HIP kernel takes a uint8 [H, W, 1 | 3 | 4] tensor on the ROCm device (out: rows of contiguous "
                             f"pixels), got {img.dtype} {tuple(img.shape)} on {img.device}")
        src = img if _rows_ok(img, (1, 3, 4)) else img.contiguous()
        dst = out if out is not None else torch.empty((out_h, out_w, c), dtype=torch.uint8, device=img.device)
        _hip_call(src, "nesr_resize_cv_u8", _ptr(src), h, w, c, _row_bytes(src), _ptr(dst), out_h, out_w, _row_bytes(dst), int(interp))
        return dst
    res = _resize_u8_chain(img, out_h, out_w, interp)
    if out is not None:
        out.copy_(res)
        return out
    return res


# ----------------------------------------------------------------------------------------------- Gaussian blur
def gaussian_kernel_u8(sigma, ksize=0):
    """Fixed-point Gaussian kernel of OpenCV's 8-bit path: ksize = round(6 sigma + 1) | 1 when not given, float kernel
    exp(-x^2 / 2 sigma^2) normalised, x256 rounded, the centre adjusted so that the taps sum to 256."""
    if ksize <= 0:
        ksize = int(round(sigma * 6 + 1)) | 1
    r = ksize // 2
    small = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
    if sigma <= 0 and ksize in small:              # OpenCV's tabulated small kernels
        k = torch.tensor(small[ksize], dtype=torch.float64)
    else:
        if sigma <= 0:
            sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
        xs = torch.arange(-r, r + 1, dtype=torch.float64)
        k = torch.exp(-(xs * xs) / (2.0 * sigma * sigma))
        k = k / k.sum()
    q = torch.round(k * 256.0).to(torch.int64)
    q[r] += 256 - int(q.sum())
    return q


def gaussian_blur_u8(img, sigma, ksize=0, use_hip=None):
    """cv2.GaussianBlur(img, (ksize, ksize) or (0, 0), sigma) on HWC (or HW) uint8: separable fixed-point filter,
    BORDER_REFLECT_101, one rounding at the end ((v + 2^15) >> 16).  On a ROCm device one HIP kernel (csrc/filters.hip,
    nesr_gaussian_u8: 1 or 3 channels, an odd kernel of at most 31 taps) unless use_hip=False selects the torch composition
    below -- the two agree bit for bit."""
    squeeze = img.dim() == 2
    if use_hip is None:
        n = ksize if ksize > 0 else int(round(sigma * 6 + 1)) | 1
        use_hip = _hip_default(img) and (squeeze or (img.dim() == 3 and img.shape[-1] in (1, 3))) and 1 <= n <= 31 and n % 2 == 1
    if use_hip:
        _hip_require(img, squeeze or (img.dim() == 3 and img.shape[-1] in (1, 3)), "gaussian_blur_u8", "[H, W], [H, W, 1] or [H, W, 3]")
        src = img.contiguous()
        out = torch.empty_like(src)
        if src.numel():
            _hip_call(src, "nesr_gaussian_u8", _ptr(src), src.shape[0], src.shape[1], 1 if squeeze else src.shape[2], float(sigma), int(ksize),
                      _ptr(out))
        return out
    x = (img[:, :, None] if squeeze else img).permute(2, 0, 1).unsqueeze(0)
    k = gaussian_kernel_u8(sigma, ksize).to(img.device)
    r = k.numel() // 2
    h, w = x.shape[-2:]
    xi = x.to(torch.int32)                                                # every partial sum < 2^24
    cols = _reflect101_index(w, r, img.device)
    rows = _reflect101_index(h, r, img.device)
    hp = xi[..., cols]                                                    # [1, C, H, W + 2r]
    hs = sum(int(k[t]) * hp[..., t:t + w] for t in range(2 * r + 1))
    vp = hs[..., rows, :]
    vs = sum(int(k[t]) * vp[..., t:t + h, :] for t in range(2 * r + 1))
    out = ((vs + (1 << 15)) >> 16).clamp_(0, 255).to(torch.uint8).squeeze(0).permute(1, 2, 0)
    return out[:, :, 0].contiguous() if squeeze else out.contiguous()


# ----------------------------------------------------------------------------------------------- colour
def rgb2gray_u8(img):
    """cv2.cvtColor(img, COLOR_RGB2GRAY) on uint8: (R 4899 + G 9617 + B 1868 + 2^13) >> 14."""
    x = img.to(torch.int64)
    return ((x[..., 0] * 4899 + x[..., 1] * 9617 + x[..., 2] * 1868 + (1 << 13)) >> 14).to(torch.uint8)


_D65 = (0.950456, 1.0, 1.088754)
_M = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))


def _lab_f(t):
    return torch.where(t > 0.008856, torch.pow(t.clamp_min(1e-12), 1.0 / 3.0), 7.787 * t + 16.0 / 116.0)


def _srgb_to_linear(c):
    return torch.where(c <= 0.04045, c / 12.92, torch.pow((c + 0.055) / 1.055, 2.4))


def _linear_to_srgb(c):
    return torch.where(c <= 0.0031308, c * 12.92, 1.055 * torch.pow(c.clamp_min(1e-12), 1.0 / 2.4) - 0.055)


def _lab_hip(x, mode, planar_in):
    """nesr_lab_u8 on an [H, W, 3] tensor (planar_in: a [3, H, W] one) -> the other layout when mode has LAB_PLANAR."""
    from . import _lib
    what = "lab2rgb_u8" if mode & _lib.LAB_FROM_LAB else "rgb2lab_u8"
    if planar_in:
        _hip_require(x, x.dim() == 3 and x.shape[0] == 3, what, "[3, H, W] (planar=True)")
    else:
        _hip_require(x, x.dim() == 3 and x.shape[-1] == 3, what, "[H, W, 3]")
    src = x.contiguous()
    h, w = src.shape[1:] if planar_in else src.shape[:2]
    shape = (h, w, 3) if planar_in or not mode & _lib.LAB_PLANAR else (3, h, w)
    out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    if src.numel():
        _hip_call(src, "nesr_lab_u8", _ptr(src), h, w, mode, _ptr(out))
    return out


def rgb2lab_u8(img, linear=False, first_is_blue=False, use_hip=None, planar=False):
    """cv2.cvtColor(img, COLOR_RGB2Lab | COLOR_LRGB2Lab | COLOR_LBGR2Lab) on uint8 -> uint8 (L 255/100, a + 128, b + 128).
    linear=True: no sRGB gamma (the L* variants); first_is_blue=True: channel 0 is taken as blue (the *BGR* variants);
    planar=True: an [H, W, 3] image -> [3, H, W] planes.  On a ROCm device one HIP kernel (csrc/filters.hip, nesr_lab_u8)
    unless use_hip=False selects the torch composition below -- the two agree bit for bit."""
    if use_hip is None:
        use_hip = _hip_default(img) and img.dim() == 3 and img.shape[-1] == 3
    if use_hip:
        from . import _lib
        return _lab_hip(img, (_lib.LAB_LINEAR if linear else 0) | (_lib.LAB_FIRST_IS_BLUE if first_is_blue else 0)
                        | (_lib.LAB_PLANAR if planar else 0), False)
    if planar:
        return rgb2lab_u8(img, linear, first_is_blue, use_hip=False).permute(2, 0, 1).contiguous()
    c = img.float() / 255.0
    if not linear:
        c = _srgb_to_linear(c)
    r, g, b = (c[..., 2], c[..., 1], c[..., 0]) if first_is_blue else (c[..., 0], c[..., 1], c[..., 2])
    X = (_M[0][0] * r + _M[0][1] * g + _M[0][2] * b) / _D65[0]
    Y = _M[1][0] * r + _M[1][1] * g + _M[1][2] * b
    Z = (_M[2][0] * r + _M[2][1] * g + _M[2][2] * b) / _D65[2]
    fx, fy, fz = _lab_f(X), _lab_f(Y), _lab_f(Z)
    L = torch.where(Y > 0.008856, 116.0 * fy - 16.0, 903.3 * Y)
    A = 500.0 * (fx - fy) + 128.0
    B = 200.0 * (fy - fz) + 128.0
    out = torch.stack([L * 255.0 / 100.0, A, B], -1)
    return torch.round(out).clamp_(0, 255).to(torch.uint8)


def lab2rgb_u8(lab, linear=False, first_is_blue=False, use_hip=None, planar=False):
    """cv2.cvtColor(lab, COLOR_Lab2RGB | COLOR_Lab2LRGB | COLOR_Lab2LBGR) on uint8 -> uint8; planar=True: [3, H, W] Lab
    planes -> an [H, W, 3] image.  HIP on a ROCm device (nesr_lab_u8) unless use_hip=False, as rgb2lab_u8."""
    if use_hip is None:
        use_hip = _hip_default(lab) and lab.dim() == 3 and lab.shape[0 if planar else -1] == 3
    if use_hip:
        from . import _lib
        return _lab_hip(lab, _lib.LAB_FROM_LAB | (_lib.LAB_LINEAR if linear else 0) | (_lib.LAB_FIRST_IS_BLUE if first_is_blue else 0)
                        | (_lib.LAB_PLANAR if planar else 0), planar)
    if planar:
        return lab2rgb_u8(lab.permute(1, 2, 0), linear, first_is_blue, use_hip=False)
    x = lab.float()
    L = x[..., 0] * 100.0 / 255.0
    a = x[..., 1] - 128.0
    b = x[..., 2] - 128.0
    fy = (L + 16.0) / 116.0
    Y = torch.where(L <= 8.0, L / 903.3, fy * fy * fy)
    fy = torch.where(L <= 8.0, 7.787 * Y + 16.0 / 116.0, fy)
    fx = fy + a / 500.0
    fz = fy - b / 200.0

    def inv(f):
        return torch.where(f <= 6.0 / 29.0, (f - 16.0 / 116.0) / 7.787, f * f * f)

    X = inv(fx) * _D65[0]
    Z = inv(fz) * _D65[2]
    r = 3.240479 * X - 1.537150 * Y - 0.498535 * Z
    g = -0.969256 * X + 1.875991 * Y + 0.041556 * Z
    bl = 0.055648 * X - 0.204043 * Y + 1.057311 * Z
    c = torch.stack([bl, g, r] if first_is_blue else [r, g, bl], -1).clamp_(0, 1)
    if not linear:
        c = _linear_to_srgb(c)
    return torch.round(c * 255.0).clamp_(0, 255).to(torch.uint8)


# ----------------------------------------------------------------------------------------------- CLAHE
def clahe_tile_size(h, w, grid=(8, 8)):
    """(tile height, tile width) cv2's CLAHE uses for an h x w image (clahe.cpp, CLAHE_Impl::apply)."""
    gx, gy = grid
    ph, pw = (gy - h % gy, gx - w % gx) if (h % gy or w % gx) else (0, 0)
    return (h + ph) // gy, (w + pw) // gx


def clahe_u8(gray, clip_limit=2.0, grid=(8, 8), use_hip=None):
    """cv2.createCLAHE(clipLimit, tileGridSize).apply(gray) on an HW uint8 tensor: the image is padded (REFLECT_101) to a
    multiple of the grid, every tile gets a clipped, redistributed histogram and a look-up table, and a pixel takes the
    bilinear blend of the four surrounding tiles' tables.  On a ROCm device the two HIP kernels of csrc/imgproc.hip
    (nesr_clahe_u8) unless use_hip=False selects the torch composition below -- the two agree bit for bit."""
    h, w = gray.shape
    gx, gy = grid
    if use_hip is None:
        use_hip = gray.device.type == "cuda" and gray.dtype == torch.uint8
    if use_hip:
        src = gray.contiguous()
        out = torch.empty_like(src)
        lut = torch.empty((gy * gx * 256,), dtype=torch.float32, device=src.device)
        _hip_call(src, "nesr_clahe_u8", src, h, w, float(clip_limit), gx, gy, lut, out)
        return out
    # clahe.cpp: only when BOTH sides divide by the grid is the image used as it is; otherwise copyMakeBorder pads the bottom by
    # tilesY - h % tilesY and the right by tilesX - w % tilesX -- a side that does divide gets a whole extra tilesY / tilesX pixels
    ph, pw = (gy - h % gy, gx - w % gx) if (h % gy or w % gx) else (0, 0)
    src = gray
    if ph or pw:
        ry = torch.arange(h + ph, device=gray.device)
        rx = torch.arange(w + pw, device=gray.device)
        ry = torch.where(ry >= h, 2 * (h - 1) - ry, ry).clamp_(0, h - 1)              # BORDER_REFLECT_101 at the bottom / right
        rx = torch.where(rx >= w, 2 * (w - 1) - rx, rx).clamp_(0, w - 1)
        src = gray[ry][:, rx]
    H, W = src.shape
    th, tw = H // gy, W // gx
    area = th * tw
    clip = max(int(clip_limit * area / 256.0), 1)
    tiles = src.reshape(gy, th, gx, tw).permute(0, 2, 1, 3).reshape(gy * gx, area).long()
    hist = torch.zeros((gy * gx, 256), dtype=torch.int64, device=gray.device)
    hist.scatter_add_(1, tiles, torch.ones_like(tiles))
    clipped = (hist - clip).clamp_min(0).sum(1)
    hist = hist.clamp_max(clip)
    batch = clipped // 256
    residual = clipped - batch * 256
    hist = hist + batch[:, None]
    step = torch.where(residual > 0, (256 // residual.clamp_min(1)).clamp_min(1), torch.ones_like(residual))
    i = torch.arange(256, device=gray.device)[None, :]
    # one extra count at bins 0, step, 2 step, ... until `residual` of them have been handed out
    extra = ((i % step[:, None]) == 0) & ((i // step[:, None]) < residual[:, None])
    hist = hist + extra.long()
    lut = torch.round(hist.cumsum(1).float() * (255.0 / area)).clamp_(0, 255)            # [tiles, 256]
    lut = lut.reshape(gy, gx, 256)
    ys = torch.arange(h, device=gray.device).float() / th - 0.5
    xs = torch.arange(w, device=gray.device).float() / tw - 0.5
    ty1, tx1 = torch.floor(ys), torch.floor(xs)
    ya, xa = ys - ty1, xs - tx1
    ty1, tx1 = ty1.long(), tx1.long()
    ty2, tx2 = (ty1 + 1).clamp(0, gy - 1), (tx1 + 1).clamp(0, gx - 1)
    ty1, tx1 = ty1.clamp(0, gy - 1), tx1.clamp(0, gx - 1)
    v = gray.long()
    l11 = lut[ty1[:, None], tx1[None, :], v]
    l12 = lut[ty1[:, None], tx2[None, :], v]
    l21 = lut[ty2[:, None], tx1[None, :], v]
    l22 = lut[ty2[:, None], tx2[None, :], v]
    xa, ya = xa[None, :], ya[:, None]
    res = (l11 * (1 - xa) + l12 * xa) * (1 - ya) + (l21 * (1 - xa) + l22 * xa) * ya
    return torch.round(res).clamp_(0, 255).to(torch.uint8)


# ----------------------------------------------------------------------------------------------- non-local means
def _reflect101_index(n, r, device):
    """Source index of positions -r .. n + r - 1 under BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba)."""
    idx = torch.arange(-r, n + r, device=device)
    if n == 1:
        return torch.zeros_like(idx)
    period = 2 * (n - 1)
    idx = idx % period
    return torch.where(idx >= n, period - idx, idx)


def _reflect101_pad(x, r):
    """[..., H, W] tensor -> padded by r on both axes with BORDER_REFLECT_101 (any r, also larger than the image)."""
    h, w = x.shape[-2:]
    return x[..., _reflect101_index(h, r, x.device), :][..., _reflect101_index(w, r, x.device)]


def nl_means_weights(C, h, template=7, search=21):
    """(int64 table of weights over the binned template distance, shift): OpenCV's almost_dist2weight -- round(M exp(-d / (h^2 C)))
    with the fixed-point multiplier M = INT_MAX // (search^2 * 255), 0 below 0.001 M; bins = distance >> shift, 2^shift the next
    power of two above template^2."""
    tsq = template * template
    shift = 0
    while (1 << shift) < tsq:
        shift += 1
    mult = (1 << shift) / tsq                                                        # almost_dist -> actual dist
    max_est = search * search * 255
    M = (2 ** 31 - 1) // max_est                                                     # fixed_point_mult: 19,096 for a 21x21 search window
    max_dist = 255 * 255 * C
    nbins = ((max_dist * tsq) >> shift) + 1                                          # bins of the 'almost' distance
    d = torch.arange(nbins, dtype=torch.float64) * mult
    wt = torch.round(M * torch.exp(-d / (h * h * C)))
    wt = torch.where(wt < 0.001 * M, torch.zeros_like(wt), wt).to(torch.int64)
    return wt, shift


def fast_nl_means_u8(planes, h, template=7, search=21, rows_per_block=0, use_hip=None):
    """cv2.fastNlMeansDenoising on [C, H, W] uint8 planes treated as ONE C-channel image (C = 1: the L plane, C = 2: the ab
    planes of fastNlMeansDenoisingColored): for every pixel and every offset of the search window the summed squared
    difference of the template windows (over all channels) is binned (>> 6 for the 7x7 template, as OpenCV's
    'almost' distance), turned into an integer weight round(M exp(-d / (h^2 C))) (0 below 0.001 M) and the pixels of the
    search window are averaged with these weights in integer arithmetic (rounded division).

    On the ROCm device with the reference's window sizes (7, 21: nesr/nesr.py:674) this is one HIP kernel
    (csrc/imgproc.hip, nesr_nl_means_u8); the torch composition below is kept for other sizes, the CPU and the tests
    (use_hip=False) -- the two agree bit for bit."""
    C, H, W = planes.shape
    wt, shift = nl_means_weights(C, h, template, search)
    nbins = wt.numel()
    if use_hip is None:
        use_hip = planes.device.type == "cuda" and template == 7 and search == 21 and 1 <= C <= 3
    if use_hip:
        nz = int((wt != 0).sum().item())                                             # the weights fall monotonically to 0: a short table is enough
        lut = wt[:max(nz + 1, 1)].to(torch.int32).to(planes.device)
        src = planes.contiguous()
        out = torch.empty_like(src)
        _hip_call(src, "nesr_nl_means_u8", src, C, H, W, template, search, lut, lut.numel(), out)
        return out
    tr, sr = template // 2, search // 2
    border = tr + sr
    x = _reflect101_pad(planes.long(), border)                                      # [C, H + 2b, W + 2b]
    wt = wt.to(planes.device)
    centre = x[:, sr:sr + H + 2 * tr, sr:sr + W + 2 * tr]                            # template-padded view of the image
    acc = torch.zeros((C, H, W), dtype=torch.int64, device=planes.device)
    wsum = torch.zeros((H, W), dtype=torch.int64, device=planes.device)
    box = torch.ones((1, 1, template, template), dtype=torch.float32, device=planes.device)   # sums < 2^24: exact in f32
    for dy in range(-sr, sr + 1):
        for dx in range(-sr, sr + 1):
            other = x[:, sr + dy:sr + dy + H + 2 * tr, sr + dx:sr + dx + W + 2 * tr]
            sq = ((centre - other) ** 2).sum(0).to(torch.float32)
            dist = F.conv2d(sq[None, None], box)[0, 0].to(torch.int64)               # [H, W] template sums
            wgt = wt[(dist >> shift).clamp_max(nbins - 1)]
            wsum += wgt
            acc += wgt[None] * x[:, border + dy:border + dy + H, border + dx:border + dx + W]
    out = (acc + (wsum // 2)[None]) // wsum.clamp_min(1)[None]
    return out.clamp_(0, 255).to(torch.uint8)


def fast_nl_means_colored_u8(img, h, h_color, template=7, search=21, use_hip=None):
    """cv2.fastNlMeansDenoisingColored(img, None, h, hColor, template, search): COLOR_LBGR2Lab (no gamma, channel 0 taken
    as blue -- whatever order the caller's image is in: the reference hands it RGB, nesr/nesr.py:674), non-local means on
    L with h and on (a, b) with hColor, COLOR_Lab2LBGR.  use_hip goes to every step."""
    p = rgb2lab_u8(img, linear=True, first_is_blue=True, use_hip=use_hip, planar=True)
    L = fast_nl_means_u8(p[0:1], h, template, search, use_hip=use_hip)
    ab = fast_nl_means_u8(p[1:3], h_color, template, search, use_hip=use_hip)
    return lab2rgb_u8(torch.cat([L, ab], 0), linear=True, first_is_blue=True, use_hip=use_hip, planar=True)


# ----------------------------------------------------------------------------------------------- the pipeline's filters
def preprocess_image(img, denoise_level=0.5, use_hip=None):
    """SuperResolutionPipeline._preprocess_image (nesr/nesr.py:668-689) on an HWC uint8 RGB device tensor.  On a ROCm device
    one C call (nesr_preprocess_u8: the Lab, NL-means and CLAHE kernels in stream order, device scratch from here) unless
    use_hip=False selects the torch chain below, every step of it torch -- the two agree bit for bit."""
    if use_hip is None:
        use_hip = _hip_default(img) and img.dim() == 3 and img.shape[-1] == 3
    if use_hip:
        from . import _lib
        _hip_require(img, img.dim() == 3 and img.shape[-1] == 3, "preprocess_image", "[H, W, 3]")
        src = img.contiguous()
        h, w = src.shape[:2]
        out = torch.empty_like(src)
        if src.numel():
            nbytes = _lib.load().nesr_preprocess_scratch_bytes(h, w)
            scratch = torch.empty((nbytes,), dtype=torch.uint8, device=src.device)
            _hip_call(src, "nesr_preprocess_u8", _ptr(src), h, w, float(denoise_level), _ptr(scratch), nbytes, _ptr(out))
        return out
    if denoise_level > 0:
        strength = denoise_level * 10
        img = fast_nl_means_colored_u8(img, strength, strength, 7, 21, use_hip=False)
    lab = rgb2lab_u8(img, use_hip=False)                                             # COLOR_RGB2LAB
    L = clahe_u8(lab[..., 0].contiguous(), 2.0, (8, 8), use_hip=False)
    lab = torch.cat([L[..., None], lab[..., 1:]], -1)
    return lab2rgb_u8(lab, use_hip=False)                                            # COLOR_LAB2RGB


def postprocess_image(img, adaptive_sharpening=True, use_hip=None):
    """SuperResolutionPipeline._postprocess_image (nesr/nesr.py:1056-1084): unsharp (1.5 img - 0.5 blur_3) where the local
    detail |gray - blur_2(gray)| exceeds 10, the image itself elsewhere.  On a ROCm device one fused HIP kernel
    (csrc/filters.hip, nesr_postprocess_u8) unless use_hip=False selects the torch chain below -- the two agree bit for bit."""
    if not adaptive_sharpening:
        return img
    if use_hip is None:
        use_hip = _hip_default(img) and img.dim() == 3 and img.shape[-1] == 3
    if use_hip:
        _hip_require(img, img.dim() == 3 and img.shape[-1] == 3, "postprocess_image", "[H, W, 3]")
        src = img.contiguous()
        out = torch.empty_like(src)
        if src.numel():
            _hip_call(src, "nesr_postprocess_u8", _ptr(src), src.shape[0], src.shape[1], 1, _ptr(out))
        return out
    gray = rgb2gray_u8(img)
    variance = (gray.to(torch.int16) - gaussian_blur_u8(gray, 2.0, use_hip=False).to(torch.int16)).clamp_(0, 255)   # cv2.subtract saturates; convertScaleAbs keeps it
    blurred = gaussian_blur_u8(img, 3.0, use_hip=False)
    sharpened = torch.round(img.float() * 1.5 - blurred.float() * 0.5).clamp_(0, 255).to(torch.uint8)   # addWeighted: saturate_cast<uchar>
    mask = (variance > 10)[..., None]
    return torch.where(mask, sharpened, img)


# ----------------------------------------------------------------------------------------------- segmentation mask stage, ensemble
def dilate3x3_u8(mask, use_hip=None):
    """cv2.dilate(mask, np.ones((3, 3), np.uint8), iterations=1) on an HW uint8 tensor (nesr/nesr.py:735-736): the max over the
    neighbours that lie inside the image (cv2's default border value for a dilate never wins a max).  A torch chain only: the
    library fuses the dilate into segment_enhance's stencil and has no entry for it alone, so use_hip=True is an error."""
    if use_hip:
        raise ValueError("dilate3x3_u8: the HIP kernel takes the dilate only fused into segment_enhance (nesr_segment_enhance_u8); "
                         "there is no entry for it alone")
    if mask.dim() != 2 or mask.dtype != torch.uint8:
        raise ValueError(f"dilate3x3_u8: an [H, W] uint8 tensor, got {mask.dtype} {tuple(mask.shape)}")
    p = F.pad(mask.to(torch.int16), (1, 1, 1, 1), value=-1)
    h, w = mask.shape
    out = p[1:h + 1, 1:w + 1]
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, p[dy:dy + h, dx:dx + w])
    return out.to(torch.uint8)


SEGMENT_MAX_SIZE = 1024      # nesr/nesr.py:705: above it the segmenter sees a downscaled frame


def segment_enhance(img, seg_map, use_hip=None):
    """The image half of SuperResolutionPipeline._segment_and_enhance (nesr/nesr.py:726-747) on an HWC uint8 RGB tensor:
    seg_map is the segmenter's class map (any integer dtype, a tensor or an ndarray, on the host or the device), and

        object_mask = (seg_map > 0).astype(np.uint8)                        :731
        object_mask = cv2.resize(object_mask, (w, h))                        :732   resize_u8(INTER_LINEAR); {0, 1} again
        object_mask = cv2.dilate(object_mask, np.ones((3, 3)))               :735   dilate3x3_u8
        sharpened = addWeighted(img, 1.5, GaussianBlur(img, (0, 0), 3), -0.5)  :739   postprocess_image's value
        np.where(object_mask[..., None] == 1, sharpened, img)                :743

    For a frame whose longer side exceeds 1024 the reference runs the segmenter on a downscaled frame and resizes the class map back
    with INTER_NEAREST (:703-724); nearest commutes with `> 0`, so that step is done here on the mask, resize_u8(INTER_NEAREST).  In
    the reference that branch hands an int64 array to cv2.resize, which throws, and its except clause silently skips the whole
    stage; that throw is NOT reproduced: the stage runs.  The class map comes from the segmenter, segformer.SegFormer.segment on the HIP
    path (or any callable of the caller's).

    On a ROCm device one C call (nesr_segment_enhance_u8: the mask's linear resize and one fused stencil, csrc/filters.hip) unless
    use_hip=False selects the torch chain below -- the two agree bit for bit."""
    if img.dim() != 3 or img.shape[-1] != 3 or img.dtype != torch.uint8:
        raise ValueError(f"segment_enhance: an [H, W, 3] uint8 tensor, got {img.dtype} {tuple(img.shape)}")
    seg = torch.as_tensor(seg_map)
    if seg.dim() != 2 or seg.dtype.is_floating_point or seg.dtype == torch.bool or seg.numel() == 0:
        raise ValueError(f"segment_enhance: the class map is an [h, w] integer array, got {seg.dtype} {tuple(seg.shape)}")
    if use_hip is None:
        use_hip = _hip_default(img)
    if use_hip:
        _hip_require(img, True, "segment_enhance", "[H, W, 3]")
    h, w = img.shape[:2]
    if img.numel() == 0:
        return img
    mask = (seg > 0).to(torch.uint8).to(img.device).contiguous()
    if max(h, w) > SEGMENT_MAX_SIZE and tuple(mask.shape) != (h, w):
        mask = resize_u8(mask[:, :, None], h, w, INTER_NEAREST, use_hip=use_hip)[:, :, 0]
    if use_hip:
        from . import _lib
        src = img.contiguous()
        out = torch.empty_like(src)
        nbytes = _lib.load().nesr_segment_enhance_scratch_bytes(h, w)
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=src.device)
        _hip_call(src, "nesr_segment_enhance_u8", _ptr(src), h, w, _ptr(mask), mask.shape[0], mask.shape[1], _ptr(scratch), nbytes, _ptr(out))
        return out
    if tuple(mask.shape) != (h, w):
        mask = resize_u8(mask[:, :, None], h, w, INTER_LINEAR, use_hip=False)[:, :, 0]
    mask = dilate3x3_u8(mask)
    blurred = gaussian_blur_u8(img, 3.0, use_hip=False)
    sharpened = torch.round(img.float() * 1.5 - blurred.float() * 0.5).clamp_(0, 255).to(torch.uint8)
    return torch.where((mask == 1)[..., None], sharpened, img)


def ensemble_results(images, use_hip=None):
    """SuperResolutionPipeline._ensemble_results (nesr/nesr.py:1033-1054) on a list of HWC uint8 tensors:

        if len(images) == 1: return images[0]                                             :1035   as it is
        target_h, target_w = max([(img.shape[0], img.shape[1]) for img in images])       :1039   max over TUPLES: lexicographic
        every other image: cv2.resize(img, (target_w, target_h), INTER_LANCZOS4)          :1044   lanczos4_resize
        ensemble += img.astype(np.float32) * weights[i];  ensemble.astype(np.uint8)       :1052   float32 mean, truncated

    The target is restated as written: Python's max of (h, w) tuples is the tallest image's size (ties: the widest of those), not
    the per-axis maximum.  The mean is NumPy 1.x's arithmetic, every step rounded to float32: w = float32(1 / n), acc = 0, acc =
    fl32(acc + fl32(fl32(x) w)) in order, truncated toward zero, not rounded (n <= 8 copies of one image still give it back: float32(1 / n)
    is exact or rounded up; tests/test_stages_host.py counts it).
    NumPy >= 2 would promote the product to float64 (the weight is a float64 scalar); the NumPy 1.x result is the one restated.

    On a ROCm device one elementwise HIP kernel for up to 8 images (csrc/filters.hip, nesr_ensemble_u8) unless use_hip=False
    selects the torch chain below -- the two agree bit for bit."""
    images = list(images)
    if not images:
        raise ValueError("ensemble_results: no image")
    if len(images) == 1:
        return images[0]
    for im in images:
        if im.dim() != 3 or im.dtype != torch.uint8 or im.shape[2] != images[0].shape[2] or im.device != images[0].device:
            raise ValueError("ensemble_results: [H, W, C] uint8 tensors with one channel count on one device")
    th, tw = max([(int(im.shape[0]), int(im.shape[1])) for im in images])
    fits = _hip_default(images[0]) and len(images) <= 8 and images[0].numel() > 0
    if use_hip is None:
        use_hip = fits
    if use_hip and not fits:
        raise ValueError(f"ensemble_results: the HIP kernel takes 2 to 8 uint8 [H, W, C] tensors on the ROCm device, got {len(images)} of "
                         f"{images[0].dtype} on {images[0].device}")
    lanczos_hip = use_hip and images[0].shape[2] in (1, 3, 4)
    aligned = [im if (im.shape[0], im.shape[1]) == (th, tw) else lanczos4_resize(im, th, tw, use_hip=lanczos_hip) for im in images]
    if use_hip:
        import ctypes
        aligned = [im.contiguous() for im in aligned]
        out = torch.empty_like(aligned[0])
        ptrs = (ctypes.c_void_p * len(aligned))(*[im.data_ptr() for im in aligned])
        _hip_call(out, "nesr_ensemble_u8", ptrs, len(aligned), th, tw, int(out.shape[2]), _ptr(out))
        return out
    wgt = torch.tensor(1.0 / len(aligned), dtype=torch.float64).to(torch.float32).item()     # float32(1 / n), exactly representable in a Python float
    acc = torch.zeros(aligned[0].shape, dtype=torch.float32, device=aligned[0].device)
    for im in aligned:
        acc = acc + im.to(torch.float32) * wgt
    return acc.to(torch.uint8)


# ----------------------------------------------------------------------------------------------- JPEG
def _encode_file_hip(frame, entry, args, need, cap, who):
    """One run of a file encoder's entry, `args` then the scratch of `need` bytes, the buffer of `cap` bytes and the two words
    -> the file's bytes; NesrNoFitError (with the size the device reported) when the file needs more.  Two transfers come back: the
    16 bytes of the length and status words, then exactly the file."""
    from . import _lib
    scratch = torch.empty(need, dtype=torch.uint8, device=frame.device)
    out = torch.empty(cap, dtype=torch.uint8, device=frame.device)
    words = torch.empty(2, dtype=torch.int64, device=frame.device)
    _hip_call(frame, entry, *args, _ptr(scratch), need, _ptr(out), cap, _ptr(words))
    length, status = (int(v) for v in words.cpu())            # D2H: 16 bytes (waits for the encode)
    if status != 0:
        raise _lib.NesrNoFitError(length, cap, who)
    return out[:length].cpu().numpy().tobytes()               # D2H: the file


def _jpeg_encode_hip(frame, quality, bgr, cap, options=None):
    """One run of nesr_jpeg_encode_u8 (csrc/jpeg.hip) into a buffer of `cap` bytes -> the file's bytes (_encode_file_hip).
    options: (sampling, optimize, restart_interval) for nesr_jpeg_encode_ex_u8, None for the defaults."""
    from . import _lib
    h, w, c = frame.shape
    lib = _lib.load()
    if options is None:
        entry, opt, need = "nesr_jpeg_encode_u8", int(quality), int(lib.nesr_jpeg_scratch_bytes(h, w, c))
    else:
        import ctypes
        sampling, optimize, restart_interval = options
        opts = _lib.JpegOpts(int(quality), _lib.JPEG_SAMPLING[sampling], int(bool(optimize)), int(restart_interval))
        entry, opt, need = "nesr_jpeg_encode_ex_u8", ctypes.byref(opts), int(lib.nesr_jpeg_scratch_bytes_ex(h, w, c, ctypes.byref(opts)))
    args = (_ptr(frame), _row_bytes(frame), h, w, c, _lib.ORDER_BGR if bgr else _lib.ORDER_RGB, opt)
    return _encode_file_hip(frame, entry, args, need, cap, "nesr_jpeg_encode_u8")


def encode_jpeg_u8(frame, quality=95, order="rgb", use_hip=None, *, sampling="4:2:0", optimize=False, restart_interval=0):
    """cv2.imwrite(path.jpg, frame)'s bytes (standalone/direct_esrgan.py:169, nesr/nesr.py:646; cv2's defaults: quality 95, 4:2:0,
    baseline, standard Huffman tables) for an [H, W, 3] (order "rgb" or "bgr": the channel that comes first), [H, W, 1] or [H, W]
    uint8 frame -> bytes.

    A uint8 tensor on the ROCm device goes through the HIP kernels (csrc/jpeg.hip, nesr_jpeg_encode_u8), a row-strided window
    (frame[y0:y1, x0:x1]) as it is: the frame stays on the device and only the length words and the file come back.  The output
    buffer starts at H W C // 2 + 4096 bytes; when the file does not fit, the call runs once more at the size the device reported.
    use_hip=False, a CPU tensor or an ndarray: Pillow's libjpeg-turbo, whose bytes the kernels reproduce (tests/jpeg_ref.py is
    pinned against both); without Pillow that raises -- there is no third route.

    sampling "4:2:0" | "4:2:2" | "4:4:4" (cv2's IMWRITE_JPEG_SAMPLING_FACTOR; a gray frame ignores it), optimize (IMWRITE_JPEG_OPTIMIZE:
    Huffman tables built for the frame, on the device) and restart_interval in MCUs, 0 .. 65535 (IMWRITE_JPEG_RST_INTERVAL) take the
    same two routes: nesr_jpeg_encode_ex_u8, or Pillow's subsampling, optimize and restart_marker_blocks
    (tests/jpeg_options_ref.py is pinned against both).  The defaults are the call without them."""
    if order not in ("rgb", "bgr"):
        raise ValueError(f"encode_jpeg_u8: order must be 'rgb' or 'bgr', got {order!r}")
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"encode_jpeg_u8: quality {quality} outside 1..100")
    if sampling not in ("4:2:0", "4:2:2", "4:4:4"):
        raise ValueError(f"encode_jpeg_u8: sampling must be '4:2:0', '4:2:2' or '4:4:4', got {sampling!r} (4:4:0 and 4:1:1 are not encoded)")
    if not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"encode_jpeg_u8: restart_interval {restart_interval} outside 0..65535 MCUs")
    is_tensor = isinstance(frame, torch.Tensor)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    if frame.ndim != 3 or frame.shape[2] not in (1, 3) or min(frame.shape) < 1 or max(frame.shape[:2]) > 65535 or str(frame.dtype).split(".")[-1] != "uint8":
        raise ValueError(f"encode_jpeg_u8: an [H, W, 3], [H, W, 1] or [H, W] uint8 frame of at most 65535 x 65535 pixels, got {frame.dtype} "
                         f"{tuple(frame.shape)}")
    fits = is_tensor and _hip_default(frame)
    if use_hip is None:
        use_hip = fits
    if use_hip:
        from . import _lib
        if not fits:
            raise ValueError(f"encode_jpeg_u8: the HIP kernels take a uint8 tensor on the ROCm device, got {frame.dtype} on "
                             f"{frame.device if is_tensor else 'the host'}")
        src = frame if _rows_ok(frame, (1, 3)) else frame.contiguous()
        h, w, c = src.shape
        # the default options go the way they always went; anything else names its options
        plain = (sampling == "4:2:0" or c == 1) and not optimize and not int(restart_interval)
        options = () if plain else ((sampling, bool(optimize), int(restart_interval)),)
        try:
            return _jpeg_encode_hip(src, quality, order == "bgr", h * w * c // 2 + 4096, *options)
        except _lib.NesrNoFitError as e:
            return _jpeg_encode_hip(src, quality, order == "bgr", e.needed, *options)
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("encode_jpeg_u8: the host route needs Pillow (the device route: a uint8 tensor on the ROCm device)") from e
    import io
    arr = frame.cpu().numpy() if is_tensor else frame
    arr = arr[:, :, 0] if arr.shape[2] == 1 else (arr[:, :, ::-1] if order == "bgr" else arr)
    buf = io.BytesIO()
    import numpy as np
    extra = {"subsampling": sampling} if arr.ndim == 3 and sampling != "4:2:0" else {}
    if optimize:
        extra["optimize"] = True
    if int(restart_interval):
        extra["restart_marker_blocks"] = int(restart_interval)
    Image.fromarray(np.ascontiguousarray(arr)).save(buf, format="JPEG", quality=int(quality), **extra)
    return buf.getvalue()


# ----------------------------------------------------------------------------------------------- PNG
def _png_encode_hip(frame, depth, bgr, cap=None):
    """One run of nesr_png_encode (csrc/png.hip) on an [H, W, C] device tensor (uint8, or 16-bit samples in 2-byte elements) into a
    buffer of `cap` bytes (default nesr_png_bound, which always fits) -> the file's bytes (_encode_file_hip)."""
    from . import _lib
    h, w, c = frame.shape
    lib = _lib.load()
    need = int(lib.nesr_png_scratch_bytes(h, w, c, depth))
    if cap is None:
        cap = int(lib.nesr_png_bound(h, w, c, depth))
    args = (_ptr(frame), _row_bytes(frame), h, w, c, depth, _lib.ORDER_BGR if bgr else _lib.ORDER_RGB)
    return _encode_file_hip(frame, "nesr_png_encode", args, need, cap, "nesr_png_encode")


def _png_chunk(kind, payload):
    import struct
    import zlib
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def encode_png(frame, order="rgb", use_hip=None):
    """cv2.imwrite(path.png, frame) (standalone/superres_project.py:203-206, nesr/nesr.py:619-625, standalone/direct_esrgan.py:169 for a
    PNG input) for an [H, W], [H, W, 1], [H, W, 3] or [H, W, 4] frame (order "rgb" or "bgr": the channel that comes first; alpha stays
    last) -> the file's bytes.  8 bit: uint8.  16 bit: as frame_io holds it, an int16 tensor carrying the uint16 bit pattern, or
    torch.uint16 / numpy uint16.  The file is lossless: a standard decoder returns the frame bit for bit (in R G B (A) order).

    A tensor on the ROCm device goes through the HIP kernels (csrc/png.hip, nesr_png_encode), a row-strided window
    (frame[y0:y1, x0:x1]) as it is: the frame stays on the device and only the length words and the file come back.  The output
    buffer is nesr_png_bound, the exact worst case, so one run always fits.  Its bytes are those of tests/png_ref.py: adaptive row
    filters, deflate in independent 32 KiB chunks with distance-1 matches.
    use_hip=False, a CPU tensor or an ndarray: cv2's default settings restated with the standard library -- the Sub filter on every
    row, zlib.compressobj(1, DEFLATED, 15, 8, Z_RLE), one IDAT.  That file holds THE SAME PIXELS as the device route's and DIFFERENT
    BYTES (neither is cv2's own: zlib's output depends on its version)."""
    if order not in ("rgb", "bgr"):
        raise ValueError(f"encode_png: order must be 'rgb' or 'bgr', got {order!r}")
    is_tensor = isinstance(frame, torch.Tensor)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    kind = str(frame.dtype).split(".")[-1]
    depth = {"uint8": 8, "int16": 16, "uint16": 16}.get(kind) if is_tensor or kind != "int16" else None
    if frame.ndim != 3 or frame.shape[2] not in (1, 3, 4) or min(frame.shape) < 1 or max(frame.shape[:2]) > 65535 or depth is None:
        raise ValueError(f"encode_png: an [H, W], [H, W, 1], [H, W, 3] or [H, W, 4] uint8 or 16-bit frame of at most 65535 x 65535 pixels, got "
                         f"{frame.dtype} {tuple(frame.shape)}")
    fits = is_tensor and frame.device.type == "cuda"
    if use_hip is None:
        use_hip = fits
    if use_hip:
        if not fits:
            raise ValueError(f"encode_png: the HIP kernels take a tensor on the ROCm device, got {frame.dtype} on "
                             f"{frame.device if is_tensor else 'the host'}")
        src = frame if _rows_ok(frame, (1, 3, 4)) else frame.contiguous()
        return _png_encode_hip(src, depth, order == "bgr")
    import struct
    import zlib
    import numpy as np
    arr = frame.cpu() if is_tensor else frame
    if is_tensor:
        arr = (arr.view(torch.int16) if depth == 16 else arr).numpy()
    arr = arr.view(np.uint16) if depth == 16 else arr
    h, w, c = arr.shape
    if order == "bgr" and c >= 3:
        arr = np.concatenate([arr[:, :, 2::-1], arr[:, :, 3:]], axis=2)
    bpp = c * depth // 8
    raw = np.ascontiguousarray(arr.astype(">u2") if depth == 16 else arr).view(np.uint8).reshape(h, w * bpp)
    rows = np.empty((h, 1 + w * bpp), np.uint8)
    rows[:, 0] = 1                                            # Sub on every row: cv2's IMWRITE_PNG_STRATEGY default path
    rows[:, 1:] = raw
    rows[:, 1 + bpp:] -= raw[:, :-bpp]
    deflate = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    stream = deflate.compress(rows.tobytes()) + deflate.flush()
    ihdr = struct.pack(">IIBBBBB", w, h, depth, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", stream) + _png_chunk(b"IEND", b"")


# ----------------------------------------------------------------------------------------------- PNG in
# What inflate=None sends to the device inflater (profiles/png_decode/bench_png_decode.json).  A segment is walked
# by one lane, about 1.6 us per compressed byte over both passes, and all segments run side by side; the host needs about 11 us per byte
# of the file.  So the device wins only when the largest segment is small AND small against the file: it won at every measured file with
# file / largest segment >= 379 (largest segment up to 28,974 bytes) and lost at every one with that ratio <= 188.
PNG_DEVICE_SEGMENT_MAX = 33 * 1024     # compressed bytes of the largest segment: encode_png's own chunks (<= 32.8 KB) and nothing larger
PNG_DEVICE_MIN_RATIO = 384             # file bytes / largest segment's bytes: just above the smallest ratio at which the device won


def _png_default_on_device(info, segs, nbytes):
    """inflate=None: True when the file goes to the device inflater (a contiguous plan of at least two segments inside the measured
    region where that route beat the host's), False for the hybrid route"""
    largest = max(int(s.bytes) for s in segs[:info.n_segments])
    return bool(info.contiguous) and info.n_segments >= 2 and largest <= PNG_DEVICE_SEGMENT_MAX and nbytes >= PNG_DEVICE_MIN_RATIO * largest


def _png_status_error(who, word):
    from . import _lib
    return _lib.NesrBadFileError(f"{who} failed ({_lib.ERR_BADFILE}): the device rejected the file, status {word:#x}", word)


def _png_frame(info, device, out):
    """The [H, W, C] tensor the kernels write (`out` when given, as a 3-d view) and what the caller gets back"""
    h, w, c = int(info.H), int(info.W), int(info.C)
    dtype = torch.uint8 if info.depth == 8 else torch.int16
    if out is None:
        out = torch.empty((h, w, c), dtype=dtype, device=device)
    view = out if out.dim() == 3 else out[:, :, None]
    return view, (out[:, :, 0] if c == 1 and out.dim() == 3 else out)


def _png_decode_hip(file_dev, n, info, segs, order, out):
    """One run of nesr_png_decode (csrc/png_decode.hip): the file and the segment table on the device -> (frame, status word).  One
    word comes back."""
    from . import _lib
    import ctypes
    import numpy as np
    lib = _lib.load()
    view, ret = _png_frame(info, file_dev.device, out)
    need = int(lib.nesr_png_decode_scratch_bytes(ctypes.byref(info)))
    scratch = torch.empty(need, dtype=torch.uint8, device=file_dev.device)
    status = torch.empty(1, dtype=torch.int32, device=file_dev.device)
    table = np.frombuffer(bytes(segs), np.int64).copy()
    segs_dev = torch.from_numpy(table).to(file_dev.device)                                        # H2D: 24 bytes per segment
    _hip_call(file_dev, "nesr_png_decode", _ptr(file_dev), int(n), ctypes.byref(info), _ptr(segs_dev), _ptr(view), _row_bytes(view),
              _lib.ORDER_BGR if order == "bgr" else _lib.ORDER_RGB, _ptr(scratch), need, _ptr(status))
    return ret, int(status.item()) & 0xFFFFFFFF                                                  # D2H: 4 bytes (waits for the decode)


def _png_idat(data):
    """The IDAT payloads of a file nesr_png_parse accepted, joined: the zlib stream"""
    import struct
    at, parts = 8, []
    while at + 12 <= len(data):
        length, kind = struct.unpack(">I4s", data[at:at + 8])
        if kind == b"IDAT":
            parts.append(data[at + 8:at + 8 + length])
        at += 12 + length
    return b"".join(parts)


def _png_inflate_host(data, info):
    """zlib on the host -> the filtered stream's bytes; NesrBadFileError for a stream zlib rejects or one of the wrong size (status 64)"""
    from . import _lib
    import zlib
    try:
        stream = zlib.decompress(_png_idat(data))
    except zlib.error as e:
        raise _lib.NesrBadFileError(f"decode_png failed ({_lib.ERR_BADFILE}): {e}") from e
    if len(stream) != info.stream_bytes:
        raise _png_status_error("decode_png", 64)
    return stream


def _png_unfilter_hip(stream, info, device, order, out):
    """The hybrid route's device half: the filtered stream goes up, nesr_png_unfilter undoes the filters into the frame"""
    from . import _lib
    import numpy as np
    lib = _lib.load()
    filt = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(device)                   # H2D: the filtered stream
    view, ret = _png_frame(info, device, out)
    need = int(lib.nesr_png_unfilter_scratch_bytes(info.H, info.W, info.C, info.depth))
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    _hip_call(filt, "nesr_png_unfilter", _ptr(filt), int(info.H), int(info.W), int(info.C), int(info.depth), _ptr(view), _row_bytes(view),
              _lib.ORDER_BGR if order == "bgr" else _lib.ORDER_RGB, _ptr(scratch), need, _ptr(status))
    word = int(status.item()) & 0xFFFFFFFF                                                       # D2H: 4 bytes
    if word != 0:
        raise _png_status_error("nesr_png_unfilter", word)
    return ret


def _png_unfilter_numpy(filt, bpp):
    """The five PNG row filters undone on the host (numpy): whole-row operations for None / Up, a running sum for Sub, a walk over the
    pixels for Average / Paeth"""
    import numpy as np
    h, n = filt.shape[0], filt.shape[1] - 1
    raw = np.zeros((h + 1, n + bpp), np.int64)
    for y in range(h):
        t, line, cur, up = int(filt[y, 0]), filt[y, 1:].astype(np.int64), raw[y + 1], raw[y]
        if t == 0:
            cur[bpp:] = line
        elif t == 1:
            lanes = np.concatenate([line, np.zeros((-n) % bpp, np.int64)]).reshape(-1, bpp)
            cur[bpp:] = (np.cumsum(lanes, axis=0) & 255).reshape(-1)[:n]
        elif t == 2:
            cur[bpp:] = (line + up[bpp:]) & 255
        elif t == 3:
            for i in range(0, n, bpp):
                cur[i + bpp:i + 2 * bpp] = (line[i:i + bpp] + ((cur[i:i + bpp] + up[i + bpp:i + 2 * bpp]) >> 1)) & 255
        elif t == 4:
            for i in range(0, n, bpp):
                a, b, c = cur[i:i + bpp], up[i + bpp:i + 2 * bpp], up[i:i + bpp]
                p = a + b - c
                pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
                cur[i + bpp:i + 2 * bpp] = (line[i:i + bpp] + np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))) & 255
        else:
            raise _png_status_error("decode_png", 256)
    return np.ascontiguousarray(raw[1:, bpp:].astype(np.uint8))


def _png_decode_host(data, info, order):
    """The specification's route: stdlib zlib and a numpy unfilter -> CPU tensor"""
    import numpy as np
    h, w, c, depth = int(info.H), int(info.W), int(info.C), int(info.depth)
    bpp = c * depth // 8
    filt = np.frombuffer(_png_inflate_host(data, info), np.uint8).reshape(h, 1 + w * bpp)
    raw = _png_unfilter_numpy(filt, bpp)
    img = (raw.view(">u2").astype(np.uint16).view(np.int16) if depth == 16 else raw).reshape(h, w, c)
    if order == "bgr" and c >= 3:
        img = np.concatenate([img[:, :, 2::-1], img[:, :, 3:]], axis=2)
    return torch.from_numpy(np.ascontiguousarray(img[:, :, 0] if c == 1 else img))


def _png_decode_pillow(data, order):
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("decode_png: a palette, gray + alpha, 1 / 2 / 4-bit or interlaced file needs Pillow") from e
    import io
    import numpy as np
    img = Image.open(io.BytesIO(bytes(data)))
    if img.format != "PNG":
        raise ValueError(f"decode_png: a PNG file, got {img.format}")
    if img.mode in ("I;16", "I;16B", "I"):
        arr = np.asarray(img).astype(np.uint16).view(np.int16)
    else:
        if img.mode not in ("L", "RGB", "RGBA"):
            img = img.convert("RGBA" if img.mode in ("LA", "PA") or "transparency" in img.info else ("L" if img.mode == "1" else "RGB"))
        arr = np.asarray(img)
    if arr.ndim == 3 and order == "bgr":
        arr = np.concatenate([arr[:, :, 2::-1], arr[:, :, 3:]], axis=2)
    return torch.from_numpy(np.array(arr))


def decode_png(data, order="rgb", device=None, use_hip=None, inflate=None, out=None):
    """cv2.imread(path.png, cv2.IMREAD_UNCHANGED)'s pixels (standalone/direct_esrgan.py:130) for a PNG file's bytes -> tensor [H, W]
    (gray), [H, W, 3] or [H, W, 4] (order "rgb" or "bgr": the channel that comes first; alpha stays last); uint8, or for a 16-bit file
    int16 carrying the uint16 bit pattern (frame_io's convention, what encode_png takes).  Non-interlaced files of depth 8 or 16 and
    colour type 0, 2 or 6 are decoded here; the chunk CRCs are not checked, the Adler-32 of the inflated stream is.

    On a ROCm device (device=None: the current one when there is one) two routes end in the same frame (csrc/png_decode.hip):
      all-device   the file goes up; every segment between two flush points (nesr_png_parse: an IDAT boundary behind 00 00 FF FF) is
                   inflated by its own wave, then the filters are undone.  encode_png's own files are one segment per 32 KiB chunk.
      hybrid       stdlib zlib inflates on the host, the filtered stream goes up, nesr_png_unfilter finishes.
    inflate=None takes the all-device route where it was measured faster than the host's (_png_default_on_device: a contiguous plan
    of at least two segments, the largest at most PNG_DEVICE_SEGMENT_MAX compressed bytes and at most 1 / PNG_DEVICE_MIN_RATIO of the
    file: encode_png's files from about 2160p up, not its 1024 x 1024 ones), and falls back to the hybrid route when a segment proves
    DEPENDENT on an earlier one (Z_SYNC_FLUSH files).  inflate="device" forces the device inflater on any contiguous plan (a one-stream file is one segment, one
    wave) and raises NesrUnsupportedError for a plan that is not contiguous or is dependent; inflate="host" forces the hybrid route.
    `out`: a window [H, W, C] (or [H, W]) of the frame's dtype on that device; its rows may be strided, nothing outside it is written.
    use_hip=False or a CPU device: stdlib zlib and a numpy unfilter, no Pillow needed.  use_hip=None hands a kind the kernels do not
    take (palette, gray + alpha, 1 / 2 / 4 bit, Adam7) to Pillow and copies the frame up; use_hip=True raises NesrUnsupportedError.
    A malformed file, and any device status but DEPENDENT, raises NesrBadFileError (`status`: the bits)."""
    from . import _lib
    if order not in ("rgb", "bgr"):
        raise ValueError(f"decode_png: order must be 'rgb' or 'bgr', got {order!r}")
    if inflate not in (None, "device", "host"):
        raise ValueError(f"decode_png: inflate must be None, 'device' or 'host', got {inflate!r}")
    if device is None:
        device = out.device if out is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    on_gpu = device.type == "cuda"
    if use_hip is None:
        use_hip, fallback = on_gpu, True
    else:
        fallback = False
    if use_hip and not on_gpu:
        raise ValueError(f"decode_png: the HIP kernels run on the ROCm device, got {device}")
    data = bytes(data)
    try:
        info, segs = _lib.png_parse(data)
    except _lib.NesrUnsupportedError:
        if not fallback:
            raise
        frame = _png_decode_pillow(data, order).to(device)
        if out is not None:
            out.copy_(frame.reshape(out.shape))
            return out
        return frame
    if not use_hip:
        frame = _png_decode_host(data, info, order).to(device)
        if out is not None:
            out.copy_(frame.reshape(out.shape))
            return out
        return frame
    if out is not None:
        shape = (info.H, info.W) if info.C == 1 else (info.H, info.W, info.C)
        dtype = torch.uint8 if info.depth == 8 else torch.int16
        ok = out.dtype == dtype and out.device.type == "cuda" and (tuple(out.shape) == shape or tuple(out.shape) == (info.H, info.W, info.C))
        if not ok or not _rows_ok(out if out.dim() == 3 else out[:, :, None], (1, 3, 4)):
            raise ValueError(f"decode_png: out must be a {dtype} {shape} window on the ROCm device with contiguous pixels in a row, got "
                             f"{out.dtype} {tuple(out.shape)} on {out.device}")
    on_device = inflate == "device" or (inflate is None and _png_default_on_device(info, segs, len(data)))
    if on_device:
        if not info.contiguous:
            raise _lib.NesrUnsupportedError(f"decode_png failed ({_lib.ERR_UNSUPPORTED}): a deflate segment spans an IDAT boundary; the device "
                                            "inflater takes contiguous plans (inflate='host' or None)")
        import numpy as np
        file_dev = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(device)             # H2D: the file
        frame, word = _png_decode_hip(file_dev, len(data), info, segs, order, out)
        if word == 0:
            return frame
        if word != _lib.PNG_DEPENDENT:
            raise _png_status_error("nesr_png_decode", word)
        if inflate == "device":
            raise _lib.NesrUnsupportedError(f"decode_png failed ({_lib.ERR_UNSUPPORTED}): a segment depends on the one before it (a "
                                            "Z_SYNC_FLUSH file); inflate='host' or None")
    return _png_unfilter_hip(_png_inflate_host(data, info), info, device, order, out)


def _jpeg_decode_hip(file_dev, n, info, order, out):
    """One run of nesr_jpeg_decode_u8 (csrc/jpeg_decode.hip) on the file's bytes on the device -> the [H, W, 3] / [H, W] uint8 frame
    (`out` when given: a window whose rows may be strided).  One word comes back, the status; NesrBadFileError when it is not 0."""
    from . import _lib
    lib = _lib.load()
    import ctypes
    h, w, c = int(info.H), int(info.W), int(info.C)
    if out is None:
        out = torch.empty((h, w, c), dtype=torch.uint8, device=file_dev.device)
    view = out if out.dim() == 3 else out[:, :, None]
    need = int(lib.nesr_jpeg_decode_scratch_bytes(ctypes.byref(info)))
    scratch = torch.empty(need, dtype=torch.uint8, device=file_dev.device)
    status = torch.empty(1, dtype=torch.int32, device=file_dev.device)
    _hip_call(file_dev, "nesr_jpeg_decode_u8", _ptr(file_dev), int(n), ctypes.byref(info), _ptr(view), _row_bytes(view), _lib.ORDER_BGR if order == "bgr" else _lib.ORDER_RGB,
              _ptr(scratch), need, _ptr(status))
    word = int(status.item()) & 0xFFFFFFFF                     # D2H: 4 bytes (waits for the decode)
    if word != 0:
        raise _lib.NesrBadFileError(f"nesr_jpeg_decode_u8 failed ({_lib.ERR_BADFILE}): the device rejected the scan, status {word:#x}", word)
    return out[:, :, 0] if c == 1 and out.dim() == 3 else out


def _jpeg_decode_pillow(data, order):
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("decode_jpeg_u8: the host route needs Pillow (the device route: a ROCm device)") from e
    import io
    import numpy as np
    img = Image.open(io.BytesIO(bytes(data)))
    if img.format != "JPEG":
        raise ValueError(f"decode_jpeg_u8: a JPEG file, got {img.format}")
    if img.mode not in ("L", "RGB"):
        img = img.convert("RGB")
    arr = np.asarray(img)
    return torch.from_numpy(np.array(arr[:, :, ::-1] if arr.ndim == 3 and order == "bgr" else arr))


def decode_jpeg_u8(data, order="rgb", device=None, use_hip=None, out=None):
    """cv2.imread(path.jpg, cv2.IMREAD_UNCHANGED)'s pixels (the reference reads with cv2.imread, nesr/nesr.py:661-666,
    standalone/direct_esrgan.py:130) for a JPEG file's bytes -> uint8 tensor [H, W, 3] (order "rgb" or "bgr": the channel that comes
    first) or [H, W] for a gray file.  EXIF orientation is not applied: IMREAD_UNCHANGED and Pillow leave it alone, cv2.imread's
    default flag would rotate a file whose orientation is not 1.

    On a ROCm device (device=None: the current one when there is one) the file's bytes go up and the HIP kernels decode them
    (csrc/jpeg_decode.hip, nesr_jpeg_parse + nesr_jpeg_decode_u8): baseline Huffman files, 8 bits, gray, 4:4:4, 4:2:2 or 4:2:0, any
    tables, any restart interval -- pixel for pixel what libjpeg-turbo gives (tests/jpeg_decode_ref.py).  `out`: a uint8 window
    [H, W, C] (or [H, W]) on that device to decode into; its rows may be strided and nothing outside it is written.
    use_hip=False or a CPU device: Pillow's libjpeg-turbo; without Pillow that raises.  use_hip=None: a file the kernels do not
    support (NesrUnsupportedError: progressive, CMYK, ...) is decoded by Pillow and copied up; a malformed file or a scan the device
    rejects raises NesrBadFileError.  use_hip=True raises on both."""
    from . import _lib
    if order not in ("rgb", "bgr"):
        raise ValueError(f"decode_jpeg_u8: order must be 'rgb' or 'bgr', got {order!r}")
    if device is None:
        device = out.device if out is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    on_gpu = device.type == "cuda"
    if use_hip is None:
        use_hip, fallback = on_gpu, True
    else:
        fallback = False
    if use_hip and not on_gpu:
        raise ValueError(f"decode_jpeg_u8: the HIP kernels run on the ROCm device, got {device}")
    data = bytes(data)
    if use_hip:
        try:
            info = _lib.jpeg_parse(data)
        except _lib.NesrUnsupportedError:
            if not fallback:
                raise
            info = None
        if info is not None:
            if out is not None:
                shape = (info.H, info.W, 3) if info.C == 3 else (info.H, info.W)
                ok = out.dtype == torch.uint8 and out.device.type == "cuda" and (tuple(out.shape) == shape or tuple(out.shape) == (info.H, info.W, info.C))
                if not ok or not _rows_ok(out if out.dim() == 3 else out[:, :, None], (1, 3)):
                    raise ValueError(f"decode_jpeg_u8: out must be a uint8 {shape} window on the ROCm device with contiguous pixels in a row, got "
                                     f"{out.dtype} {tuple(out.shape)} on {out.device}")
            import numpy as np
            file_dev = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(device)         # H2D: the file
            return _jpeg_decode_hip(file_dev, len(data), info, order, out)
    frame = _jpeg_decode_pillow(data, order).to(device)
    if out is not None:
        out.copy_(frame.reshape(out.shape))
        return out
    return frame


def jpeg_roundtrip_u8(frame, quality=75, order="rgb"):
    """apply_jpeg_compression (nesr/utils/image_utils.py:130-152: cv2.imencode('.jpg', img, [IMWRITE_JPEG_QUALITY, quality]) then
    cv2.imdecode) on a uint8 [H, W, 3], [H, W, 1] or [H, W] tensor on the ROCm device -> the decoded frame, same shape.  Neither the
    frame nor the file leaves the device: the encoder's output buffer feeds the decoder, and only the length words are read, to size
    the decoder's launches.  The header the decoder's parser needs is the one the host wrote for the encoder (nesr_jpeg_header)."""
    from . import _lib
    import ctypes
    if order not in ("rgb", "bgr"):
        raise ValueError(f"jpeg_roundtrip_u8: order must be 'rgb' or 'bgr', got {order!r}")
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"jpeg_roundtrip_u8: quality {quality} outside 1..100")
    if not isinstance(frame, torch.Tensor) or not _hip_default(frame):
        raise ValueError("jpeg_roundtrip_u8: a uint8 tensor on the ROCm device")
    squeeze = frame.dim() == 2
    src = frame[:, :, None] if squeeze else frame
    if src.dim() != 3 or src.shape[2] not in (1, 3) or min(src.shape) < 1 or max(src.shape[:2]) > 65535:
        raise ValueError(f"jpeg_roundtrip_u8: an [H, W, 3], [H, W, 1] or [H, W] uint8 frame of at most 65535 x 65535 pixels, got {tuple(frame.shape)}")
    if not _rows_ok(src, (1, 3)):
        src = src.contiguous()
    h, w, c = src.shape
    lib = _lib.load()
    head = (ctypes.c_uint8 * 1024)()
    n_head = ctypes.c_int(0)
    _lib.check(lib.nesr_jpeg_header(h, w, c, int(quality), head, 1024, ctypes.byref(n_head)), "nesr_jpeg_header")
    info = _lib.jpeg_parse(bytes(head[:n_head.value]) + b"\0")      # the scan's length is patched in below
    need = int(lib.nesr_jpeg_scratch_bytes(h, w, c))
    scratch = torch.empty(need, dtype=torch.uint8, device=src.device)
    cap = h * w * c // 2 + 4096
    while True:
        file_dev = torch.empty(cap, dtype=torch.uint8, device=src.device)
        words = torch.empty(2, dtype=torch.int64, device=src.device)
        _hip_call(src, "nesr_jpeg_encode_u8", _ptr(src), _row_bytes(src), h, w, c, _lib.ORDER_BGR if order == "bgr" else _lib.ORDER_RGB, int(quality),
                  _ptr(scratch), need, _ptr(file_dev), cap, _ptr(words))
        length, status = (int(v) for v in words.cpu())          # D2H: 16 bytes
        if status == 0:
            break
        cap = length
    info.scan_bytes = length - n_head.value - 2                  # the file ends with EOI
    out = _jpeg_decode_hip(file_dev, length, info, order, None)
    if c == 1 and not squeeze:
        out = out[:, :, None]
    return out
