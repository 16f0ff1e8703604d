"""The specification of the x4 diffusion stage over windows (csrc/sdx4_tiled.hip, nesr_sdx4_upscale_tiled_u8, nesr_vae_decode_latents_
tiled_u8): the window plan, the separable weights and their normaliser, the windowed denoising loop on one shared latent frame
and the tiled VAE decode, in float64 (or the dtype asked for), composed from tests/sdx4_ref.py, tests/unet_ref.py and
tests/vae_ref.py unchanged.  Then emulations of the five kernels on flat buffers with the kernels' own offsets, and the cases both
test files run.  The tiling is this project's own specification; how diffusers tiles is recalled, not checked, and not reproduced.

  plan      per axis t = min(tile, n); starts 0, t - O, ... below n - t, then n - t; windows in row-major order
  weight    window [a, a + t) of an axis of n, ramp R = O: left = (a > 0 and R > 0) ? min(i - a + 1, R) / R : 1, right = (a + t < n and
            R > 0) ? min(a + t - i, R) / R : 1, w_axis = min(left, right); w(y, x) = w_y(y) w_x(x)
  S         S(y, x) = Sy(y) Sx(x), each the sum of w_axis over the axis's windows that cover the pixel, ascending
  loop      per step and window: the UNet on the window of cat(latents, image), acc += w (neg + g (prompt - neg)); per step
            m = acc / S and sdx4_ref.ddim_step on the whole frame
  decode    per window the VAE's sample of latents / scaling_factor, acc += w sample with origin, length and ramp times s; then
            acc / S / 2 + 0.5

`fault` names one deliberate mistake (FAULTS); tests/test_sdx4_tiled_host.py shows that each is seen by a case the device runs.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import clip_text_ref as TR
from tests import sdx4_cases as C
from tests import sdx4_ref as R
from tests import unet_ref as UR
from tests import vae_ref as VR

FAULTS = ("uniform_weights", "ramp_on_frame_edge", "last_window_on_stride", "normalise_by_count", "normalise_by_sy_only", "acc_not_cleared",
          "image_from_origin_0", "window_stride_as_plane_stride", "output_ramp_unscaled")
SENTINEL = -777.0


# ------------------------------------------------------------------------------------------------ the plan and the weights
def axis_starts(n, t, overlap, fault=None):
    assert 1 <= t <= n and 0 <= overlap < t, (n, t, overlap)
    starts, a = [], 0
    while a < n - t:
        starts.append(a)
        a += t - overlap
    starts.append(a if fault == "last_window_on_stride" else n - t)      # the fault's window runs past the edge; its pixels there are dropped
    return starts


def plan(h, w, tile, overlap, fault=None):
    """((tiles_y, tiles_x), (ty, tx), [(y, x)]) in the order the windows run."""
    ty, tx = min(tile, h), min(tile, w)
    ys, xs = axis_starts(h, ty, overlap, fault), axis_starts(w, tx, overlap, fault)
    return (len(ys), len(xs)), (ty, tx), [(y, x) for y in ys for x in xs]


def axis_weight(n, t, a, ramp, fault=None):
    """float64 [t]: the weights of window [a, a + t) on an axis of n."""
    i = np.arange(a, a + t)
    if fault == "uniform_weights" or ramp == 0:
        return np.ones(t)
    edge = fault == "ramp_on_frame_edge"
    left = np.minimum(i - a + 1, ramp) / ramp if (a > 0 or edge) else np.ones(t)
    right = np.minimum(a + t - i, ramp) / ramp if (a + t < n or edge) else np.ones(t)
    return np.minimum(left, right)


def axis_sum(n, t, overlap, ramp, fault=None, dtype=np.float64):
    """[n]: Sy or Sx, the windows' weights summed in ascending order of their origins (each weight rounded to `dtype` first)."""
    s = np.zeros(n, dtype=dtype)
    for a in axis_starts(n, t, overlap, fault):
        w = np.ones(t, dtype=dtype) if fault == "normalise_by_count" else axis_weight(n, t, a, ramp, fault).astype(dtype)
        keep = min(t, n - a)
        s[a:a + keep] += w[:keep]
    return s


def normaliser(h, w, tile, overlap, scale=1, fault=None):
    """float64 [h scale, w scale]."""
    ty, tx = min(tile, h), min(tile, w)
    ramp = overlap if fault == "output_ramp_unscaled" else overlap * scale
    sy = axis_sum(h * scale, ty * scale, overlap * scale, ramp, fault)
    sx = axis_sum(w * scale, tx * scale, overlap * scale, ramp, fault)
    return np.outer(sy, np.ones_like(sx) if fault == "normalise_by_sy_only" else sx)


def window_weight(h, w, tile, overlap, y, x, scale=1, fault=None):
    """float64 [ty scale, tx scale] of the window at (y, x), low-res coordinates."""
    ty, tx = min(tile, h), min(tile, w)
    ramp = overlap if fault == "output_ramp_unscaled" else overlap * scale
    return np.outer(axis_weight(h * scale, ty * scale, y * scale, ramp, fault), axis_weight(w * scale, tx * scale, x * scale, ramp, fault))


def brute_force_sum(h, w, tile, overlap, scale=1):
    """The weight sum per pixel with no use of separability: every window's plane added at its place."""
    s = np.zeros((h * scale, w * scale))
    (_, _), (ty, tx), rows = plan(h, w, tile, overlap)
    for y, x in rows:
        s[y * scale:(y + ty) * scale, x * scale:(x + tx) * scale] += window_weight(h, w, tile, overlap, y, x, scale)
    return s


def blend(frame_shape, windows, h, w, tile, overlap, scale, dtype, fault=None):
    """sum of w window / S over [(y, x, tensor [..., ty scale, tx scale])] -> [..., h scale, w scale] in `dtype`."""
    acc = torch.zeros(frame_shape, dtype=dtype)
    H, W = h * scale, w * scale
    for y, x, v in windows:
        wt = torch.from_numpy(window_weight(h, w, tile, overlap, y, x, scale, fault)).to(dtype)
        y0, x0 = y * scale, x * scale
        ky, kx = min(v.shape[-2], H - y0), min(v.shape[-1], W - x0)      # a faulty plan's window may run past the edge
        acc[..., y0:y0 + ky, x0:x0 + kx] += (wt * v.to(dtype))[..., :ky, :kx]
    return acc / torch.from_numpy(normaliser(h, w, tile, overlap, scale, fault)).to(dtype)


def take(frame, y, x, ty, tx):
    """The window of [..., H, W] at (y, x); past the edge (a faulty plan) the last row and column repeat."""
    H, W = frame.shape[-2:]
    rows, cols = torch.arange(y, y + ty).clamp(max=H - 1), torch.arange(x, x + tx).clamp(max=W - 1)
    return frame[..., rows, :][..., cols]


# ------------------------------------------------------------------------------------------------ the loop and the decode
def loop(unet, frame_u8, text, noise, latents, noise_level, steps, guidance_scale, tile, overlap, dtype=torch.float64, fault=None, scheduler=R.DDIM, forward=UR.forward):
    """sdx4_ref.loop over windows -> the final latents [1, lc, h, w] in `dtype`.  `forward` is the UNet's restatement: unet_ref.forward,
    or one of its signature (tests/unet_f16_emu.forward: the fp16 compute form)."""
    T = scheduler["num_train_timesteps"]
    abar = R.ddim_alpha_bars(T, scheduler["beta_start"], scheduler["beta_end"], scheduler["beta_schedule"])
    low = R.low_res_alpha_bars(R.LOW_RES["num_train_timesteps"])
    n = text.shape[0]
    image = R.image_input(frame_u8, noise, noise_level, low, dtype)
    x = latents.to(dtype).clone()
    lc, h, w = x.shape
    sd, cfg = unet
    (_, _), (ty, tx), rows = plan(h, w, tile, overlap, fault)
    carried = torch.zeros_like(x)
    for t in R.timesteps(steps, T, scheduler["steps_offset"]):
        a, p = R.step_alphas(t, steps, abar, T, scheduler["set_alpha_to_one"])
        outs = []
        for y0, x0 in rows:
            img = take(image, 0, 0, ty, tx) if fault == "image_from_origin_0" else take(image, y0, x0, ty, tx)
            sample = torch.cat([take(x, y0, x0, ty, tx), img], dim=0)[None].expand(n, -1, -1, -1).contiguous()
            with torch.no_grad():
                m = forward(sd, sample, float(t), text.to(dtype), noise_level, **cfg)
            outs.append((y0, x0, R.guide(m, guidance_scale)))
        m = blend(x.shape, outs, h, w, tile, overlap, 1, dtype, fault)
        if fault == "acc_not_cleared":      # the sum of w m of every step so far is what gets normalised
            s = torch.from_numpy(normaliser(h, w, tile, overlap, 1, fault)).to(dtype)
            carried = carried + m * s
            m = carried / s
        x = R.ddim_step(x, m, a, p, scheduler["prediction_type"])
    return x[None]


def decode(vae, latents, tile, overlap, dtype=torch.float64, fault=None):
    """latents [1, lc, h, w] -> the frame before the clamp [h s, w s, 3] in `dtype`."""
    vsd, vcfg = vae
    c = VR.config(**vcfg)
    scale = 2 ** (len(c["block_out_channels"]) - 1)
    z = latents.to(dtype)[0] / c["scaling_factor"]
    lc, h, w = z.shape
    (_, _), (ty, tx), rows = plan(h, w, tile, overlap, fault)
    outs = []
    for y0, x0 in rows:
        with torch.no_grad():
            outs.append((y0, x0, VR.decode(vsd, take(z, y0, x0, ty, tx)[None].contiguous(), **vcfg)[0]))
    y = blend((3, h * scale, w * scale), outs, h, w, tile, overlap, scale, dtype, fault) / 2 + 0.5
    return y.permute(1, 2, 0).contiguous()


def upscale(models, frame_u8, ids, noise, latents, noise_level, steps, guidance_scale, tile, overlap, dtype=torch.float64, fault=None, vae_tile=None, vae_overlap=None):
    """sdx4_ref.upscale over windows -> (final latents [1, lc, h, w], the frame before the clamp [4h, 4w, 3])."""
    tsd, tcfg = models["text"]
    with torch.no_grad():
        text = TR.forward(tsd, ids, dtype, **tcfg)
    final = loop(models["unet"], frame_u8, text, noise, latents, noise_level, steps, guidance_scale, tile, overlap, dtype, fault)
    return final, decode(models["vae"], final, tile if vae_tile is None else vae_tile, overlap if vae_overlap is None else vae_overlap, dtype, fault)


# the crafted tiled call of the pipeline tests: a 24 x 40 frame, tile 16, overlap 8 (2 x 4 windows; x starts 0, 8, 16, 24), 3 steps
H, W, TILE, OVERLAP, STEPS = 24, 40, 16, 8, 3
FRAME_SEED, DRAW_SEED = 74, 75
_refs = {}


def crafted():
    """(frame u8 [24, 40, 3], noise [3, 24, 40], latents [4, 24, 40])."""
    noise, latents = C.draws(H, W, DRAW_SEED)
    return C.frame(H, W, FRAME_SEED), noise, latents


def reference(guidance=C.GUIDANCE):
    """(final latents f64, frame before the clamp f64, tol of the latents, tol of the frame, the float32 restatement's frame) of the
    crafted tiled call: tol = 8 x max |float32 restatement - float64|, computed here and never written down."""
    if guidance not in _refs:
        frame, noise, latents = crafted()
        tok = C.ids() if guidance > 1.0 else C.ids()[1:]
        args = (C.models(), frame, tok, noise, latents, C.NOISE_LEVEL, STEPS, guidance, TILE, OVERLAP)
        lat64, y64 = upscale(*args, torch.float64)
        lat32, y32 = upscale(*args, torch.float32)
        _refs[guidance] = (lat64, y64, 8.0 * float((lat32.double() - lat64).abs().max()), 8.0 * float((y32.double() - y64).abs().max()), y32)
    return _refs[guidance]


def reference_f16(guidance=C.GUIDANCE, steps=2):
    """(final latents of the float64 loop, of the loop with the fp16 form's emulated forward in float64, bound) of the crafted tiled
    call with `steps` steps: bound = max |emulation64 - float64| + 8 x max |emulation32 - emulation64|, tests/unet_f16_emu.py's bound
    for a network, here for the whole windowed loop (a bound, not a pin: a rounding may flip)."""
    from tests import unet_f16_emu as E
    key = ("f16", guidance, steps)
    if key not in _refs:
        frame, noise, latents = crafted()
        tok = C.ids() if guidance > 1.0 else C.ids()[1:]
        tsd, tcfg = C.models()["text"]
        with torch.no_grad():
            text = TR.forward(tsd, tok, torch.float64, **tcfg)
        args = (C.models()["unet"], frame, text, noise, latents, C.NOISE_LEVEL, steps, guidance, TILE, OVERLAP)
        lat64, emu64, emu32 = loop(*args), loop(*args, forward=E.forward), loop(*args, torch.float32, forward=E.forward)
        _refs[key] = (lat64, emu64, float((emu64 - lat64).abs().max()) + 8.0 * float((emu32.double() - emu64).abs().max()))
    return _refs[key]


# ------------------------------------------------------------------------------------------------ the kernels' indexing
def axes(h, w, tile, overlap, y=0, x=0, scale=1):
    """The eight integers a hook takes: (n, t, r, a) of y, then of x."""
    ty, tx = min(tile, h), min(tile, w)
    return [v * scale for v in (h, ty, overlap, y, w, tx, overlap, x)]


def k_gather(src, n, ax, dtype=np.float64, fault=None):
    """src [channels, H, W] flat -> dst [n, channels, ty, tx]."""
    H, ty, _, ay, W, tx, _, axx = ax
    src = np.asarray(src).reshape(-1)
    channels = src.size // (H * W)
    plane = ty * tx if fault == "window_stride_as_plane_stride" else H * W
    dst = np.full((n, channels, ty, tx), SENTINEL, dtype=dtype)
    for c in range(channels):
        oy, ox = (0, 0) if (fault == "image_from_origin_0" and c >= channels - 3) else (ay, axx)
        for y in range(ty):
            at = c * plane + (oy + y) * W + ox
            dst[:, c, y, :] = src[at:at + tx].astype(dtype)
    return dst


def _ramps(ax, fault, scale):
    return (ax[2] // scale, ax[6] // scale) if fault == "output_ramp_unscaled" else (ax[2], ax[6])


def _w(ax, fault, dtype, scale=1):
    """[ty, tx] as the kernels form it: each axis's weight rounded to `dtype`, then one product."""
    H, ty, _, ay, W, tx, _, axx = ax
    ry, rx = _ramps(ax, fault, scale)
    wy, wx = axis_weight(H, ty, ay, ry, fault).astype(dtype), axis_weight(W, tx, axx, rx, fault).astype(dtype)
    return wy[:, None] * wx[None, :]


def _s(ax, fault, dtype, scale=1):
    """[H, W]: each axis's sum accumulated in `dtype`, then one product."""
    H, ty, oy, _, W, tx, ox, _ = ax
    ry, rx = _ramps(ax, fault, scale)
    sy, sx = axis_sum(H, ty, oy, ry, fault, dtype), axis_sum(W, tx, ox, rx, fault, dtype)
    return sy[:, None] * (np.ones_like(sx) if fault == "normalise_by_sy_only" else sx)[None, :]


def k_accumulate(model, acc, ax, g, dtype=np.float64, fault=None):
    """model [n, lc, ty, tx], acc [lc, H, W] -> acc with w m added at the window's place."""
    H, ty, _, ay, W, tx, _, axx = ax
    m = model.astype(dtype)
    mm = m[0] + dtype(g) * (m[1] - m[0]) if m.shape[0] == 2 else m[0]
    out = acc.astype(dtype).copy()
    out[:, ay:ay + ty, axx:axx + tx] += _w(ax, fault, dtype)[None] * mm
    return out


def k_tiled_step(acc, frame, lc, ax, coef, dtype=np.float64, fault=None):
    """acc [lc, H, W], frame [lc + 3, H, W] -> (acc zeroed, frame with the step taken on channels 0 .. lc - 1)."""
    c0x, c0m, cex, cem, sp, sq = (dtype(v) for v in coef)
    out = frame.astype(dtype).copy()
    x, m = out[:lc], acc.astype(dtype) / _s(ax, fault, dtype)[None]
    x0, e = c0x * x + c0m * m, cex * x + cem * m
    out[:lc] = sp * x0 + sq * e
    return (acc.astype(dtype).copy() if fault == "acc_not_cleared" else np.zeros_like(acc, dtype=dtype)), out


def k_blend_add(sample, acc, ax, dtype=np.float64, fault=None, scale=4):
    """sample [3, ty, tx], acc [H, W, 3] (output resolution) -> acc."""
    H, ty, ry, ay, W, tx, rx, axx = ax
    out = acc.astype(dtype).copy()
    out[ay:ay + ty, axx:axx + tx, :] += (_w(ax, fault, dtype, scale)[None] * sample.astype(dtype)).transpose(1, 2, 0)
    return out


def k_blend_finish_float(acc, ax, dtype=np.float64, fault=None, scale=4):
    """acc [H, W, 3] -> acc / S / 2 + 0.5, before the clamp."""
    return acc.astype(dtype) / _s(ax, fault, dtype, scale)[:, :, None] / dtype(2.0) + dtype(0.5)


def quantise(y):
    return np.round(np.clip(y, 0.0, 1.0) * 255.0).astype(np.uint8)      # numpy rounds half to even


# ------------------------------------------------------------------------------------------------ the cases both test files run
# (h, w, tile, overlap): one window; plain; x starts 0, 6, 12, 14 (off-stride, and 6 and 14 are 2 mod 4); several rows; an overlap
# above half the window (rows of 6 floats: three windows cover a pixel, and a ramp put on a frame edge would show)
PLANS = ((8, 8, 8, 0), (8, 24, 8, 4), (12, 22, 8, 2), (40, 16, 16, 8), (8, 22, 6, 4))
BLEND_PLANS = ((8, 24, 8, 4), (12, 22, 8, 2))      # at s = 4
LC, EXACT_G, EXACT_COEF = 4, 8.0, (0.5, -2.0, 4.0, 0.25, 2.0, -0.5)
RANDOM_G, RANDOM_COEF = 7.5, (0.83, -0.56, 0.56, 0.83, 0.9, 0.43)


def toy_model(window, n, exact):
    """A stand-in for the UNet in the kernel chains, elementwise so that both sides compute it alike: sample s of [n, lc + 3, ty, tx] ->
    [n, lc, ty, tx].  It reads the image channels, so a window gathered from the wrong place shows, and the place inside the window,
    so two windows disagree about a pixel they share and the weights show."""
    k = (0.5, 0.25, 0.125) if exact else (0.37, 0.61, 0.05)
    t = window.dtype.type
    ty, tx = window.shape[-2:]
    pos = (np.arange(ty)[:, None] - np.arange(tx)[None, :]).astype(window.dtype)
    return np.stack([window[s, :LC] * t(k[0]) + window[s, LC + s % 3][None] * t(k[1] * (s + 1)) + pos[None] * t(k[2]) for s in range(n)])


def chain_case(h, w, seed, exact):
    """The full-frame buffer [lc + 3, h, w]: integers (exact) or unit normals."""
    rng = np.random.default_rng(900 + seed)
    if exact:
        return rng.integers(-8, 9, size=(LC + 3, h, w)).astype(np.float32)
    return rng.standard_normal((LC + 3, h, w)).astype(np.float32)


def chain(frame, h, w, tile, overlap, n, steps, exact, dtype=np.float64, fault=None):
    """`steps` steps of gather -> toy model -> accumulate per window, then the tiled step: the kernels' emulations chained as
    nesr_sdx4_upscale_tiled_u8 chains the kernels -> the full-frame buffer."""
    g, coef = (EXACT_G, EXACT_COEF) if exact else (RANDOM_G, RANDOM_COEF)
    frame = frame.astype(dtype)
    acc = np.zeros((LC, h, w), dtype=dtype)
    (_, _), (ty, tx), rows = plan(h, w, tile, overlap, fault)
    for _ in range(steps):
        for y, x in rows:
            if y + ty > h or x + tx > w:      # last_window_on_stride: the part past the edge is dropped
                continue
            ax = axes(h, w, tile, overlap, y, x)
            win = k_gather(frame, n, ax, dtype, fault)
            acc = k_accumulate(toy_model(win, n, exact), acc, ax, g, dtype, fault)
        acc, frame = k_tiled_step(acc, frame, LC, axes(h, w, tile, overlap), coef, dtype, fault)
    return frame


def blend_case(h, w, tile, overlap, seed, scale=4):
    """One f32 sample [3, ty s, tx s] per window of the plan, unit normals times 1.5."""
    rng = np.random.default_rng(950 + seed)
    (_, _), (ty, tx), rows = plan(h, w, tile, overlap)
    return [(y, x, (1.5 * rng.standard_normal((3, ty * scale, tx * scale))).astype(np.float32)) for y, x in rows]


def blend_chain(samples, h, w, tile, overlap, dtype=np.float64, fault=None, scale=4):
    """blend-add per window, then the finish before the clamp -> [h s, w s, 3]."""
    acc = np.zeros((h * scale, w * scale, 3), dtype=dtype)
    for y, x, v in samples:
        acc = k_blend_add(v, acc, axes(h, w, tile, overlap, y, x, scale), dtype, fault, scale)
    return k_blend_finish_float(acc, axes(h, w, tile, overlap, 0, 0, scale), dtype, fault, scale)
