"""What each launch of csrc/vae.hip computes, twice over (the shape of tests/unet_kernel_ref.py, whose helpers are reused).

The references (`conv`, `rows`, `group_norm`, `attention`, `vin`) are plain torch restatements on dense tensors with no layout in
them, in whatever float dtype they are handed: float64 is the reference, float32 the yardstick of a tolerance.

The emulations (`emu_*`) restate each kernel's INDEXING in float64 on the packed buffers of csrc/vae_api.h (rows [m][cs], a 3x3
weight [9 cinp][coutp], Wt[cs_in][np], VaeNorm [cs]), as tests/vae_kernels.py packs them, and return the output buffer the kernel
would leave, sentinels included, plus under "past" what it would leave in the memory right behind that buffer.  A read past a
buffer's end gives the sentinel.  `fault` names one deliberate mistake (FAULTS); tests/test_vae_kernels_host.py shows that every one
of them fails its case.  What a fault means where the name leaves room:

  k_tail_dropped                      a chunk's 4-wide tail loop is not run: its channels past the last multiple of 16 are lost
  chunk_weight_offset_ignores_c0      every K chunk reads the weight rows of the first one
  weight_rows_by_cs_not_cinp          a tap's weight rows start at tap cs_in, not tap cinp
  z_block_channel_offset_dropped      a block with blockIdx.z >= 1 computes and stores the tiles of block 0: channels from 128 stay unwritten
  absent_tile_stored                  the second tile of a wave is stored where coutp / 16 is odd: sixteen columns past the row
  edge_store_unguarded                pixels past H or W of a ragged tile are stored at y W + x: into the next row, or past the end
  padding_normalised                  a tap outside the image goes through the norm and the SiLU, as if it were a 0 inside
  nearest2_source_width_not_halved    the source row of a NEAREST2 tap is sy W + sx, not sy (W / 2) + sx
  res_stride_is_coutp                 the residual is read with the row stride coutp, not cs_res
  f32_plane_stride                    the NCHW sample is stored with plane stride 1 and pixel stride cout (interleaved)
  u8_round_half_up                    floor(v + 0.5) in float32, not round to nearest even
  u8_no_clamp                         no clamp to [0, 1]: the conversion wraps modulo 256
  last_block_not_clamped              the last block of 512 pixels reads 512 pixels whatever m is
  finish_first_trip_only              the finish adds the first 256 (block, channel) slots of a group only
  cpg_over_256_unwritten              a group's channels from the 257th on are not written
  idle_pixel_lane_counted             the threads past npl nq form one more pixel lane, which repeats lane 0's pixels but the first
  tiles_past_the_fourth_dropped       (rows) a wave runs its first column tile only: columns from 64 stay unwritten
  ragged_rows_written                 the rows past m of the last block of 32 are written, behind the buffer
  ragged_keys_score_zero              the keys past n of the last chunk score 0, not -inf
  sum_not_rescaled                    the running sum is not rescaled when the maximum moves (the accumulator is)
  tiles_past_the_first_round_dropped  (attention) a wave keeps its first column tile only: columns from 64 stay unwritten
  plane_stride                        (in) z is read as [m][c], not [c][m]
  mean_lo_dropped                     the mean's low float is left 0
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import unet_kernel_ref as U
from tests.unet_kernel_ref import SENT, up4, up16      # noqa: F401

FAULTS = {"conv": ("k_tail_dropped", "chunk_weight_offset_ignores_c0", "weight_rows_by_cs_not_cinp", "z_block_channel_offset_dropped", "absent_tile_stored",
                   "edge_store_unguarded", "padding_normalised", "nearest2_source_width_not_halved", "res_stride_is_coutp", "f32_plane_stride",
                   "u8_round_half_up", "u8_no_clamp"),
          "group_norm": ("last_block_not_clamped", "finish_first_trip_only", "cpg_over_256_unwritten", "idle_pixel_lane_counted", "variance_unbiased",
                         "raw_moments_f32", "padded_channels_not_zero"),
          "rows": ("ragged_rows_written", "norm_with_silu", "res_dropped", "tiles_past_the_fourth_dropped"),
          "attention": ("scale_by_cs_not_c", "ragged_keys_score_zero", "no_rescale_on_new_max", "sum_not_rescaled", "tiles_past_the_first_round_dropped"),
          "in": ("multiplied_not_divided", "plane_stride", "columns_past_c_not_zero")}
MEAN_FAULT = "mean_lo_dropped"                      # held to the mean's own bound, in every statistics case
U8_SENT = 90                                        # the guards of a u8 frame
# csrc/vae_api.h
GN_PIXELS, ATTN_BK, CONV_KC, CONV_NB, CONV_TW, CONV_TH, BM, MAX_TOKENS = 512, 32, 64, 128, 16, 4, 32, 1 << 16
IN_ROWS, IN_NEAREST2, OUT_ROWS, OUT_F32, OUT_U8 = 0, 1, 0, 1, 2


# ------------------------------------------------------------------------------------------------ references (dense)
def u8_epilogue(y, fault=None):
    """v / 2 + 0.5, clamp to [0, 1], x 255, round to nearest even, in y's dtype: [1, c, H, W] -> [H, W, c]."""
    t = y / 2.0 + 0.5
    if fault != "u8_no_clamp":
        t = t.clamp(0.0, 1.0)
    t = t * 255.0
    t = torch.floor(t + 0.5) if fault == "u8_round_half_up" else torch.round(t)
    return torch.remainder(t, 256.0).permute(0, 2, 3, 1)[0]


def conv(d, dtype=torch.float64):
    """x [1, cin, h, w] (the source grid) -> nearest x2 where `up` -> GroupNorm's affine + SiLU where a norm is given -> conv 3x3 /
    pad 1 -> + res; [1, cout, H, W], or the u8 frame [H, W, cout].  `epilogue32`: the frame's epilogue runs in float32 whatever
    dtype is (a tie of float32 is not one of float64)."""
    x = d["x"].to(dtype)
    if d.get("up"):
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    y = F.conv2d(U._affine_silu(x, d.get("norm"), dtype), d["w"].to(dtype), d["b"].to(dtype), padding=1)
    if d.get("res") is not None:
        y = y + d["res"].to(dtype)
    if d.get("out") == "u8":
        return u8_epilogue(y.float() if d.get("epilogue32") else y).to(dtype)
    return y


def rows(d, dtype=torch.float64):
    """x [m, c] -> GroupNorm's affine (no activation) -> x w^T + b -> + res [m, nout]."""
    x = U._affine_silu(d["x"].t()[None], d.get("norm"), dtype, act=False)[0].t()
    y = F.linear(x, d["w"].to(dtype), d["b"].to(dtype))
    return y if d.get("res") is None else y + d["res"].to(dtype)


def group_norm(d, dtype=torch.float64):
    """(mean, a, beta) [c] each of GroupNorm over x0 [1, c, m]: the population mean and variance of a group."""
    return tuple(t[0] for t in U.group_norm(d, dtype))


def attention(d, dtype=torch.float64):
    """q, k, v [1, 1, n, c] -> softmax(q k^T / sqrt(c)) v [n, c]."""
    q, k, v = (d[x][0, 0].to(dtype) for x in "qkv")
    return torch.softmax((q @ k.t()) / math.sqrt(q.shape[-1]), dim=-1) @ v


def divisor_of(d):
    return torch.tensor(d["divisor"], dtype=torch.float32)      # the float the launch is handed


def vin(d, dtype=torch.float64):
    """z [c, m] -> [m, c] / divisor."""
    return (d["z"].to(dtype) / divisor_of(d).to(dtype)).t()


# ------------------------------------------------------------------------------------------------ emulations (packed)
def _past(*hits):
    """What lies right behind the output buffer: [(offset from the end, value)] of stray stores; sentinels elsewhere."""
    hits = [(int(o), float(v)) for o, v in hits]
    out = torch.full((max([o for o, _ in hits], default=-1) + 1,), SENT, dtype=torch.float64)
    for o, v in hits:
        out[o] = v
    return out


def _scatter(buf, idx, val):
    """buf[idx] = val where idx is inside; the rest is what a kernel would store behind the buffer."""
    idx, val = idx.reshape(-1), val.reshape(-1)
    ok = idx < buf.numel()
    buf[idx[ok]] = val[ok]
    return list(zip((idx[~ok] - buf.numel()).tolist(), val[~ok].tolist()))


def emu_conv(a, fault=None):
    H, W, cinp, cs_in, cout, coutp = a["H"], a["W"], a["cinp"], a["cs_in"], a["cout"], a["coutp"]
    up = a["in_mode"] == IN_NEAREST2
    sh, sw = (H // 2, W // 2) if up else (H, W)
    DH, DW = ((H + CONV_TH - 1) // CONV_TH * CONV_TH, (W + CONV_TW - 1) // CONV_TW * CONV_TW) if fault == "edge_store_unguarded" else (H, W)
    ys, xs = torch.arange(DH)[:, None] - 1 + torch.arange(3)[None], torch.arange(DW)[:, None] - 1 + torch.arange(3)[None]
    inside = ((ys >= 0) & (ys < H))[:, None, :, None] & ((xs >= 0) & (xs < W))[None, :, None, :]      # [DH, DW, 3, 3]
    sy, sx = ys.clamp(0, H - 1), xs.clamp(0, W - 1)
    if up:
        sy, sx = sy >> 1, sx >> 1
    stride = W if (up and fault == "nearest2_source_width_not_halved") else sw
    src = torch.cat([a["in"].double().reshape(sh * sw, cs_in), torch.full((1, cs_in), SENT, dtype=torch.float64)])
    flat = (sy[:, None, :, None] * stride + sx[None, :, None, :]).clamp(max=sh * sw).reshape(-1)
    v = src[flat, :cinp].reshape(DH, DW, 3, 3, cinp)
    zero = torch.zeros((), dtype=torch.float64)
    if a["norm"] is not None:
        nm = a["norm"].double().reshape(cs_in, 4)[:cinp]
        v = F.silu(U._norm_apply(v, nm))
        if fault == "padding_normalised":
            zero = F.silu(U._norm_apply(torch.zeros_like(v), nm))
    v = torch.where(inside[..., None], v, zero)
    ch = torch.arange(cinp)
    c0 = ch // CONV_KC * CONV_KC
    if fault == "k_tail_dropped":
        kc = (cinp - c0).clamp(max=CONV_KC)
        v = v * ((ch - c0) < kc // 16 * 16).double()
    wflat = torch.cat([a["w"].double().reshape(9 * cinp, coutp), torch.full((1, coutp), SENT, dtype=torch.float64)])
    wch = ch - c0 if fault == "chunk_weight_offset_ignores_c0" else ch
    wr = (torch.arange(9)[:, None] * (cs_in if fault == "weight_rows_by_cs_not_cinp" else cinp) + wch[None]).clamp(max=9 * cinp).reshape(-1)
    acc = v.reshape(DH, DW, 9 * cinp) @ wflat[wr]
    val = acc + a["bias"].double()
    out = a["out"].double().clone()
    if a["res"] is not None:
        res = torch.cat([(out if a["res"] is a["out"] else a["res"].double()), torch.full((1,), SENT, dtype=torch.float64)])
        p = (torch.arange(DH)[:, None] * W + torch.arange(DW)[None]).reshape(DH, DW, 1)
        ridx = p * (coutp if fault == "res_stride_is_coutp" else a["cs_res"]) + torch.arange(coutp)
        val = val + res[ridx.clamp(max=res.numel() - 1)]
    legit, hits = val[:H, :W], []
    if a["out_mode"] == OUT_ROWS:
        o = out.reshape(H * W, a["cs_out"])
        keep = CONV_NB if (fault == "z_block_channel_offset_dropped") else coutp
        o[:, :min(keep, coutp)] = legit.reshape(H * W, coutp)[:, :keep]
        o = o.reshape(-1)
        if fault == "absent_tile_stored" and (coutp // 16) % 2:      # the last tile's sums, the bias read past its end taken as 0
            idx = torch.arange(H * W)[:, None] * a["cs_out"] + coutp + torch.arange(16)[None]
            hits += _scatter(o, idx, acc[:H, :W, coutp - 16:].reshape(H * W, 16))
        if fault == "edge_store_unguarded":
            yy, xx = torch.meshgrid(torch.arange(DH), torch.arange(DW), indexing="ij")
            stray = (yy >= H) | (xx >= W)
            idx = (yy * W + xx)[stray][:, None] * a["cs_out"] + torch.arange(coutp)[None]
            hits += _scatter(o, idx, val[stray])
    elif a["out_mode"] == OUT_F32:
        o = legit[..., :cout].reshape(-1) if fault == "f32_plane_stride" else legit[..., :cout].permute(2, 0, 1).reshape(-1)
    else:                                                            # every float32 step of the epilogue, as the kernel takes it
        o = u8_epilogue(legit[..., :cout].permute(2, 0, 1)[None].float(), fault).double().reshape(-1)
    return {"out": o, "past": _past(*hits)}


def emu_rows(a, fault=None):
    m, cs_in, np_ = a["m"], a["cs_in"], a["np"]
    x = a["in"].double().reshape(m, cs_in)
    if a["norm"] is not None:
        x = U._norm_apply(x, a["norm"].double().reshape(cs_in, 4))
        if fault == "norm_with_silu":
            x = F.silu(x)
    acc = x @ a["w"].double().reshape(cs_in, np_) + a["b"].double()
    out = a["out"].double().clone()
    if a["res"] is not None and fault != "res_dropped":
        acc = acc + (out if a["res"] is a["out"] else a["res"].double()).reshape(m, np_)
    keep = 64 if fault == "tiles_past_the_fourth_dropped" else np_
    o = out.reshape(m, np_)
    o[:, :keep] = acc[:, :keep]
    hits = []
    if fault == "ragged_rows_written" and m % BM:                    # x = 0 past m: the bias, and whatever the residual has there
        hits = [(r * np_ + j, float(a["b"][j])) for r in range(BM - m % BM) for j in range(np_)]
    return {"out": o.reshape(-1), "past": _past(*hits)}


def emu_group_norm(a, fault=None):
    m, c, cs, groups = a["m"], a["c0"], a["cs0"], a["groups"]
    cpg, nblocks = c // groups, (m + GN_PIXELS - 1) // GN_PIXELS
    x = a["in0"].double().reshape(m, cs)
    fill = SENT if fault == "last_block_not_clamped" else 0.0
    xb = torch.cat([x, torch.full((nblocks * GN_PIXELS - m, cs), fill, dtype=torch.float64)]).reshape(nblocks, GN_PIXELS, cs)
    if fault == "raw_moments_f32":
        s, ss = xb.float().sum(1).double(), (xb.float() * xb.float()).sum(1).double()
    else:
        s, ss = xb.sum(1), (xb * xb).sum(1)                          # [nblocks, cs]: one slot a block and channel
    if fault == "idle_pixel_lane_counted":
        nq = cs // 4
        npl = 256 // nq
        again = xb[:, npl::npl, :4 * (256 - npl * nq)]
        s[:, :again.shape[2]] += again.sum(1)
        ss[:, :again.shape[2]] += (again * again).sum(1)
    s, ss = s[:, :c].reshape(nblocks, groups, cpg), ss[:, :c].reshape(nblocks, groups, cpg)
    if fault == "finish_first_trip_only":
        first = (torch.arange(nblocks)[:, None] * cpg + torch.arange(cpg)[None] < 256).double()[:, None, :]
        s, ss = s * first, ss * first
    n = float(m * cpg)
    if fault == "raw_moments_f32":
        gs, gss = s.float().sum((0, 2)), ss.float().sum((0, 2))
        mean32 = gs / n
        mean, var = mean32.double(), (gss / n - mean32 * mean32).double()
    else:
        mean = s.sum((0, 2)) / n
        var = ss.sum((0, 2)) / n - mean * mean
    if fault == "variance_unbiased":
        var = var * n / max(n - 1.0, 1.0)
    rstd = 1.0 / torch.sqrt(var.clamp_min(0) + float(torch.tensor(a["eps"], dtype=torch.float32)))
    mean, rstd = mean.repeat_interleave(cpg), rstd.repeat_interleave(cpg)
    hi = mean.float()
    full = torch.stack([hi, torch.zeros_like(hi) if fault == MEAN_FAULT else (mean - hi.double()).float(), (a["gamma"].double()[:c] * rstd).float(), a["beta"].float()[:c]], -1)
    o = a["norm0"].double().clone().reshape(cs, 4)
    written = (torch.arange(c) % cpg < 256) if fault == "cpg_over_256_unwritten" else torch.ones(c, dtype=torch.bool)
    o[:c][written] = full.double()[written]
    if fault != "padded_channels_not_zero":
        o[c:] = 0.0
    return {"norm0": o.reshape(-1), "past": _past()}


def streamed(q, k, v, scale, n_real, fault=None):
    """vae_attn_kernel's chunk loop: keys from n_real on score -inf."""
    m = torch.full((q.shape[0], 1), -math.inf, dtype=q.dtype)
    l, o = torch.zeros_like(m), torch.zeros((q.shape[0], v.shape[1]), dtype=q.dtype)
    for k0 in range(0, k.shape[0], ATTN_BK):
        s = (q @ k[k0:k0 + ATTN_BK].t()) * scale
        s[:, max(n_real - k0, 0):] = -math.inf
        m_new = torch.maximum(m, s.max(dim=-1, keepdim=True).values)
        pr, alpha = torch.exp(s - m_new), torch.exp(m - m_new)
        l = (l if fault == "sum_not_rescaled" else l * alpha) + pr.sum(dim=-1, keepdim=True)
        o = (o if fault == "no_rescale_on_new_max" else o * alpha) + pr @ v[k0:k0 + ATTN_BK]
        m = m_new
    return o / l


def emu_attention(a, fault=None):
    n, c, cs = a["n"], a["c"], a["cs"]
    qkv = a["qkv"].double().reshape(n, 3 * cs)
    q, k, v = qkv[:, :cs], qkv[:, cs:2 * cs], qkv[:, 2 * cs:]
    padded = (n + ATTN_BK - 1) // ATTN_BK * ATTN_BK
    k, v = (torch.cat([t, torch.zeros((padded - n, cs), dtype=torch.float64)]) for t in (k, v))      # the loader's zeros past n
    res = streamed(q, k, v, 1.0 / math.sqrt(cs if fault == "scale_by_cs_not_c" else c), padded if fault == "ragged_keys_score_zero" else n, fault)
    o = a["out"].double().clone().reshape(n, cs)
    keep = 64 if fault == "tiles_past_the_first_round_dropped" else cs
    o[:, :keep] = res[:, :keep]
    return {"out": o.reshape(-1), "past": _past()}


def emu_in(a, fault=None):
    c, m = a["c"], a["m"]
    z, div = a["z"].double(), float(torch.tensor(a["divisor"], dtype=torch.float32))
    zt = z.reshape(m, c) if fault == "plane_stride" else z.reshape(c, m).t()
    o = a["out"].double().clone().reshape(m, 16)
    o[:, :c] = zt * div if fault == "multiplied_not_divided" else zt / div
    if fault != "columns_past_c_not_zero":
        o[:, c:] = 0.0
    return {"out": o.reshape(-1), "past": _past()}


EMU = {"conv": emu_conv, "rows": emu_rows, "group_norm": emu_group_norm, "attention": emu_attention, "in": emu_in}
