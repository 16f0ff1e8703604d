"""What each launch of csrc/unet.hip computes, twice over.

The references (`conv`, `rows`, `group_norm`, `layer_norm_stats`, `attention`, `embedding`, `temb`, `rows_in`) are plain torch
restatements on dense tensors with no layout in them, in whatever float dtype they are handed: float64 is the reference, float32
the yardstick of a tolerance.  They reuse tests/unet_ref.py where it already states the operation.

The emulations (`emu_*`) restate each kernel's INDEXING in float64 on the packed buffers of csrc/unet_api.h (rows [n m][cs],
Wt[K][N], VaeNorm [n][cs], float4 statistics), as tests/unet_kernels.py packs them, and return the output buffers the kernel
would leave, sentinels included.  `fault` names one deliberate indexing mistake (FAULTS); tests/test_unet_kernels_host.py shows
that every one of them fails its case.  What a fault means where the name leaves room:

  sample_ignores_channel_blocks     sample = min(blockIdx.z, n - 1): sample 0 gets its first channel block only
  weight_offset_by_cs_not_cinp      the second source's weight rows start at cs0, not at c0 rounded up to 4
  k_tail_dropped                    a source's last, partial K chunk is not run
  second_tile_of_ragged_block_kept  the absent second tile of the last wave is stored, sixteen columns past the row
  gate_tile_mispaired               GEGLU pairs a value tile with its neighbour's gate (an absent neighbour reads tile 0)
  second_source_weight_row_offset   the second source's weight rows start at 0
  seam_group_split_at_cs            the group across the seam is normalised per source, each part by its own moments
  last_partial_block_full           the last block of 512 pixels reads 512 pixels whatever m is (zeros past the buffer)
  ragged_chunk_unmasked             the keys past nk of the last chunk score 0, not -inf
  kv_stride_of_q                    k and v rows are addressed with ldq
  class_row_of_label_0              the class row is row 0 of the table, not the label's
  mean_lo_dropped                   (GroupNorm and LayerNorm statistics) the mean's low float is left 0
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import unet_ref as U

SENT = -777.0
FAULTS = {"conv": ("sample_ignores_channel_blocks", "weight_offset_by_cs_not_cinp", "k_tail_dropped", "up_reads_gx_not_halved", "stride2_pad_right_bottom",
                   "norm_on_padding_taps", "second_tile_of_ragged_block_kept"),
          "rows": ("gate_tile_mispaired", "norm_of_sample_0_for_all_rows", "second_source_weight_row_offset"),
          "group_norm": ("seam_group_split_at_cs", "last_partial_block_full", "padded_norm_left"),
          "layer_norm_stats": ("mean_over_cs", "one_pass_f32"),
          "attention": ("no_rescale_on_new_max", "ragged_chunk_unmasked", "head_offset_by_dp", "pad_columns_left", "kv_stride_of_q"),
          "embedding": ("sin_cos_order", "class_row_of_label_0")}
EXTRA_FAULTS = {"mean_lo_dropped": ("group_norm", "layer_norm_stats")}      # beyond the issue's list: held to the mean's own bound
GN_PIXELS, ATTN_BK, CONV_NB = 512, 32, 128       # csrc/vae_api.h: VAE_GN_PIXELS, VAE_CONV_NB; csrc/unet_api.h: UNET_ATTN_BK


def up16(c):
    return (c + 15) // 16 * 16


def up4(c):
    return (c + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ references (dense)
def _affine_silu(x, nm, dtype, act=True):
    """x [n, c, ...] through a given norm (mean [n, c] float64, a [n, c], beta [c]); SiLU for a conv's loader."""
    x = x.to(dtype)
    if nm is None:
        return x
    mean, a, beta = (t.to(dtype) for t in nm)
    shape = mean.shape + (1,) * (x.dim() - 2)
    y = (x - mean.reshape(shape)) * a.reshape(shape) + beta.reshape((1, -1) + (1,) * (x.dim() - 2))
    return F.silu(y) if act else y


def conv(d, dtype=torch.float64):
    x = _affine_silu(d["x0"], d.get("norm0"), dtype)
    if d.get("x1") is not None:
        x = torch.cat([x, _affine_silu(d["x1"], d.get("norm1"), dtype)], 1)
    if d.get("up"):
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    y = F.conv2d(x, d["w"].to(dtype), d["b"].to(dtype), stride=d.get("stride", 1), padding=1)
    return y if d.get("res") is None else y + d["res"].to(dtype)


def rows(d, dtype=torch.float64):
    """x0 | x1 [n, rows_per_sample, c] -> prologue -> x w^T + b -> (+ res | GEGLU) [n, rows_per_sample, nout]."""
    if d.get("prologue") == "layernorm":
        mean, rstd = d["ln"]
        x = (d["x0"].to(dtype) - mean.to(dtype)[..., None]) * rstd.to(dtype)[..., None] * d["ln_g"].to(dtype) + d["ln_b"].to(dtype)
    else:
        gn = d.get("prologue") == "groupnorm"
        x = _affine_silu(d["x0"].transpose(1, 2), d["norm0"] if gn else None, dtype, act=False).transpose(1, 2)
        if d.get("x1") is not None:
            x = torch.cat([x, _affine_silu(d["x1"].transpose(1, 2), d["norm1"] if gn else None, dtype, act=False).transpose(1, 2)], -1)
    y = F.linear(x, d["w"].to(dtype), d["b"].to(dtype))
    if d.get("geglu"):
        value, gate = y.chunk(2, dim=-1)
        y = value * F.gelu(gate)
    return y if d.get("res") is None else y + d["res"].to(dtype)


def group_norm(d, dtype=torch.float64):
    """(mean, a, beta) [n, C] each of GroupNorm over cat(x0, x1) [n, C, m]: x -> (x - mean) a + beta, a = gamma rstd."""
    x = d["x0"].to(dtype) if d.get("x1") is None else torch.cat([d["x0"], d["x1"]], 1).to(dtype)
    n, c, m = x.shape
    g = x.reshape(n, d["groups"], -1)
    mean, var = g.mean(-1), g.var(-1, unbiased=False)
    cpg = c // d["groups"]
    rstd = 1.0 / torch.sqrt(var + d["eps"])
    return (mean.repeat_interleave(cpg, 1), d["gamma"].to(dtype)[None] * rstd.repeat_interleave(cpg, 1), d["beta"].to(dtype)[None].expand(n, c).clone())


def layer_norm_stats(d, dtype=torch.float64):
    x = d["x"].to(dtype)
    return x.mean(-1), 1.0 / torch.sqrt(x.var(-1, unbiased=False) + d["eps"])


def attention(d, dtype=torch.float64):
    """q [s, heads, nq, d], k and v [s, heads, nk, d] -> [s, nq, heads d]."""
    q, k, v = (d[x].to(dtype) for x in "qkv")
    o = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1]), dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[2], -1)


def embedding(d, dtype=torch.float64, fault=None):
    """silu(time_embedding(sinusoid(t)) + the label's class row) [td]: tests/unet_ref.py's time_embedding, then the SiLU every consumer applies."""
    p = {"time_embedding.linear_1.weight": d["w1"], "time_embedding.linear_1.bias": d["b1"], "time_embedding.linear_2.weight": d["w2"],
         "time_embedding.linear_2.bias": d["b2"], "class_embedding.weight": d["table"]}
    p = {k: v.to(dtype) for k, v in p.items()}
    return F.silu(U.time_embedding(p, d["t"], d["label"], d["w1"].shape[1], dtype, fault))[0]


def temb(d, dtype=torch.float64):
    """per resnet: conv1.bias + time_emb_proj(semb)."""
    return [cb.to(dtype) + F.linear(d["semb"].to(dtype), w.to(dtype), b.to(dtype)) for w, b, cb in d["resnets"]]


def rows_in(d):
    """NCHW [n, c, m] -> [n m, c]; row-major stays."""
    return d["src"].permute(0, 2, 1).reshape(-1, d["src"].shape[1]) if d["nchw"] else d["src"]


# ------------------------------------------------------------------------------------------------ emulations (packed)
def _norm_apply(v, nm):
    return ((v - nm[..., 0]) - nm[..., 1]) * nm[..., 2] + nm[..., 3]


def _out_start(a):
    """The output buffer as the launch finds it: sentinels, or the residual where res is the output."""
    return a["out"].double().clone()


def emu_conv(a, fault=None):
    n, H, W, S, up, coutp = a["n"], a["H"], a["W"], a["stride"], a["up"], a["coutp"]
    DH, DW = H * S, W * S
    sh, sw = (H // 2, W // 2) if up else (DH, DW)
    sm, KC = sh * sw, 64 // S
    cinp = [up4(a["c0"]), up4(a["c1"]) if a["in1"] is not None else 0]
    wflat = torch.cat([a["w"].double(), torch.zeros((1, coutp), dtype=torch.float64)])      # one zero row: every read past the end
    acc = torch.zeros((n, H, W, coutp), dtype=torch.float64)
    off = 0 if (fault == "stride2_pad_right_bottom" and S == 2) else -1
    ys = torch.arange(H)[:, None] * S + off + torch.arange(3)[None]
    xs = torch.arange(W)[:, None] * S + off + torch.arange(3)[None]
    inside = ((ys >= 0) & (ys < DH))[:, None, :, None] & ((xs >= 0) & (xs < DW))[None, :, None, :]      # [H, W, 3, 3]
    sy, sx = ys.clamp(0, DH - 1), xs.clamp(0, DW - 1)
    if up:
        sy, sx = sy >> 1, (sx if fault == "up_reads_gx_not_halved" else sx >> 1)
    flat = (sy[:, None, :, None] * sw + sx[None, :, None, :]).clamp(max=sm - 1).reshape(-1)
    for seg in (0, 1):
        src = a[f"in{seg}"]
        if src is None:
            break
        cs, cseg = a[f"cs{seg}"], cinp[seg]
        wrow = 0 if seg == 0 else (a["cs0"] if fault == "weight_offset_by_cs_not_cinp" else cinp[0])
        kept = cseg // KC * KC if fault == "k_tail_dropped" else cseg
        v = src.double().reshape(n, sm, cs)[:, flat, :cseg].reshape(n, H, W, 3, 3, cseg)
        zero = torch.zeros((), dtype=torch.float64)
        if a[f"norm{seg}"] is not None:
            nm = a[f"norm{seg}"].double().reshape(n, 1, 1, 1, 1, cs, 4)[..., :cseg, :]
            v = F.silu(_norm_apply(v, nm))
            if fault == "norm_on_padding_taps":
                zero = F.silu(_norm_apply(torch.zeros_like(v), nm))
        v = torch.where(inside[None, ..., None], v, zero)[..., :kept]
        wr = (torch.arange(9)[:, None] * (cinp[0] + cinp[1]) + wrow + torch.arange(kept)[None]).clamp(max=wflat.shape[0] - 1).reshape(-1)
        acc += v.reshape(n, H, W, 9 * kept) @ wflat[wr]
    out = _out_start(a)
    val = acc + a["bias"].double()
    if a["res"] is not None:
        val = val + (out if a["res"] is a["out"] else a["res"].double()).reshape(n, H, W, coutp)
    if a["out_nchw"]:
        return {"out": val[..., :a["cout"]].permute(0, 3, 1, 2).reshape(-1)}
    o = out.reshape(n, H, W, coutp)
    o[:] = val
    if fault == "sample_ignores_channel_blocks" and n > 1 and coutp > CONV_NB:
        o[0, ..., CONV_NB:] = a["out"].double().reshape(n, H, W, coutp)[0, ..., CONV_NB:]
    o = o.reshape(-1)
    if fault == "second_tile_of_ragged_block_kept" and (coutp // 16) % 2:
        idx = (torch.arange(n * H * W)[:, None] * coutp + coutp + torch.arange(16)[None]).reshape(-1)
        stray = acc[..., coutp - 16:].reshape(-1)      # the last tile's sums, the bias read past its end taken as 0
        ok = idx < o.numel()
        o[idx[ok]] = stray[ok]
    return {"out": o}


def emu_rows(a, fault=None):
    m, np_, cs0 = a["m"], a["np"], a["cs0"]
    x = [a["in0"].double().reshape(m, cs0)]
    if a["in1"] is not None:
        x.append(a["in1"].double().reshape(m, a["cs1"]))
    if a["prologue"] == 1:
        sample = torch.zeros(m, dtype=torch.long) if fault == "norm_of_sample_0_for_all_rows" else torch.arange(m) // a["rows_per_sample"]
        x = [_norm_apply(t, a[f"norm{i}"].double().reshape(-1, t.shape[1], 4)[sample]) for i, t in enumerate(x)]
    elif a["prologue"] == 2:
        st = a["ln"].double().reshape(m, 4)
        x = [((x[0] - st[:, 0:1]) - st[:, 1:2]) * st[:, 2:3] * a["ln_g"].double() + a["ln_b"].double()]
    w = a["w"].double().reshape(-1, a["ldw"])
    acc = x[0] @ w[:cs0]
    if len(x) > 1:
        krow = 0 if fault == "second_source_weight_row_offset" else cs0
        acc = acc + x[1] @ w[krow:krow + a["cs1"]]
    acc = acc + a["b"].double()
    out = _out_start(a)
    if a["geglu"]:
        value, gate = acc[:, :np_], acc[:, np_:]
        if fault == "gate_tile_mispaired":
            tiles = np_ // 16
            other = [(t ^ 1) if (t ^ 1) < tiles else 0 for t in range(tiles)]
            gate = gate.reshape(m, tiles, 16)[:, other].reshape(m, np_)
        acc = value * F.gelu(gate)
    if a["res"] is not None:
        acc = acc + (out if a["res"] is a["out"] else a["res"].double()).reshape(m, np_)
    return {"out": acc.reshape(-1)}


def emu_group_norm(a, fault=None):
    n, m, groups = a["n"], a["m"], a["groups"]
    c = [a["c0"], a["c1"] if a["in1"] is not None else 0]
    cpg = (c[0] + c[1]) // groups
    s, ss = [], []
    for i in (0, 1):
        if not c[i]:
            break
        cs = a[f"cs{i}"]
        x = a[f"in{i}"].double().reshape(n * m, cs)
        if fault == "last_partial_block_full":
            reach = (m + GN_PIXELS - 1) // GN_PIXELS * GN_PIXELS
            x = torch.cat([x, torch.zeros((reach, cs), dtype=torch.float64)])
            x = torch.stack([x[k * m:k * m + reach] for k in range(n)])
        else:
            x = x.reshape(n, m, cs)
        s.append(x.sum(1)[:, :c[i]])
        ss.append((x * x).sum(1)[:, :c[i]])
    s, ss = torch.cat(s, 1), torch.cat(ss, 1)      # [n, C]: the concatenation's order
    count = torch.full((n, groups), float(m * cpg), dtype=torch.float64)
    gs, gss = s.reshape(n, groups, cpg).sum(-1), ss.reshape(n, groups, cpg).sum(-1)
    mean = (gs / count).repeat_interleave(cpg, 1)
    var = (gss / count).repeat_interleave(cpg, 1) - mean * mean
    if fault == "seam_group_split_at_cs" and c[1] and c[0] % cpg:
        g = c[0] // cpg
        for lo, hi in ((g * cpg, c[0]), (c[0], (g + 1) * cpg)):
            mu = s[:, lo:hi].sum(-1, keepdim=True) / (m * (hi - lo))
            mean[:, lo:hi] = mu
            var[:, lo:hi] = ss[:, lo:hi].sum(-1, keepdim=True) / (m * (hi - lo)) - mu * mu
    rstd = 1.0 / torch.sqrt(var.clamp_min(0) + float(a["eps"]))
    hi = mean.float()
    full = torch.stack([hi, torch.zeros_like(hi) if fault == "mean_lo_dropped" else (mean - hi.double()).float(), (a["gamma"].double()[None] * rstd).float(), a["beta"].float()[None].expand(n, -1)], -1)
    outs, at = {}, 0
    for i in (0, 1):
        if not c[i]:
            break
        o = a[f"norm{i}"].double().clone().reshape(n, a[f"cs{i}"], 4)
        o[:, :c[i]] = full[:, at:at + c[i]].double()
        if fault != "padded_norm_left":
            o[:, c[i]:] = 0.0
        outs[f"norm{i}"] = o.reshape(-1)
        at += c[i]
    return outs


def emu_layer_norm_stats(a, fault=None):
    c = a["c"]
    x = a["in"].double().reshape(a["m"], a["cs"])[:, :c]
    over = a["cs"] if fault == "mean_over_cs" else c
    if fault == "one_pass_f32":
        x32 = x.float()
        mean = (x32.sum(-1) / over).double()
        var = ((x32 * x32).sum(-1) / over - (x32.sum(-1) / over) ** 2).clamp_min(0).double()
    else:
        mean = x.sum(-1) / over
        var = ((x - mean[:, None]) ** 2).sum(-1) / over
    hi = mean.float()
    st = torch.stack([hi, torch.zeros_like(hi) if fault == "mean_lo_dropped" else (mean - hi.double()).float(), (1.0 / torch.sqrt(var + float(a["eps"]))).float(), torch.zeros_like(hi)], -1)
    return {"out": st.double().reshape(-1)}


def emu_attention(a, fault=None):
    s_, nq, nk, heads, d = a["samples"], a["nq"], a["nk"], a["heads"], a["d"]
    dp = up16(d)
    hoff = dp if fault == "head_offset_by_dp" else d
    ldkv = a["ldq"] if fault == "kv_stride_of_q" else a["ldkv"]

    def take(buf, off, rows, ld, sample, head):
        idx = off + (sample * rows + torch.arange(rows)[:, None]) * ld + head * hoff + torch.arange(d)[None]
        return buf.double().reshape(-1)[idx.clamp(max=buf.numel() - 1)]

    out = _out_start(a).reshape(s_ * nq, a["ldo"])
    for sample in range(s_):
        for head in range(heads):
            q = take(a["qbuf"], a["q_off"], nq, a["ldq"], sample, head)
            k = take(a["kvbuf"], a["k_off"], nk, ldkv, sample, head)
            v = take(a["kvbuf"], a["v_off"], nk, ldkv, sample, head)
            if fault == "ragged_chunk_unmasked" and nk % ATTN_BK:
                pad = torch.zeros((ATTN_BK - nk % ATTN_BK, d), dtype=torch.float64)
                k, v = torch.cat([k, pad]), torch.cat([v, pad])
            o = U.streamed_attention(q, k, v, 1.0 / math.sqrt(d), chunk=ATTN_BK, rescale=fault != "no_rescale_on_new_max")
            out[sample * nq:(sample + 1) * nq, head * d:(head + 1) * d] = o
    if fault != "pad_columns_left":
        out[:, heads * d:] = 0.0
    return {"out": out.reshape(-1)}


def emu_embedding(a, fault=None):
    c0, td, tdp = a["c0"], a["td"], a["tdp"]
    half = c0 // 2
    ang = float(a["t"]) * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    sn = torch.cat([torch.sin(ang), torch.cos(ang)] if fault == "sin_cos_order" else [torch.cos(ang), torch.sin(ang)]).float().double()
    hid = F.silu(a["b1"].double()[:td] + sn @ a["w1"].double().reshape(c0, tdp)[:, :td])
    row = a["table"].double().reshape(-1, tdp)[0 if fault == "class_row_of_label_0" else a["label"]]
    out = _out_start(a)
    out[:td] = F.silu(a["b2"].double()[:td] + hid @ a["w2"].double().reshape(td, tdp)[:, :td] + row[:td])
    out[td:tdp] = 0.0
    return {"out": out}


def emu_temb(a, fault=None):
    out = _out_start(a).reshape(a["count"], -1)
    wts = a["weights"].double()
    for r in range(a["count"]):
        cp = a["coutp"][r]
        w = wts[a["w_off"][r]:a["w_off"][r] + a["td"] * cp].reshape(a["td"], cp)
        out[r, :cp] = wts[a["cb_off"][r]:a["cb_off"][r] + cp] + wts[a["b_off"][r]:a["b_off"][r] + cp] + a["semb"].double()[:a["td"]] @ w
    return {"out": out.reshape(-1)}


def emu_in(a, fault=None):
    c, cs, rows_ = a["c"], a["cs"], a["rows"]
    out = torch.zeros((rows_, cs), dtype=torch.float64)
    src = a["src"].double()
    out[:, :c] = src.reshape(rows_ // a["m"], c, a["m"]).permute(0, 2, 1).reshape(rows_, c) if a["nchw"] else src.reshape(rows_, c)
    return {"out": out.reshape(-1)}


EMU = {"conv": emu_conv, "rows": emu_rows, "group_norm": emu_group_norm, "layer_norm_stats": emu_layer_norm_stats, "attention": emu_attention,
       "embedding": emu_embedding, "temb": emu_temb, "in": emu_in}
