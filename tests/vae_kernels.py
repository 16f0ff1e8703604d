"""The per-launch cases of csrc/vae.hip: one launch (or one short chain) of a kernel on a frame of a few pixels, through the
nesr_vae_k_* test hooks.  The shape, and where they fit the helpers, of tests/unet_kernels.py.  This module holds

  * the packing, written from csrc/vae_api.h's comments and not by calling nesr_vae_finalize: dense torch tensors -> rows [m][cs]
    with cs the width rounded up to 16 and zeros past the width, a 3x3 weight [9 cinp][coutp] with cinp the input width rounded up
    to 4, a 1x1 weight Wt[cs_in][np], VaeNorm [cs], the NEAREST2 source as its (H / 2) x (W / 2) grid of rows, the NCHW f32 sample
    and the HWC u8 frame; and back (`unpack`), which also says whether every padded column holds what the header documents;
  * the cases (`CASES` by name).  Exact cases carry small integers (activations in [-3, 3], weights in {-1, 0, 1}; the u8 case
    integers x 2^-7): every partial sum is exact in float32 in any order, so the GPU must give the float64 reference bit for bit.
    Toleranced cases carry random floats; their tolerance is 8 x max |float32 restatement - float64| per compared quantity,
    computed where it is used and never written down;
  * `launch`: the GPU run of a case's arguments, every output embedded in sentinels whose guards are asserted.

tests/vae_kernel_ref.py holds the references and the float64 emulations; FAULT_CASE says which case must expose which fault.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

from tests import unet_kernels as K
from tests import vae_kernel_ref as R
from tests.unet_kernels import Case, GUARD, SELECTOR_LEAD, from_rows, gen, ints, is_exact, pack_norm, pad_cols, ratios, rnd, sentinels, to_rows      # noqa: F401
from tests.vae_cases import _tie_bias
from tests.vae_kernel_ref import SENT, up4, up16

TIE_LEVELS = (100, 101, 200)          # conv_u8_ties: sample x 255 is k + 0.5 in float32 for these k, one per channel
RES_JUNK = 5.0                        # what the columns past coutp of a wide residual hold


# ------------------------------------------------------------------------------------------------ packing
def pack_conv(d):
    x, w = d["x"], d["w"]
    cin, (h, wd) = x.shape[1], x.shape[2:]
    up, cout = int(bool(d.get("up"))), w.shape[0]
    H, W = (2 * h, 2 * wd) if up else (h, wd)
    cinp, coutp, mode = up4(cin), up16(cout), {"rows": R.OUT_ROWS, "f32": R.OUT_F32, "u8": R.OUT_U8}[d.get("out", "rows")]
    wp = torch.zeros((9, cinp, coutp), dtype=torch.float32)
    wp[:, :cin, :cout] = w.float().permute(2, 3, 1, 0).reshape(9, cin, cout)      # [ky kx][cin][cout]
    a = dict(in_mode=R.IN_NEAREST2 if up else R.IN_ROWS, H=H, W=W, cin=cin, cinp=cinp, cs_in=up16(cin), norm=None, w=wp.reshape(-1),
             bias=pad_cols(d["b"].float()[None], coutp).reshape(-1), cout=cout, coutp=coutp, res=None, cs_res=0, out_mode=mode,
             cs_out=coutp if mode == R.OUT_ROWS else 0, **{"in": to_rows(x)})
    if d.get("norm") is not None:
        a["norm"] = pack_norm(d["norm"], a["cs_in"])
    a["out"] = (sentinels(H * W * coutp) if mode == R.OUT_ROWS else sentinels(cout * H * W) if mode == R.OUT_F32
                else torch.full((H * W * cout,), R.U8_SENT, dtype=torch.uint8))
    if d.get("res") is not None:
        a["cs_res"] = coutp + d.get("res_extra", 0)
        r = torch.full((H * W, a["cs_res"]), RES_JUNK, dtype=torch.float32)
        r[:, :coutp] = to_rows(d["res"]).reshape(H * W, coutp)
        a["res"] = r.reshape(-1)
        if d.get("inplace"):
            a["out"] = a["res"]
    return a


def pack_rows(d):
    x, w = d["x"], d["w"]
    m, c = x.shape
    nout, cs_in = w.shape[0], up16(c)
    np_ = up16(nout)
    a = dict(m=m, cs_in=cs_in, np=np_, nout=nout, norm=None, w=K.pack_wt(w, cs_in, np_).reshape(-1), b=pad_cols(d["b"].float()[None], np_).reshape(-1), res=None,
             out=sentinels(m * np_), **{"in": pad_cols(x.float(), cs_in).reshape(-1)})
    if d.get("norm") is not None:
        a["norm"] = pack_norm(d["norm"], cs_in)
    if d.get("res") is not None:
        a["res"] = pad_cols(d["res"].float(), np_).reshape(-1)
        if d.get("inplace"):
            a["out"] = a["res"]
    if d.get("out_is_in"):
        a["out"] = a["in"]
    return a


def pack_group_norm(d):
    c = d["x0"].shape[1]
    a = K.pack_group_norm(d)                       # one sample, one source
    a["gamma"], a["beta"] = (pad_cols(d[k].float()[None], up16(c)).reshape(-1) for k in ("gamma", "beta"))
    return a


def pack_attention(d):
    q, k, v = (d[x][0, 0].float() for x in "qkv")
    n, c = q.shape
    cs = up16(c)
    return dict(n=n, c=c, cs=cs, qkv=torch.cat([pad_cols(t, cs) for t in (q, k, v)], 1).reshape(-1), out=sentinels(n * cs))


def pack_in(d):
    c, m = d["z"].shape
    return dict(z=d["z"].float().reshape(-1), c=c, m=m, divisor=float(R.divisor_of(d)), out=sentinels(m * 16))


PACK = {"conv": pack_conv, "rows": pack_rows, "group_norm": pack_group_norm, "attention": pack_attention, "in": pack_in}
REF = {"conv": R.conv, "rows": R.rows, "group_norm": R.group_norm, "attention": R.attention, "in": R.vin}
OUTPUTS = {"group_norm": ("norm0",)}               # the output buffer of a family's arguments; ("out",) otherwise


def unpack(family, a, outs):
    """The dense result of the output buffer, as a tuple of the quantities that are compared, and whether every padded column
    holds what csrc/vae_api.h documents."""
    zero = lambda t: bool((t == 0).all())
    if family == "conv":
        if a["out_mode"] == R.OUT_F32:
            return (outs["out"].reshape(1, a["cout"], a["H"], a["W"]),), True
        if a["out_mode"] == R.OUT_U8:
            return (outs["out"].reshape(a["H"], a["W"], a["cout"]).float(),), True
        y, pad = from_rows(outs["out"], 1, a["cout"], a["H"], a["W"])
        return (y,), zero(pad)
    if family == "rows":
        r = outs["out"].reshape(a["m"], a["np"])
        return (r[:, :a["nout"]],), zero(r[:, a["nout"]:])
    if family == "group_norm":
        o = outs["norm0"].reshape(a["cs0"], 4).double()
        c = a["c0"]
        return (o[:c, 0] + o[:c, 1], o[:c, 2], o[:c, 3]), zero(o[c:])
    if family == "attention":
        o = outs["out"].reshape(a["n"], a["cs"])
        return (o[:, :a["c"]],), zero(o[:, a["c"]:])
    if family == "in":
        r = outs["out"].reshape(a["m"], 16)
        return (r[:, :a["c"]],), zero(r[:, a["c"]:])
    raise KeyError(family)


def reference(case, dtype=torch.float64):
    with torch.no_grad():
        return K.as_tuple(REF[case.family](case.dense, dtype))


def exact_bound(case):
    """max over the outputs of sum_k |x_k| |w_k| (+ |bias|, + |residual|) in units of the case's grid (1; 2^-7 for the u8 case):
    below 2^24 every partial sum is an exact float32."""
    d = {k: (v.abs() if torch.is_tensor(v) else v) for k, v in case.dense.items()}
    if case.family == "in":
        return float(case.dense["z"].abs().max()) / min(1.0, case.dense["divisor"])
    unit = case.dense.get("unit", 1.0)
    d["out"] = "rows"
    with torch.no_grad():
        return max(float(t.max()) for t in K.as_tuple(REF[case.family](d, torch.float64))) / unit


def mean_bound(case):
    """2^-38 max |x|, the bound of the UNet's statistics pins (K.mean_bound, used where its premise of at most 2^13 terms a mean
    holds).  The two cases with more terms (m = 20000; 512 channels a group) are held to the same figure on vae.hip's own order of
    summation: the error of a sum is at most (the longest chain of additions) 2^-53 sum |x|, and no double here ends a chain of 2^13
    additions: a pixel lane adds at most 512 / npl <= 256 pixels, a channel its npl <= 128 lanes, a thread of the finish
    ceil(nblocks cpg / 256) slots, the tree 8 levels."""
    c, m = case.dense["x0"].shape[1:]
    cpg = c // case.dense["groups"]
    if m * cpg <= 2 ** 13:
        return K.mean_bound(case)
    assert 256 + 128 + ((m + R.GN_PIXELS - 1) // R.GN_PIXELS * cpg + 255) // 256 + 8 <= 2 ** 13
    return 2.0 ** -38 * float(case.dense["x0"].abs().max())


def split_mean(mean64):
    """A double mean as the (hi, lo) pair of floats carries it."""
    hi = mean64.float()
    return hi.double() + (mean64 - hi.double()).float().double()


def selected_chunks(case):
    """Per query the chunk of its best key (float64)."""
    q, k = case.dense["q"][0, 0].double(), case.dense["k"][0, 0].double()
    return (q @ k.t()).argmax(-1) // R.ATTN_BK


# ------------------------------------------------------------------------------------------------ the GPU run
def launch(family, a, expect_rc=0):
    """One nesr_vae_k_* call on the packed arguments: ({name: output buffer on the host}, {name: the same on the device}).  Every
    output lies between guards of sentinels, which are asserted; a tensor that is both an input and the output (res == out,
    out == in) is one device buffer; a tensor that is on the device already (a chain) is used where it lies."""
    import ctypes

    from neural_enhanced_super_resolution_amd import _lib
    lib, dev = _lib.load(), "cuda:0"
    held, bufs = {}, {}
    for name in OUTPUTS.get(family, ("out",)):
        t = a[name]
        sent = R.U8_SENT if t.dtype == torch.uint8 else SENT
        buf = torch.full((GUARD + t.numel() + GUARD,), sent, dtype=t.dtype)
        buf[GUARD:GUARD + t.numel()] = t.cpu()
        bufs[name] = (buf.to(dev), sent)
        held[id(t)] = bufs[name][0][GUARD:GUARD + t.numel()]

    def ptr(t):
        if t is None:
            return None
        if id(t) not in held:
            held[id(t)] = t.contiguous().to(dev)
        return ctypes.c_void_p(held[id(t)].data_ptr())

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if family == "conv":
        rc = lib.nesr_vae_k_conv(a["in_mode"], ptr(a["in"]), a["H"], a["W"], a["cin"], a["cinp"], a["cs_in"], ptr(a["norm"]), ptr(a["w"]), ptr(a["bias"]),
                                 a["cout"], a["coutp"], ptr(a["res"]), a["cs_res"], a["out_mode"], ptr(a["out"]), a["cs_out"], stream)
    elif family == "rows":
        rc = lib.nesr_vae_k_rows(a["m"], a["cs_in"], a["np"], ptr(a["in"]), ptr(a["norm"]), ptr(a["w"]), ptr(a["b"]), ptr(a["res"]), ptr(a["out"]), stream)
    elif family == "group_norm":
        part = torch.zeros(max((a["m"] + R.GN_PIXELS - 1) // R.GN_PIXELS, 1) * a["cs0"] * 2, dtype=torch.float64, device=dev)
        rc = lib.nesr_vae_k_group_norm(ptr(a["in0"]), a["m"], a["c0"], a["cs0"], a["groups"], ctypes.c_void_p(part.data_ptr()), ptr(a["gamma"]), ptr(a["beta"]),
                                       a["eps"], ptr(a["norm0"]), stream)
    elif family == "attention":
        rc = lib.nesr_vae_k_attention(a["n"], a["c"], a["cs"], ptr(a["qkv"]), ptr(a["out"]), stream)
    elif family == "in":
        rc = lib.nesr_vae_k_in(ptr(a["z"]), a["c"], a["m"], a["divisor"], ptr(a["out"]), stream)
    else:
        raise KeyError(family)
    torch.cuda.synchronize()
    assert rc == expect_rc, f"nesr_vae_k_* ({family}) returned {rc}: {(lib.nesr_last_error() or b'').decode()}"
    outs, on_dev = {}, {}
    for name, (buf, sent) in bufs.items():
        host, count = buf.cpu(), a[name].numel()
        assert bool((host[:GUARD] == sent).all()) and bool((host[GUARD + count:] == sent).all()), f"{family}: the launch wrote outside `{name}`"
        outs[name], on_dev[name] = host[GUARD:GUARD + count], buf[GUARD:GUARD + count]
    return outs, on_dev


# ------------------------------------------------------------------------------------------------ the cases
def _conv_exact(seed, cin, cout, h, w, **more):
    """h x w: the SOURCE grid.  Integer activations, weights in {-1, 0, 1}, integer bias."""
    g = gen(seed)
    d = dict(x=ints(g, (1, cin, h, w)), w=ints(g, (cout, cin, 3, 3), -1, 1), b=ints(g, (cout,)), **more)
    if more.get("inplace") or "res_extra" in more:
        d["res"] = ints(g, (1, cout, h, w))
    return d


def _conv_u8_exact():
    """Every result is k / 128: integer activations in [-3, 3], weights and bias integers in [-4, 4] x 2^-7; the bias of channel 0
    is moved so that the first pixel's k is 0 (127.5, which rounds to 128)."""
    g = gen(230)
    d = dict(x=ints(g, (1, 16, 5, 17)), w=ints(g, (3, 16, 3, 3), -4, 4) / 128.0, b=ints(g, (3,), -4, 4) / 128.0, out="u8", unit=1.0 / 128.0)
    with torch.no_grad():
        d["b"][0] -= float(R.conv(dict(d, out="rows"))[0, 0, 0, 0])
    return d


def u8_levels(case):
    """conv_u8_exact: the integer k of every sample before the epilogue."""
    with torch.no_grad():
        k = R.conv(dict(case.dense, out="rows")) * 128.0
    assert bool((k == k.round()).all())
    return k


def _conv_u8_ties():
    return dict(x=ints(gen(231), (1, 16, 4, 16)), w=torch.zeros((3, 16, 3, 3)), b=torch.tensor([_tie_bias(k) for k in TIE_LEVELS], dtype=torch.float32),
                out="u8", epilogue32=True)


def _conv_norm():
    """A given VaeNorm at 80 channels on 9 x 19: the group means are not float32 numbers (mean_lo is not zero) and beta is about 2,
    so a tap outside the image that went through the norm would add silu(beta - mean a), not 0."""
    g = gen(240)
    x = rnd(g, (1, 80, 9, 19)) + 0.5 + 0.3 * rnd(g, (1, 80, 1, 1))
    return dict(x=x, norm=K.given_norm(x, 8, 1.0 + 0.3 * rnd(g, (80,)), 2.0 + 0.2 * rnd(g, (80,)), 1e-6), w=rnd(g, (24, 80, 3, 3), 1.0 / math.sqrt(720)),
                b=rnd(g, (24,), 0.2))


def _conv_random():
    g = gen(241)
    return dict(x=rnd(g, (1, 512, 3, 5)), w=rnd(g, (128, 512, 3, 3), 1.0 / math.sqrt(4608)), b=rnd(g, (128,), 0.2))


def _rows_exact(seed, m, c, nout, **more):
    g = gen(seed)
    d = dict(x=ints(g, (m, c)), w=ints(g, (nout, c), -1, 1), b=ints(g, (nout,)), **more)
    if more.get("inplace") or more.get("with_res"):
        d["res"] = ints(g, (m, nout))
    return d


def _rows_norm():
    g = gen(260)
    x = rnd(g, (33, 40)) + 0.5
    return dict(x=x, norm=K.given_norm(x.t()[None], 8, 1.0 + 0.3 * rnd(g, (40,)), 1.0 + 0.2 * rnd(g, (40,)), 1e-6), w=rnd(g, (40, 40), 1.0 / math.sqrt(40)),
                b=rnd(g, (40,), 0.2))


def _rows_random():
    g = gen(261)
    return dict(x=rnd(g, (33, 512)), w=rnd(g, (1536, 512), 1.0 / math.sqrt(512)), b=rnd(g, (1536,), 0.2))


def _gn(seed, c, groups, m, integer=False, offset=0.0, scale=1.0, eps=1e-6):
    g = gen(seed)
    x = ints(g, (1, c, m)) if integer else (offset + scale * (rnd(g, (1, c, m)) + 0.5 * rnd(g, (1, c, 1)))).float()      # every channel its own mean
    return dict(x0=x, groups=groups, gamma=1.0 + 0.3 * rnd(g, (c,)), beta=0.2 * rnd(g, (c,)), eps=eps, integer=integer)


ATTN_SHAPES = OrderedDict([(f"{c}_{cs}_{n}", (c, cs, n)) for c, cs, n in ((16, 16, 1), (16, 16, 33), (24, 32, 32), (80, 80, 97), (512, 512, 200), (32, 32, 135))])


def _attn_selector(seed, c, cs, n):
    """Up to three beacon keys (one in the first chunk, one in the middle, the last key: in the ragged chunk where there is one),
    each 64 on an axis of its own; query i carries `big` on the axis of beacon i mod 3 and nothing on the other beacons' axes;
    everything else is in {-1, 0, 1}.  The beacon scores 64 big / sqrt(c), any other key at most (big + c) / sqrt(c); `big` is the
    power of two that makes the lead at least 130.  V is integer, so the output is the beacon's V row."""
    g = gen(seed)
    q, k, v = ints(g, (n, c), -1, 1), ints(g, (n, c), -1, 1), ints(g, (n, c))
    big = 32.0
    while (63.0 * big - c) / math.sqrt(c) < 130.0:
        big *= 2.0
    pos = sorted({min(3, n - 1), n // 2, n - 1})
    axes = torch.randperm(c, generator=g)[:len(pos)].tolist()
    q[:, axes] = 0.0
    for b, (p, ax) in enumerate(zip(pos, axes)):
        k[p] = 0.0
        k[p, ax] = 64.0
        q[b::len(pos), ax] = big
    return dict(q=q[None, None], k=k[None, None], v=v[None, None])


def _attn_random(seed, c, cs, n):
    g = gen(seed)
    return dict(q=rnd(g, (1, 1, n, c)), k=rnd(g, (1, 1, n, c)), v=rnd(g, (1, 1, n, c)))


def _attn_spread():
    """Scores within +-3 of each other that rise with the key's index: the running maximum moves in every one of the four chunks
    and no weight vanishes, so what the accumulator and the sum held before counts in the result."""
    g = gen(290)
    n, c = 97, 80
    u = torch.nn.functional.normalize(rnd(g, (1, c)), dim=-1)
    ramp = (torch.arange(n).float() / (n - 1) * 2.0 - 1.0)[:, None]
    q = u * (1.0 + 2.0 * torch.rand((n, 1), generator=g))
    k = u * ramp * math.sqrt(c) + 0.02 * rnd(g, (n, c))
    return dict(q=q[None, None].float(), k=k[None, None].float(), v=rnd(g, (1, 1, n, c)))


def _in(seed, c, m, divisor, integer=True):
    g = gen(seed)
    return dict(z=ints(g, (c, m)) if integer else rnd(g, (c, m)), divisor=divisor)


BUILDERS = OrderedDict()


def _add(name, family, kind, build):
    BUILDERS[name] = (family, kind, build)


# conv, exact
_add("conv_cin72_5x17", "conv", "exact", lambda: _conv_exact(200, 72, 16, 5, 17))                     # the second chunk is 8 wide: the tail loop only
_add("conv_cin100_4x16", "conv", "exact", lambda: _conv_exact(201, 100, 16, 4, 16))                   # the last chunk is 36 wide: two 16-steps and a 4-tail
_add("conv_cin6_1x1", "conv", "exact", lambda: _conv_exact(202, 6, 16, 1, 1))                         # cinp 8 > cin, cs_in 16
_add("conv_cin66_1x17", "conv", "exact", lambda: _conv_exact(215, 66, 16, 1, 17))                     # cinp 68 in cs_in 80: a last chunk of one 4-step
_add("conv_cin76_4x16", "conv", "exact", lambda: _conv_exact(216, 76, 16, 4, 16))                     # a last chunk of three 4-steps
_add("conv_512_512_3x5", "conv", "exact", lambda: _conv_exact(203, 512, 512, 3, 5))                   # eight chunks, four z blocks
_add("conv_cout144_3x5", "conv", "exact", lambda: _conv_exact(204, 16, 144, 3, 5))                    # z = 1 holds one tile
_add("conv_cout176_3x5", "conv", "exact", lambda: _conv_exact(205, 16, 176, 3, 5))                    # z = 1 holds three tiles
_add("conv_37x50", "conv", "exact", lambda: _conv_exact(206, 16, 16, 37, 50))                         # 10 x 4 tiles, ragged both ways
_add("conv_cin20_cout40_6x33", "conv", "exact", lambda: _conv_exact(207, 20, 40, 6, 33))              # three tile columns, the last of one pixel
_add("conv_up_6x34", "conv", "exact", lambda: _conv_exact(208, 16, 16, 3, 17, up=True))               # odd source width
_add("conv_up_2x2", "conv", "exact", lambda: _conv_exact(209, 16, 16, 1, 1, up=True))
_add("conv_res_wide", "conv", "exact", lambda: _conv_exact(210, 16, 24, 5, 7, res_extra=16))          # cs_res = coutp + 16
_add("conv_res_in_place", "conv", "exact", lambda: _conv_exact(211, 20, 40, 5, 7, inplace=True))      # res == out
_add("conv_f32_cout1", "conv", "exact", lambda: _conv_exact(212, 16, 1, 5, 17, out="f32"))
_add("conv_f32_cout3", "conv", "exact", lambda: _conv_exact(213, 16, 3, 5, 17, out="f32"))
_add("conv_f32_cout4", "conv", "exact", lambda: _conv_exact(214, 32, 4, 4, 16, out="f32"))
_add("conv_u8_exact", "conv", "exact", _conv_u8_exact)
_add("conv_u8_ties", "conv", "exact", _conv_u8_ties)
# conv, toleranced
_add("conv_norm_80_9x19", "conv", "tol", _conv_norm)
_add("conv_random_512_128", "conv", "tol", _conv_random)
# rows, exact
_add("rows_m1_16_16", "rows", "exact", lambda: _rows_exact(250, 1, 16, 16))
_add("rows_m31_16_80", "rows", "exact", lambda: _rows_exact(251, 31, 12, 72))                         # c 12 in cs 16, 72 outputs in np 80: a fifth tile
_add("rows_m32_512_16", "rows", "exact", lambda: _rows_exact(252, 32, 512, 16))
_add("rows_m33_48_48", "rows", "exact", lambda: _rows_exact(253, 33, 48, 48))
_add("rows_m1000_512_1536", "rows", "exact", lambda: _rows_exact(254, 1000, 512, 1536))
_add("rows_res", "rows", "exact", lambda: _rows_exact(255, 33, 16, 80, with_res=True))
_add("rows_res_in_place", "rows", "exact", lambda: _rows_exact(256, 33, 40, 40, inplace=True))        # res == out
_add("rows_in_place", "rows", "exact", lambda: _rows_exact(257, 65, 40, 40, out_is_in=True))          # out == in, np = cs_in = 48
# rows, toleranced
_add("rows_norm_48", "rows", "tol", _rows_norm)
_add("rows_random_512_1536", "rows", "tol", _rows_random)
# GroupNorm statistics: toleranced, the integer ones too (the device's double rstd need not be torch's to the last bit)
_add("gn_m1", "group_norm", "tol", lambda: _gn(300, 32, 4, 1, integer=True))
_add("gn_m511", "group_norm", "tol", lambda: _gn(301, 32, 4, 511, integer=True))
_add("gn_m512", "group_norm", "tol", lambda: _gn(302, 32, 4, 512, integer=True))
_add("gn_m513", "group_norm", "tol", lambda: _gn(303, 32, 4, 513, integer=True))
_add("gn_m20000", "group_norm", "tol", lambda: _gn(304, 32, 4, 20000))                               # nblocks cpg = 320: the finish's second trip
_add("gn_cpg512", "group_norm", "tol", lambda: _gn(305, 512, 1, 40, integer=True))                   # the second trip of the finish's last loop
_add("gn_512_m600", "group_norm", "tol", lambda: _gn(312, 512, 32, 600))                             # two pixel lanes, two blocks, the second of 88 pixels
_add("gn_groups_eq_c","group_norm", "tol", lambda: _gn(306, 32, 32, 40, integer=True))              # cpg 1
_add("gn_c24_cs32", "group_norm", "tol", lambda: _gn(307, 24, 8, 100))
_add("gn_c40_cs48", "group_norm", "tol", lambda: _gn(308, 40, 8, 100))                               # 21 pixel lanes, four idle threads
_add("gn_c80", "group_norm", "tol", lambda: _gn(309, 80, 8, 100))                                    # 12 pixel lanes, sixteen idle threads
_add("gn_mean_1000", "group_norm", "tol", lambda: _gn(310, 32, 4, 40, offset=1000.0))
_add("gn_small_variance", "group_norm", "tol", lambda: _gn(311, 32, 4, 40, scale=0.001))             # variance of the order of eps = 1e-6
# attention
for _i, (_name, _shape) in enumerate(ATTN_SHAPES.items()):
    _add("attn_selector_" + _name, "attention", "exact", lambda i=_i, s=_shape: _attn_selector(270 + i, *s))
    _add("attn_random_" + _name, "attention", "tol" if _shape[2] > 1 else "exact", lambda i=_i, s=_shape: _attn_random(280 + i, *s))      # one key: the output is its V row
_add("attn_spread_80_97", "attention", "tol", _attn_spread)
# in
_add("in_c1_m1", "in", "exact", lambda: _in(320, 1, 1, 1.0))
_add("in_c4_m15", "in", "exact", lambda: _in(321, 4, 15, 0.5))
_add("in_c16_m1000", "in", "exact", lambda: _in(322, 16, 1000, 1.0))
_add("in_c4_m1000_scaled", "in", "tol", lambda: _in(323, 4, 1000, 0.08333, integer=False))

NAMES = tuple(BUILDERS)
SELECTORS = tuple(n for n in NAMES if n.startswith("attn_selector_"))
EXACT_SUMS = tuple(n for n in NAMES if BUILDERS[n][1] == "exact" and BUILDERS[n][0] != "attention" and n != "conv_u8_ties")
STATISTICS = tuple(n for n in NAMES if BUILDERS[n][0] == "group_norm")

# which case must expose which fault of tests/vae_kernel_ref.py (tests/test_vae_kernels_host.py)
FAULT_CASE = {"k_tail_dropped": "conv_cin72_5x17", "chunk_weight_offset_ignores_c0": "conv_cin100_4x16", "weight_rows_by_cs_not_cinp": "conv_cin6_1x1",
              "z_block_channel_offset_dropped": "conv_512_512_3x5", "absent_tile_stored": "conv_cout144_3x5", "edge_store_unguarded": "conv_cin72_5x17",
              "padding_normalised": "conv_norm_80_9x19", "nearest2_source_width_not_halved": "conv_up_6x34", "res_stride_is_coutp": "conv_res_wide",
              "f32_plane_stride": "conv_f32_cout3", "u8_round_half_up": "conv_u8_ties", "u8_no_clamp": "conv_u8_exact",
              "last_block_not_clamped": "gn_m513", "finish_first_trip_only": "gn_m20000", "cpg_over_256_unwritten": "gn_cpg512",
              "idle_pixel_lane_counted": "gn_c40_cs48", "variance_unbiased": "gn_m1", "raw_moments_f32": "gn_mean_1000", "padded_channels_not_zero": "gn_c24_cs32",
              "ragged_rows_written": "rows_m33_48_48", "norm_with_silu": "rows_norm_48", "res_dropped": "rows_res", "tiles_past_the_fourth_dropped": "rows_m31_16_80",
              "scale_by_cs_not_c": "attn_random_24_32_32", "ragged_keys_score_zero": "attn_random_16_16_33", "no_rescale_on_new_max": "attn_selector_512_512_200",
              "sum_not_rescaled": "attn_spread_80_97", "tiles_past_the_first_round_dropped": "attn_selector_80_80_97",
              "multiplied_not_divided": "in_c4_m15", "plane_stride": "in_c4_m15", "columns_past_c_not_zero": "in_c1_m1"}

_cases, _refs = {}, {}


def by_name(name):
    if name not in _cases:
        family, kind, build = BUILDERS[name]
        dense = build()
        _cases[name] = Case(name, family, kind, dense, PACK[family](dense))
    return _cases[name]


def references(name):
    """(float64 reference, float32 restatement or None for an exact case), computed once and shared."""
    if name not in _refs:
        case = by_name(name)
        _refs[name] = (reference(case), reference(case, torch.float32) if case.kind == "tol" else None)
    return _refs[name]
