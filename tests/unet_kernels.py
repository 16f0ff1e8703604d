"""The per-launch cases of csrc/unet.hip: one launch (or one short chain) of a kernel on a frame of a few pixels, through the
nesr_unet_k_* test hooks.  This module holds

  * the packing, written from csrc/unet_api.h's comments and not by calling nesr_unet_finalize: dense torch tensors -> rows
    [n m][cs] with cs the width rounded up to 16 and zeros past the width, weights Wt[K][N], conv weights [9 (cinp0 + cinp1)][coutp]
    with each source's K rounded up to 4, VaeNorm [n][cs], float4 statistics; and back (`unpack`), which also says whether
    every padded column holds what the header documents (zeros, or the sentinel where nothing may be written);
  * the cases (`CASES`): dense inputs, and the packed arguments made from them.  Exact cases carry small integers (activations
    in [-3, 3], weights in {-1, 0, 1}): every partial sum is an integer below 2^24 in any order, so the GPU must give the
    float64 reference bit for bit.  Toleranced cases carry random floats; their tolerance is 8 x max |float32 restatement -
    float64| per compared quantity, computed where it is used and never written down;
  * `launch`: the GPU run of a case's arguments, every output embedded in sentinels whose guards are asserted.

tests/unet_kernel_ref.py holds the references and the float64 emulations; FAULT_CASE says which case must expose which fault.
"""
from __future__ import annotations

import math
from collections import OrderedDict, namedtuple

import torch

from tests import unet_kernel_ref as R
from tests.unet_kernel_ref import SENT, up4, up16

Case = namedtuple("Case", "name family kind dense args")
GUARD = 4096
TEMB_LD = 1024                        # csrc/unet_api.h: UNET_MAX_WIDTH, the row stride of the time-embedding table
SELECTOR_LEAD = 120.0                 # exp(-120) is 0 in float32: the softmax of a selector case is exactly one-hot


# ------------------------------------------------------------------------------------------------ packing
def pad_cols(r, cs):
    out = torch.zeros((r.shape[0], cs), dtype=torch.float32)
    out[:, :r.shape[1]] = r
    return out


def to_rows(x):
    """[n, c, ...] -> rows [n m][cs], zero past c."""
    n, c = x.shape[:2]
    return pad_cols(x.reshape(n, c, -1).permute(0, 2, 1).reshape(-1, c).float(), up16(c)).reshape(-1)


def from_rows(flat, n, c, *grid):
    """rows [n m][cs] -> ([n, c, *grid], the columns past c)."""
    r = flat.reshape(n, -1, up16(c))
    return r[..., :c].permute(0, 2, 1).reshape(n, c, *grid), r[..., c:]


def pack_norm(nm, cs):
    """(mean [n, c] float64, a [n, c], beta [c]) -> VaeNorm [n][cs]: (mean hi, mean lo, a, beta), zero past c."""
    mean, a, beta = nm
    n, c = mean.shape
    out = torch.zeros((n, cs, 4), dtype=torch.float32)
    hi = mean.double().float()
    out[:, :c, 0], out[:, :c, 1], out[:, :c, 2], out[:, :c, 3] = hi, (mean.double() - hi.double()).float(), a.float(), beta.float()[None]
    return out.reshape(-1)


def given_norm(x, groups, gamma, beta, eps):
    """A GroupNorm's result as a launch takes it: the float64 moments of x [n, c, ...], the mean kept in float64 (the hi + lo
    pair carries it), a and beta rounded to the float32 the buffer holds."""
    mean, a, _ = R.group_norm(dict(x0=x.reshape(x.shape[0], x.shape[1], -1), groups=groups, gamma=gamma, beta=beta, eps=eps))
    hi = mean.float()
    return (hi.double() + (mean - hi.double()).float().double(), a.float(), beta.float())


def pack_wt(w, rows, cols, row_at=0):
    """torch's [out, in] -> Wt [rows][cols] with the in channels from row `row_at`, zero elsewhere."""
    out = torch.zeros((rows, cols), dtype=torch.float32)
    out[row_at:row_at + w.shape[1], :w.shape[0]] = w.t().float()
    return out


def sentinels(count):
    return torch.full((count,), SENT, dtype=torch.float32)


def pack_conv(d):
    x0, x1, w = d["x0"], d.get("x1"), d["w"]
    n, c0 = x0.shape[:2]
    c1 = x1.shape[1] if x1 is not None else 0
    cout, stride, up = w.shape[0], d.get("stride", 1), int(bool(d.get("up")))
    H, W = (x0.shape[2] * 2, x0.shape[3] * 2) if up else (x0.shape[2] // stride, x0.shape[3] // stride)
    coutp, cinp0, cinp1 = up16(cout), up4(c0), up4(c1)
    wp = torch.zeros((9, cinp0 + cinp1, coutp), dtype=torch.float32)
    taps = w.float().permute(2, 3, 1, 0).reshape(9, c0 + c1, cout)      # [ky kx][cin][cout]
    wp[:, :c0, :cout] = taps[:, :c0]
    wp[:, cinp0:cinp0 + c1, :cout] = taps[:, c0:]
    a = dict(n=n, H=H, W=W, stride=stride, up=up, in0=to_rows(x0), c0=c0, cs0=up16(c0), norm0=None, in1=None, c1=0, cs1=0, norm1=None,
             w=wp.reshape(-1, coutp), bias=pad_cols(d["b"].float()[None], coutp).reshape(-1), cout=cout, coutp=coutp, res=None,
             out_nchw=int(bool(d.get("out_nchw"))))
    if d.get("norm0") is not None:
        a["norm0"] = pack_norm(d["norm0"], a["cs0"])
    if x1 is not None:
        a.update(in1=to_rows(x1), c1=c1, cs1=up16(c1), norm1=pack_norm(d["norm1"], up16(c1)) if d.get("norm1") is not None else None)
    a["out"] = sentinels(n * cout * H * W if a["out_nchw"] else n * H * W * coutp)
    if d.get("res") is not None:
        a["res"] = to_rows(d["res"])
        if d.get("inplace"):
            a["out"] = a["res"]
    return a


def pack_rows(d):
    x0, x1, w = d["x0"], d.get("x1"), d["w"]
    n, rps, c0 = x0.shape
    c1 = x1.shape[2] if x1 is not None else 0
    cs0, cs1, geglu = up16(c0), up16(c1) if c1 else 0, int(bool(d.get("geglu")))
    nout = w.shape[0] // 2 if geglu else w.shape[0]
    np_ = up16(nout)
    ldw = 2 * np_ if geglu else np_
    wt, b = torch.zeros((cs0 + cs1, ldw), dtype=torch.float32), torch.zeros(ldw, dtype=torch.float32)
    for half in range(2 if geglu else 1):      # GEGLU: the value half at column 0, the gate half at column np
        wh, bh = w[half * nout:(half + 1) * nout].float(), d["b"][half * nout:(half + 1) * nout].float()
        wt[:c0, half * np_:half * np_ + nout] = wh[:, :c0].t()
        wt[cs0:cs0 + c1, half * np_:half * np_ + nout] = wh[:, c0:].t()
        b[half * np_:half * np_ + nout] = bh
    rows_ = lambda x: to_rows(x.transpose(1, 2))
    a = dict(m=n * rps, rows_per_sample=rps, in0=rows_(x0), c0=c0, cs0=cs0, norm0=None, in1=None, c1=0, cs1=0, norm1=None,
             prologue={None: 0, "groupnorm": 1, "layernorm": 2}[d.get("prologue")], ln=None, ln_g=None, ln_b=None, w=wt.reshape(-1), b=b, ldw=ldw,
             np=np_, nout=nout, n=n, geglu=geglu, res=None, out=sentinels(n * rps * np_))
    if x1 is not None:
        a.update(in1=rows_(x1), c1=c1, cs1=cs1)
    if a["prologue"] == 1:
        a["norm0"] = pack_norm(d["norm0"], cs0)
        if x1 is not None:
            a["norm1"] = pack_norm(d["norm1"], cs1)
    if a["prologue"] == 2:
        mean, rstd = (t.reshape(-1).double() for t in d["ln"])
        hi = mean.float()
        a["ln"] = torch.stack([hi, (mean - hi.double()).float(), rstd.float(), torch.zeros_like(hi)], -1).reshape(-1)
        a["ln_g"], a["ln_b"] = pad_cols(d["ln_g"].float()[None], cs0).reshape(-1), pad_cols(d["ln_b"].float()[None], cs0).reshape(-1)
    if d.get("res") is not None:
        a["res"] = to_rows(d["res"].transpose(1, 2))
        if d.get("inplace"):
            a["out"] = a["res"]
    return a


def given_ln(x, eps=1e-5):
    """LayerNorm statistics as a launch takes them: float64 moments, the mean as its hi + lo pair carries it, rstd in float32."""
    mean, rstd = R.layer_norm_stats(dict(x=x, eps=eps))
    hi = mean.float()
    return (hi.double() + (mean - hi.double()).float().double(), rstd.float())


def pack_group_norm(d):
    x0, x1 = d["x0"], d.get("x1")
    n, c0, m = x0.shape
    a = dict(n=n, m=m, in0=to_rows(x0), c0=c0, cs0=up16(c0), in1=None, c1=0, cs1=0, norm1=None, groups=d["groups"], gamma=d["gamma"].float(),
             beta=d["beta"].float(), eps=float(d["eps"]), norm0=sentinels(n * up16(c0) * 4))
    if x1 is not None:
        c1 = x1.shape[1]
        a.update(in1=to_rows(x1), c1=c1, cs1=up16(c1), norm1=sentinels(n * up16(c1) * 4))
    return a


def pack_layer_norm_stats(d):
    m, c = d["x"].shape
    cs = up16(c)
    return dict(m=m, c=c, cs=cs, eps=float(d["eps"]), out=sentinels(4 * m), **{"in": pad_cols(d["x"].float(), cs).reshape(-1)})


def pack_attention(d):
    q, k, v = d["q"], d["k"], d["v"]
    s_, heads, nq, hd = q.shape
    nk, dim = k.shape[2], heads * hd
    dimp = up16(dim)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(s_ * t.shape[2], dim).float()
    a = dict(samples=s_, nq=nq, nk=nk, heads=heads, d=hd, ldo=dimp, out=sentinels(s_ * nq * dimp))
    if d["layout"] == "fused":      # a self-attention's q | k | v product: one buffer, ldq = ldkv = 3 dimp
        buf = torch.zeros((s_ * nq, 3 * dimp), dtype=torch.float32)
        buf[:, :dim], buf[:, dimp:dimp + dim], buf[:, 2 * dimp:2 * dimp + dim] = flat(q), flat(k), flat(v)
        a.update(qbuf=buf.reshape(-1), q_off=0, ldq=3 * dimp, k_off=dimp, v_off=2 * dimp, ldkv=3 * dimp)
        a["kvbuf"] = a["qbuf"]
    else:                           # the text states' k | v product: ldkv = 2 dimp
        kv = torch.zeros((s_ * nk, 2 * dimp), dtype=torch.float32)
        kv[:, :dim], kv[:, dimp:dimp + dim] = flat(k), flat(v)
        a.update(qbuf=pad_cols(flat(q), dimp).reshape(-1), q_off=0, ldq=dimp, kvbuf=kv.reshape(-1), k_off=0, v_off=dimp, ldkv=2 * dimp)
    return a


def pack_embedding(d):
    td, c0 = d["w1"].shape
    tdp = up16(td)
    vec = lambda t: pad_cols(t.float()[None], tdp).reshape(-1)
    return dict(t=float(d["t"]), c0=c0, td=td, tdp=tdp, w1=pack_wt(d["w1"], c0, tdp).reshape(-1), b1=vec(d["b1"]), w2=pack_wt(d["w2"], td, tdp).reshape(-1),
                b2=vec(d["b2"]), table=pad_cols(d["table"].float(), tdp).reshape(-1), label=int(d["label"]), out=sentinels(tdp))


def pack_temb(d):
    td = d["semb"].shape[0]
    parts, w_off, b_off, cb_off, coutp, at = [], [], [], [], [], 0
    for w, b, cb in d["resnets"]:
        cp = up16(w.shape[0])
        for t, offs in ((pack_wt(w, td, cp).reshape(-1), w_off), (pad_cols(b.float()[None], cp).reshape(-1), b_off), (pad_cols(cb.float()[None], cp).reshape(-1), cb_off)):
            parts.append(t)
            offs.append(at)
            at += t.numel()
        coutp.append(cp)
    return dict(count=len(coutp), td=td, semb=d["semb"].float(), weights=torch.cat(parts), w_off=w_off, b_off=b_off, cb_off=cb_off, coutp=coutp,
                cout=[w.shape[0] for w, _, _ in d["resnets"]], out=sentinels(len(coutp) * TEMB_LD))


def pack_in(d):
    src = d["src"]
    if d["nchw"]:
        n, c, m = src.shape
        return dict(src=src.float().reshape(-1), nchw=1, c=c, cs=up16(c), m=m, rows=n * m, out=sentinels(n * m * up16(c)))
    rows_, c = src.shape
    return dict(src=src.float().reshape(-1), nchw=0, c=c, cs=up16(c), m=1, rows=rows_, out=sentinels(rows_ * up16(c)))


PACK = {"conv": pack_conv, "rows": pack_rows, "group_norm": pack_group_norm, "layer_norm_stats": pack_layer_norm_stats, "attention": pack_attention,
        "embedding": pack_embedding, "temb": pack_temb, "in": pack_in}
REF = {"conv": R.conv, "rows": R.rows, "group_norm": R.group_norm, "layer_norm_stats": R.layer_norm_stats, "attention": R.attention,
       "embedding": R.embedding, "temb": R.temb, "in": lambda d, dtype=torch.float64: R.rows_in(d).to(dtype)}
OUTPUTS = {"group_norm": ("norm0", "norm1")}      # the output buffers of a family's arguments; ("out",) otherwise


def unpack(family, a, outs):
    """The dense result of the output buffers, as a tuple of the quantities that are compared, and whether every padded column
    holds what csrc/unet_api.h documents."""
    zero = lambda t: bool((t == 0).all())
    if family == "conv":
        if a["out_nchw"]:
            return (outs["out"].reshape(a["n"], a["cout"], a["H"], a["W"]),), True
        y, pad = from_rows(outs["out"], a["n"], a["cout"], a["H"], a["W"])
        return (y,), zero(pad)
    if family == "rows":
        r = outs["out"].reshape(a["n"], a["rows_per_sample"], a["np"])
        return (r[..., :a["nout"]],), zero(r[..., a["nout"]:])
    if family == "group_norm":
        parts, ok = [], True
        for i in (0, 1):
            if a[f"in{i}"] is None:
                break
            o = outs[f"norm{i}"].reshape(a["n"], a[f"cs{i}"], 4)
            parts.append(o[:, :a[f"c{i}"]])
            ok = ok and zero(o[:, a[f"c{i}"]:])
        o = torch.cat(parts, 1).double()
        return (o[..., 0] + o[..., 1], o[..., 2], o[..., 3]), ok
    if family == "layer_norm_stats":
        o = outs["out"].reshape(a["m"], 4).double()
        return (o[:, 0] + o[:, 1], o[:, 2]), zero(o[:, 3])
    if family == "attention":
        o = outs["out"].reshape(a["samples"], a["nq"], a["ldo"])
        return (o[..., :a["heads"] * a["d"]],), zero(o[..., a["heads"] * a["d"]:])
    if family == "embedding":
        return (outs["out"][:a["td"]],), zero(outs["out"][a["td"]:])
    if family == "temb":
        o = outs["out"].reshape(a["count"], TEMB_LD)
        ok = all(zero(o[r, a["cout"][r]:a["coutp"][r]]) and bool((o[r, a["coutp"][r]:] == SENT).all()) for r in range(a["count"]))
        return tuple(o[r, :a["cout"][r]] for r in range(a["count"])), ok      # each row is written to its coutp and not past it
    if family == "in":
        r = outs["out"].reshape(a["rows"], a["cs"])
        return (r[:, :a["c"]],), zero(r[:, a["c"]:])
    raise KeyError(family)


def as_tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def reference(case, dtype=torch.float64):
    with torch.no_grad():
        return as_tuple(REF[case.family](case.dense, dtype))


def is_exact(got, ref64):
    """Bit for bit: the float64 reference cast to the kernel's float32 equals the result."""
    return all(g.shape == r.shape and torch.equal(g.float(), r.float()) for g, r in zip(got, ref64))


def ratios(got, ref64, ref32):
    """err / tol per compared quantity, tol = 8 x max |float32 restatement - float64|; a quantity both restatements and the
    result agree on exactly counts 0."""
    out = []
    for g, r64, r32 in zip(got, ref64, ref32):
        err, tol = float((g.double() - r64).abs().max()), 8.0 * float((r32.double() - r64).abs().max())
        out.append(0.0 if err == 0.0 else (math.inf if tol == 0.0 or not math.isfinite(err) else err / tol))
    return out


def exact_bound(case):
    """max over the outputs of sum_k |x_k| |w_k| (+ |bias|, + |residual|): below 2^24 every partial sum is an exact float32."""
    d = {k: (v.abs() if torch.is_tensor(v) else v) for k, v in case.dense.items()}
    if case.family == "temb":
        d["resnets"] = [tuple(t.abs() for t in r) for r in case.dense["resnets"]]
    if case.family == "in":
        return float(case.dense["src"].abs().max())
    with torch.no_grad():
        return max(float(t.max()) for t in as_tuple(REF[case.family](d, torch.float64)))


def mean_bound(case):
    """What the mean of a statistics launch is held to besides its tolerance, which the float32 restatement makes too wide to see
    a dropped mean_lo: the kernels sum in double, at most 2^13 terms a mean here, so the sum is off by at most 2^13 2^-53 max |x|,
    and the (hi, lo) pair carries the mean to 2^-48 of itself.  2^-38 max |x| leaves a factor of four; mean_hi alone is off by
    up to 2^-25 |mean|."""
    d = case.dense
    xs = [d["x"]] if case.family == "layer_norm_stats" else [d["x0"]] + ([d["x1"]] if d.get("x1") is not None else [])
    terms = d["x"].shape[1] if case.family == "layer_norm_stats" else d["x0"].shape[2] * sum(x.shape[1] for x in xs) // d["groups"]
    assert terms <= 2 ** 13
    return 2.0 ** -38 * max(float(x.abs().max()) for x in xs)


def selector_lead(case):
    """The smallest lead, over every query of every head and sample, of the best key's scaled score over the runner-up's
    (float64); inf where there is one key."""
    q, k = case.dense["q"].double(), case.dense["k"].double()
    if k.shape[2] == 1:
        return math.inf
    top = ((q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])).topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


# ------------------------------------------------------------------------------------------------ the GPU run
def launch(family, a, expect_rc=0):
    """One nesr_unet_k_* call on the packed arguments: {name: output buffer on the host}.  Every output lies between guards of
    sentinels, which are asserted; a tensor that is both an input and the output (res == out) is one device buffer."""
    import ctypes

    from neural_enhanced_super_resolution_amd import _lib
    lib, dev = _lib.load(), "cuda:0"
    held, bufs = {}, {}
    for name in OUTPUTS.get(family, ("out",)):
        if a.get(name) is None:
            continue
        t = a[name]
        buf = torch.full((GUARD + t.numel() + GUARD,), SENT, dtype=torch.float32)
        buf[GUARD:GUARD + t.numel()] = t
        bufs[name] = buf.to(dev)
        held[id(t)] = bufs[name][GUARD:GUARD + t.numel()]

    def ptr(t, off=0):
        if t is None:
            return None
        if id(t) not in held:
            held[id(t)] = t.contiguous().to(dev)
        return ctypes.c_void_p(held[id(t)].data_ptr() + 4 * off)

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if family == "conv":
        rc = lib.nesr_unet_k_conv(a["n"], a["H"], a["W"], a["stride"], a["up"], ptr(a["in0"]), a["c0"], a["cs0"], ptr(a["norm0"]), ptr(a["in1"]), a["c1"],
                                  a["cs1"], ptr(a["norm1"]), ptr(a["w"]), ptr(a["bias"]), a["cout"], a["coutp"], ptr(a["res"]), a["out_nchw"], ptr(a["out"]), stream)
    elif family == "rows":
        rc = lib.nesr_unet_k_rows(a["m"], a["rows_per_sample"], ptr(a["in0"]), a["c0"], a["cs0"], ptr(a["norm0"]), ptr(a["in1"]), a["c1"], a["cs1"],
                                  ptr(a["norm1"]), a["prologue"], ptr(a["ln"]), ptr(a["ln_g"]), ptr(a["ln_b"]), ptr(a["w"]), ptr(a["b"]), a["ldw"], a["np"],
                                  a["geglu"], ptr(a["res"]), ptr(a["out"]), stream)
    elif family == "group_norm":
        blocks = (a["m"] + R.GN_PIXELS - 1) // R.GN_PIXELS
        part = [torch.zeros(a["n"] * blocks * a[f"cs{i}"] * 2, dtype=torch.float64, device=dev) if a[f"in{i}"] is not None else None for i in (0, 1)]
        pp = [ctypes.c_void_p(p.data_ptr()) if p is not None else None for p in part]
        rc = lib.nesr_unet_k_group_norm(a["n"], a["m"], ptr(a["in0"]), a["c0"], a["cs0"], ptr(a["norm0"]), pp[0], ptr(a["in1"]), a["c1"], a["cs1"],
                                        ptr(a["norm1"]), pp[1], a["groups"], ptr(a["gamma"]), ptr(a["beta"]), a["eps"], stream)
    elif family == "layer_norm_stats":
        rc = lib.nesr_unet_k_layer_norm_stats(ptr(a["in"]), a["m"], a["c"], a["cs"], a["eps"], ptr(a["out"]), stream)
    elif family == "attention":
        rc = lib.nesr_unet_k_attention(a["samples"], a["nq"], a["nk"], a["heads"], a["d"], ptr(a["qbuf"], a["q_off"]), ptr(a["kvbuf"], a["k_off"]),
                                       ptr(a["kvbuf"], a["v_off"]), a["ldq"], a["ldkv"], a["ldo"], ptr(a["out"]), stream)
    elif family == "embedding":
        rc = lib.nesr_unet_k_embedding(a["t"], a["c0"], a["td"], a["tdp"], ptr(a["w1"]), ptr(a["b1"]), ptr(a["w2"]), ptr(a["b2"]),
                                       ptr(a["table"], a["label"] * a["tdp"]), ptr(a["out"]), stream)
    elif family == "temb":
        u64, i32 = ctypes.c_ulonglong * a["count"], ctypes.c_int * a["count"]
        rc = lib.nesr_unet_k_temb(a["count"], a["td"], ptr(a["semb"]), ptr(a["weights"]), u64(*a["w_off"]), u64(*a["b_off"]), u64(*a["cb_off"]),
                                  i32(*a["coutp"]), ptr(a["out"]), stream)
    elif family == "in":
        rc = lib.nesr_unet_k_in(ptr(a["src"]), a["nchw"], a["c"], a["cs"], a["m"], a["rows"], ptr(a["out"]), stream)
    else:
        raise KeyError(family)
    torch.cuda.synchronize()
    assert rc == expect_rc, f"nesr_unet_k_* ({family}) returned {rc}: {(lib.nesr_last_error() or b'').decode()}"
    outs = {}
    for name, buf in bufs.items():
        host = buf.cpu()
        count = a[name].numel()
        assert bool((host[:GUARD] == SENT).all()) and bool((host[GUARD + count:] == SENT).all()), f"{family}: the launch wrote outside `{name}`"
        outs[name] = host[GUARD:GUARD + count]
    return outs


# ------------------------------------------------------------------------------------------------ the cases
def gen(seed):
    return torch.Generator().manual_seed(9000 + seed)


def ints(g, shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def rnd(g, shape, scale=1.0):
    return (scale * torch.randn(shape, generator=g)).float()


def _conv_exact(seed, n, c0, c1, cout, h, w, **more):
    """h x w: the SOURCE grid.  Integer activations, weights in {-1, 0, 1}, integer bias."""
    g = gen(seed)
    d = dict(x0=ints(g, (n, c0, h, w)), x1=ints(g, (n, c1, h, w)) if c1 else None, w=ints(g, (cout, c0 + c1, 3, 3), -1, 1), b=ints(g, (cout,)), **more)
    if more.get("inplace") or more.get("with_res"):
        s = more.get("stride", 1)
        d["res"] = ints(g, (n, cout, h * 2 // s if more.get("up") else h // s, w * 2 // s if more.get("up") else w // s))
    return d


def _rows_exact(seed, n, rps, c0, c1, nout, **more):
    g = gen(seed)
    d = dict(x0=ints(g, (n, rps, c0)), x1=ints(g, (n, rps, c1)) if c1 else None, w=ints(g, (nout, c0 + c1), -1, 1), b=ints(g, (nout,)), **more)
    if more.get("inplace"):
        d["res"] = ints(g, (n, rps, nout))
    return d


def _conv_gn_loader():
    """GroupNorm + SiLU in the loader on a 5 x 17 frame, two sources: beta is large, so a tap outside the image that went through
    the norm would add silu(beta - mean a), not 0."""
    g = gen(40)
    x0, x1 = rnd(g, (2, 24, 5, 17)) + 0.5, rnd(g, (2, 8, 5, 17))
    gamma, beta = 1.0 + 0.3 * rnd(g, (32,)), 2.0 + 0.2 * rnd(g, (32,))
    nm = given_norm(torch.cat([x0, x1], 1), 8, gamma, beta, 1e-5)
    return dict(x0=x0, x1=x1, norm0=(nm[0][:, :24], nm[1][:, :24], nm[2][:24]), norm1=(nm[0][:, 24:], nm[1][:, 24:], nm[2][24:]),
                w=rnd(g, (20, 32, 3, 3), 1.0 / math.sqrt(288)), b=rnd(g, (20,), 0.2))


def _rows_tol(seed, n, rps, c, nout, prologue=None, geglu=False):
    g = gen(seed)
    x = rnd(g, (n, rps, c)) + (0.5 * torch.arange(n).float()[:, None, None] if prologue == "groupnorm" else 0.0)      # the samples' moments differ
    d = dict(x0=x, w=rnd(g, ((2 if geglu else 1) * nout, c), 1.0 / math.sqrt(c)), b=rnd(g, ((2 if geglu else 1) * nout,), 0.2), prologue=prologue, geglu=geglu)
    if prologue == "groupnorm":
        d["norm0"] = given_norm(x.transpose(1, 2), 4, 1.0 + 0.3 * rnd(g, (c,)), 0.2 * rnd(g, (c,)), 1e-6)
    if prologue == "layernorm":
        d.update(ln=tuple(t.reshape(n, rps) for t in given_ln(x.reshape(n * rps, c))), ln_g=1.0 + 0.3 * rnd(g, (c,)), ln_b=0.2 * rnd(g, (c,)))
    return d


def _gn(seed, n, c0, c1, groups, m, offset=0.0, scale=1.0, eps=1e-5):
    g = gen(seed)
    mk = lambda c: (offset + scale * (rnd(g, (n, c, m)) + 0.5 * rnd(g, (1, c, 1)))).float()      # every channel its own mean
    return dict(x0=mk(c0), x1=mk(c1) if c1 else None, groups=groups, gamma=1.0 + 0.3 * rnd(g, (c0 + c1,)), beta=0.2 * rnd(g, (c0 + c1,)), eps=eps)


def _ln(seed, m, c, offset=0.0, scale=1.0):
    return dict(x=(offset + scale * rnd(gen(seed), (m, c))).float(), eps=1e-5)


ATTN_SHAPES = OrderedDict([      # name: (head width, heads, nq, nk, samples, layout)
    ("d8_h3_fused", (8, 3, 33, 33, 2, "fused")),          # heads d = 24 in ldo 32
    ("d24_h1_text", (24, 1, 31, 256, 1, "text")),         # heads d = 24 in ldo 32; eight key chunks
    ("d72_h5_text", (72, 5, 1, 32, 2, "text")),
    ("d128_h3_one_key", (128, 3, 33, 1, 1, "text")),
    ("d128_h1_fused", (128, 1, 33, 33, 2, "fused")),
    ("d24_h5_text", (24, 5, 31, 33, 2, "text")),
    ("d8_h1_one_query", (8, 1, 1, 33, 1, "text")),
])


def _attn_selector(seed, hd, heads, nq, nk, samples, layout):
    """Per head and sample up to three beacon keys (one in the first chunk, one in a middle chunk, the last key: in the ragged chunk
    where there is one), each 64 on an axis of its own; query i carries 32 on the axis of beacon (i + head + sample) mod 3 and
    nothing on the other beacons' axes; everything else is in {-1, 0, 1}.  The beacon scores 2048 / sqrt(d), any other key at
    most (32 + d) / sqrt(d): a lead of at least 166.  V is integer, so the output is the beacon's V row."""
    g = gen(seed)
    q, k, v = ints(g, (samples, heads, nq, hd), -1, 1), ints(g, (samples, heads, nk, hd), -1, 1), ints(g, (samples, heads, nk, hd))
    pos = sorted({min(3, nk - 1), nk // 2, nk - 1})
    for s in range(samples):
        for h in range(heads):
            axes = torch.randperm(hd, generator=g)[:len(pos)].tolist()
            q[s, h][:, axes] = 0.0
            for b, (p, ax) in enumerate(zip(pos, axes)):
                k[s, h, p] = 0.0
                k[s, h, p, ax] = 64.0
                mine = [i for i in range(nq) if (i + h + s) % len(pos) == b]
                if mine:
                    q[s, h, mine, ax] = 32.0
    return dict(q=q, k=k, v=v, layout=layout)


def _attn_random(seed, hd, heads, nq, nk, samples, layout):
    g = gen(seed)
    return dict(q=rnd(g, (samples, heads, nq, hd)), k=rnd(g, (samples, heads, nk, hd)), v=rnd(g, (samples, heads, nk, hd)), layout=layout)


def _attn_spread():
    """Scores spread over +-200 that rise with the key's index: the running maximum moves in every one of the eight chunks, and
    what the accumulator held before is worth exp(-50) a chunk."""
    g = gen(70)
    samples, heads, nq, nk, hd = 1, 2, 33, 256, 24
    u = torch.nn.functional.normalize(rnd(g, (samples, heads, 1, hd)), dim=-1)
    ramp = (torch.arange(nk).float() / (nk - 1) * 2.0 - 1.0)[None, None, :, None]
    q = u * (0.5 + 0.5 * torch.rand((samples, heads, nq, 1), generator=g)) * 20.0
    k = u * ramp * 10.0 * math.sqrt(hd) + 0.05 * rnd(g, (samples, heads, nk, hd))
    return dict(q=q.float(), k=k.float(), v=rnd(g, (samples, heads, nk, hd)), layout="text")


def _emb(seed, c0, t):
    g = gen(seed)
    td = 4 * c0
    return dict(t=t, label=2, w1=rnd(g, (td, c0), 1.0 / math.sqrt(c0)), b1=rnd(g, (td,), 0.2), w2=rnd(g, (td, td), 1.0 / math.sqrt(td)), b2=rnd(g, (td,), 0.2),
                table=rnd(g, (4, td), 0.5))


def _temb_exact():
    g = gen(80)
    couts = [8, 16, 24, 48, 250, 272, 1000, 1024, 32, 512]
    return dict(semb=ints(g, (64,)), resnets=[(ints(g, (couts[r % len(couts)], 64), -1, 1), ints(g, (couts[r % len(couts)],)), ints(g, (couts[r % len(couts)],)))
                                              for r in range(30)])


BUILDERS = OrderedDict()


def _add(name, family, kind, build):
    BUILDERS[name] = (family, kind, build)


# conv, exact
_add("conv_cat_1024_1024", "conv", "exact", lambda: _conv_exact(1, 2, 1024, 1024, 32, 2, 3))
_add("conv_1024_out", "conv", "exact", lambda: _conv_exact(2, 2, 16, 0, 1024, 3, 5))                  # eight channel blocks: the blockIdx.z split
_add("conv_144_out", "conv", "exact", lambda: _conv_exact(3, 2, 16, 0, 144, 3, 5))                    # the second block has one tile
_add("conv_cat_6_10", "conv", "exact", lambda: _conv_exact(4, 1, 6, 10, 16, 4, 5))                    # K rounded to 4 a source: the weight row offset is 8
_add("conv_cat_80_48", "conv", "exact", lambda: _conv_exact(5, 1, 80, 48, 16, 4, 5))                  # K chunks 64 + 16, then 48
_add("conv_up_6x20", "conv", "exact", lambda: _conv_exact(6, 2, 16, 0, 16, 3, 10, up=True))
_add("conv_stride2_1024", "conv", "exact", lambda: _conv_exact(7, 1, 1024, 0, 16, 10, 34, stride=2))  # 32 K chunks of 32; 5 x 17: a ragged tile row, two tile columns
_add("conv_stride2_48", "conv", "exact", lambda: _conv_exact(8, 1, 48, 0, 16, 6, 8, stride=2))        # chunks 32 + 16
_add("conv_1x1", "conv", "exact", lambda: _conv_exact(9, 1, 16, 0, 16, 1, 1))
_add("conv_1x17", "conv", "exact", lambda: _conv_exact(10, 1, 16, 0, 16, 1, 17))
_add("conv_res_in_place", "conv", "exact", lambda: _conv_exact(11, 2, 20, 0, 24, 5, 7, inplace=True))
_add("conv_res", "conv", "exact", lambda: _conv_exact(12, 1, 16, 0, 40, 5, 7, with_res=True))
_add("conv_out_nchw", "conv", "exact", lambda: _conv_exact(13, 2, 32, 0, 4, 5, 7, out_nchw=True))
# conv, toleranced
_add("conv_gn_loader_5x17", "conv", "tol", _conv_gn_loader)
# rows, exact
_add("rows_k4096", "rows", "exact", lambda: _rows_exact(20, 1, 33, 4096, 0, 1024))
_add("rows_272_out", "rows", "exact", lambda: _rows_exact(21, 1, 5, 32, 0, 272))                      # the second column block has one tile
_add("rows_cat_80_48", "rows", "exact", lambda: _rows_exact(22, 1, 1, 80, 48, 24))                    # the shortcut over a concatenation, m = 1
_add("rows_res_in_place", "rows", "exact", lambda: _rows_exact(23, 2, 17, 40, 0, 40, inplace=True))
# rows, toleranced
_add("rows_groupnorm_two_samples", "rows", "tol", lambda: _rows_tol(24, 2, 20, 32, 24, "groupnorm"))  # a 32-row block straddles the samples
_add("rows_layernorm_1000", "rows", "tol", lambda: _rows_tol(25, 1, 5, 1000, 24, "layernorm"))
_add("rows_geglu_4096", "rows", "tol", lambda: _rows_tol(26, 1, 3, 1024, 4096, "layernorm", geglu=True))      # ldw 8192: 33 MB
_add("rows_geglu_144", "rows", "tol", lambda: _rows_tol(27, 1, 5, 32, 144, "layernorm", geglu=True))          # the block's second tile is absent
# in, temb: exact
_add("in_nchw_7", "in", "exact", lambda: dict(src=ints(gen(30), (2, 7, 15)), nchw=True))
_add("in_text_24", "in", "exact", lambda: dict(src=ints(gen(31), (154, 24)), nchw=False))             # 154 x 32 elements: 19.25 blocks
_add("temb_30_resnets", "temb", "exact", _temb_exact)
# GroupNorm statistics
_add("gn_seam_16_8", "group_norm", "tol", lambda: _gn(50, 2, 16, 8, 8, 513))                          # group 5 = channels 15 .. 17; two partial blocks, the second of one pixel
_add("gn_1024", "group_norm", "tol", lambda: _gn(51, 1, 1024, 0, 32, 6))                              # one pixel lane
_add("gn_48", "group_norm", "tol", lambda: _gn(52, 2, 48, 0, 8, 7))                                   # 21 pixel lanes, four idle threads
_add("gn_cat_one_group", "group_norm", "tol", lambda: _gn(53, 1, 1024, 1024, 1, 3))                   # 2048 channels a group
_add("gn_mean_1000", "group_norm", "tol", lambda: _gn(54, 2, 16, 8, 8, 40, offset=1000.0))
_add("gn_small_variance", "group_norm", "tol", lambda: _gn(55, 2, 32, 0, 8, 40, scale=0.003))
# LayerNorm statistics
_add("ln_1024", "layer_norm_stats", "tol", lambda: _ln(60, 5, 1024))
_add("ln_1000", "layer_norm_stats", "tol", lambda: _ln(61, 5, 1000))
_add("ln_8", "layer_norm_stats", "tol", lambda: _ln(62, 5, 8))
_add("ln_mean_1000", "layer_norm_stats", "tol", lambda: _ln(63, 5, 320, offset=1000.0, scale=0.01))
# attention
for _i, (_name, _shape) in enumerate(ATTN_SHAPES.items()):
    _add("attn_selector_" + _name, "attention", "exact", lambda i=_i, s=_shape: _attn_selector(100 + i, *s))
    _add("attn_random_" + _name, "attention", "tol", lambda i=_i, s=_shape: _attn_random(120 + i, *s))
_add("attn_spread_200", "attention", "tol", _attn_spread)
# embedding
_add("emb_1024", "embedding", "tol", lambda: _emb(90, 1024, 487.25))
_add("emb_16_t0", "embedding", "tol", lambda: _emb(91, 16, 0.0))
_add("emb_16_t487", "embedding", "tol", lambda: _emb(92, 16, 487.25))
_add("emb_16_t999", "embedding", "tol", lambda: _emb(93, 16, 999.0))

NAMES = tuple(BUILDERS)
SELECTORS = tuple(n for n in NAMES if n.startswith("attn_selector_"))
EXACT_SUMS = tuple(n for n in NAMES if BUILDERS[n][1] == "exact" and BUILDERS[n][0] != "attention")

# which case must expose which fault of tests/unet_kernel_ref.py (tests/test_unet_kernels_host.py)
FAULT_CASE = {"sample_ignores_channel_blocks": "conv_1024_out", "weight_offset_by_cs_not_cinp": "conv_cat_6_10", "k_tail_dropped": "conv_cat_80_48",
              "up_reads_gx_not_halved": "conv_up_6x20", "stride2_pad_right_bottom": "conv_stride2_48", "norm_on_padding_taps": "conv_gn_loader_5x17",
              "second_tile_of_ragged_block_kept": "conv_144_out", "gate_tile_mispaired": "rows_geglu_144",
              "norm_of_sample_0_for_all_rows": "rows_groupnorm_two_samples", "second_source_weight_row_offset": "rows_cat_80_48",
              "seam_group_split_at_cs": "gn_seam_16_8", "last_partial_block_full": "gn_seam_16_8", "padded_norm_left": "gn_seam_16_8",
              "mean_over_cs": "ln_1000", "one_pass_f32": "ln_mean_1000", "no_rescale_on_new_max": "attn_spread_200",
              "ragged_chunk_unmasked": "attn_random_d24_h5_text", "head_offset_by_dp": "attn_selector_d24_h5_text",
              "pad_columns_left": "attn_selector_d8_h3_fused", "kv_stride_of_q": "attn_selector_d72_h5_text", "sin_cos_order": "emb_16_t999",
              "class_row_of_label_0": "emb_16_t487"}

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
