"""An exact specification of the default f32 form (compute_dtype="f32": every f32 operand an f16 pair) on the CPU, per value.

The four kernels of the form (conv3x3_f16x2.hip, rdb_f16x2.hip, upconv2x2_f16x2.hip, conv_last in its narrow geometry) carry a
value x as hi + lo 2^-11 and accumulate w_hi x_hi + 2^-11 (w_hi x_lo + w_lo x_hi) in f32.  Products of two halves are exact in
f32 (11 x 11 significant bits), so the form has a closed value in float64 and all a correct kernel adds to it is the order of
its f32 sums.  Rounding points, read off the code (f16x2_common.h split2, pack_weights_f16x2, pack_elem.h, the epilogues):

  split     hi = f16(x) (nearest even, subnormals kept), lo = f16((x - hi) 2^11) (x - hi and the scaling are exact in f32);
            pair(x) = hi + lo / 2048.  |x| >= 65520 or non-finite is outside this specification (test_gpu_range.py owns it).
  weights   split once on the host; the folded 2x2 taps of an up-conv are summed in float32 (ky, then kx ascending:
            fold_upconv_weights) and split after that.  Biases stay float32.
  input     split after pixel_unshuffle
  a layer   main = sum w_hi x_hi, cross = sum (w_hi x_lo + w_lo x_hi)  (lo x lo is not formed)
            v = main + cross / 2048 + bias            in the accumulation type, see below
            LeakyReLU: max(v, v s) with s = float32(0.2)   (fmaxf(v, v * 0.2f))
            -> float32, then * s1 + res1, then * s2 + res2, each operation rounded to float32 (scale_add_2r: no fma);
            residuals are the stored pairs re-joined (load_regrouped: fma(lo, 2^-11, hi), exact in f32)
            feature maps store pair(v) -- the single-layer hook nesr_conv3x3 too (oneshot_api.cpp: the layer writes its pair
            map, launch_nhwc_to_nchw re-joins it); conv_last's planar output is v itself.
  a block   x1..x4 stored as pairs, conv5 * 0.2 + x0; the third block of an RRDB then * 0.2 + the RRDB's input with no pair
            rounding in between.
The accumulation type is a parameter, as in tests/rrdbnet_emu16.py:
  torch.float64   the specification
  torch.float32   torch's f32 conv for main and for cross (another summation order than the kernels', the same precision),
                  joined by one fma, the bias added in f32
  "f32-chunked"   the kernels' K order: 16-channel chunks ascending, main and cross in separate f32 accumulators, joined once
                  by one fma (cout_exchange_acc), then the bias
  "f32-steps"     "f32-chunked" cut finer, at the MFMA: within a chunk the five tap-steps of f16x2_common.h in order, each
                  MFMA's 32 (step 4: 16 or 32) products summed and added to its accumulator (3x3 layers; a 2x2 layer: per
                  chunk and tap column b, the two tap rows of one MFMA together)

`conditions` judges a kernel's output against the float64 variant with the float32 variants as the yardstick; see there why
condition (a) of the 16-bit tests has no counterpart."""
import torch
import torch.nn.functional as F

from oracle.rrdbnet_ref import pixel_unshuffle

LO = 2048.0
S = float(torch.tensor(0.2, dtype=torch.float32))         # float32(0.2) = 0.20000000298..., what `* 0.2f` multiplies by
STANDINS = (torch.float32, "f32-chunked")


# ------------------------------------------------------------------------------------------------------------ the pair
def split(x):
    """float32 -> (hi, scaled lo), both f16 values held in float32."""
    x = x.float()
    hi = x.half().float()
    lo = ((x - hi) * LO).half().float()
    return hi, lo


def join(p):
    """(hi, scaled lo) -> hi + lo / 2048 in float64 (exact; the same value is exact in float32)."""
    return p[0].double() + p[1].double() / LO


def pair(x):
    return join(split(x))


def pair_bytes(x):
    """[1, C, h, w] float32, C a multiple of 16 -> the staging bytes of nesr_band_rows for rows 0..h-1 in the pair form:
    [chunk][row][column][16 hi halves | 16 scaled-lo halves] as a flat uint8 tensor."""
    hi, lo = split(x)
    _, c, h, w = x.shape
    planes = torch.stack([hi[0].view(c // 16, 16, h, w), lo[0].view(c // 16, 16, h, w)], 0)      # [plane, chunk, k, h, w]
    return planes.permute(1, 3, 4, 0, 2).contiguous().half().view(torch.uint8).reshape(-1)


def pair_values(raw, h, w):
    """The inverse: staging bytes -> [1, C, h, w] float64."""
    v = raw.cpu().contiguous().view(torch.float16).view(-1, h, w, 2, 16).double()                  # [chunk, h, w, plane, k]
    v = v[:, :, :, 0] + v[:, :, :, 1] / LO
    return v.permute(0, 3, 1, 2).reshape(1, -1, h, w)


def nearest_x2(p):
    return tuple(F.interpolate(t, scale_factor=2, mode="nearest") for t in p)


def fold_restated(weight):
    """nesr_fold_upconv_weights restated: OIHW f32 -> [py][px][a][b][cout][cin], f32 sums, ky ascending, then kx
    (test_upconv_fold_host.py ties this to the library's)."""
    w = weight.float()
    out = torch.zeros(2, 2, 2, 2, w.shape[0], w.shape[1])
    for py in range(2):
        for px in range(2):
            for ky in range(3):
                for kx in range(3):
                    a, b = (py + ky + 1) // 2 - py, (px + kx + 1) // 2 - px
                    out[py, px, a, b] = out[py, px, a, b] + w[:, :, ky, kx]
    return out


def make_case(cin, cout, h, w, seed, n=2, scale=1.0):
    """The per-layer case of test_gpu_conv.py: randn input, weights randn sqrt(2 / (9 cin)), bias 0.1 randn; `scale` scales
    the activations (input and bias)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x * scale, wt, b * scale


# 3x3: the (ky, kx) taps of the MFMAs of tap-steps 0..4 (f16x2_common.h: tap_pixel_offset)
STEPS_3X3 = [[(0, 0), (1, 0)], [(0, 1), (1, 1)], [(0, 2), (1, 2)], [(2, 0), (2, 1)], [(2, 2)]]


# ------------------------------------------------------------------------------------------------------------ the arithmetic
class PairSpec:
    """One layer / one dense block of the pair form.  The small methods are the pieces a test may replace
    (tests/test_pair_spec_host.py plays wrong kernels with them)."""

    def __init__(self, accumulate=torch.float64):
        self.accumulate = accumulate

    # ---- pieces
    def store(self, v):
        """float32 value -> the stored pair."""
        return split(v)

    def residual(self, p):
        """A stored pair as a residual operand: re-joined, float32 (exact)."""
        return join(p).float()

    def _corr(self, xs, ws, pad, t):
        """sum of the correlations of the (x, w) pairs in type t, as ONE sum."""
        return F.conv2d(torch.cat([x.to(t) for x in xs], 1), torch.cat([w.to(t) for w in ws], 1), None, padding=pad)

    def sums(self, xp, wp, name, pad=1, wh_x=None):
        """(main, cross) of one layer in the accumulation type.  xp, wp: (hi, lo) of input and weights; wh_x: the w_hi that
        meets x_lo (a mutant's handle; the kernels read the same w_hi for both)."""
        xh, xl = xp
        wh, wl = wp
        wh_x = wh if wh_x is None else wh_x
        acc = self.accumulate
        if acc in (torch.float64, torch.float32):
            return self._corr([xh], [wh], pad, acc), self._corr([xl, xh], [wh_x, wl], pad, acc)
        main = cross = 0.0
        for c in range(0, xh.shape[1], 16):
            k = slice(c, c + 16)
            if acc == "f32-chunked":
                main = main + self._corr([xh[:, k]], [wh[:, k]], pad, torch.float32)
                cross = cross + self._corr([xl[:, k], xh[:, k]], [wh_x[:, k], wl[:, k]], pad, torch.float32)
                continue
            assert acc == "f32-steps", acc
            if wh.shape[-1] == 3:
                for step in STEPS_3X3:
                    m = torch.zeros(1, 1, 3, 3)
                    for ky, kx in step:
                        m[0, 0, ky, kx] = 1.0
                    main = main + self._corr([xh[:, k]], [wh[:, k] * m], pad, torch.float32)
                    if len(step) == 2:      # mfma_tap3: cr += WH XL, then cr += WL XH
                        cross = cross + self._corr([xl[:, k]], [wh_x[:, k] * m], pad, torch.float32)
                        cross = cross + self._corr([xh[:, k]], [wl[:, k] * m], pad, torch.float32)
                    else:                   # mfma_tap2: both cross terms of the last tap in one MFMA
                        cross = cross + self._corr([xl[:, k], xh[:, k]], [wh_x[:, k] * m, wl[:, k] * m], pad, torch.float32)
            else:                           # 2x2: one MFMA triple per tap column b, K = 16 channels x the two tap rows
                for b in range(2):
                    m = torch.zeros(1, 1, 2, 2)
                    m[0, 0, :, b] = 1.0
                    main = main + self._corr([xh[:, k]], [wh[:, k] * m], pad, torch.float32)
                    cross = cross + self._corr([xl[:, k]], [wh_x[:, k] * m], pad, torch.float32)
                    cross = cross + self._corr([xh[:, k]], [wl[:, k] * m], pad, torch.float32)
        return main, cross

    def combine(self, main, cross, bias):
        """v = main + cross / 2048 + bias in the accumulation type (float32: one fma, then the bias)."""
        if self.accumulate == torch.float64:
            return main + cross / LO + bias.double().view(1, -1, 1, 1)
        v = (main.double() + cross.double() / LO).float()       # fma(cross, 2^-11, main): one rounding
        return v + bias.float().view(1, -1, 1, 1)

    # ---- a layer
    def pre(self, xp, wp, bias, name="", folded=False):
        """v before the activation, on the layer's output grid.  folded: wp are the split [2, 2, 2, 2, cout, cin] taps of an
        up-conv in its 2x2 form and xp the low-res pairs."""
        if not folded:
            return self.combine(*self.sums(xp, wp, name), bias)
        n, _, h, w = xp[0].shape
        padded = tuple(F.pad(t, (1, 1, 1, 1)) for t in xp)
        out = None
        for py in range(2):
            for px in range(2):
                win = tuple(t[:, :, py:py + h + 1, px:px + w + 1] for t in padded)      # low-res pixels (y + py - 1 + a, x + px - 1 + b)
                wpp = tuple(t[py, px].permute(2, 3, 0, 1) for t in wp)                  # [cout, cin, a, b]
                v = self.combine(*self.sums(win, wpp, name, pad=0), bias)
                if out is None:
                    out = torch.zeros(n, v.shape[1], 2 * h, 2 * w, dtype=v.dtype)
                out[:, :, py::2, px::2] = v
        return out

    def layer(self, xp, wp, bias, name="", lrelu=False, s1=None, res1=None, s2=None, res2=None, upconv=None, planar=False):
        """One layer of stored pairs -> the stored pair (planar: v itself, in the accumulation type).  upconv: None | "3x3"
        (wp the split 3x3 weights) | "2x2" (wp the split folded taps)."""
        if upconv == "3x3":
            xp = nearest_x2(xp)
        v = self.pre(xp, wp, bias, name, folded=upconv == "2x2")
        if lrelu:
            v = torch.maximum(v, v * S)
        if planar:
            return v
        v = v.float()
        if res1 is not None:
            v = v * s1 + self.residual(res1)
        if res2 is not None:
            v = v * s2 + self.residual(res2)
        return self.store(v)

    @torch.no_grad()
    def one_layer(self, x, weight, bias, lrelu=False, upsample=False, upconv="3x3", folded=None):
        """What nesr_conv3x3 / nesr_conv3x3_up compute in the f16-pair form: x NCHW float32 -> the joined stored pair, float64.
        folded: the [2, 2, 2, 2, cout, cin] taps for upconv="2x2" (default: fold_restated(weight))."""
        if upsample and upconv == "2x2":
            wp = split(fold_restated(weight) if folded is None else folded)
        else:
            wp = split(weight)
        return join(self.layer(split(x), wp, bias, "_one", lrelu=lrelu, upconv=upconv if upsample else None))


class PairRRDBNet(PairSpec):
    """RRDBNet in the pair form, shaped like RRDBNetEmu16.  upconv: "2x2" | "3x3"; fold: the fold of a 3x3 weight
    (rrdbnet.fold_upconv_weights in the GPU tests, fold_restated in the host tests)."""

    def __init__(self, state_dict, scale, num_block, accumulate=torch.float64, upconv="2x2", fold=fold_restated):
        super().__init__(accumulate)
        self.scale, self.num_block, self.upconv = scale, num_block, upconv
        self.w = {k[:-7]: split(v.detach()) for k, v in state_dict.items() if k.endswith(".weight")}
        self.b = {k[:-5]: v.detach().float() for k, v in state_dict.items() if k.endswith(".bias")}
        if upconv == "2x2":
            for name in ("conv_up1", "conv_up2"):
                if name + ".weight" in state_dict:
                    self.w[name] = split(fold(state_dict[name + ".weight"].detach().float()))

    def conv(self, xp, name, **kw):
        return self.layer(xp, self.w[name], self.b[name], name, **kw)

    @torch.no_grad()
    def dense_block(self, x0, prefix, rrdb_in=None):
        """x0: the block's stored input pair.  rrdb_in: the RRDB's stored input pair for the third block, else None."""
        feats = [x0]
        for k in range(1, 5):
            cat = tuple(torch.cat([f[i] for f in feats], 1) for i in range(2))
            feats.append(self.conv(cat, f"{prefix}.conv{k}", lrelu=True))
        cat = tuple(torch.cat([f[i] for f in feats], 1) for i in range(2))
        return self.conv(cat, f"{prefix}.conv5", s1=0.2, res1=x0, s2=0.2 if rrdb_in is not None else None, res2=rrdb_in)

    def rrdb(self, x, prefix):
        out = self.dense_block(x, prefix + ".rdb1")
        out = self.dense_block(out, prefix + ".rdb2")
        return self.dense_block(out, prefix + ".rdb3", rrdb_in=x)

    @torch.no_grad()
    def first(self, x):
        """pixel_unshuffle, the input split, conv_first -> its stored pair."""
        x = x.float()
        x = pixel_unshuffle(x, 2) if self.scale == 2 else (pixel_unshuffle(x, 4) if self.scale == 1 else x)
        return self.conv(split(x), "conv_first")

    @torch.no_grad()
    def features(self, x):
        """x NCHW float32 -> the stored pair of conv_body + skip (what the up-convs read; the same for both of their forms)."""
        feat = self.first(x)           # one value, stored twice: the trunk's x0 and the skip
        trunk = feat
        for b in range(self.num_block):
            trunk = self.rrdb(trunk, f"body.{b}")
        return self.conv(trunk, "conv_body", s1=1.0, res1=feat)

    @torch.no_grad()
    def __call__(self, x):
        """x NCHW float32 -> conv_last's planar output in the accumulation type."""
        return self.tail(self.features(x))

    @torch.no_grad()
    def tail(self, feat):
        feat = self.conv(feat, "conv_up1", lrelu=True, upconv=self.upconv)
        feat = self.conv(feat, "conv_up2", lrelu=True, upconv=self.upconv)
        feat = self.conv(feat, "conv_hr", lrelu=True)
        return self.conv(feat, "conv_last", planar=True)


# ------------------------------------------------------------------------------------------------------------ the judgement
def _band_means(d, px):
    """Mean |d| over every band of `px` rows and of `px` columns, all channels and images."""
    m = d.abs().mean(dim=(0, 1))
    rows, cols = m.mean(1), m.mean(0)
    return torch.cat([rows[:rows.numel() // px * px].view(-1, px).mean(1), cols[:cols.numel() // px * px].view(-1, px).mean(1)])


def conditions(got, spec64, spec32, band_px=1):
    """The conditions a kernel's output `got` must meet against the specification `spec64`, and their figures.  spec32: the
    float32 stand-ins of the same input (one tensor or several); the order figures are the larger of theirs against spec64.
      (b)  max |got - spec64| <= 4 order max
      (b') for every band of rows and of columns `band_px` wide (one pixel of the layer): mean over the band |got - spec64|
           <= 4 order mean (over the image)
      (b") mean |got - spec64| <= 4 order mean
    with the factor 4 and its reasons as in rrdbnet_emu16.conditions.  Nothing measured on a kernel enters.
    Condition (a) of the 16-bit tests (closer to the specification than the specification is to the exact network) does NOT
    carry over and is not asserted: here the specification is closer to the exact network (mean 5.8e-8 at the output of
    x4plus with one RRDB: the pairs lose 2^-22 per operand) than a correct f32 accumulation is to the specification (1.3e-7),
    so (a) would fail every correct kernel."""
    if torch.is_tensor(spec32):
        spec32 = [spec32]
    got, spec64 = got.double(), spec64.double()
    orders = [(s.double() - spec64).abs() for s in spec32]
    d = (got - spec64).abs()
    fig = {"max_to_spec": float(d.max()), "mean_to_spec": float(d.mean()), "band_max": float(_band_means(d, band_px).max()),
           "order_max": max(float(o.max()) for o in orders), "order_mean": max(float(o.mean()) for o in orders)}

    def ratio(a, b):
        return a / b if b > 0 else (0.0 if a == 0 else float("inf"))
    fig["ratio"] = ratio(fig["max_to_spec"], fig["order_max"])
    fig["band_ratio"] = ratio(fig["band_max"], fig["order_mean"])
    fig["mean_ratio"] = ratio(fig["mean_to_spec"], fig["order_mean"])
    fig["b"] = fig["max_to_spec"] <= 4 * fig["order_max"]
    fig["b_band"] = fig["band_max"] <= 4 * fig["order_mean"]
    fig["b_mean"] = fig["mean_to_spec"] <= 4 * fig["order_mean"]
    fig["ok"] = fig["b"] and fig["b_band"] and fig["b_mean"]
    band = _band_means(d, band_px)
    fig["worst_band"] = int(band.argmax())                       # rows first, then columns
    fig["argmax"] = tuple(int(i) for i in torch.unravel_index(d.argmax(), d.shape))
    return fig


def describe(fig):
    return (f"order max {fig['order_max']:.3e} mean {fig['order_mean']:.3e} | (b) max ratio {fig['ratio']:.2f}: {fig['b']} at {fig['argmax']} | "
            f"(b') band ratio {fig['band_ratio']:.2f}: {fig['b_band']} (band {fig['worst_band']}) | (b\") mean ratio {fig['mean_ratio']:.2f}: {fig['b_mean']}")


def worst_ratio(fig):
    return max(fig["ratio"], fig["band_ratio"], fig["mean_ratio"])
