"""An exact 16-bit specification of RRDBNet on the CPU: oracle/rrdbnet_ref.py's network with what the bf16 / f16 kernels keep
in 16 bits rounded through `store` (torch.bfloat16 | torch.float16), and nothing else.

Rounding points, read off the stores of conv3x3_mfma.hip, conv3x3_bf16.hip and rdb_bf16_strip.hip (E16<K>::pack4, round to
nearest even) and the host-side packing (pack_weights_bf16 / _f16, pack.hip):
  weights                once, when they are packed; biases stay float32
  the packed input       after pixel_unshuffle
  every feature map      conv_first (one value, stored twice: the trunk's x0 and the skip), x1..x4 of every dense block, every
                         dense block's output, every RRDB's output, conv_body + skip, conv_up1, conv_up2, conv_hr
  conv_last              float32, not rounded
Arithmetic of one layer, in the kernels' order:
  acc = conv + bias [-> LeakyReLU(0.2)]     in the accumulation type: float64 here (the specification), float32 with
                                            accumulate=torch.float32 (torch's conv: another summation order than the kernels',
                                            the same precision), or float32 summed serially in 16-channel chunks with
                                            accumulate="f32-chunked" (the kernels' K-chunk order)
  -> float32, then * s1 + res1, then * s2 + res2, each operation rounded to float32 (__fmul_rn / __fadd_rn: no fma)
  -> one rounding to `store`
The third dense block of an RRDB applies both residuals (x5 * 0.2 + x0, then * 0.2 + the RRDB's input) with no 16-bit
rounding between them.  The variants differ by the accumulation alone, which is all that separates a correct kernel from the
float64 variant.  (torch rounds float64 to a 16-bit type through float32, as this does: a single layer of the float64 variant
is bit for bit tests/conv_pin.py's reference.)"""
import torch
import torch.nn.functional as F

from oracle.rrdbnet_ref import pixel_unshuffle


class RRDBNetEmu16:
    def __init__(self, state_dict, scale, num_block, store, accumulate=torch.float64):
        self.scale, self.num_block, self.store_type, self.accumulate = scale, num_block, store, accumulate
        self.w = {k[:-7]: v.detach().float().to(store).float() for k, v in state_dict.items() if k.endswith(".weight")}
        self.b = {k[:-5]: v.detach().float() for k, v in state_dict.items() if k.endswith(".bias")}

    # ---- the pieces a test may replace (tests/test_rrdb_emu16_host.py plays wrong kernels with them)
    def store(self, x):
        """float32 -> the storage type (nearest even) -> float32."""
        return x.to(self.store_type).float()

    def conv(self, x, name, lrelu=False):
        """conv + bias [+ LeakyReLU] of 16-bit operands held in float32, in the accumulation type; the result as float32."""
        w, b = self.w[name], self.b[name]
        if self.accumulate == "f32-chunked":
            acc = torch.zeros(x.shape[0], w.shape[0], x.shape[2], x.shape[3])
            for c in range(0, x.shape[1], 16):      # the kernels' order: K-chunks ascending into a zeroed accumulator, the bias last
                acc = acc + F.conv2d(x[:, c:c + 16], w[:, c:c + 16], None, padding=1)
            acc = acc + b.view(1, -1, 1, 1)
        else:
            t = self.accumulate
            acc = F.conv2d(x.to(t), w.to(t), b.to(t), padding=1)
        if lrelu:
            acc = F.leaky_relu(acc, 0.2)
        return acc.float()

    def dense_block(self, x0, prefix, rrdb_in=None):
        """x0: the block's stored input.  rrdb_in: the RRDB's stored input for the third block, else None."""
        feats = [x0]
        for k in range(1, 5):
            feats.append(self.store(self.conv(torch.cat(feats, 1), f"{prefix}.conv{k}", lrelu=True)))
        v = self.conv(torch.cat(feats, 1), f"{prefix}.conv5") * 0.2 + x0
        if rrdb_in is not None:
            v = v * 0.2 + rrdb_in
        return self.store(v)

    # ---- the network
    def rrdb(self, x, prefix):
        out = self.dense_block(x, prefix + ".rdb1")
        out = self.dense_block(out, prefix + ".rdb2")
        return self.dense_block(out, prefix + ".rdb3", rrdb_in=x)

    @torch.no_grad()
    def __call__(self, x):
        """x NCHW float32 in [0, 1] (any float32 values) -> NCHW float32, as RRDBNet.forward."""
        x = x.float()
        x = pixel_unshuffle(x, 2) if self.scale == 2 else (pixel_unshuffle(x, 4) if self.scale == 1 else x)
        feat = self.store(self.conv(self.store(x), "conv_first"))
        trunk = feat
        for b in range(self.num_block):
            trunk = self.rrdb(trunk, f"body.{b}")
        feat = self.store(self.conv(trunk, "conv_body") * 1.0 + feat)
        feat = self.store(self.conv(F.interpolate(feat, scale_factor=2, mode="nearest"), "conv_up1", lrelu=True))
        feat = self.store(self.conv(F.interpolate(feat, scale_factor=2, mode="nearest"), "conv_up2", lrelu=True))
        feat = self.store(self.conv(feat, "conv_hr", lrelu=True))
        return self.conv(feat, "conv_last")

    @torch.no_grad()
    def one_layer(self, x, weight, bias, lrelu=False, upsample=False):
        """The same rounding for a single conv given by hand (what nesr_conv3x3 computes): store(conv(store(x)))."""
        self.w["_one"], self.b["_one"] = weight.float().to(self.store_type).float(), bias.float()
        x = self.store(x.float())
        if upsample:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        return self.store(self.conv(x, "_one", lrelu=lrelu))


def oracle_f64(state_dict, scale, num_block, x):
    """The exact network: oracle/rrdbnet_ref.py in float64."""
    from oracle.rrdbnet_ref import rrdbnet_forward
    with torch.no_grad():
        return rrdbnet_forward(x.double(), {k: v.double() for k, v in state_dict.items()}, scale=scale, num_block=num_block)


def _band_means(d, px):
    """Mean |d| over every band of `px` output rows and of `px` output columns (one trunk pixel wide), all channels and images."""
    m = d.abs().mean(dim=(0, 1))
    rows, cols = m.mean(1), m.mean(0)
    return torch.cat([rows[:rows.numel() // px * px].view(-1, px).mean(1), cols[:cols.numel() // px * px].view(-1, px).mean(1)])


def conditions(got, emu64, emu32, exact, band_px=4):
    """The conditions a kernel's output `got` must meet against the specification, and their figures.
      (a)  mean |got - emu64| < mean |emu64 - exact|: closer to its specification than the specification is to the exact network
      (b)  max |got - emu64| <= 4 max |emu32 - emu64|: no local error beyond what accumulation order alone produces through
           flipped 16-bit roundings (4: the maximum over 10^4..10^5 pixels varies between two draws, and a k-ordered f32 chain
           errs somewhat more than blocked sums)
      (b') the same per band: for every band of output rows and of output columns one trunk pixel wide (band_px = 4 output
           pixels), mean over the band |got - emu64| <= 4 mean over the image |emu32 - emu64|.  A flipped rounding is a spike, and
           the maximum of (b) is as large as a lost halo column or a misplaced rounding is after the network's 0.2 x 0.2 residual
           scaling; a band's mean (>= 10^3 values) averages the spikes out -- between two accumulation orders it stays within about
           twice the image's mean -- while an error that sits along a seam, or everywhere, stays in it.
      (b") the same over the image: mean |got - emu64| <= 4 mean |emu32 - emu64|.  A mean over >= 10^5 values hardly varies
           between two draws, so the factor has only the k-ordered chain to cover: an error made at every pixel (a rounding too
           many, a wrong operand) shows here with more room than in any maximum."""
    got, emu64, emu32, exact = got.double(), emu64.double(), emu32.double(), exact.double()
    fig = {"mean_to_spec": float((got - emu64).abs().mean()), "spec_to_exact": float((emu64 - exact).abs().mean()),
           "max_to_spec": float((got - emu64).abs().max()), "order_max": float((emu32 - emu64).abs().max()),
           "order_mean": float((emu32 - emu64).abs().mean()), "band_max": float(_band_means(got - emu64, band_px).max())}
    fig["a"] = fig["mean_to_spec"] < fig["spec_to_exact"]
    fig["ratio"] = fig["max_to_spec"] / fig["order_max"] if fig["order_max"] > 0 else float("inf")
    fig["b"] = fig["max_to_spec"] <= 4 * fig["order_max"]
    fig["band_ratio"] = fig["band_max"] / fig["order_mean"] if fig["order_mean"] > 0 else float("inf")
    fig["b_band"] = fig["band_max"] <= 4 * fig["order_mean"]
    fig["mean_ratio"] = fig["mean_to_spec"] / fig["order_mean"] if fig["order_mean"] > 0 else float("inf")
    fig["b_mean"] = fig["mean_to_spec"] <= 4 * fig["order_mean"]
    return fig


def describe(fig):
    return (f"(a) {fig['mean_to_spec']:.3e} < {fig['spec_to_exact']:.3e}: {fig['a']} | (b) max ratio {fig['ratio']:.2f}: {fig['b']} | "
            f"(b') band ratio {fig['band_ratio']:.2f}: {fig['b_band']} | (b\") mean ratio {fig['mean_ratio']:.2f}: {fig['b_mean']}")
