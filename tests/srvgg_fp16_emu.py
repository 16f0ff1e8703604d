"""Test helper: the specification of SRVGGNetCompact's 16-bit compute forms on the CPU.  ``SRVGGRef`` (tests/srvgg_ref.py)
with what the kernels keep in 16 bits rounded through that type, and nothing else changed:

  * every conv weight, once (as compact_finalize packs it: round to nearest even, torch's ``.half()`` / ``.bfloat16()``);
  * every stored activation: the image the pack kernel stages for the first conv, and each feature layer's output after
    bias and activation;
  * accumulation in float64, bias and slope as the checkpoint's float32 values; the last conv's result, the residual (the
    float32 image, nearest-upsampled) and the sum stay unrounded, as the tail's f32 epilogue keeps them.

With ``store=torch.float16`` it is the "fp16" form, with ``torch.bfloat16`` the "bf16" form: the kernels differ from it by
the order of their f32 accumulation only.

``accumulate`` (default ``torch.float64``: the specification above, unchanged) selects how a layer is summed:
  torch.float32        torch's f32 conv with the f32 bias (emu32: the kernels' precision in another order)
  "f32-kernel-order"   a zeroed f32 accumulator that takes, serially and in srvgg_compact.hip's order, the 32-channel partial
                       sum of every (dx, 32-channel chunk, dy), then the bias: the stand-in for a correct kernel
Both f32 variants then do as the kernel's epilogue does: the slope as an f32 multiply (v < 0 ? v * slope : v), one rounding
to `store`; in the tail the f32 sum plus the f32 image, one f32 add.  ``slope_f32=True`` makes the float64 variant apply the
slope that way too (float32(conv) * slope in f32, then the store's rounding): one layer of it is then bit for bit the
reference of the per-layer pins (tests/srvgg_pin.py).

The pieces a test may replace (tests/test_srvgg_pin_host.py plays wrong kernels with them): ``store``, ``weight``, ``image``,
``conv``, ``act``, ``tail``; each gets the index of the layer's conv in ``body``."""
import torch
import torch.nn.functional as F
from torch import nn

from tests.srvgg_ref import SRVGGRef

KERNEL_ORDER = "f32-kernel-order"


class SRVGGEmu16(SRVGGRef):
    def __init__(self, *a, store=torch.float16, accumulate=torch.float64, slope_f32=False, **k):
        super().__init__(*a, **k)
        assert accumulate in (torch.float64, torch.float32, KERNEL_ORDER), accumulate
        self.store_type, self.accumulate = store, accumulate
        self.work = torch.float64 if accumulate == torch.float64 else torch.float32
        self.slope_f32 = slope_f32 or self.work == torch.float32

    # ---- the pieces
    def store(self, t, idx=None):
        """-> the storage type (nearest even) -> the working type."""
        return t.to(self.store_type).to(self.work)

    def weight(self, m, idx):
        return m.weight.to(self.store_type).to(self.work)

    def image(self, x):
        """What the first conv reads: the image as the pack kernel stages it."""
        return self.store(x.to(self.work), -1)

    def conv(self, x, m, idx):
        w = self.weight(m, idx)
        if self.accumulate != KERNEL_ORDER:
            return F.conv2d(x, w, m.bias.to(self.work), padding=1)
        n, cin, h, wd = x.shape
        xp = F.pad(x, (1, 1, 1, 1))
        acc = torch.zeros(n, w.shape[0], h, wd, dtype=torch.float32)
        for dx in range(3):
            for kc in range(0, cin, 32):
                for dy in range(3):
                    acc = acc + F.conv2d(xp[:, kc:kc + 32, dy:dy + h, dx:dx + wd], w[:, kc:kc + 32, dy:dy + 1, dx:dx + 1])
        return acc + m.bias.float().view(1, -1, 1, 1)

    def slopes(self, m):
        """The activation as the kernel holds it: one float32 slope per channel."""
        if isinstance(m, nn.PReLU):
            return m.weight.float()
        return torch.full((1,), m.negative_slope if isinstance(m, nn.LeakyReLU) else 0.0, dtype=torch.float32)

    def act(self, v, m, idx):
        if not self.slope_f32:
            return m(v)
        v32 = v.float()
        return torch.where(v32 < 0, v32 * self.slopes(m).view(1, -1, 1, 1), v32).to(self.work)

    def tail(self, v, x):
        """v: the last conv's result.  Pixel shuffle plus the nearest-upsampled unrounded image."""
        return self.upsampler(v) + F.interpolate(x.to(self.work), scale_factor=self.upscale, mode="nearest")

    # ---- the network
    def forward(self, x, preact=None, features=None):
        """`preact`: optional list that receives every activation's input (the largest magnitudes a layer sees).
        `features`: optional list that receives every stored activation."""
        out = self.image(x)
        idx = 0
        for i, m in enumerate(self.body):
            if isinstance(m, nn.Conv2d):
                idx = i
                out = self.conv(out, m, i)
            else:
                if preact is not None:
                    preact.append(out)
                out = self.store(self.act(out, m, idx), idx)
                if features is not None:
                    features.append(out)
        return self.tail(out, x).to(x.dtype)
