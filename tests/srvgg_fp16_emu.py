"""Test helper: the specification of SRVGGNetCompact's 16-bit compute forms on the CPU.  ``SRVGGRef`` (tests/srvgg_ref.py)
with what the kernels keep in 16 bits rounded through that type, and nothing else changed:

  * every conv weight, once (as compact_finalize packs it: round to nearest even, torch's ``.half()`` / ``.bfloat16()``);
  * every stored activation: the image the pack kernel stages for the first conv, and each feature layer's output after
    bias and activation;
  * accumulation in float64, bias and slope as the checkpoint's float32 values; the last conv's result, the residual (the
    float32 image, nearest-upsampled) and the sum stay unrounded, as the tail's f32 epilogue keeps them.

With ``store=torch.float16`` it is the "fp16" form, with ``torch.bfloat16`` the "bf16" form: the kernels differ from it by
the order of their f32 accumulation only."""
import torch
import torch.nn.functional as F
from torch import nn

from tests.srvgg_ref import SRVGGRef


class SRVGGEmu16(SRVGGRef):
    def __init__(self, *a, store=torch.float16, **k):
        super().__init__(*a, **k)
        self.store = store

    def _q(self, t):
        return t.to(self.store).double()

    def forward(self, x, preact=None):
        """`preact`: optional list that receives every activation's input (the largest magnitudes a layer sees)."""
        out = self._q(x.double())
        for m in self.body:
            if isinstance(m, nn.Conv2d):
                out = F.conv2d(out, self._q(m.weight), m.bias, padding=1)
            else:
                if preact is not None:
                    preact.append(out)
                out = self._q(m(out))
        out = self.upsampler(out) + F.interpolate(x.double(), scale_factor=self.upscale, mode="nearest")
        return out.to(x.dtype)
