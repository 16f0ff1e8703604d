"""Test helper: upstream's SRVGGNetCompact (realesrgan/archs/srvgg_arch.py) restated as a plain torch CPU module in float64,
with upstream's structure and state_dict key names.  Takes and returns the caller's dtype (RealESRGANerRef hands it f32)."""
import torch
import torch.nn.functional as F
from torch import nn


class SRVGGRef(nn.Module):
    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type="prelu"):
        super().__init__()
        self.upscale = upscale

        def act():
            return {"prelu": lambda: nn.PReLU(num_parameters=num_feat), "relu": lambda: nn.ReLU(),
                    "leakyrelu": lambda: nn.LeakyReLU(negative_slope=0.1)}[act_type]()

        self.body = nn.ModuleList([nn.Conv2d(num_in_ch, num_feat, 3, 1, 1), act()])
        for _ in range(num_conv):
            self.body.extend([nn.Conv2d(num_feat, num_feat, 3, 1, 1), act()])
        self.body.append(nn.Conv2d(num_feat, num_out_ch * upscale * upscale, 3, 1, 1))
        self.upsampler = nn.PixelShuffle(upscale)
        self.double()

    def forward(self, x, preact=None):
        """`preact`: optional list that receives every activation's input (for the synthetic-weight statistics)."""
        out = x.double()
        for m in self.body:
            if preact is not None and not isinstance(m, nn.Conv2d):
                preact.append(out)
            out = m(out)
        out = self.upsampler(out) + F.interpolate(x.double(), scale_factor=self.upscale, mode="nearest")
        return out.to(x.dtype)
