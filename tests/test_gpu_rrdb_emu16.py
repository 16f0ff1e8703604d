"""GPU: whole RRDBNets in bf16 and f16 against their exact 16-bit specification on the CPU (tests/rrdbnet_emu16.py), on each
of the three routes a 16-bit trunk can take -- the generic per-layer kernel, the large-tile per-layer kernel (whose epilogue:
res1 / res2 with s1 / s2, out_coff, out2, the NCHW tail, ragged sizes, is otherwise judged by PSNR floors only) and the
LDS-resident strip kernel.  The route is asserted by the trunk's launch count, as test_gpu_strip.py does.

No measured constant is asserted: with emu64 the specification, emu32 the same with float32 accumulation and `exact` the float64
network, all computed here on the same input,
  (a)  mean |kernel - emu64| < mean |emu64 - exact|
  (b)  max |kernel - emu64| <= 4 max |emu32 - emu64|
  (b') per band of rows / columns one trunk pixel wide: mean |kernel - emu64| <= 4 mean over the image |emu32 - emu64|
  (b") over the image: mean |kernel - emu64| <= 4 mean |emu32 - emu64|
(rrdbnet_emu16.conditions; test_rrdb_emu16_host.py shows which wrong kernels each one catches).  The measured ratios are in
DESIGN.md, "The 16-bit specification of RRDBNet"."""
import os

import pytest
import torch

from tests import conv_pin
from tests.rrdbnet_emu16 import RRDBNetEmu16, conditions, describe, oracle_f64

pytestmark = pytest.mark.gpu

INPUT = {2: (66, 94), 4: (23, 47)}        # x2plus: trunk 33 x 47 after the unshuffle; x4plus: trunk 23 x 47
ROUTES = {"generic": dict(size_independent=False, strip="0", per_rdb=5),
          "xl": dict(size_independent=True, strip="0", per_rdb=5),
          "strip": dict(size_independent=True, strip="1", per_rdb=1)}
_cpu = {}


def _weights(scale, num_block):
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    return synthetic_state_dict(seed=0, num_in_ch=3, scale=scale, num_block=num_block)


def _spec(scale, num_block, dtype, x, key):
    """(emu64, emu32, exact) of x, computed once per case and shared by the routes."""
    k = (scale, num_block, dtype, key)
    if k not in _cpu:
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        sd, st = _weights(scale, num_block), conv_pin.STORE[dtype]
        _cpu[k] = (RRDBNetEmu16(sd, scale, num_block, st)(x), RRDBNetEmu16(sd, scale, num_block, st, accumulate=torch.float32)(x),
                   oracle_f64(sd, scale, num_block, x))
    return _cpu[k]


def _net(scale, num_block, dtype, route):
    """An RRDBNet whose device context is created now, under the route's NESR_STRIP (read when the context is created)."""
    from neural_enhanced_super_resolution_amd import RRDBNet
    r = ROUTES[route]
    old = os.environ.get("NESR_STRIP")
    os.environ["NESR_STRIP"] = r["strip"]
    try:
        net = RRDBNet(3, 3, scale=scale, num_block=num_block, compute_dtype=dtype)
        net.load_state_dict(_weights(scale, num_block))
        net.eval().to("cuda:0")
        net.size_independent = r["size_independent"]
        u = 2 if scale == 2 else 1
        net(torch.zeros(1, 3, 4 * u, 4 * u, device="cuda:0"))
        net.check_status()
    finally:
        if old is None:
            os.environ.pop("NESR_STRIP", None)
        else:
            os.environ["NESR_STRIP"] = old
    net.set_kernel_timing("cuda:0", True)
    net.kernel_time()
    return net


def _judge(tag, got, spec, bands=True):
    fig = conditions(got, *spec)
    print(f"emu16 {tag}: {describe(fig)}")
    assert bool(torch.isfinite(got).all())
    assert fig["a"], describe(fig)
    assert fig["b"], describe(fig)
    assert fig["b_mean"], describe(fig)
    if bands:
        assert fig["b_band"], describe(fig)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("scale,num_block", [(2, 1), (2, 2), (4, 1), (4, 2)])
def test_network_against_its_16_bit_specification(cuda_device, scale, num_block, dtype, route):
    x = torch.rand(1, 3, *INPUT[scale], generator=torch.Generator().manual_seed(scale * 100 + num_block))
    net = _net(scale, num_block, dtype, route)
    got = net(x.to(cuda_device)).cpu()
    net.check_status()
    assert net.kernel_time()[1] == 3 * num_block * ROUTES[route]["per_rdb"], f"the trunk did not take the {route} route"
    assert got.shape == (1, 3, INPUT[scale][0] * net.out_scale(), INPUT[scale][1] * net.out_scale())
    _judge(f"x{scale}plus num_block {num_block} {dtype} {route}", got, _spec(scale, num_block, dtype, x, "whole"))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_ragged_batch_on_the_large_tile_route(cuda_device, dtype):
    """Three images of different sizes in one forward_ragged batch (vh / vw and rag_shift in every layer of the large-tile
    kernel, the up-convs included): each against the specification of that image alone."""
    scale, num_block = 2, 1
    g = torch.Generator().manual_seed(17)
    sizes = [(66, 94), (40, 62), (18, 130)]          # trunks 33 x 47, 20 x 31, 9 x 65
    imgs = [torch.rand(1, 3, h, w, generator=g) for h, w in sizes]
    net = _net(scale, num_block, dtype, "xl")
    H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
    x = torch.full((len(imgs), 3, H, W), 3.0, device=cuda_device)          # what lies outside an image must not matter
    for j, im in enumerate(imgs):
        x[j, :, :sizes[j][0], :sizes[j][1]] = im[0].to(cuda_device)
    out = net.forward_ragged(x, sizes)
    net.check_status()
    assert net.kernel_time()[1] == 15 * num_block
    s = net.out_scale()
    for j, (h, w) in enumerate(sizes):
        # (b') on the full-size image only: a column band of the 9-row trunk is 432 values, too few for a mean to average
        # the spikes of single flipped roundings out (its figure is printed all the same)
        _judge(f"ragged {h}x{w} {dtype} xl", out[j:j + 1, :, :h * s, :w * s].cpu(), _spec(scale, num_block, dtype, imgs[j], ("ragged", j)),
               bands=(h, w) == INPUT[scale])
