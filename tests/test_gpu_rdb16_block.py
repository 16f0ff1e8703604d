"""GPU: one bf16 / f16 dense block, per value, on each of the three routes a 16-bit trunk can take -- the generic per-layer
kernel, the large-tile per-layer kernel and the LDS-resident strip kernel (rdb_bf16_strip.hip) -- through the band entries
(tests/rdb16_block.py: band_begin, a chosen x0 into the block's input buffer, band_rdb(r), the output buffer read back).

Exact cases.  Routing weights, integer biases and integer inputs: the block has one right answer, whatever the summation order
(test_rdb16_block_host.py proves it for every case here and shows the wrong kernels that equality catches: a lost halo column, a
stale window row, a late second residual, swapped growth channels, a truncating store, an fma, 0.25 for 0.2).  The kernel's
values must be that answer bit for bit, on the shapes that stress the strip kernel's geometry (below one strip of 16 columns and
one position of 12 rows, one off the multiples, the multiples, one strip wide, long and thin), for r = 0, 1, 2 (r = 2: the second
residual, read and overwritten in place), and on the strip route also with the strips cut into row segments.

Random weights, for what integers cannot show (accumulation precision on realistic values): the two rules of
rdb16_block.share_and_size against the float64 specification computed here on the same input.  Nothing measured on a kernel is
asserted.

The route is asserted by the launch count of the block (1 on the strip route, 5 per layer) and fixed by the settings the
context is created with; last_conv_kernel() records the single-layer hooks only, so between the two per-layer kernels the
setting is what decides (size_independent: conv3x3_mfma.hip's launch16), as in test_gpu_rrdb_emu16.py.  The figures this
file showed on an MI355X are in DESIGN.md, "The 16-bit dense block, per block".

What it found: the per-layer kernels' residuals had compiled to one fused multiply-add (every signed case, by the fma mutant's
counts), and the strip kernel folded the first residual into conv5's sums, (x5 + x0 / s1) * s1 in one rounding, which is one f16
ulp off where x5 * s1 cancels x0 (32 signed f16 cases, 1 to 8 values each).  Both are now the specification's two roundings."""
import pytest
import torch

from tests import rdb16_block as B

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
SIGNS = [False, True]
_want, _imgs = {}, {}


def _image(hw, device):
    """What band_begin runs conv_first on: it sizes the band image and leaves the buffers filled with something else than zeros."""
    if hw not in _imgs:
        _imgs[hw] = torch.rand(1, 3, *hw, generator=torch.Generator().manual_seed(hw[0] * 100 + hw[1]))
    return _imgs[hw].to(device)


def _exact(hw, r, signed, dtype):
    """(weights, x0, rrdb_in, expected) of one exact case, computed once and shared by the routes."""
    key = (hw, r, signed, dtype)
    if key not in _want:
        sd, x0, rrdb_in = B.exact_case(hw, r, signed, dtype)
        _want[key] = (sd, x0, rrdb_in, B.expected(sd, x0, r, rrdb_in, dtype))
    return _want[key]


def _check_exact(cuda_device, dtype, route, r, signed, hw, seg=None):
    sd, x0, rrdb_in, want = _exact(hw, r, signed, dtype)
    net = B.block_net(dtype, route, sd, seg)
    got, launches = B.run_block(net, _image(hw, cuda_device), x0, r, rrdb_in)
    assert launches == B.ROUTES[route]["launches"], f"{launches} launches: the block did not take the {route} route"
    assert got.shape == want.shape
    assert torch.equal(got, want), B.describe_difference(got, want)


@pytest.mark.parametrize("hw", B.SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("signed", SIGNS, ids=["nonneg", "signed"])
@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("route", list(B.ROUTES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_block(cuda_device, dtype, route, r, signed, hw):
    _check_exact(cuda_device, dtype, route, r, signed, hw)


@pytest.mark.parametrize("hw", B.SEG_SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("signed", SIGNS, ids=["nonneg", "signed"])
@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("seg", B.SEGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_block_in_row_segments(cuda_device, dtype, seg, r, signed, hw):
    """6 and 11 positions, uncut (-1), in segments of at most 2 positions and as the packer cuts them (0): every segment starts
    one position early, and its rows must be the closed form's, not only the uncut sweep's."""
    _check_exact(cuda_device, dtype, "strip", r, signed, hw, seg=seg)


# ------------------------------------------------------------------------------------------------------------ random weights
_specs = {}


def _random(hw, r, dtype):
    key = (hw, r, dtype)
    if key not in _specs:
        x0, rrdb_in = B.random_inputs(hw[0], hw[1], dtype)
        _specs[key] = (x0, rrdb_in) + B.specs(B.random_state_dict(), x0, r, rrdb_in, dtype)
    return _specs[key]


@pytest.mark.parametrize("hw,seg", B.RANDOM_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"seg{v}")
@pytest.mark.parametrize("r", [0, 2])
@pytest.mark.parametrize("route", list(B.ROUTES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_block_against_the_float64_specification(cuda_device, dtype, route, r, hw, seg):
    x0, rrdb_in, spec64, standins = _random(hw, r, dtype)
    net = B.block_net(dtype, route, B.random_state_dict(), seg if route == "strip" else None)
    got, launches = B.run_block(net, _image(hw, cuda_device), x0, r, rrdb_in)
    assert launches == B.ROUTES[route]["launches"], f"{launches} launches: the block did not take the {route} route"
    fig = B.share_and_size(got, spec64, standins, dtype)
    print(f"rdb16 random {hw} r {r} {dtype} {route}{' seg ' + seg if seg and route == 'strip' else ''}: {B.describe(fig)}")
    assert fig["finite"]
    assert fig["share"], B.describe(fig)
    assert fig["size"], B.describe(fig)
