"""CPU: the weight folding of the nearest-x2 up-convs (nesr_fold_upconv_weights, no device needed).

conv3x3(nearest_x2(x)) at output parity (py, px) reads the low-res pixels (y + py - 1 + a, x + px - 1 + b), a, b in {0, 1},
with the 3x3 taps that share a pixel summed: W[py][px][a][b].  The folded weights, applied as four 2x2-tap convolutions on the
low-res input, must give the 3x3 conv of the upsampled image."""
import pytest
import torch
import torch.nn.functional as F

from neural_enhanced_super_resolution_amd.rrdbnet import fold_upconv_weights


def _apply_folded(x, folded, bias):
    """x [n, cin, h, w] f64, folded [2, 2, 2, 2, cout, cin] f64 -> [n, cout, 2h, 2w]: four 2x2-tap convs on the low-res image."""
    n, cin, h, w = x.shape
    cout = folded.shape[4]
    xp = F.pad(x, (1, 1, 1, 1))     # zero padding: a high-res tap outside the image is a low-res tap outside the image
    out = torch.zeros(n, cout, 2 * h, 2 * w, dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            acc = torch.zeros(n, cout, h, w, dtype=x.dtype)
            for a in range(2):
                for b in range(2):
                    win = xp[:, :, py + a:py + a + h, px + b:px + b + w]      # low-res pixel (y + py - 1 + a, x + px - 1 + b)
                    acc += torch.einsum("oc,nchw->nohw", folded[py, px, a, b], win)
            out[:, :, py::2, px::2] = acc
    return out + bias.view(1, -1, 1, 1)


def _ref(x, wgt, bias):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wgt, bias, padding=1)


# which parity slabs tap (ky, kx) must land in: row ky of the kernel reads low-res row offset a at row parity py
ROWS = {0: [(0, 0), (1, 0)], 1: [(0, 1), (1, 0)], 2: [(0, 1), (1, 1)]}   # ky -> [(py, a), (py, a)]


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (6, 1), (5, 9), (13, 21)])
def test_folded_weights_reproduce_the_upsampled_conv_in_float64(h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    cin, cout = 6, 5
    # weights that are exact in float32 with room to spare, so the f32 sums of the folding are exact and the
    # comparison below measures the algebra, not f32 rounding: multiples of 2^-10 below 4
    wgt = torch.randint(-4096, 4096, (cout, cin, 3, 3), generator=g).to(torch.float32) / 1024.0
    x = torch.randn(2, cin, h, w, generator=g, dtype=torch.float64)
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    folded = fold_upconv_weights(wgt).double()
    got = _apply_folded(x, folded, bias)
    ref = _ref(x, wgt.double(), bias)
    assert got.shape == ref.shape == (2, cout, 2 * h, 2 * w)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_random_f32_weights_fold_to_f32_sums_in_ky_kx_order():
    """General f32 weights: every folded value is the f32 sum of its taps, ky ascending, then kx ascending."""
    g = torch.Generator().manual_seed(3)
    wgt = torch.randn(4, 3, 3, 3, generator=g)
    folded = fold_upconv_weights(wgt)
    exp = torch.zeros(2, 2, 2, 2, 4, 3)
    for py in range(2):
        for px in range(2):
            for ky in range(3):
                for kx in range(3):
                    a = dict(ROWS[ky])[py]
                    b = dict(ROWS[kx])[px]
                    exp[py, px, a, b] = exp[py, px, a, b] + wgt[:, :, ky, kx]      # f32 adds in this order
    assert torch.equal(folded, exp)
    # and in float64 it is the upsampled conv to f32 rounding of the sums (three adds of values below 8: 4 * 2^-24 * 8)
    x = torch.randn(1, 3, 5, 4, generator=g, dtype=torch.float64)
    got = _apply_folded(x, folded.double(), torch.zeros(4, dtype=torch.float64))
    ref = _ref(x, wgt.double(), torch.zeros(4, dtype=torch.float64))
    assert (got - ref).abs().max().item() < 1e-5


@pytest.mark.parametrize("tap", range(9))
def test_one_hot_tap_lands_in_exactly_the_predicted_slabs(tap):
    ky, kx = tap // 3, tap % 3
    cout, cin = 3, 4
    wgt = torch.zeros(cout, cin, 3, 3)
    for o in range(cout):
        wgt[o, (o + tap) % cin, ky, kx] = float(o + 2)
    folded = fold_upconv_weights(wgt)
    exp = torch.zeros_like(folded)
    for py, a in ROWS[ky]:
        for px, b in ROWS[kx]:
            exp[py, px, a, b] = wgt[:, :, ky, kx]
    assert torch.equal(folded, exp)
    assert int((folded != 0).sum()) == 4 * cout      # one slab per output parity, nothing else


def test_small_integer_weights_fold_exactly():
    g = torch.Generator().manual_seed(11)
    wgt = torch.randint(-7, 8, (8, 16, 3, 3), generator=g).to(torch.float32)
    folded = fold_upconv_weights(wgt)
    assert torch.equal(folded, folded.round())
    # every parity's four slabs hold all nine taps once
    total = wgt.sum(dim=(2, 3))
    for py in range(2):
        for px in range(2):
            assert torch.equal(folded[py, px].sum(dim=(0, 1)), total)
    x = torch.randint(-5, 6, (1, 16, 4, 7), generator=g).to(torch.float64)
    got = _apply_folded(x, folded.double(), torch.zeros(8, dtype=torch.float64))
    ref = _ref(x, wgt.double(), torch.zeros(8, dtype=torch.float64))
    assert torch.equal(got, ref)
