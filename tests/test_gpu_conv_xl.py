"""GPU: the large-tile LDS-DMA kernel (conv3x3_bf16_xl_kernel, csrc/conv3x3_bf16.hip) one layer at a time, pinned per value.

Every case asserts through nesr_debug_last_conv_kernel that the large-tile kernel is what its launcher chose: the size switch of
launch_conv3x3_bf16 / _f16 is not copied here, the frames are simply well above it, and a switch that moves makes these tests
fail instead of passing under another kernel.

  in process   N = 2, 258 x 290: 17 x 10 tiles of 16 x 32, the last tile row 2 rows high (three of four waves inactive), the
               last tile column 2 pixels wide; every (cin, cout) whose instantiation or prologue differs -- cin 16 (one K-chunk:
               no second input chunk in the prologue), 32 (two), many; cout 32 (three-slot input ring) and 64 (two-slot);
               cout 3 (padded to 32) -- with and without LeakyReLU, both element types for the extremes of cin; an upsampled layer
               with odd source sizes; one-hot taps, exact
  child        the sizes where the edge bookkeeping lives (an image smaller than a tile, fewer than 4 rows: wave 0 alone, one
               pixel past each tile multiple) are below the switch: a fresh process with NESR_BF16_KERNEL=xl runs
               tests/xl_layer_child.py once; a second one adds NESR_XL_GEOMETRY=8 (8 waves, 32 x 32 tiles)
The pin itself is tests/conv_pin.py."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import conv_pin

pytestmark = pytest.mark.gpu

N, H, W = 2, 258, 290
CASES = [(16, 64, "bf16"), (16, 64, "f16"), (32, 32, "bf16"), (64, 32, "bf16"), (160, 32, "bf16"), (192, 64, "bf16"), (192, 64, "f16"),
         (64, 64, "bf16"), (64, 3, "bf16")]

_last = {}      # the float64 conv of the last case: LeakyReLU on and off share it (they run one after the other)


def _reference(key, x, wt, b, up=False):
    if _last.get("key") != key:
        _last.clear()
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        _last.update(key=key, ref=conv_pin.conv_f64(x, wt, b, up))
    return _last["ref"]


def _run(cuda_device, cin, cout, dtype, lrelu, hw, up=False):
    from neural_enhanced_super_resolution_amd import conv3x3, last_conv_kernel
    x, wt, b = conv_pin.make_case(cin, cout, hw[0], hw[1], dtype, seed=cin * 7 + cout, n=N)
    y = conv3x3(x.to(cuda_device), wt, b, lrelu=lrelu, upsample=up, dtype=dtype).cpu()
    ran = last_conv_kernel()
    pre, mag = _reference((cin, cout, dtype, hw, up), x, wt, b, up)
    fig = conv_pin.pin(y, pre, mag, cin, lrelu, dtype)
    print(f"kernel {ran}: {dtype} cin {cin} cout {cout} {hw} lrelu {lrelu} up {up}: outside {fig['outside']}, worst {fig['worst_ulps']:.2f} ulp, "
          f"not bitwise {fig['miss']:.2e}")
    assert ran == "xl", f"{hw} ran the {ran} kernel, not the large-tile kernel"
    conv_pin.assert_pin(fig, dtype, f"{dtype} {cin}->{cout} {hw}")


@pytest.mark.parametrize("lrelu", [False, True])      # (the upper decorator varies fastest: a case's two forms run in a row)
@pytest.mark.parametrize("cin,cout,dtype", CASES)
def test_xl_layer_rounding_pin(cuda_device, cin, cout, dtype, lrelu):
    _run(cuda_device, cin, cout, dtype, lrelu, (H, W))


def test_xl_layer_rounding_pin_upsampled(cuda_device):
    """129 x 145 in, 258 x 290 out: odd source sizes, the upsample shift in the DMA source address."""
    _run(cuda_device, 64, 64, "bf16", True, (H // 2, W // 2), up=True)


def test_xl_one_hot_taps(cuda_device):
    """Tap / row-reuse / channel bookkeeping, exactly: 258 x 259 (one pixel past a tile column, two rows past a tile row)."""
    from neural_enhanced_super_resolution_amd import conv3x3, last_conv_kernel
    for tap in range(9):
        x, wt, b, ref = conv_pin.one_hot_case(32, 64, 258, 259, tap)
        got = conv3x3(x.to(cuda_device), wt, b, dtype="bf16").cpu()
        assert last_conv_kernel() == "xl"
        assert torch.equal(got, ref), f"tap {tap}"
    print("kernel xl: one-hot taps 258 x 259 exact")


# ------------------------------------------------------------------------------------------------------------ child process
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xl_layer_child.py")


@pytest.mark.parametrize("geometry", ["default", "8"])
def test_xl_layer_edge_sizes_in_a_child_process(cuda_device, geometry):
    """NESR_BF16_KERNEL is read once per process: the small sizes run the large-tile kernel in a child of their own.  One run, no
    retry; a signal, a time limit or a non-zero status is a failure, and the child starts nothing after its first failure.
    The identity entry reports the kernel family only: that NESR_XL_GEOMETRY=8 selected the 8-wave instantiations is not
    verified here -- were the variable ignored or renamed, that run would pass on the default geometry."""
    env = dict(os.environ, NESR_BF16_KERNEL="xl")
    args = [sys.executable, CHILD]
    if geometry == "8":
        env["NESR_XL_GEOMETRY"] = "8"
        args.append("--reduced")
    else:
        env.pop("NESR_XL_GEOMETRY", None)
    done = subprocess.run(args, env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(done.stdout)
    assert done.returncode == 0, f"child ended with {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-2000:]}"
    lines = [json.loads(ln) for ln in done.stdout.splitlines() if ln.startswith("{")]
    cases = [ln for ln in lines if "case" in ln]
    assert cases and all(ln["ok"] and ln["kernel"] == "xl" for ln in cases)
    assert len(cases) == lines[-1]["cases"] and lines[-1]["done"]
