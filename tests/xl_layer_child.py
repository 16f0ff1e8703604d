"""Body of test_gpu_conv_xl.py's child-process tests: a plain script, started once per parametrisation with
NESR_BF16_KERNEL=xl in its environment (the variable is read once per process), optionally NESR_XL_GEOMETRY=8.

Runs the per-value pin of tests/conv_pin.py on the large-tile kernel at the sizes where its edge bookkeeping lives, prints one
JSON line per case and exits non-zero at the first failure (nothing is launched after it).  --reduced: the short list of the
8-wave geometry."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import conv_pin  # noqa: E402

# smaller than a tile; fewer than 4 rows (wave 0 alone); a tile less one, a tile, a tile plus one; ragged; one long row of tiles
SIZES = [(1, 1), (2, 3), (3, 40), (7, 5), (15, 31), (16, 32), (17, 33), (33, 47), (16, 130)]
REDUCED = [(17, 33), (33, 47), (16, 130)]
CHANNELS = [(64, 32), (64, 64)]


def say(**kw):
    print(json.dumps(kw), flush=True)


def main():
    from neural_enhanced_super_resolution_amd import conv3x3, last_conv_kernel
    reduced = "--reduced" in sys.argv[1:]
    if os.environ.get("NESR_BF16_KERNEL") != "xl":
        say(error="NESR_BF16_KERNEL=xl must be set before this process starts")
        return 2
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    dev = torch.device("cuda:0")
    pool = conv_pin.MissPool()
    cases = 0

    def layer(cin, cout, hw, dtype, lrelu, up):
        x, wt, b = conv_pin.make_case(cin, cout, hw[0], hw[1], dtype, seed=cin * 7 + cout + 1000 * hw[0] + hw[1], n=2)
        y = conv3x3(x.to(dev), wt, b, lrelu=lrelu, upsample=up, dtype=dtype).cpu()
        ran = last_conv_kernel()
        pre, mag = conv_pin.conv_f64(x, wt, b, up)
        fig = conv_pin.pin(y, pre, mag, cin, lrelu, dtype)
        ok = ran == "xl" and fig["finite"] and fig["outside"] == 0 and fig["missed"] <= conv_pin.miss_allowance(fig["values"], dtype)
        say(case=f"{dtype} {cin}->{cout} {hw[0]}x{hw[1]} lrelu {int(lrelu)} up {int(up)}", kernel=ran, ok=ok, **fig)
        pool.add(dtype, fig)
        return ok

    for hw in (REDUCED if reduced else SIZES):
        for cin, cout in CHANNELS:
            for dtype in ("bf16", "f16"):
                for lrelu in (False, True):
                    cases += 1
                    if not layer(cin, cout, hw, dtype, lrelu, False):
                        return 1
    if not reduced:
        cases += 1
        if not layer(64, 64, (13, 21), "bf16", True, True):
            return 1
    for tap in range(9):
        x, wt, b, ref = conv_pin.one_hot_case(32, 64, 10, 12, tap)
        got = conv3x3(x.to(dev), wt, b, dtype="bf16").cpu()
        ran = last_conv_kernel()
        ok = ran == "xl" and torch.equal(got, ref)
        cases += 1
        say(case=f"one-hot tap {tap} 10x12", kernel=ran, ok=ok)
        if not ok:
            return 1
    shares = pool.shares()
    capped = all(shares[d] <= conv_pin.MISS_CAP[d] for d in shares)
    say(done=capped, cases=cases, pooled_miss=shares)
    return 0 if capped else 1


if __name__ == "__main__":
    sys.exit(main())
