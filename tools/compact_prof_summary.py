"""Per-kernel share of the binding bound for SRVGGNetCompact, from a `rocprofv3 --kernel-trace --stats` kernel_stats.csv of
`tools/bench_compact.py` on ONE whole-frame case (no tiling: every launch of a kernel has the frame's geometry).

    python tools/compact_prof_summary.py STATS.csv --dtype bf16|f32 --h 1080 --w 1920 [--upscale 4] [--key NAME] [--out F.json]

Bounds (chip level): 2.5 PFLOP/s dense bf16 / f16 MFMA, the f32 form issuing three f16 MFMAs per product; 8 TB/s HBM.
FLOPs are the arithmetic the kernel issues (the first conv's 3 input channels padded to 32, the x2 tail's 12 outputs to 16);
bytes are each map read once and written once (halo re-reads come from L2).
"""
from __future__ import annotations

import argparse
import csv
import json
import os

PEAK, HBM = 2.5e15, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stats")
    ap.add_argument("--dtype", required=True, choices=["bf16", "f32"])
    ap.add_argument("--h", type=int, required=True)
    ap.add_argument("--w", type=int, required=True)
    ap.add_argument("--upscale", type=int, default=4)
    ap.add_argument("--key", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    px = a.h * a.w
    e = 4 if a.dtype == "f32" else 2
    mul = 3 if a.dtype == "f32" else 1
    tail_c = 48 if a.upscale == 4 else 16
    out_bytes = 3 * a.upscale ** 2   # u8 result (forward_u8, what enhance() runs)
    # kernel name fragment -> (issued FLOPs, bytes)
    model = {
        "compact_pack_kernel": (0.0, px * (3 + 32 * e + 16)),
        "compact_conv_kernel<{s}, 32, 4, false>": (2 * 9 * 32 * 64 * px, px * (32 + 64) * e),
        "compact_conv_kernel<{s}, 64, 4, false>": (2 * 9 * 64 * 64 * px, px * 128 * e),
        "compact_conv_kernel<{s}, 64, {t}, true>": (2 * 9 * 64 * tail_c * px, px * (64 * e + 16 + out_bytes)),
    }
    split = "true" if a.dtype == "f32" else "false"
    rows = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            for frag, (flop, byt) in model.items():
                frag = frag.format(s=split, t=3 if a.upscale == 4 else 1)
                if frag in r["Name"]:
                    us = float(r["AverageNs"]) / 1e3
                    t_f, t_b = flop * mul / PEAK * 1e6, byt / HBM * 1e6
                    bound = max(t_f, t_b)
                    rows[frag] = {"calls": int(r["Calls"]), "us_per_launch": round(us, 1), "mfma_bound_us": round(t_f, 1),
                                  "hbm_bound_us": round(t_b, 1), "binding": "mfma" if t_f >= t_b else "hbm",
                                  "share_of_bound": round(bound / us, 3)}
    res = {"case": a.key or f"{a.dtype} {a.h}x{a.w} x{a.upscale}", "kernels": rows}
    print(json.dumps(res))
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else []
        old = [o for o in old if o["case"] != res["case"]] + [res]
        with open(a.out, "w") as f:
            json.dump(old, f, indent=1)


if __name__ == "__main__":
    main()
