"""The stages of enhance_image's loop around its networks (imgproc.resize_u8, segment_enhance, ensemble_results), each timed as the
HIP kernel (csrc/resize.hip, csrc/filters.hip) and as the torch chain (use_hip=False) in one session, with a check of the two
against each other at every size where the chain runs.  Writes profiles/stages/bench_stages.json.

    python tools/bench_stages.py [--sizes 2048,8192,16384] [--reps 7] [--chain-max 8192] [--only NAME] [--out F]

Cases per size S (an S x S RGB u8 frame): the four resizes x2 up and /2 down (INTER_LINEAR /2 is cv2's area switch), the mask stage
from a 128 x 128 mask, the ensemble of 2.  Per case: the median of `reps` event-timed calls of the kernel route, the bytes the entry
must move (source read once + destination written once; the mask stage also writes and reads its H x W mask), the share of the HBM
bound (8 TB/s: arithmetic), and the chain timed the same way -- one call where S > 2048 (its int64 intermediates make it slow), none
where S > --chain-max (recorded as null)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 8.0          # MI355X peak HBM bandwidth, TB/s


def _median_ms(fn, reps):
    import torch
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        del out
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chain-max", type=int, default=8192)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stages", "bench_stages.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stages.py needs the GPU (ROCm device); there is no CPU measurement")
    from neural_enhanced_super_resolution_amd import imgproc as P
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    rows = []
    for S in [int(v) for v in args.sizes.split(",")]:
        img = torch.randint(0, 256, (S, S, 3), dtype=torch.uint8, generator=g).to(dev)
        other = img.flip(0).contiguous()
        seg = (torch.rand((128, 128), generator=g) > 0.5).to(torch.int64).to(dev)
        cases = []
        for name, interp in (("nearest", P.INTER_NEAREST), ("linear", P.INTER_LINEAR), ("cubic", P.INTER_CUBIC), ("lanczos4", P.INTER_LANCZOS4)):
            for tag, o in (("x2", 2 * S), ("/2", S // 2)):
                cases.append((f"resize {name} {tag}", (lambda hip, i=interp, o=o: P.resize_u8(img, o, o, i, use_hip=hip)), 3 * (S * S + o * o)))
        cases.append(("segment_enhance mask 128", (lambda hip: P.segment_enhance(img, seg, use_hip=hip)), 3 * S * S * 2 + 128 * 128 + 2 * S * S))
        cases.append(("ensemble of 2", (lambda hip: P.ensemble_results([img, other], use_hip=hip)), 3 * S * S * 3))
        for name, fn, moved in cases:
            if args.only and args.only not in name:
                continue
            got = fn(True)                                   # also the warm-up (tables, allocator)
            hip_ms = _median_ms(lambda: fn(True), args.reps)
            chain_ms, equal, chain_reps = None, None, 0
            if S <= args.chain_max:
                try:
                    want = fn(False)
                    equal = bool(torch.equal(got, want))
                    del want
                    chain_reps = args.reps if S <= 2048 else 1
                    chain_ms = round(_median_ms(lambda: fn(False), chain_reps), 3)
                except torch.OutOfMemoryError:
                    chain_ms, equal, chain_reps = None, None, -1     # -1: the chain did not fit the device
            del got
            torch.cuda.empty_cache()
            bound_ms = moved / (HBM_TBPS * 1e12) * 1e3
            row = {"case": name, "side": S, "hip_ms": round(hip_ms, 4), "hbm_bytes": moved, "hbm_bound_ms": round(bound_ms, 4),
                   "share_of_hbm_bound": round(bound_ms / hip_ms, 3), "chain_ms": chain_ms, "chain_reps": chain_reps, "bitwise_equal": equal}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del img, other, seg
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": args.reps,
              "timing": "hipEvents around one call on an otherwise idle stream, output allocation included; median of reps", "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
