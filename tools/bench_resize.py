"""The cv2 resizes (imgproc.lanczos4_resize, linear_resize_f32), each case timed as the torch chain (use_hip=False) and as the HIP
kernel (csrc/resize.hip), the two alternating in one session, with a check of the two against each other at every timed size.
Writes profiles/resize/bench_resize.json.

    python tools/bench_resize.py [--reps N] [--rounds R] [--out F] [--enhance] [--only NAME]

Cases: u8 RGB 4320 x 7680 -> 3240 x 5760 and -> 6480 x 11520 (enhance(outscale=1.5 | 3) on the 2160p frame through the x2 model);
2112^2 -> 1024^2 and 2176^2 -> 1024^2 (the tiler's regions of the forced-tiling route); u16 RGB 2160 x 3840 -> 3240 x 5760; one f32
plane 1080 x 1920 -> x4.  Per case: the median of `reps` event-timed calls per round, `rounds` rounds alternating chain / kernel, the
spread of the chain's round medians (its A/A), bytes read + written once, and the share of the HBM bound (8 TB/s: arithmetic).
--enhance adds RealESRGANer.enhance of the 2160p frame (bf16, tile 512 / 10), host u8 -> host u8, with outscale 1.5 and 3, the HIP
resize on and off (realesrganer.HIP_RESIZE) alternating."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

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
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--enhance", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize", "bench_resize.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize.py needs the GPU (ROCm device); there is no CPU measurement")
    from neural_enhanced_super_resolution_amd import imgproc as P
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    cases = [("u8 rgb outscale 1.5", "u8", (4320, 7680, 3), (3240, 5760)), ("u8 rgb outscale 3", "u8", (4320, 7680, 3), (6480, 11520)),
             ("u8 rgb tiler 2112", "u8", (2112, 2112, 3), (1024, 1024)), ("u8 rgb tiler 2176", "u8", (2176, 2176, 3), (1024, 1024)),
             ("u16 rgb 2160p x1.5", "u16", (2160, 3840, 3), (3240, 5760)), ("f32 plane 1080p x4", "f32", (1080, 1920), (4320, 7680))]
    rows = []
    for name, kind, shape, (oh, ow) in cases:
        if args.only and args.only not in name:
            continue
        if kind == "u8":
            img = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(dev)
        elif kind == "u16":
            img = torch.randint(0, 65536, shape, dtype=torch.int32, generator=g).to(dev)
        else:
            img = torch.rand(shape, generator=g).to(dev)
        fn = P.linear_resize_f32 if kind == "f32" else P.lanczos4_resize
        esize = {"u8": 1, "u16": 2, "f32": 4}[kind]
        chain, hip = (lambda: fn(img, oh, ow, use_hip=False)), (lambda: fn(img, oh, ow, use_hip=True))
        want, got = chain(), hip()                       # also the warm-up of both (tables, allocator)
        diff = int((want.to(torch.float64) - got.to(torch.float64)).abs().max().item())
        del want, got
        t_chain, t_hip = [], []
        for _ in range(args.rounds):
            t_chain.append(_median_ms(chain, args.reps))
            t_hip.append(_median_ms(hip, args.reps))
        torch.cuda.empty_cache()
        c = shape[2] if len(shape) == 3 else 1
        moved = (shape[0] * shape[1] + oh * ow) * c * esize
        bound_ms = moved / (HBM_TBPS * 1e12) * 1e3
        mc, mh = sorted(t_chain)[len(t_chain) // 2], sorted(t_hip)[len(t_hip) // 2]
        row = {"case": name, "src": list(shape), "dst": [oh, ow], "chain_ms": round(mc, 3), "hip_ms": round(mh, 4),
               "chain_rounds_ms": [round(v, 3) for v in t_chain], "hip_rounds_ms": [round(v, 4) for v in t_hip],
               "chain_aa_spread_ms": round(max(t_chain) - min(t_chain), 3), "speedup": round(mc / mh, 1), "max_abs_diff": diff,
               "hbm_bytes": moved, "hbm_bound_ms": round(bound_ms, 4), "share_of_hbm_bound": round(bound_ms / mh, 3),
               "hip_faster_beyond_spread": bool(mc - mh > max(t_chain) - min(t_chain))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del img
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": args.reps, "rounds": args.rounds,
              "timing": "hipEvents around one call on an otherwise idle stream; median of reps per round; chain and kernel alternate by round",
              "cases": rows}
    if args.enhance:
        from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, realesrganer as R
        from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
        sd = synthetic_state_dict(seed=3, num_in_ch=3, scale=2, num_block=23)
        up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=23), tile=512, tile_pad=10, pre_pad=0,
                          half=True, device=dev)
        frame = synthetic_frame(2160, 3840, seed=4)
        ends = []
        for s in (1.5, 3.0):
            t = {True: [], False: []}
            outs = {}
            for rnd in range(args.rounds + 1):           # round 0 warms both up
                for on in (False, True):
                    R.HIP_RESIZE = on
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    outs[on], _ = up.enhance(frame, outscale=s)
                    dt = (time.perf_counter() - t0) * 1e3
                    if rnd:
                        t[on].append(dt)
            R.HIP_RESIZE = True
            row = {"enhance_outscale": s, "frame": [2160, 3840, 3], "hip_resize_ms": [round(v, 1) for v in t[True]],
                   "host_chain_ms": [round(v, 1) for v in t[False]], "bitwise_equal": bool((outs[True] == outs[False]).all())}
            ends.append(row)
            print(json.dumps(row), flush=True)
        result["enhance"] = ends
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
