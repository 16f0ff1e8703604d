"""The NESR pipeline's ESRGAN stage (nesr_adapter.apply_esrgan, device frame in, device frame out) on its two routes, alternating in
one process: use_hip=False (the torch chains: 12-channel synthesis, float output, quantiser, Python tile loop) and use_hip=None (one
call of the C ABI: nesr_apply_esrgan_u8).  Writes profiles/nesr_stage/bench.json.

    python tools/bench_nesr_stage.py [--rounds R] [--blocks B] [--only NAME] [--commit SHA] [--out F]

Cases: the reference's RRDBNet(num_in_ch=12) with seeded weights as f32 at 512 x 512 untiled, at 1024 x 1024 with tile 512 (the second
iteration of bench.py --workload c5) and at 2048 x 2048 untiled, and as bf16 at 2048 x 2048 untiled.  Per case one warm-up call of each
route, then `rounds` rounds of (torch route, HIP route), wall clock around the call between two torch.cuda.synchronize(); the median per
route, the spread (max - min) of the torch route's own timed calls, torch.cuda.max_memory_allocated per route (the context's workspace is
not torch's and is the same on both), and a bitwise comparison of the two results.  The network dominates the stage: the HIP route counts
as slower only if its median exceeds the torch route's by more than that spread; the peak memory is the figure the route changes."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("f32 512x512 untiled 12-channel", "f32", 512, {"enable_tiling": False}),
         ("f32 1024x1024 tile 512 12-channel", "f32", 1024, {"max_tile_size": 512, "cuda_megapixel_threshold": 0.5}),
         ("f32 2048x2048 untiled 12-channel", "f32", 2048, {"enable_tiling": False}),
         ("bf16 2048x2048 untiled 12-channel", "bf16", 2048, {"enable_tiling": False}))


def _commit(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=23)
    ap.add_argument("--only", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nesr_stage", "bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_nesr_stage.py needs the GPU (ROCm device); there is no CPU measurement")
    from neural_enhanced_super_resolution_amd import RRDBNet, nesr_adapter as A
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    dev = torch.device("cuda:0")
    sd = synthetic_state_dict(seed=3, num_in_ch=12, scale=4, num_block=args.blocks)
    ups, rows = {}, []
    for name, form, side, cfg in CASES:
        if args.only and args.only not in name:
            continue
        if form not in ups:
            class Up:
                model, device = RRDBNet(12, 3, num_block=args.blocks, compute_dtype=form), dev
            Up.model.load_state_dict(sd)
            Up.model.to(dev)
            ups[form] = Up
        up = ups[form]
        frame = torch.from_numpy(np.ascontiguousarray(synthetic_frame(side, side, seed=4)[:, :, ::-1])).to(dev)
        t, peak, outs, traces = {False: [], None: []}, {False: 0, None: 0}, {}, {False: [], None: []}
        for rnd in range(args.rounds + 1):                   # round 0 warms both routes up (context, workspace, resize tables, allocator)
            for route in (False, None):
                outs.pop(route, None)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                t0 = time.perf_counter()
                outs[route] = A.apply_esrgan(up, frame, cfg, as_numpy=False, trace=traces[route], use_hip=route)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rnd:
                    t[route].append(dt)
                    peak[route] = max(peak[route], torch.cuda.max_memory_allocated(dev) - before)
        up.model.check_range()
        chain, hip = float(np.median(t[False])), float(np.median(t[None]))
        spread = max(t[False]) - min(t[False])
        row = {"case": name, "blocks": args.blocks, "frame": list(frame.shape), "out": list(outs[None].shape), "tiles": traces[None][-1]["model_calls"],
               "torch_route_ms": round(chain, 2), "hip_route_ms": round(hip, 2), "torch_route_calls_ms": [round(v, 2) for v in t[False]],
               "hip_route_calls_ms": [round(v, 2) for v in t[None]], "torch_route_spread_ms": round(spread, 2), "speedup": round(chain / hip, 4),
               "hip_route_slower_beyond_spread": bool(hip - chain > spread),
               "torch_route_peak_bytes": int(peak[False]), "hip_route_peak_bytes": int(peak[None]),
               "bitwise_equal": bool(torch.equal(outs[None], outs[False])), "trace_equal": traces[None][-1] == traces[False][-1]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del outs, frame
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "commit": _commit(args.commit), "rounds": args.rounds,
              "timing": "time.perf_counter around apply_esrgan(as_numpy=False) between two torch.cuda.synchronize(); one warm-up call per route, then "
                        "the routes alternate call by call; median per route; spread = max - min of the torch route's timed calls",
              "memory": "torch.cuda.max_memory_allocated during the call minus memory_allocated before it (the frame and the other route's result stay "
                        "resident), the largest over the timed calls; the context's workspace is outside torch's allocator and equal on both routes",
              "comparison": "nesr_adapter.apply_esrgan(use_hip=False) against use_hip=None, in one process",
              "any_hip_route_slower_beyond_spread": any(r["hip_route_slower_beyond_spread"] for r in rows),
              "all_bitwise_equal": all(r["bitwise_equal"] for r in rows), "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
