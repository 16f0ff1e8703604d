"""RealESRGANer(devices=[...]) from one process: host u8 -> host u8 frames/s of the in-process multi-device mode.

    python tools/bench_devices.py [--steps 10] [--warmup 3] [--shared 2,3,4,8] [--many-frames 8] [--inflight 2]
                                  [--timeout 300] [--out profiles/devices/bench_devices.json]

  c3    3840x2160 RealESRGAN_x2plus bf16 (half=True), tile 512 / pad 10: enhance() with the tiles split over the devices
  many  1920x1080 RealESRGAN_x2plus bf16, untiled (tile=0): enhance_many() of --many-frames frames, frame i to devices[i % n]

Device lists: devices=None (the one-device wrapper), the first k visible devices for k = 2 .. N, and [0] * k for every k in
--shared (k contexts sharing one GPU: the cost of the split when the device is shared).  Every case runs in a child process
of its own under --timeout seconds; after a failure or a time-out no further case is started.  A case reports the median
of --steps timed steps after --warmup untimed ones (c3: one frame per step; many: --many-frames frames per step) and checks
its output bit for bit against devices=None.  With one visible GPU there is no scaling number, and the JSON says so.
Weights are seeded synthetic (synth.py).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_case(spec):
    import numpy as np
    import torch

    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict

    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2)

    def make(devices):
        return RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2), tile=512 if spec["case"] == "c3" else 0,
                            tile_pad=10, pre_pad=0, half=True, device="cuda:0", devices=devices)

    if spec["case"] == "c3":
        frames = [synthetic_frame(2160, 3840, seed=0)]
        step = lambda up: [up.enhance(frames[0])[0]]                          # noqa: E731
    else:
        frames = [synthetic_frame(1080, 1920, seed=i) for i in range(spec["many_frames"])]
        step = lambda up: [o for o, _ in up.enhance_many(frames, inflight=spec["inflight"])]   # noqa: E731
    up = make(spec["devices"])
    got = step(up)
    bitwise = None
    if spec["devices"] is not None:
        ref = make(None)
        want = step(ref)
        bitwise = all(np.array_equal(a, b) for a, b in zip(got, want))
        del ref
    for _ in range(spec["warmup"]):
        step(up)
    times = []
    for _ in range(spec["steps"]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(up)
        times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    return {"case": spec["case"], "devices": spec["devices"], "frames_per_step": len(frames), "steps": spec["steps"],
            "warmup": spec["warmup"], "median_ms": round(med * 1e3, 2), "min_ms": round(min(times) * 1e3, 2),
            "max_ms": round(max(times) * 1e3, 2), "frames_per_s": round(len(frames) / med, 3), "bitwise_vs_one_device": bitwise,
            "gpu": torch.cuda.get_device_name(0), "visible_devices": torch.cuda.device_count()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shared", default="2,3,4,8", help="k of the [0] * k lists")
    ap.add_argument("--many-frames", type=int, default=8)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--cases", default="c3,many")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "devices", "bench_devices.json"))
    ap.add_argument("--one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run_case(json.loads(a.one))), flush=True)
        return

    import torch
    n = torch.cuda.device_count()
    lists = [None] + [list(range(k)) for k in range(2, n + 1)] + [[0] * int(k) for k in a.shared.split(",") if k]
    results, failed = [], None
    for case in a.cases.split(","):
        for devices in lists:
            spec = {"case": case, "devices": devices, "steps": a.steps, "warmup": a.warmup, "many_frames": a.many_frames,
                    "inflight": a.inflight}
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", json.dumps(spec)], capture_output=True,
                                   text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                failed = {"spec": spec, "error": f"timed out after {a.timeout} s"}
                break
            if p.returncode != 0:
                failed = {"spec": spec, "error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
                break
            r = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(r), flush=True)
            results.append(r)
        if failed:
            break
    base = {r["case"]: r["frames_per_s"] for r in results if r["devices"] is None}
    for r in results:
        if r["case"] in base:
            r["vs_one_device"] = round(r["frames_per_s"] / base[r["case"]], 4)
    out = {"tool": "tools/bench_devices.py", "visible_devices": n, "results": results,
           "scaling": ("unmeasured: one visible GPU, no k-device number exists" if n < 2 else
                       {c: {len(r["devices"]): r["vs_one_device"] for r in results if r["case"] == c and r["devices"] and len(set(r["devices"])) > 1}
                        for c in base})}
    if failed:
        out["failed"] = failed
        print(json.dumps(failed), file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
