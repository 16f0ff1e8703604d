"""Swin2SR's fp16 compute form against the f32 form: upscale() on device-resident u8 frames, the two forms alternating call by
call.  Writes profiles/swin2sr/bench_swin2sr_f16.json.

    python tools/bench_swin2sr_f16.py [--frames 64x64,256x256,512x512] [--reps 9] [--warmup 2] [--out F]

Configuration and conventions are tools/bench_swin2sr.py's: classical x2 (embed 180, six stages of six layers, window 8,
pixelshuffle), random seeded weights, u8 HWC on the device in and out, event-timed calls, medians with min .. max of `reps` calls
after `warmup` calls of each form.  The f32 form is the parent commit's path (the sha256 of its 64 x 64 result is recorded and is
the one of profiles/swin2sr/bench_swin2sr_tiled.json).  The fp16 form's calls wait for the stream to read the range word; that wait is
inside its time.  Per form and frame, one extra call with the per-group event timing on gives the kernel groups' times.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(embed_dim=180, depths=(6,) * 6, num_heads=(6,) * 6, window_size=8, upsampler="pixelshuffle", upscale=2, image_size=64)


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(v):
    s = sorted(v)
    return {"median_ms": round(s[len(s) // 2], 3), "min_max_ms": [round(s[0], 3), round(s[-1], 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64x64,256x256,512x512")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin2sr", "bench_swin2sr_f16.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_swin2sr_f16.py needs the GPU (ROCm device); there is no CPU measurement")
    from neural_enhanced_super_resolution_amd import Swin2SR
    from tests import swin2sr_ref as R
    dev = torch.device("cuda:0")
    sd = R.seeded_state_dict(seed=7, **CFG)
    models = {}
    for form in ("f32", "fp16"):
        models[form] = Swin2SR(compute_dtype=form, **CFG).to(dev)
        models[form].load_state_dict(sd)
    out = {"device": torch.cuda.get_device_name(0), "config": "classical x2: embed 180, 6 x 6 layers, 6 heads, window 8, pixelshuffle, random weights",
           "reps": args.reps, "warmup": args.warmup, "frames": []}
    for spec in args.frames.split(","):
        w, h = (int(v) for v in spec.lower().split("x"))
        frame = torch.from_numpy(R.seeded_frame(h, w, seed=11)).to(dev)
        for _ in range(args.warmup):
            for m in models.values():
                m.upscale(frame)
        times = {k: [] for k in models}
        for _ in range(args.reps):
            for k, m in models.items():
                times[k].append(_timed(lambda: m.upscale(frame))[0])
        row = {"frame": f"{w}x{h}"}
        results = {}
        for k, m in models.items():
            m.set_kernel_timing(True)
            m.kernel_time_ms()
            results[k] = m.upscale(frame)
            kt = m.kernel_time_ms()
            m.set_kernel_timing(False)
            row[k] = dict(_stats(times[k]), launches=kt["launches"], groups_ms={g: round(v, 3) for g, v in kt["groups"].items()})
        row["fp16_over_f32"] = round(row["fp16"]["median_ms"] / row["f32"]["median_ms"], 3)
        diff = (results["fp16"].to(torch.int16) - results["f32"].to(torch.int16)).abs()
        row["u8_largest_difference"] = int(diff.max())
        row["u8_share_differing"] = round(float((diff > 0).float().mean()), 5)
        if (w, h) == (64, 64):
            row["f32_sha256"] = hashlib.sha256(results["f32"].cpu().numpy().tobytes()).hexdigest()
        print(json.dumps(row), flush=True)
        out["frames"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
