"""RealESRGANer(half=True) in its two 16-bit forms on one MI355X: the default bf16 model against RRDBNet(compute_dtype="f16")
(upstream's fp16 numerics), interleaved in one process, host u8 -> host u8.

    python tools/bench_half.py [--rounds 6] [--warmup 2] [--frames c3,c4] [--out profiles/f16/bench_half.json]

  c3  3840x2160 RealESRGAN_x2plus, tile 512 / pad 10 (40 tiles: ragged batches through the LDS-resident dense-block kernel)
  c4  1920x1080 RealESRGAN_x4plus, tile 512 / pad 10 (12 tiles)

For each frame and form: frames/s (median of the rounds; the forms alternate which one goes first), and the u8 output against
the f32 form's (RealESRGANer(half=False), compute_dtype "f32"): PSNR (peak 255), max and mean abs difference in 8-bit levels.
Weights are seeded synthetic (synth.py).  Prints one JSON line per case and writes them all to --out.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet  # noqa: E402
from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict  # noqa: E402

FRAMES = {"c3": (2160, 3840, 2), "c4": (1080, 1920, 4)}     # height, width, scale; tile 512 / pad 10 for both


def upsampler(sd, scale, dtype, half):
    return RealESRGANer(scale=scale, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=scale, compute_dtype=dtype), tile=512,
                        tile_pad=10, pre_pad=0, half=half, device="cuda:0")


def compare(a, b):
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    mse = float((d.astype(np.float64) ** 2).mean())
    return {"psnr_db": round(10 * math.log10(255.0 ** 2 / mse), 2) if mse > 0 else float("inf"), "max_abs": int(d.max()),
            "mean_abs": round(float(d.mean()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", default="c3,c4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16", "bench_half.json"))
    args = ap.parse_args()
    results = []
    for name in args.frames.split(","):
        h, w, scale = FRAMES[name]
        sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=scale)
        frame = synthetic_frame(h, w, seed=0)
        ref, _ = upsampler(sd, scale, "f32", False).enhance(frame)
        ups = {"bf16": upsampler(sd, scale, "f32", True), "f16": upsampler(sd, scale, "f16", True)}
        assert ups["bf16"].model.compute_dtype == "bf16" and ups["f16"].model.compute_dtype == "f16"
        outs = {}
        for dt, up in ups.items():
            for _ in range(args.warmup):
                outs[dt], _ = up.enhance(frame)
        torch.cuda.synchronize()
        times = {dt: [] for dt in ups}
        for r in range(args.rounds):
            for dt in (("bf16", "f16") if r % 2 == 0 else ("f16", "bf16")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[dt], _ = ups[dt].enhance(frame)
                torch.cuda.synchronize()
                times[dt].append(time.perf_counter() - t0)
        for dt in ups:
            med = statistics.median(times[dt])
            rec = {"frame": name, "size": [h, w], "scale": scale, "tile": 512, "tile_pad": 10, "form": dt, "rounds": args.rounds,
                   "ms_median": round(med * 1e3, 2), "ms_min": round(min(times[dt]) * 1e3, 2), "frames_per_s": round(1.0 / med, 3),
                   "vs_f32": compare(outs[dt], ref)}
            results.append(rec)
            print(json.dumps(rec), flush=True)
        f16, bf = results[-1], results[-2]
        ratio = {"frame": name, "f16_over_bf16_frames_per_s": round(f16["frames_per_s"] / bf["frames_per_s"], 4)}
        results.append(ratio)
        print(json.dumps(ratio), flush=True)
        del ups
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
