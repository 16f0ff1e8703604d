"""Swin2SR.upscale(tile=, tile_pad=) against the untiled upscale() on device-resident u8 frames, and the untiled path by itself
(what the batch dimension of the kernels costs it).  Writes profiles/swin2sr/bench_swin2sr_tiled.json.

    python tools/bench_swin2sr_tiled.py [--mode all|untiled|tiled] [--root DIR] [--baseline A.json,B.json] [--out F]
                                        [--untiled-frames 64x64,256x256,512x512] [--frames 512x512,1024x1024] [--tiles 64,128,256]
                                        [--pad 16] [--large 2048x2048,4096x4096] [--large-tile 256] [--reps 9] [--warmup 2] [--large-reps 3]

Configuration and conventions are tools/bench_swin2sr.py's: classical x2 (embed 180, six stages of six layers, window 8,
pixelshuffle), random seeded weights, u8 HWC on the device in and out, event-timed calls, medians with min .. max of `reps` calls
after `warmup` calls of each route, the routes of a frame taken alternately call by call.

  untiled   upscale(frame) per frame, and the sha256 of the 64 x 64 result.  `--root DIR` imports the package of another checkout
            (one built from an earlier commit, say) instead of this tree's: run it there and here in turn in one session and hand
            the files to `--baseline`; they are kept in the output next to this tree's figures.
  tiled     per frame and tile: untiled, tiled with max_batch = 1 and tiled with the default batch, alternating; the pixel overhead
            ((T + 2 P) / T)^2, tiles, windows a batch, launches, workspace bytes; whether the two tiled results are equal and the
            share of samples in which they differ from the untiled frame (seams are expected: a window sees less context).
  large     frames the untiled path is not asked to do: tiled time (fewer reps) and workspace.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(embed_dim=180, depths=(6,) * 6, num_heads=(6,) * 6, window_size=8, upsampler="pixelshuffle", upscale=2, image_size=64)
BUDGET = 2 << 30          # NESR_SWIN2SR_TILE_WORKSPACE_BYTES (include/nesr_hip.h)


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


def _alternate(routes, reps, warmup):
    """{name: times} of the callables of `routes`, one call of each in turn."""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            times[k].append(_timed(fn)[0])
    return times


def _sizes(text):
    return [tuple(int(v) for v in spec.lower().split("x")) for spec in text.split(",") if spec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=("all", "untiled", "tiled"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--baseline", default="")
    ap.add_argument("--untiled-frames", default="64x64,256x256,512x512")
    ap.add_argument("--frames", default="512x512,1024x1024")
    ap.add_argument("--tiles", default="64,128,256")
    ap.add_argument("--pad", type=int, default=16)
    ap.add_argument("--large", default="2048x2048,4096x4096")
    ap.add_argument("--large-tile", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--large-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin2sr", "bench_swin2sr_tiled.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_swin2sr_tiled.py needs the GPU (ROCm device); there is no CPU measurement")
    from neural_enhanced_super_resolution_amd import Swin2SR
    from tests import swin2sr_ref as R
    dev = torch.device("cuda:0")
    model = Swin2SR(**CFG).to(dev)
    model.load_state_dict(R.seeded_state_dict(seed=7, **CFG))
    frame_of = lambda w, h: torch.from_numpy(R.seeded_frame(h, w, seed=11)).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "config": "classical x2: embed 180, 6 x 6 layers, 6 heads, window 8, pixelshuffle, random weights",
           "root": "this tree" if os.path.abspath(args.root) == ROOT else "another checkout (--root)", "reps": args.reps, "warmup": args.warmup,
           "quality": "unmeasured: seams and PSNR against the untiled frame need a real checkpoint, and none is at hand; with random weights only "
                      "the share of differing samples is reported"}

    if args.mode in ("all", "untiled"):
        rows = []
        for w, h in _sizes(args.untiled_frames):
            frame = frame_of(w, h)
            t = _alternate({"untiled": lambda: model.upscale(frame)}, args.reps, args.warmup)
            row = {"frame": f"{w}x{h}", **_stats(t["untiled"])}
            if (w, h) == (64, 64):
                row["sha256"] = hashlib.sha256(model.upscale(frame).cpu().numpy().tobytes()).hexdigest()
            print(json.dumps(row), flush=True)
            rows.append(row)
        out["untiled"] = rows
    if args.baseline:
        out["untiled_baseline_runs"] = []
        for path in args.baseline.split(","):
            with open(path) as f:
                out["untiled_baseline_runs"].append({"file": os.path.basename(path), "rows": json.load(f)["untiled"]})

    def batch_for(win, tiles):
        per = model.workspace_bytes(win[0], win[1], 1)
        b = max(1, min(tiles, BUDGET // per))
        while b > 1 and model.workspace_bytes(win[0], win[1], b) > BUDGET:
            b -= 1
        return b

    def launches_of(fn):
        model.kernel_time_ms()
        fn()
        return model.kernel_time_ms()["launches"]

    if args.mode in ("all", "tiled"):
        rows = []
        for w, h in _sizes(args.frames):
            frame = frame_of(w, h)
            for T in (int(v) for v in args.tiles.split(",")):
                p = model.tile_plan(h, w, T, args.pad)
                tiles, win = p["tiles"][0] * p["tiles"][1], p["window"]
                b = batch_for(win, tiles)
                routes = {"untiled": lambda: model.upscale(frame), "tiled_batch_1": lambda: model.upscale(frame, tile=T, tile_pad=args.pad, max_batch=1),
                          "tiled_default": lambda: model.upscale(frame, tile=T, tile_pad=args.pad)}
                t = _alternate(routes, args.reps, args.warmup)
                whole, one, many = (fn() for fn in routes.values())
                row = {"frame": f"{w}x{h}", "tile": T, "tile_pad": args.pad, "pixel_overhead": round(((T + 2 * args.pad) / T) ** 2, 3), "tiles": tiles,
                       "window": list(win), "default_batch": b, "workspace_bytes_default": model.workspace_bytes(win[0], win[1], b),
                       "workspace_bytes_batch_1": model.workspace_bytes(win[0], win[1], 1), "workspace_bytes_untiled": model.workspace_bytes(h, w, 1),
                       "launches_batch_1": launches_of(routes["tiled_batch_1"]), "launches_default": launches_of(routes["tiled_default"]),
                       "untiled": _stats(t["untiled"]), "tiled_batch_1": _stats(t["tiled_batch_1"]), "tiled_default": _stats(t["tiled_default"]),
                       "batches_equal": bool(torch.equal(one, many)), "share_differing_from_untiled": round(float((many != whole).float().mean()), 4)}
                row["default_over_batch_1"] = round(row["tiled_default"]["median_ms"] / row["tiled_batch_1"]["median_ms"], 3)
                row["default_over_untiled"] = round(row["tiled_default"]["median_ms"] / row["untiled"]["median_ms"], 3)
                print(json.dumps(row), flush=True)
                rows.append(row)
        out["tiled"] = rows
        rows = []
        for w, h in _sizes(args.large):
            frame = frame_of(w, h)
            T = args.large_tile
            p = model.tile_plan(h, w, T, args.pad)
            tiles, win = p["tiles"][0] * p["tiles"][1], p["window"]
            b = batch_for(win, tiles)
            fn = lambda: model.upscale(frame, tile=T, tile_pad=args.pad)
            t = _alternate({"tiled_default": fn}, args.large_reps, 1)
            row = {"frame": f"{w}x{h}", "tile": T, "tile_pad": args.pad, "pixel_overhead": round(((T + 2 * args.pad) / T) ** 2, 3), "tiles": tiles,
                   "window": list(win), "default_batch": b, "workspace_bytes_default": model.workspace_bytes(win[0], win[1], b), "reps": args.large_reps,
                   "launches_default": launches_of(fn), "tiled_default": _stats(t["tiled_default"])}
            print(json.dumps(row), flush=True)
            rows.append(row)
        out["large"] = rows

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
