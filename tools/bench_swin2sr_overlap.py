"""Swin2SR.upscale(tile=, tile_overlap=), the authors' overlapped tiles with averaged seams, against the untiled upscale() and the
tiled route upscale(tile=, tile_pad=) on device-resident u8 frames.  Writes profiles/swin2sr/bench_swin2sr_overlap.json.

    python tools/bench_swin2sr_overlap.py [--frames 512x512,1024x1024] [--tile 256] [--pad 16] [--overlaps 256:32,128:32]
                                          [--large 2048x2048] [--reps 9] [--warmup 2] [--large-reps 3] [--out F]

Configuration and conventions are tools/bench_swin2sr_tiled.py's: classical x2 (embed 180, six stages of six layers, window 8,
pixelshuffle), random seeded weights, u8 HWC on the device in and out, event-timed calls, medians with min .. max of `reps` calls
after `warmup` calls of each route, the routes of a frame taken alternately call by call, all in one session.

  rows    per frame: untiled, tiled at T / P, overlapped at each T:O; per route the time, the window count, the windows a batch,
          the launches and the workspace from the two query entries (nesr_swin2sr_workspace_bytes for a route that pads its
          windows, nesr_swin2sr_overlap_workspace_bytes for the overlapped one).
  share   of the two overlap kernels in an overlapped call, from the kernel timing: they count under the `upsample` group, so the
          group's time in one timed call, less the same group's time of forward_batch over batches of the same sizes (the network's
          own upsampling head, same kernels, same f32 output), is theirs; it is given in ms and as a share of the timed call's sum.
  large   frames the untiled path is not asked to do: the two tiled routes only, fewer reps.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_swin2sr_tiled import BUDGET, CFG, _alternate, _sizes, _stats      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="512x512,1024x1024")
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--pad", type=int, default=16)
    ap.add_argument("--overlaps", default="256:32,128:32")
    ap.add_argument("--large", default="2048x2048")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--large-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin2sr", "bench_swin2sr_overlap.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_swin2sr_overlap.py needs the GPU (ROCm device); there is no CPU measurement")
    from neural_enhanced_super_resolution_amd import Swin2SR
    from tests import swin2sr_ref as R
    dev = torch.device("cuda:0")
    model = Swin2SR(**CFG).to(dev)
    model.load_state_dict(R.seeded_state_dict(seed=7, **CFG))
    frame_of = lambda w, h: torch.from_numpy(R.seeded_frame(h, w, seed=11)).to(dev)
    overlaps = [tuple(int(v) for v in spec.split(":")) for spec in args.overlaps.split(",") if spec]
    out = {"device": torch.cuda.get_device_name(0), "config": "classical x2: embed 180, 6 x 6 layers, 6 heads, window 8, pixelshuffle, random weights",
           "reps": args.reps, "warmup": args.warmup,
           "quality": "unmeasured: seams against the untiled frame need a real checkpoint, and none is at hand; with random weights only the share "
                      "of differing samples is reported"}

    def launches_of(fn):
        model.kernel_time_ms()
        fn()
        return model.kernel_time_ms()["launches"]

    def fit(per_batch, n):
        """Windows a batch under the library's budget: per_batch(b) bytes, at least one, at most n."""
        b = max(1, min(n, BUDGET // per_batch(1)))
        while b > 1 and per_batch(b) > BUDGET:
            b -= 1
        return b

    def tiled_facts(h, w, T, P):
        p = model.tile_plan(h, w, T, P)
        n, win = p["tiles"][0] * p["tiles"][1], p["window"]
        b = fit(lambda k: model.workspace_bytes(win[0], win[1], k), n)
        return {"windows": n, "window": list(win), "batch": b, "workspace_bytes": model.workspace_bytes(win[0], win[1], b)}

    def overlap_facts(h, w, T, O):
        p = model.overlap_plan(h, w, T, O)
        n, t, s = p["tiles"][0] * p["tiles"][1], p["tile"], CFG["upscale"]
        px = p["padded"][0] * s * p["padded"][1] * s
        acc = -(-12 * (-(-px // 4) * 4) // 256) * 256            # the accumulator as the library sizes it: planes of a multiple of 4 floats, 256-byte granules
        b = fit(lambda k: model.overlap_workspace_bytes(h, w, T, O, k) - acc, n)      # the budget holds the per-batch part, not the accumulator
        # checked against the call's launch count: ceil(n / B) x (launches of one forward + 1) + 1
        per_forward = launches_of(lambda: model.forward_batch(torch.zeros(1, 3, t, t, device=dev)))
        batches = (launches_of(lambda: model.upscale(frame_of(w, h), tile=T, tile_overlap=O)) - 1) // (per_forward + 1)
        return {"windows": n, "window": [t, t], "batch": b, "batches": batches, "batch_matches_launches": batches == -(-n // b), "workspace_bytes": model.overlap_workspace_bytes(h, w, T, O, b),
                "accumulator_bytes": acc, "workspace_bytes_batch_1": model.overlap_workspace_bytes(h, w, T, O, 1)}

    def kernel_share(frame, T, O, facts):
        """ms of the two overlap kernels in one call, and their share of the call's kernel time (see the module's text)."""
        n, b, t = facts["windows"], facts["batch"], facts["window"][0]
        model.kernel_time_ms()
        model.set_kernel_timing(True)
        try:
            model.upscale(frame, tile=T, tile_overlap=O)
            whole = model.kernel_time_ms()["groups"]
            sizes = [b] * (n // b) + ([n % b] if n % b else [])
            net = 0.0
            for k in sizes:
                model.forward_batch(torch.rand(k, 3, t, t, device=dev))
                net += model.kernel_time_ms()["groups"]["upsample"]
        finally:
            model.set_kernel_timing(False)
        total = sum(whole[g] for g in model.KERNEL_GROUPS)
        mine = whole["upsample"] - net
        return {"kernel_ms": round(total, 3), "upsample_group_ms": round(whole["upsample"], 3), "network_upsample_ms": round(net, 3),
                "overlap_kernels_ms": round(mine, 3), "overlap_kernels_share": round(mine / total, 5)}

    rows = []
    for w, h in _sizes(args.frames):
        frame = frame_of(w, h)
        routes = {"untiled": lambda: model.upscale(frame), f"tiled_{args.tile}_{args.pad}": lambda: model.upscale(frame, tile=args.tile, tile_pad=args.pad)}
        facts = {"untiled": {"windows": 1, "window": [h, w], "batch": 1, "workspace_bytes": model.workspace_bytes(h, w, 1)},
                 f"tiled_{args.tile}_{args.pad}": tiled_facts(h, w, args.tile, args.pad)}
        for T, O in overlaps:
            routes[f"overlap_{T}_{O}"] = (lambda T=T, O=O: model.upscale(frame, tile=T, tile_overlap=O))
            facts[f"overlap_{T}_{O}"] = overlap_facts(h, w, T, O)
        t = _alternate(routes, args.reps, args.warmup)
        results = {k: fn() for k, fn in routes.items()}
        row = {"frame": f"{w}x{h}"}
        for k, fn in routes.items():
            row[k] = {**_stats(t[k]), **facts[k], "launches": launches_of(fn),
                      "share_differing_from_untiled": round(float((results[k] != results["untiled"]).float().mean()), 4)}
            row[k]["ms_per_window"] = round(row[k]["median_ms"] / facts[k]["windows"], 3)
            row[k]["over_untiled"] = round(row[k]["median_ms"] / row["untiled"]["median_ms"], 3)
        for T, O in overlaps:
            row[f"overlap_{T}_{O}"].update(kernel_share(frame, T, O, facts[f"overlap_{T}_{O}"]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    out["rows"] = rows
    rows = []
    for w, h in _sizes(args.large):
        frame = frame_of(w, h)
        T, O = overlaps[0]
        routes = {f"tiled_{args.tile}_{args.pad}": lambda: model.upscale(frame, tile=args.tile, tile_pad=args.pad),
                  f"overlap_{T}_{O}": lambda: model.upscale(frame, tile=T, tile_overlap=O)}
        facts = {f"tiled_{args.tile}_{args.pad}": tiled_facts(h, w, args.tile, args.pad), f"overlap_{T}_{O}": overlap_facts(h, w, T, O)}
        t = _alternate(routes, args.large_reps, 1)
        row = {"frame": f"{w}x{h}", "reps": args.large_reps}
        for k, fn in routes.items():
            row[k] = {**_stats(t[k]), **facts[k], "launches": launches_of(fn)}
            row[k]["ms_per_window"] = round(row[k]["median_ms"] / facts[k]["windows"], 3)
        row[f"overlap_{T}_{O}"].update(kernel_share(frame, T, O, facts[f"overlap_{T}_{O}"]))
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
