"""UNet2DCondition.forward() in its two compute forms, f32 and fp16, on device-resident inputs, alternating call by call in one
process.  Writes profiles/unet/bench_unet_f16.json.

    python tools/bench_unet_f16.py [--latents 32x32,64x64,128x128] [--reps 9] [--warmup 2] [--out F]

Configuration: the published one (widths (256, 512, 512, 1024), 8 heads, cross dim 1024, 1000 classes), random weights (seeded as in
the tests; no checkpoint is fetched), n = 2 samples, 77 text states, timestep 487.25, label 20: tools/bench_unet.py's, whose native
column the f32 column here repeats.  Per size: medians and min .. max of `reps` event-timed calls of each form, taken alternately
after `warmup` calls of each; fp16 / f32; the event time per kernel group of one extra timed call of each form; max |fp16 - f32| over
the result; the workspace.  Once: the bytes of weights each form holds on the device.  The fp16 forward is synchronous (it reads its
range word), the f32 forward is not; both are timed to the completion of their last launch.

The one condition DESIGN section 21 states: the fp16 median does not exceed the f32 form's lowest observed time at any size
("fp16_median_below_f32_min").  It is reported, not asserted: a form is a capability first."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latents", default="32x32,64x64,128x128")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet", "bench_unet_f16.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_unet_f16.py needs the GPU (ROCm device); there is no CPU measurement")

    from neural_enhanced_super_resolution_amd import UNet2DCondition
    from tests import unet_ref as R
    dev = torch.device("cuda:0")
    cfg = R.config()
    n, tokens, timestep, label = 2, 77, 487.25, 20
    sd = R.seeded_state_dict(seed=7)
    forms = {}
    for name in ("f32", "fp16"):
        forms[name] = UNet2DCondition(compute_dtype=name).to(dev)
        forms[name].load_state_dict(sd)
    del sd
    weight_bytes = {name: m.weight_bytes(dev) for name, m in forms.items()}
    print(json.dumps({"device_weight_bytes": weight_bytes}), flush=True)
    rows = []
    for spec in args.latents.split(","):
        w, h = (int(v) for v in spec.lower().split("x"))
        sample, text = (t.to(dev) for t in R.seeded_inputs(n, h, w, tokens, 11, cfg["in_channels"], cfg["cross_attention_dim"]))
        run = {name: (lambda m=m: m(sample, timestep, text, label)) for name, m in forms.items()}
        out = {}
        for _ in range(args.warmup):
            for name in forms:
                out[name] = run[name]()
        ms = {name: [] for name in forms}
        for _ in range(args.reps):
            for name in forms:
                ms[name].append(_timed(run[name])[0])
        groups = {}
        for name, m in forms.items():
            m.set_kernel_timing(True)
            m.kernel_time_ms()
            run[name]()
            groups[name] = m.kernel_time_ms()
            m.set_kernel_timing(False)
        med = {name: _median(v) for name, v in ms.items()}
        diff = (out["fp16"] - out["f32"]).abs()
        row = {"latents": f"{w}x{h}", "n": n, "text_states": tokens,
               "f32_forward_ms": round(med["f32"], 3), "f32_min_max_ms": [round(min(ms["f32"]), 3), round(max(ms["f32"]), 3)],
               "fp16_forward_ms": round(med["fp16"], 3), "fp16_min_max_ms": [round(min(ms["fp16"]), 3), round(max(ms["fp16"]), 3)],
               "fp16_over_f32": round(med["fp16"] / med["f32"], 4), "fp16_median_below_f32_min": bool(med["fp16"] <= min(ms["f32"])),
               "f32_spread_ms": round(max(ms["f32"]) - min(ms["f32"]), 3), "gain_ms": round(med["f32"] - med["fp16"], 3),
               "launches": {name: g["launches"] for name, g in groups.items()},
               "kernel_group_ms": {name: {k: round(v, 3) for k, v in g["groups"].items()} for name, g in groups.items()},
               "workspace_mib": {name: round(m.workspace_bytes(n, h, w, tokens) / 2 ** 20, 1) for name, m in forms.items()},
               "max_abs_fp16_minus_f32": float(diff.max()), "max_abs_f32": float(out["f32"].abs().max()),
               "finite": bool(torch.isfinite(out["fp16"]).all())}
        del out
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    result = {"device": torch.cuda.get_device_name(0),
              "config": "published: widths (256, 512, 512, 1024), 2 layers a block, 8 heads, cross dim 1024, 1000 classes; random weights; n = 2, 77 text states",
              "comparison": "UNet2DCondition(compute_dtype='f32') against UNet2DCondition(compute_dtype='fp16'), alternating call by call",
              "reps": args.reps, "warmup": args.warmup, "device_weight_bytes": weight_bytes, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
