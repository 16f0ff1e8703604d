"""UNet2DCondition.forward() on device-resident inputs against the same network in eager float32 torch on the same device (the
restatement of tests/unet_ref.py run by torch-ROCm), alternating call by call in one process.  Writes profiles/unet/bench_unet.json.

    python tools/bench_unet.py [--latents 32x32,64x64,128x128] [--reps 9] [--warmup 2] [--out F]

Configuration: the published one (widths (256, 512, 512, 1024), 8 heads, cross dim 1024, 1000 classes), random weights (seeded as in
the tests; no checkpoint is fetched), n = 2 samples (classifier-free guidance), 77 text states, timestep 487.25, label 20.  Per size:
medians and min .. max of `reps` event-timed calls of each route, taken alternately after `warmup` calls of each; the native path's
launch count and the event time per kernel group (one extra timed call); the multiply-adds the network needs, counted from the
shapes, over the native time as a share of the f32 MFMA rate (a whole-call rate over peak, not a kernel's); max |HIP - eager| over
the result.  This is the one place the 1024-wide shapes run, so that last figure is also the check that they are finite and agree."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F32_MFMA = 157.3e12      # FLOP/s of v_mfma_f32_16x16x4_f32 on the MI355X (spec)


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


def forward_flops(cfg, n, h, w, tokens):
    """2 x the multiply-adds of every conv, projection, attention and feed-forward of one forward (the embedding path left out)."""
    widths, layers, cross = cfg["block_out_channels"], cfg["layers_per_block"], cfg["cross_attention_dim"]
    levels = len(widths)
    px = lambda l: n * (h >> l) * (w >> l)
    resnet = lambda cin, cout, p: p * (9 * cin * cout + 9 * cout * cout + (cin * cout if cin != cout else 0))

    def transformer(dim, level, only_cross):
        p, tok = px(level), (h >> level) * (w >> level)
        macs = 2 * p * dim * dim + 4 * p * dim * dim                  # proj_in, proj_out; q and to_out of both attentions
        for cross_kv in (only_cross, True):
            if cross_kv:
                macs += 2 * n * tokens * cross * dim + 2 * p * tokens * dim
            else:
                macs += 2 * p * dim * dim + 2 * p * tok * dim
        return macs + p * dim * 8 * dim + p * 4 * dim * dim             # GEGLU, ff.net.2

    macs = px(0) * 9 * cfg["in_channels"] * widths[0]
    prev = widths[0]
    for i, wd in enumerate(widths):
        for j in range(layers):
            macs += resnet(prev if j == 0 else wd, wd, px(i))
            if cfg["down_block_types"][i] == "CrossAttnDownBlock2D":
                macs += transformer(wd, i, cfg["only_cross_attention"][i])
        if i < levels - 1:
            macs += px(i + 1) * 9 * wd * wd
        prev = wd
    top = widths[-1]
    macs += 2 * resnet(top, top, px(levels - 1)) + transformer(top, levels - 1, False)
    rev = widths[::-1]
    for i, wd in enumerate(rev):
        level = levels - 1 - i
        before, in_ch = rev[max(i - 1, 0)], rev[min(i + 1, levels - 1)]
        for j in range(layers + 1):
            macs += resnet((before if j == 0 else wd) + (in_ch if j == layers else wd), wd, px(level))
            if cfg["up_block_types"][i] == "CrossAttnUpBlock2D":
                macs += transformer(wd, level, cfg["only_cross_attention"][level])
        if i < levels - 1:
            macs += px(level - 1) * 9 * wd * wd
    return 2.0 * (macs + px(0) * 9 * widths[0] * cfg["out_channels"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latents", default="32x32,64x64,128x128")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet", "bench_unet.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_unet.py needs the GPU (ROCm device); there is no CPU measurement")

    from neural_enhanced_super_resolution_amd import UNet2DCondition
    from tests import unet_ref as R
    dev = torch.device("cuda:0")
    cfg = R.config()
    n, tokens, timestep, label = 2, 77, 487.25, 20
    sd = R.seeded_state_dict(seed=7)
    native = UNet2DCondition().to(dev)
    native.load_state_dict(sd)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    del sd
    rows = []
    for spec in args.latents.split(","):
        w, h = (int(v) for v in spec.lower().split("x"))
        sample, text = (t.to(dev) for t in R.seeded_inputs(n, h, w, tokens, 11, cfg["in_channels"], cfg["cross_attention_dim"]))

        def eager():
            with torch.no_grad():
                return R.forward(sd_dev, sample, timestep, text, label)

        def hip():
            return native(sample, timestep, text, label)

        for _ in range(args.warmup):
            want = eager()
            got = hip()
        nat, eag = [], []
        for _ in range(args.reps):
            nat.append(_timed(hip)[0])
            eag.append(_timed(eager)[0])
        native.set_kernel_timing(True)
        native.kernel_time_ms()
        hip()
        groups = native.kernel_time_ms()
        native.set_kernel_timing(False)
        flops = forward_flops(cfg, n, h, w, tokens)
        diff = (got - want).abs()
        row = {"latents": f"{w}x{h}", "n": n, "text_states": tokens, "native_forward_ms": round(_median(nat), 3),
               "native_min_max_ms": [round(min(nat), 3), round(max(nat), 3)], "eager_f32_ms": round(_median(eag), 3),
               "eager_min_max_ms": [round(min(eag), 3), round(max(eag), 3)], "eager_over_native": round(_median(eag) / _median(nat), 3),
               "launches": groups["launches"], "kernel_group_ms": {k: round(v, 3) for k, v in groups["groups"].items()},
               "dominant_group": max(groups["groups"], key=groups["groups"].get), "gflop": round(flops / 1e9, 1),
               "whole_call_share_of_f32_mfma_rate": round(flops / (_median(nat) * 1e-3) / PEAK_F32_MFMA, 4),
               "workspace_mib": round(native.workspace_bytes(n, h, w, tokens) / 2 ** 20, 1),
               "max_abs_hip_minus_eager": float(diff.max()), "max_abs_eager": float(want.abs().max()), "finite": bool(torch.isfinite(got).all())}
        del want, got
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0),
           "config": "published: widths (256, 512, 512, 1024), 2 layers a block, 8 heads, cross dim 1024, 1000 classes; random weights; n = 2, 77 text states",
           "comparison": f"tests/unet_ref.py in torch {torch.__version__} eager f32 on the same device", "reps": args.reps, "warmup": args.warmup,
           "f32_mfma_peak_tflops": PEAK_F32_MFMA / 1e12, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
