"""VaeDecoder.decode_latents_u8() on device-resident latents against the same decoder in eager float32 torch on the same device
(the restatement of tests/vae_ref.py run by torch-ROCm: what the reference's pipeline computes, since diffusers upcasts this VAE),
alternating call by call in one process.  Writes profiles/vae/bench_vae.json.

    python tools/bench_vae.py [--latents 64x64,128x128,256x256] [--reps 9] [--warmup 2] [--out F]

Configuration: the published widths (128, 256, 512), 32 groups, two layers a block, random weights (seeded as in the tests; no
checkpoint is fetched).  Native: one decode_latents_u8() call, float32 latents in, u8 HWC frame out, the scaling factor and the
quantiser inside the first and the last launch.  Comparison: latents / scaling_factor, the restatement's decode, / 2 + 0.5, clamp,
x 255, round, uint8, all on the device.  Per size: medians and min .. max of `reps` event-timed calls of each, taken alternately
after `warmup` calls of each; the native path's launch count and the event time per kernel group (one extra timed call); the
multiply-adds the network needs, counted from the shapes, over the native time as a share of the f32 MFMA rate (a whole-call rate
over peak, not a kernel's); the largest difference of the two u8 frames and the share of samples where they differ.  A size the
eager route cannot run (it forms the tokens x tokens matrix) is recorded as not measured, with the reason."""
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


def decode_flops(cfg, h, w):
    """2 x the multiply-adds of every conv, projection and of the attention of one decode of h x w latents."""
    widths, layers, lat, out = cfg["block_out_channels"], cfg["layers_per_block"], cfg["latent_channels"], cfg["out_channels"]
    top, px = widths[-1], h * w
    resnet = lambda cin, cout, p: p * (9 * cin * cout + 9 * cout * cout + (cin * cout if cin != cout else 0))
    macs = px * (lat * lat + 9 * lat * top) + 2 * resnet(top, top, px)
    macs += px * 4 * top * top + 2 * px * px * top
    prev = top
    for i, wd in enumerate(reversed(widths)):
        macs += resnet(prev, wd, px) + layers * resnet(wd, wd, px)
        if i < len(widths) - 1:
            px *= 4
            macs += px * 9 * wd * wd
        prev = wd
    return 2.0 * (macs + px * 9 * prev * out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latents", default="64x64,128x128,256x256")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae", "bench_vae.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae.py needs the GPU (ROCm device); there is no CPU measurement")

    from neural_enhanced_super_resolution_amd import VaeDecoder
    from tests import vae_ref as R
    dev = torch.device("cuda:0")
    cfg = R.config()
    sd = R.seeded_state_dict(seed=7)
    native = VaeDecoder().to(dev)
    native.load_state_dict(sd)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    rows = []
    for spec in args.latents.split(","):
        w, h = (int(v) for v in spec.lower().split("x"))
        latents = R.seeded_latents(h, w, seed=11).to(dev)

        def eager():
            return R.quantise(R.decode_latents_float(sd_dev, latents, torch.float32))

        row = {"latents": f"{w}x{h}", "frame": f"{4 * w}x{4 * h}", "tokens": h * w}
        try:
            for _ in range(args.warmup):
                want = eager()
            eager_ok = True
        except Exception as e:      # the eager route's own limit (memory): the native route is still measured
            eager_ok, want = False, None
            row["eager"] = f"not measured: {type(e).__name__}: {str(e).splitlines()[0][:160]}"
            torch.cuda.empty_cache()
        for _ in range(args.warmup):
            got = native.decode_latents_u8(latents)
        nat, eag = [], []
        for _ in range(args.reps):
            nat.append(_timed(lambda: native.decode_latents_u8(latents))[0])
            if eager_ok:
                eag.append(_timed(eager)[0])
        native.set_kernel_timing(True)
        native.kernel_time_ms()
        native.decode_latents_u8(latents)
        groups = native.kernel_time_ms()
        native.set_kernel_timing(False)
        flops = decode_flops(cfg, h, w)
        row.update({"native_decode_latents_u8_ms": round(_median(nat), 3), "native_min_max_ms": [round(min(nat), 3), round(max(nat), 3)],
                    "launches": groups["launches"], "kernel_group_ms": {k: round(v, 3) for k, v in groups["groups"].items()},
                    "dominant_group": max(groups["groups"], key=groups["groups"].get), "gflop": round(flops / 1e9, 1),
                    "whole_call_share_of_f32_mfma_rate": round(flops / (_median(nat) * 1e-3) / PEAK_F32_MFMA, 4),
                    "workspace_mib": round(native.workspace_bytes(h, w) / 2 ** 20, 1)})
        if eager_ok:
            diff = (got.int() - want.int()).abs()
            row.update({"eager_f32_ms": round(_median(eag), 3), "eager_min_max_ms": [round(min(eag), 3), round(max(eag), 3)],
                        "eager_over_native": round(_median(eag) / _median(nat), 3), "u8_max_abs_diff": int(diff.max()),
                        "u8_share_differing": round(float((diff != 0).float().mean()), 6)})
            del want
        del got
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "config": "published widths (128, 256, 512), 32 groups, 2 layers a block, x4, random weights",
           "comparison": f"tests/vae_ref.py in torch {torch.__version__} eager f32 on the same device", "reps": args.reps, "warmup": args.warmup,
           "f32_mfma_peak_tflops": PEAK_F32_MFMA / 1e12, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
