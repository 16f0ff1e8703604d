"""SRVGGNetCompact (realesr-general-x4v3, realesr-animevideov3) on one MI355X: host u8 -> host u8 throughput through
RealESRGANer, per-kernel time of the body convs against their binding bound, and the same network as a torch-ROCm
composition (F.conv2d / F.prelu / pixel_shuffle / interpolate) on the same GPU and dtype as the baseline.

    python tools/bench_compact.py [--steps 5] [--warmup 2] [--out profiles/compact/bench_compact.json]
                                  [--models x4v3,animevideov3] [--dtypes f32,bf16,fp16] [--workloads 1080p,2160p-tiled] [--no-torch]
                                  [--alternate bf16,fp16 [--rounds 15]]

Prints one JSON line per case and writes them all to --out.  Weights are seeded synthetic (synth.py).  Bounds use the
chip-level peaks: 2.5 PFLOP/s dense bf16 / f16 MFMA (the f32 form issues three f16 MFMAs per product, so its compute bound
is FLOPs x 3 / 2.5 PF) and 8 TB/s HBM.  dtype fp16 is SRVGGNetCompact(compute_dtype="fp16") under half=True (upstream's fp16 run); its
torch baseline is the composition in torch.float16.  --alternate A,B times two dtypes in ONE process, their calls taking turns
round by round (what a ratio of a few per cent needs: two separate cases differ by more than that), and adds the medians and
the ratio B : A to the output; the profiles/compact/bench_compact_fp16.json of the repository is
`--dtypes bf16,fp16 --alternate bf16,fp16 --no-torch --out profiles/compact/bench_compact_fp16.json`.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")   # the torch baseline: no exhaustive MIOpen search inside the timing

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from neural_enhanced_super_resolution_amd import RealESRGANer, SRVGGNetCompact  # noqa: E402
from neural_enhanced_super_resolution_amd.synth import synthetic_compact_state_dict, synthetic_frame  # noqa: E402

PEAK_MFMA = 2.5e15
HBM = 8.0e12
MODELS = {"x4v3": dict(num_conv=32, upscale=4, act_type="prelu"), "animevideov3": dict(num_conv=16, upscale=4, act_type="prelu")}
WORKLOADS = {"1080p": (1080, 1920, 0), "2160p-tiled": (2160, 3840, 512)}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def torch_net(sd, cfg, dtype, dev):
    """The network as a torch composition (upstream's forward, torch-ROCm kernels)."""
    n = 2 * (cfg["num_conv"] + 1)
    p = {k: v.to(dev, dtype) for k, v in sd.items()}
    s = cfg["upscale"]

    def run(x):
        out = x
        for i in range(0, n + 1, 2):
            out = F.conv2d(out, p[f"body.{i}.weight"], p[f"body.{i}.bias"], padding=1)
            if i < n:
                out = F.prelu(out, p[f"body.{i + 1}.weight"])
        return F.pixel_shuffle(out, s) + F.interpolate(x, scale_factor=s, mode="nearest")
    return run


def wrapper(cfg, sd, dtype, tile, dev):
    """dtype "f32": half=False; "bf16": half=True with a default model; "fp16": half=True with a compute_dtype="fp16" model."""
    model = SRVGGNetCompact(**cfg, compute_dtype="fp16") if dtype == "fp16" else SRVGGNetCompact(**cfg)
    return RealESRGANer(scale=cfg["upscale"], model_path={"params": {k: v.clone() for k, v in sd.items()}}, model=model, tile=tile,
                        tile_pad=10, pre_pad=0, half=dtype != "f32", device=dev)


def alternated(model, pair, workload, rounds, warmup):
    """Two dtypes in one process, one call each per round: device u8 -> u8 (whole frames) and host u8 -> host u8."""
    cfg = MODELS[model]
    H, W, tile = WORKLOADS[workload]
    dev = torch.device("cuda:0")
    sd = synthetic_compact_state_dict(seed=0, **cfg)
    ups = {dt: wrapper(cfg, sd, dt, tile, dev) for dt in pair}
    img = synthetic_frame(H, W, seed=0)
    x_dev = torch.from_numpy(img).to(dev)
    res = {"tool": "bench_compact", "mode": "alternated", "model": model, "pair": list(pair), "workload": workload, "rounds": rounds}

    def turns(fns):
        ts = {dt: [] for dt in pair}
        for r in range(warmup + rounds):
            for dt in (pair if r % 2 == 0 else pair[::-1]):          # neither is always the one that runs on a cold cache
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fns[dt]()
                torch.cuda.synchronize()
                if r >= warmup:
                    ts[dt].append(time.perf_counter() - t0)
        return {dt: {"median_ms": round(statistics.median(v) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3), "max_ms": round(max(v) * 1e3, 3)}
                for dt, v in ts.items()}
    if not tile:
        res["device_u8"] = turns({dt: (lambda up=ups[dt]: up.model.forward_u8(x_dev, flip_rgb=True, round_nearest=True)) for dt in pair})
        res["device_u8"]["ratio"] = round(res["device_u8"][pair[1]]["median_ms"] / res["device_u8"][pair[0]]["median_ms"], 4)
    res["host_to_host"] = turns({dt: (lambda up=ups[dt]: up.enhance(img)) for dt in pair})
    res["host_to_host"]["ratio"] = round(res["host_to_host"][pair[1]]["median_ms"] / res["host_to_host"][pair[0]]["median_ms"], 4)
    for up in ups.values():
        up.model.check_status()
    return res


def case(model, dtype, workload, steps, warmup, with_torch):
    cfg = MODELS[model]
    H, W, tile = WORKLOADS[workload]
    s = cfg["upscale"]
    dev = torch.device("cuda:0")
    sd = synthetic_compact_state_dict(seed=0, **cfg)
    up = wrapper(cfg, sd, dtype, tile, dev)
    img = synthetic_frame(H, W, seed=0)
    sec, out = timed(lambda: up.enhance(img)[0], steps, warmup)
    out_px = H * s * W * s
    res = {"tool": "bench_compact", "model": model, "dtype": dtype, "workload": workload, "frame": [H, W], "tile": tile,
           "ms_per_frame": round(sec * 1e3, 3), "MPps_out": round(out_px / sec / 1e6, 2),
           "frame_flops": up.model.forward_flops(1, H, W)}
    res["TFLOPps_frame"] = round(res["frame_flops"] / sec / 1e12, 1)
    if not tile:
        # the same forward_u8 with the frame already on the device and the result left there: what of the host-to-host
        # time is the network (enhance() adds the upload, the copy of the result back and the numpy handling)
        x_dev = torch.from_numpy(img).to(dev)
        dsec, _ = timed(lambda: up.model.forward_u8(x_dev, flip_rgb=True, round_nearest=True), steps, warmup)
        res["device_u8_ms"] = round(dsec * 1e3, 3)
        res["host_side_ms"] = round((sec - dsec) * 1e3, 3)
    # body-conv launches: hipEvent brackets around the num_conv 64 -> 64 convs of every forward
    up.model.set_kernel_timing(dev, True)
    up.model.kernel_time()
    up.enhance(img)
    torch.cuda.synchronize()
    ms, launches, flops = up.model.kernel_time()
    up.model.set_kernel_timing(dev, False)
    if launches:
        px = flops / launches / (2 * 9 * 64 * 64)           # pixels per launch
        esz = 4 if dtype == "f32" else 2
        per = ms / launches
        t_flop = flops / launches * (3 if dtype == "f32" else 1) / PEAK_MFMA
        t_byte = px * 64 * esz * 2 / HBM                    # read the input map once, write the output map once
        bound = max(t_flop, t_byte)
        res["body_conv"] = {"launches": launches, "ms_total": round(ms, 3), "us_per_launch": round(per * 1e3, 1),
                            "pixels_per_launch": int(px), "bound_us": round(bound * 1e6, 1),
                            "binding": "mfma" if t_flop >= t_byte else "hbm", "share_of_bound": round(bound / (per * 1e-3), 3),
                            "TFLOPps": round(flops / (ms * 1e-3) / 1e12, 1)}
    if with_torch:
        tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
        net = torch_net(sd, cfg, tdt, dev)
        lut = torch.from_numpy(np.arange(256, dtype=np.float32) / 255).to(dev)

        @torch.no_grad()
        def torch_frame():
            x = lut[torch.from_numpy(img).to(dev).long()].flip(2).permute(2, 0, 1)[None].to(tdt)
            y = net(x).float()[0].clamp(0, 1).flip(0).permute(1, 2, 0)
            return (y * 255.0).round().to(torch.uint8).cpu().numpy()
        try:
            tsec, tout = timed(torch_frame, max(2, steps // 2), 1)
            d = np.abs(tout.astype(np.int32) - out.astype(np.int32))
            res["torch"] = {"ms_per_frame": round(tsec * 1e3, 3), "MPps_out": round(out_px / tsec / 1e6, 2),
                            "speedup_hip": round(tsec / sec, 2), "u8_max_diff": int(d.max()), "u8_share_differing": float(np.mean(d > 0)),
                            "note": "whole frame, untiled"}
            if not tile:   # the composition with the frame on the device and the u8 result left there (as device_u8_ms)
                x_dev = torch.from_numpy(img).to(dev)

                @torch.no_grad()
                def torch_device():
                    x = lut[x_dev.long()].flip(2).permute(2, 0, 1)[None].to(tdt)
                    y = net(x).float()[0].clamp(0, 1).flip(0).permute(1, 2, 0)
                    return (y * 255.0).round().to(torch.uint8)
                dsec_t, _ = timed(torch_device, max(2, steps // 2), 1)
                res["torch"]["device_u8_ms"] = round(dsec_t * 1e3, 3)
                res["torch"]["device_speedup_hip"] = round(dsec_t / dsec, 2)
        except RuntimeError as e:   # e.g. out of memory for the untiled 4K composition
            res["torch"] = {"error": str(e)[:200]}
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", default="x4v3,animevideov3")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--workloads", default="1080p,2160p-tiled")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--alternate", default="", help="two dtypes, e.g. bf16,fp16: timed in one process, their calls taking turns")
    ap.add_argument("--rounds", type=int, default=15, help="rounds of --alternate")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for m in a.models.split(","):
        for dt in a.dtypes.split(","):
            for wl in a.workloads.split(","):
                r = case(m, dt, wl, a.steps, a.warmup, not a.no_torch)
                print(json.dumps(r), flush=True)
                rows.append(r)
    turns = []
    if a.alternate:
        pair = a.alternate.split(",")
        assert len(pair) == 2, "--alternate takes two dtypes"
        for m in a.models.split(","):
            for wl in a.workloads.split(","):
                r = alternated(m, pair, wl, a.rounds, a.warmup)
                print(json.dumps(r), flush=True)
                turns.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "cases": rows, **({"alternated": turns} if turns else {})}, f, indent=1)


if __name__ == "__main__":
    main()
