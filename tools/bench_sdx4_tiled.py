"""StableDiffusionX4Upscaler.upscale(tile=...) on device-resident frames: what the window path costs beside the untiled call, and the
frames only it can run.  Writes profiles/sdx4/bench_sdx4_tiled.json.

    python tools/bench_sdx4_tiled.py [--shapes 256:256:0,512:128:16,512:256:32] [--dtypes f32,fp16] [--steps 20] [--reps 5] [--warmup 1] [--out F]

A shape is side:tile:overlap of a square low-res frame.  Configuration as tools/bench_sdx4.py: the published widths as recalled (text
encoder 1024 x 23 layers, UNet (256, 512, 512, 1024), VAE (128, 256, 512)), random weights (seeded as in the tests; no checkpoint is
fetched), guidance 7.5 (n = 2), 77 ids a prompt, noise level 20.  Per shape and UNet compute form: the median and min .. max of
`reps` event-timed calls after `warmup`; where the frame fits the untiled call (side <= 256) that call is timed in the same
session, the two routes alternating call by call, and the difference is the overhead of the window path; the window counts, the
launch count, the workspaces, and one extra timed call split by the contexts' own event timers into text encoder, UNet, VAE and
the pipeline's own kernel groups (the five window kernels among them).  Nothing here is a pass condition."""
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


def _stats(v):
    s = sorted(v)
    return {"median_ms": round(s[len(s) // 2], 2), "min_max_ms": [round(s[0], 2), round(s[-1], 2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256:256:0,512:128:16,512:256:32")
    ap.add_argument("--dtypes", default="f32,fp16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdx4", "bench_sdx4_tiled.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sdx4_tiled.py needs the GPU (ROCm device); there is no CPU measurement")

    from neural_enhanced_super_resolution_amd import ClipTextEncoder, StableDiffusionX4Upscaler, UNet2DCondition, VaeDecoder
    from neural_enhanced_super_resolution_amd.sdx4 import MAX_LOW_RES_PIXELS
    from tests import clip_text_ref as TR
    from tests import unet_ref as UR
    from tests import vae_ref as VR
    dev = torch.device("cuda:0")
    guidance, level, tokens = 7.5, 20, 77
    sds = {"text": TR.seeded_state_dict(1), "unet": UR.seeded_state_dict(seed=7), "vae": VR.seeded_state_dict(5)}
    text, vae = ClipTextEncoder().to(dev), VaeDecoder().to(dev)
    text.load_state_dict(sds["text"])
    vae.load_state_dict(sds["vae"])
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 49408, (2, tokens), generator=g)
    rows = []
    for dtype in args.dtypes.split(","):
        net = UNet2DCondition(compute_dtype=dtype).to(dev)
        net.load_state_dict(sds["unet"])
        pipe = StableDiffusionX4Upscaler(text, net, vae)
        for spec in args.shapes.split(","):
            side, tile, overlap = (int(v) for v in spec.split(":"))
            frame = torch.randint(0, 256, (side, side, 3), generator=g, dtype=torch.uint8).to(dev)
            noise, latents = torch.randn((3, side, side), generator=g).to(dev), torch.randn((4, side, side), generator=g).to(dev)
            kw = dict(prompt_ids=ids[1], negative_ids=ids[0], noise_level=level, num_inference_steps=args.steps, guidance_scale=guidance, noise=noise, latents=latents)
            tiled = lambda: pipe.upscale(frame, tile=tile, tile_overlap=overlap, **kw)
            untiled = (lambda: pipe.upscale(frame, **kw)) if side * side <= MAX_LOW_RES_PIXELS else None
            for _ in range(args.warmup):
                got = tiled()
                want = untiled() if untiled else None
            same = bool(torch.equal(got, want)) if untiled else None
            del got, want
            t_tiled, t_untiled = [], []
            for _ in range(args.reps):
                t_tiled.append(_timed(tiled)[0])
                if untiled:
                    t_untiled.append(_timed(untiled)[0])
            pipe.set_kernel_timing(True)
            for m in (pipe, text, net, vae):
                m.kernel_time_ms()
            call_ms = _timed(tiled)[0]
            own, parts = pipe.kernel_time_ms(), [m.kernel_time_ms() for m in (text, net, vae)]
            pipe.set_kernel_timing(False)
            nets_ms = {"text_encoder": sum(parts[0]["groups"].values()), "unet": sum(parts[1]["groups"].values()), "vae": sum(parts[2]["groups"].values())}
            total = sum(nets_ms.values()) + sum(own["groups"].values())
            window_ms = sum(v for k, v in own["groups"].items() if k not in ("prepare", "step"))
            (ky, kx), (ty, tx), _ = pipe.tile_plan(side, side, tile, overlap)
            row = {"unet_compute_dtype": dtype, "low_res": f"{side}x{side}", "out": f"{4 * side}x{4 * side}", "tile": tile, "tile_overlap": overlap, "window": f"{ty}x{tx}",
                   "windows": ky * kx, "vae_windows": ky * kx, "steps": args.steps, "guidance": guidance, "tiled": _stats(t_tiled),
                   "untiled": _stats(t_untiled) if untiled else None,
                   "tiled_over_untiled": round(_stats(t_tiled)["median_ms"] / _stats(t_untiled)["median_ms"], 4) if untiled else None,
                   "one_window_equals_untiled_bits": same if ky * kx == 1 else None, "launches": pipe.last_launches(),
                   "timed_call_ms": round(call_ms, 2), "kernel_ms": {**{k: round(v, 3) for k, v in nets_ms.items()}, **{k: round(v, 3) for k, v in own["groups"].items()}},
                   "share_of_kernel_time": {"window_kernels": round(window_ms / total, 6), "unet": round(nets_ms["unet"] / total, 4), "vae": round(nets_ms["vae"] / total, 4)},
                   "workspace_mib": {"pipeline": round(pipe.workspace_bytes(2, side, side, tokens, tile=tile, tile_overlap=overlap) / 2 ** 20, 1),
                                     "text_encoder": round(text.workspace_bytes(2, tokens) / 2 ** 20, 1), "unet": round(net.workspace_bytes(2, ty, tx, tokens) / 2 ** 20, 1),
                                     "vae": round(vae.workspace_bytes(ty, tx) / 2 ** 20, 1)}}
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            rows.append(row)
        del pipe, net
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0),
           "config": "published widths as recalled: text 1024 x 23 layers x 16 heads, UNet (256, 512, 512, 1024), VAE (128, 256, 512); random weights; n = 2, 77 ids",
           "reps": args.reps, "warmup": args.warmup,
           "note": "the networks' workspaces are those of one window; kernel_ms sums the contexts' event timers over one extra call (timing on), so it is below timed_call_ms "
                   "by the gaps between launches",
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
