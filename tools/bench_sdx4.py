"""StableDiffusionX4Upscaler.upscale() on a device-resident frame against the same loop in eager float32 torch on the same device
(the restatements of tests/unet_ref.py, tests/vae_ref.py and tests/sdx4_ref.py run by torch-ROCm; the text states are shared),
alternating call by call in one process.  Writes profiles/sdx4/bench_sdx4.json.

    python tools/bench_sdx4.py [--frames 64x64,128x128,256x256] [--steps 20] [--reps 5] [--warmup 1] [--unet-compute-dtype f32|fp16] [--out F]

--unet-compute-dtype fp16 runs the native route with the UNet in its fp16 compute form (the eager route stays float32) and writes
profiles/sdx4/bench_sdx4_unet_fp16.json.

Configuration: the published widths as recalled (text encoder 1024 x 23 layers, UNet (256, 512, 512, 1024), VAE (128, 256, 512)),
random weights (seeded as in the tests; no checkpoint is fetched), guidance 7.5 (n = 2), 77 ids a prompt, noise level 20.  Per size:
medians and min .. max of `reps` event-timed calls of each route after `warmup` calls of each; the native call split into text
encoder, prepare, UNet x 2 steps, step x steps and VAE by the contexts' own event timers (one extra timed call), the launch count
and the workspaces.  Nothing here is a pass condition."""
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
    ap.add_argument("--frames", default="64x64,128x128,256x256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--unet-compute-dtype", choices=("f32", "fp16"), default="f32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sdx4", "bench_sdx4.json" if args.unet_compute_dtype == "f32" else "bench_sdx4_unet_fp16.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sdx4.py needs the GPU (ROCm device); there is no CPU measurement")

    from neural_enhanced_super_resolution_amd import ClipTextEncoder, StableDiffusionX4Upscaler, UNet2DCondition, VaeDecoder
    from tests import clip_text_ref as TR
    from tests import sdx4_ref as R
    from tests import unet_ref as UR
    from tests import vae_ref as VR
    dev = torch.device("cuda:0")
    guidance, level, tokens = 7.5, 20, 77
    sds = {"text": TR.seeded_state_dict(1), "unet": UR.seeded_state_dict(seed=7), "vae": VR.seeded_state_dict(5)}
    nets = []
    for cls, key in ((ClipTextEncoder, "text"), (UNet2DCondition, "unet"), (VaeDecoder, "vae")):
        net = (cls(compute_dtype=args.unet_compute_dtype) if key == "unet" else cls()).to(dev)
        net.load_state_dict(sds[key])
        nets.append(net)
    pipe = StableDiffusionX4Upscaler(*nets)
    unet_dev = {k: v.to(dev) for k, v in sds["unet"].items()}
    vae_dev = {k: v.to(dev) for k, v in sds["vae"].items()}
    del sds
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 49408, (2, tokens), generator=g)
    abar, low = R.ddim_alpha_bars(), R.low_res_alpha_bars()
    rows = []
    for spec in args.frames.split(","):
        w, h = (int(v) for v in spec.lower().split("x"))
        frame = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev)
        noise, latents = torch.randn((3, h, w), generator=g).to(dev), torch.randn((4, h, w), generator=g).to(dev)
        text = pipe.text_encoder(ids, device=dev)

        def hip():
            return pipe.upscale(frame, prompt_ids=ids[1], negative_ids=ids[0], noise_level=level, num_inference_steps=args.steps, guidance_scale=guidance,
                                noise=noise, latents=latents)

        def eager():
            with torch.no_grad():
                image = R.add_noise(frame.float().permute(2, 0, 1) / 127.5 - 1.0, noise, level, low)
                x = latents.clone()
                for t in R.timesteps(args.steps):
                    a, p = R.step_alphas(t, args.steps, abar)
                    sample = torch.cat([x, image], dim=0)[None].expand(2, -1, -1, -1).contiguous()
                    m = UR.forward(unet_dev, sample, float(t), text, level)
                    x = R.ddim_step(x, m[0] + guidance * (m[1] - m[0]), a, p)
                return VR.quantise(VR.decode_latents_float(vae_dev, x[None], torch.float32))

        for _ in range(args.warmup):
            want, got = eager(), hip()
        nat, eag = [], []
        for _ in range(args.reps):
            nat.append(_timed(hip)[0])
            eag.append(_timed(eager)[0])
        pipe.set_kernel_timing(True)
        for m in (pipe, *nets):
            m.kernel_time_ms()
        hip()
        own, parts = pipe.kernel_time_ms(), [m.kernel_time_ms() for m in nets]
        pipe.set_kernel_timing(False)
        split = {"text_encoder": sum(parts[0]["groups"].values()), "prepare": own["groups"]["prepare"], f"unet_x{2 * args.steps}": sum(parts[1]["groups"].values()),
                 f"step_x{args.steps}": own["groups"]["step"], "vae": sum(parts[2]["groups"].values())}
        one_step = (split[f"unet_x{2 * args.steps}"] + split[f"step_x{args.steps}"]) / args.steps
        diff = (got.int() - want.to(dev).int()).abs()
        row = {"low_res": f"{w}x{h}", "out": f"{4 * w}x{4 * h}", "steps": args.steps, "guidance": guidance, "native_ms": round(_median(nat), 2),
               "native_min_max_ms": [round(min(nat), 2), round(max(nat), 2)], "eager_f32_ms": round(_median(eag), 2),
               "eager_min_max_ms": [round(min(eag), 2), round(max(eag), 2)], "eager_over_native": round(_median(eag) / _median(nat), 3),
               "launches": pipe.last_launches(), "kernel_ms": {k: round(v, 3) for k, v in split.items()},
               "step_kernel_share_of_a_step": round(split[f"step_x{args.steps}"] / args.steps / one_step, 5),
               "prepare_over_one_unet_forward": round(split["prepare"] / (split[f"unet_x{2 * args.steps}"] / args.steps), 5),
               "workspace_mib": {"pipeline": round(pipe.workspace_bytes(2, h, w, tokens) / 2 ** 20, 1), "text_encoder": round(nets[0].workspace_bytes(2, tokens) / 2 ** 20, 1),
                                 "unet": round(nets[1].workspace_bytes(2, h, w, tokens) / 2 ** 20, 1), "vae": round(nets[2].workspace_bytes(h, w) / 2 ** 20, 1)},
               "u8_differing_from_eager_share": round(float((diff > 0).float().mean()), 5), "u8_max_abs_difference": int(diff.max())}
        del want, got
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "unet_compute_dtype": args.unet_compute_dtype,
           "config": "published widths as recalled: text 1024 x 23 layers x 16 heads, UNet (256, 512, 512, 1024), VAE (128, 256, 512); random weights; n = 2, 77 ids",
           "comparison": f"the restatements of tests/ in torch {torch.__version__} eager f32 on the same device (text states shared)", "reps": args.reps, "warmup": args.warmup,
           "note": "unet_x40 counts the two samples of a step as two; it is 20 forwards of n = 2.  Random weights: the frames are noise, the u8 differences say the two routes agree.",
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
