"""Untiled f32 frames through RealESRGANer.enhance() as row bands over devices=[...], host u8 -> host u8.

For a 1080p and a 2160p x2plus frame (RRDBNet, 23 blocks, compute_dtype "f32", tile=0) and k = 1, 2, 4, 8 DISTINCT devices as far as
the machine has them -- on a one-GPU machine the list [0, 0] alone, which can only show the overhead -- three wrappers on the
same weights take turns, one frame each per round, in one session:

    none      devices=None                       the one-device frame
    first     devices=[...], band_devices=False  the parent commit's route for this frame: the first entry alone
    banded    devices=[...]                      row bands, one per entry

and the medians are compared with `none` and with `first`, never with an earlier run of `banded`.  Also recorded: that the three
outputs are the same bytes, the bands, the exchange bytes per step and neighbour (6 rows x internal width x 64 channels x 4 B), and
for every link whether it was local, peer-written or staged.  Writes profiles/band_devices/bench_band_devices.json.

    python tools/bench_band_devices.py [--steps 5] [--warmup 2] [--sizes 1080p,2160p] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"1080p": (1080, 1920), "2160p": (2160, 3840)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1080p,2160p")
    ap.add_argument("--num-block", type=int, default=23)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_devices", "bench_band_devices.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet, banded
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict

    ngpu = torch.cuda.device_count()
    lists = [list(range(k)) for k in (2, 4, 8) if k <= ngpu] or [[0, 0]]
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=2, num_block=args.num_block)

    def make(devices, band=True):
        up = RealESRGANer(scale=2, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=2, num_block=args.num_block), tile=0, pre_pad=0,
                          half=False, device="cuda:0", devices=devices)
        up.band_devices = band
        return up

    result = {"gpus_visible": ngpu, "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "num_block": args.num_block,
              "across_gpus": "measured" if ngpu >= 2 else "unmeasured across GPUs (one GPU visible: [0, 0] shows the overhead only)", "cases": []}
    for size in args.sizes.split(","):
        h, w = SIZES[size]
        frame = synthetic_frame(h, w, seed=0)
        for devices in lists:
            ups = {"none": make(None), "first": make(devices, band=False), "banded": make(devices)}
            times = {k: [] for k in ups}
            outs = {}
            for step in range(args.warmup + args.steps):
                for name, up in ups.items():             # alternated: one frame each per round
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out, _ = up.enhance(frame)
                    dt = time.perf_counter() - t0
                    if step >= args.warmup:
                        times[name].append(dt * 1e3)
                    outs[name] = out
            up = ups["banded"]
            lanes = [(torch.device("cuda", d), devices[:j].count(d)) for j, d in enumerate(devices)][:len(up.last_bands or [])]
            med = {k: statistics.median(v) for k, v in times.items()}
            case = {"size": size, "devices": devices, "bands": up.last_bands, "ms_median": med, "ms_all": times,
                    "banded_over_none": med["none"] / med["banded"], "banded_over_first_entry": med["first"] / med["banded"],
                    "bitwise_equal": bool(np.array_equal(outs["none"], outs["banded"]) and np.array_equal(outs["none"], outs["first"])),
                    "exchange_steps": 1 + 3 * args.num_block, "exchange_bytes_per_step_and_neighbour": banded.APRON * (w // 2) * 64 * 4,
                    "links": [up.model.band_link_state(o, d) for d, o in lanes]}
            result["cases"].append(case)
            print(json.dumps({k: case[k] for k in ("size", "devices", "bands", "ms_median", "banded_over_none", "banded_over_first_entry", "bitwise_equal", "links")}),
                  flush=True)
            del ups, up
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
