"""SegFormer.segment() on a device-resident frame against the same weights in eager torch on the same device, alternating in one
session.  Writes profiles/segformer/bench_segformer.json.

    python tools/bench_segformer.py [--frames 512x512,1024x768] [--reps 15] [--warmup 3] [--out F]

Native: one segment() call (PIL-exact resize, normalisation, network, argmax; the class map stays on the device).  Comparison:
``transformers``' SegformerForSemanticSegmentation in eval mode and float32 when it imports, else the torch restatement of
tests/segformer_ref.py; either gets the pixel_values the native pre-processing made, already on the device, and takes the argmax of
its logits, so its time leaves the pre-processing out (the reference does that part on the host with PIL).  Per frame: medians of
`reps` event-timed calls of each, taken alternately after `warmup` calls of each; the native path's launch count and the event time
per kernel group (one extra timed call); and the share of positions where the two class maps agree."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")


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
    ap.add_argument("--frames", default="512x512,1024x768")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segformer", "bench_segformer.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_segformer.py needs the GPU (ROCm device); there is no CPU measurement")
    from neural_enhanced_super_resolution_amd import SegFormer
    from tests import segformer_ref as R
    dev = torch.device("cuda:0")
    sd = R.seeded_state_dict(seed=R.WEIGHT_SEED)
    native = SegFormer().to(dev)
    native.load_state_dict(sd)
    try:
        import transformers
        eager_model = transformers.SegformerForSemanticSegmentation(transformers.SegformerConfig(num_labels=150)).eval()
        eager_model.load_state_dict(sd)
        eager_model.to(dev)
        kind = f"transformers {transformers.__version__} eager f32"

        def eager(x):
            with torch.no_grad():
                return eager_model(pixel_values=x).logits[0].argmax(dim=0)
    except ImportError:
        dsd = {k: v.to(dev) for k, v in sd.items()}
        kind = "torch restatement (tests/segformer_ref.py) f32"

        def eager(x):
            with torch.no_grad():
                return R.segformer_forward(dsd, x)[0].argmax(dim=0)
    rows = []
    for spec in args.frames.split(","):
        w, h = (int(v) for v in spec.lower().split("x"))
        frame = torch.from_numpy(R.seeded_frame(h, w, seed=11)).to(dev)
        x = native.pixel_values(frame)
        for _ in range(args.warmup):
            got = native.segment(frame)
            want = eager(x)
        nat, eag = [], []
        for _ in range(args.reps):
            nat.append(_timed(lambda: native.segment(frame))[0])
            eag.append(_timed(lambda: eager(x))[0])
        native.set_kernel_timing(True)
        native.kernel_time_ms()
        native.segment(frame)
        groups = native.kernel_time_ms()
        native.set_kernel_timing(False)
        row = {"frame": f"{w}x{h}", "native_segment_ms": round(_median(nat), 3), "eager_forward_argmax_ms": round(_median(eag), 3),
               "eager_over_native": round(_median(eag) / _median(nat), 2), "launches": groups["launches"],
               "kernel_group_ms": {k: round(v, 3) for k, v in groups["groups"].items()},
               "class_maps_agree": round(float((got.long() == want).float().mean()), 5)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "comparison": kind, "reps": args.reps, "warmup": args.warmup, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
