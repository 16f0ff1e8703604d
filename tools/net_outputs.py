"""The bits the five checkpoint networks give on their crafted cases: for every case of tests/unet_cases.py, tests/vae_cases.py,
tests/swin2sr_cases.py, tests/segformer_cases.py and tests/clip_text_cases.py, the sha256 of the output's bytes and the kernel
launches of the forward, in f32 and, where the model has that form (UNet, Swin2SR), in fp16.  Two builds that compute the same
thing write the same file, so a refactor of the host code is checked by running this on the parent and on the branch:

    python tools/net_outputs.py [--root OTHER_CHECKOUT] [--out F]

`--root`: the checkout (with its built library) whose package and cases are used, default this tree.  Each case runs through the
route its case file names (forward, upscale, segment, decode and decode_latents_u8).  An fp16 forward that leaves f16's range is
recorded by its error text instead of a hash.  Needs the GPU; there is no CPU route."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("net_outputs.py needs the GPU (ROCm device)")
    import neural_enhanced_super_resolution_amd as pkg
    from neural_enhanced_super_resolution_amd import ClipTextEncoder, SegFormer, Swin2SR, UNet2DCondition, VaeDecoder
    from neural_enhanced_super_resolution_amd._lib import NesrRangeError
    from tests import clip_text_cases, segformer_cases, swin2sr_cases, unet_cases, vae_cases
    assert os.path.abspath(pkg.__file__).startswith(root + os.sep), (pkg.__file__, root)
    dev = torch.device("cuda:0")
    rows = {}

    def record(key, model, run):
        """One forward of a fresh model: its bytes and its launches (the counter starts with the context)."""
        try:
            out = run(model)
            row = {"sha256": hashlib.sha256(out.contiguous().cpu().numpy().tobytes()).hexdigest(), "shape": list(out.shape)}
        except NesrRangeError as e:
            row = {"range_error": str(e)}
        row["launches"] = model.kernel_time_ms()["launches"]
        rows[key] = row
        print(key, json.dumps(row), flush=True)

    def loaded(cls, case, **kw):
        m = cls(**kw, **case.cfg).to(dev)
        m.load_state_dict(case.sd)
        return m

    for name in unet_cases.NAMES:
        case = unet_cases.by_name(name)
        for form in ("f32", "fp16"):
            record(f"unet/{name}/{form}", loaded(UNet2DCondition, case, compute_dtype=form),
                   lambda m: m(case.sample.to(dev), case.timestep, case.text.to(dev), case.label))
    for name in vae_cases.NAMES:
        case = vae_cases.by_name(name)
        z = vae_cases.z_of(case, torch.float32).to(dev)
        record(f"vae/{name}/decode", loaded(VaeDecoder, case), lambda m: m.decode(z))
        record(f"vae/{name}/decode_latents_u8", loaded(VaeDecoder, case), lambda m: m.decode_latents_u8(case.latents.to(dev)))
    for case in swin2sr_cases.cases() + (swin2sr_cases.rounding_ties(),):
        for form in ("f32", "fp16"):
            if case.via == "upscale":
                run = lambda m: m.upscale(torch.from_numpy(case.frame).to(dev))
            else:
                run = lambda m: m(case.x.to(dev))
            record(f"swin2sr/{case.name}/{case.via}/{form}", loaded(Swin2SR, case, compute_dtype=form), run)
    for case in segformer_cases.cases():
        if case.via == "segment":
            run = lambda m: m.segment(torch.from_numpy(case.frame).to(dev))
        else:
            run = lambda m: m(case.x.to(dev))
        record(f"segformer/{case.name}/{case.via}", loaded(SegFormer, case), run)
    for name in clip_text_cases.NAMES:
        case = clip_text_cases.by_name(name)
        record(f"clip_text/{name}", loaded(ClipTextEncoder, case), lambda m: m(case.ids, device=dev))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", args.out, len(rows), "rows")


if __name__ == "__main__":
    main()
