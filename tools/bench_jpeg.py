"""The JPEG encode of a finished frame, timed as the device route (imgproc.encode_jpeg_u8: csrc/jpeg.hip, then the copy of the
length words and of the file) and as the route it replaces (the copy of the whole frame to the host, then Pillow's libjpeg-turbo on
one thread -- what cv2.imwrite runs), the two alternating in one process on the same pixels, with the two files compared byte for
byte at every size.  Writes profiles/jpeg/bench_jpeg.json.

    python tools/bench_jpeg.py [--rounds R] [--reps N] [--only NAME] [--out F]

Sizes: 1024 x 1024, 7680 x 4320 (the 2160p frame through the x2 model) and 16384 x 16384 (the pipeline's result), RGB, quality 95.
The image is derived from the benchmark's frame (synth.synthetic_frame at an eighth of the size, enlarged bilinearly on the device,
plus seeded noise of +-3 so that it is not smoother than a photograph).  Per size and route: the median over `rounds` rounds of
the round's median over its reps, the spread of the round medians (largest - smallest), the file's size and the bytes each route
copies to the host.  Device route: HIP events around the call (the copies are on its stream) and the host's clock around it; host
route: the host's clock.  kernels_only_ms: the encode's launches alone (events, buffers allocated once, no copy), beside the bytes
they move through HBM counted from the shapes."""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("1024x1024", 1024, 1024), ("7680x4320", 4320, 7680), ("16384x16384", 16384, 16384)]


def bench_image(h, w, device):
    import torch
    from torch.nn import functional as F
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    base = torch.from_numpy(synthetic_frame(h // 8, w // 8, seed=0)[:, :, ::-1].copy()).to(device)       # RGB
    big = F.interpolate(base.permute(2, 0, 1)[None].float(), size=(h, w), mode="bilinear", align_corners=False)[0]
    g = torch.Generator(device=device).manual_seed(7)
    for c in range(3):          # a plane at a time: the 16384^2 frame's temporaries stay small
        big[c] += torch.randint(-3, 4, (h, w), generator=g, device=device, dtype=torch.int8).float()
    return big.clamp_(0, 255).round_().to(torch.uint8).permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg", "bench_jpeg.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py needs the GPU (ROCm device); there is no CPU measurement")
    import PIL
    from PIL import Image, features
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    Image.MAX_IMAGE_PIXELS = None
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rows = []
    for name, h, w in SIZES:
        if args.only and args.only != name:
            continue
        frame = bench_image(h, w, dev)
        torch.cuda.synchronize()

        def device_route():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            data = imgproc.encode_jpeg_u8(frame, args.quality)
            b.record()
            b.synchronize()
            return data, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

        def host_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = frame.cpu().numpy()                                   # the full-frame copy the encode on the host needs
            t1 = time.perf_counter()
            buf = io.BytesIO()
            Image.fromarray(host).save(buf, format="JPEG", quality=args.quality)
            t2 = time.perf_counter()
            return buf.getvalue(), (t1 - t0) * 1e3, (t2 - t1) * 1e3

        def kernels_only(reps):
            """Event time of nesr_jpeg_encode_u8's launches alone, into buffers allocated once: no copy, no allocation."""
            import ctypes
            from neural_enhanced_super_resolution_amd._contexts import device_call
            need = int(lib.nesr_jpeg_scratch_bytes(h, w, 3))
            cap = h * w * 3 // 2 + 4096
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            words = torch.zeros(2, dtype=torch.int64, device=dev)
            p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
            times = []
            for _ in range(reps + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                device_call("nesr_jpeg_encode_u8", dev, p(frame), w * 3, h, w, 3, _lib.ORDER_RGB, args.quality, p(scratch), need, p(out), cap, p(words))
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            assert words.cpu().tolist() == [len(ours), 0]
            return statistics.median(times[1:])

        ours, _, _ = device_route()                                      # warm-up of both, and the check that they are one file
        theirs, _, _ = host_route()
        if ours != theirs:
            raise SystemExit(f"{name}: the device's file ({len(ours)} bytes) is not Pillow's ({len(theirs)} bytes)")
        dev_event, dev_wall, host_copy, host_encode = [], [], [], []
        for _ in range(args.rounds):                                     # alternating: device, host, device, host ...
            r = [device_route()[1:] for _ in range(args.reps)]
            dev_event.append(statistics.median(x[0] for x in r))
            dev_wall.append(statistics.median(x[1] for x in r))
            r = [host_route()[1:] for _ in range(max(1, args.reps if h * w < 8e7 else 1))]
            host_copy.append(statistics.median(x[0] for x in r))
            host_encode.append(statistics.median(x[1] for x in r))
        host_total = [a + b for a, b in zip(host_copy, host_encode)]

        def stat(v):
            return {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "rounds_ms": [round(x, 3) for x in v]}

        row = {"size": name, "quality": args.quality, "file_bytes": len(ours), "frame_bytes": h * w * 3, "files_equal": True,
               "scratch_bytes": int(lib.nesr_jpeg_scratch_bytes(h, w, 3)),
               "kernels_only_ms": round(kernels_only(2 * args.reps + 1), 3),
               # what the passes read and write once, from the shapes: frame -> coefficients (as many bytes as the frame), read again
               # by the length pass and by the emit pass; the unstuffed stream cleared, written, counted, read; the file written
               "kernel_hbm_bytes": 4 * h * w * 3 + 5 * len(ours),
               "device_route": {"events": stat(dev_event), "wall": stat(dev_wall), "bytes_to_host": len(ours) + 16},
               "host_route": {"wall": stat(host_total), "copy": stat(host_copy), "encode_one_thread": stat(host_encode), "bytes_to_host": h * w * 3}}
        d, hst = row["device_route"]["wall"], row["host_route"]["wall"]
        row["device_faster_by_more_than_the_spread"] = bool(hst["median_ms"] - d["median_ms"] > max(d["spread_ms"], hst["spread_ms"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del frame
        torch.cuda.empty_cache()
    result = {"tool": "tools/bench_jpeg.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
              "pillow": {"version": PIL.__version__, "jpeg": features.version("jpg"),
                         "turbo": bool(features.check_feature("libjpeg_turbo"))},
              "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
