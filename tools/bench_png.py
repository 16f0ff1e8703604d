"""The PNG encode of a finished frame, timed as the device route (imgproc.encode_png: csrc/png.hip, then the copy of the length words
and of the file) and as the route it replaces (the copy of the whole frame to the host, then cv2's settings on one thread: the Sub
filter and zlib level 1 Z_RLE, imgproc.encode_png's host route; and Pillow's default PNG writer where Pillow is present and holds
the kind), the routes alternating in one process on the same pixels.  Writes profiles/png/bench_png.json.

    python tools/bench_png.py [--rounds R] [--reps N] [--only NAME] [--no-host] [--out F]

Sizes: 1024 x 1024 RGB, 7680 x 4320 RGB (the 2160p frame through the x2 model) and 7680 x 4320 RGBA 16 bit.  The image is derived
from the benchmark's frame (synth.synthetic_frame at an eighth of the size, enlarged bilinearly on the device, plus seeded noise of
+-3 so that it is not smoother than a photograph; 16 bit: times 257 plus seeded low-byte noise).  Per size and route: the median
over `rounds` rounds of the round's median over its reps, the spread of the round medians (largest - smallest), the file's size and
the bytes each route copies to the host.  Device route: HIP events around the call (the copies are on its stream) and the host's
clock around it; host routes: the host's clock.  kernels_only_ms: the encode's launches alone (events, buffers allocated once, no
copy), beside the bytes they move through HBM counted from the shapes in units of N, the filtered stream.  Each device file is
checked: zlib inflates its IDATs to N bytes with the right Adler-32, and at 1024 x 1024 it decodes to the frame bit for bit."""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("1024x1024-rgb8", 1024, 1024, 3, 8), ("7680x4320-rgb8", 4320, 7680, 3, 8), ("7680x4320-rgba16", 4320, 7680, 4, 16)]


def bench_image(h, w, c, depth, device):
    import torch
    from torch.nn import functional as F
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame
    base = torch.from_numpy(synthetic_frame(h // 8, w // 8, seed=0)[:, :, ::-1].copy()).to(device)       # RGB
    if c == 4:
        base = torch.cat([base, base[:, :, 1:2].flip(0)], dim=2)
    big = F.interpolate(base.permute(2, 0, 1)[None].float(), size=(h, w), mode="bilinear", align_corners=False)[0]
    g = torch.Generator(device=device).manual_seed(7)
    for k in range(c):          # a plane at a time: the temporaries stay small
        big[k] += torch.randint(-3, 4, (h, w), generator=g, device=device, dtype=torch.int8).float()
    q = big.clamp_(0, 255).round_().to(torch.int32).permute(1, 2, 0).contiguous()
    if depth == 8:
        return q.to(torch.uint8)
    q = q * 257 + torch.randint(-120, 121, q.shape, generator=g, device=device, dtype=torch.int32)
    return q.clamp_(0, 65535).to(torch.int16)                        # the uint16 pattern, as frame_io holds a 16-bit frame


def idat_stream(data):
    import struct
    at, parts = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        if kind == b"IDAT":
            parts.append(data[at + 8:at + 8 + n])
        at += 12 + n
    return b"".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-host", action="store_true", help="the device route alone (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png", "bench_png.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_png.py needs the GPU (ROCm device); there is no CPU measurement")
    try:
        import PIL
        from PIL import Image
        Image.MAX_IMAGE_PIXELS = None
    except ImportError:
        PIL = Image = None
    from neural_enhanced_super_resolution_amd import _lib, frame_io, imgproc
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rows = []
    for name, h, w, c, depth in SIZES:
        if args.only and args.only != name:
            continue
        frame = bench_image(h, w, c, depth, dev)
        frame_bytes = h * w * c * depth // 8
        n_stream = h * (1 + w * c * depth // 8)
        torch.cuda.synchronize()

        def device_route():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            data = imgproc.encode_png(frame)
            b.record()
            b.synchronize()
            return data, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

        def host_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = frame_io.frame_to_numpy(frame.cpu())                  # the full-frame copy the encode on the host needs
            t1 = time.perf_counter()
            data = imgproc.encode_png(host)
            t2 = time.perf_counter()
            return data, (t1 - t0) * 1e3, (t2 - t1) * 1e3, host

        def pillow_route(host):
            t0 = time.perf_counter()
            buf = io.BytesIO()
            Image.fromarray(host).save(buf, format="PNG")
            return len(buf.getvalue()), (time.perf_counter() - t0) * 1e3

        def kernels_only(reps):
            """Event time of nesr_png_encode's launches alone, into buffers allocated once: no copy, no allocation."""
            import ctypes
            from neural_enhanced_super_resolution_amd._contexts import device_call
            need = int(lib.nesr_png_scratch_bytes(h, w, c, depth))
            cap = int(lib.nesr_png_bound(h, w, c, depth))
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            words = torch.zeros(2, dtype=torch.int64, device=dev)
            p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
            times = []
            for _ in range(reps + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                device_call("nesr_png_encode", dev, p(frame), w * c * depth // 8, h, w, c, depth, _lib.ORDER_RGB, p(scratch), need, p(out), cap, p(words))
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            assert words.cpu().tolist() == [len(ours), 0]
            return statistics.median(times[1:])

        ours, _, _ = device_route()                                      # warm-up, and the checks of the file
        stream = zlib.decompress(idat_stream(ours))                      # (zlib checks the Adler-32)
        assert len(stream) == n_stream, (len(stream), n_stream)
        del stream
        if h * w <= 1024 * 1024:
            from tests import png_ref
            assert png_ref.refilter_matches(ours, frame_io.frame_to_numpy(frame.cpu())), "the device's file does not decode to the frame"
        dev_event, dev_wall, host_copy, host_encode, pil_ms = [], [], [], [], []
        theirs_len = pil_len = None
        pil_ok = Image is not None and depth == 8
        for _ in range(args.rounds):                                     # alternating: device, host, device, host ...
            r = [device_route()[1:] for _ in range(args.reps)]
            dev_event.append(statistics.median(x[0] for x in r))
            dev_wall.append(statistics.median(x[1] for x in r))
            if args.no_host:
                continue
            r = [host_route() for _ in range(args.reps if h * w < 8e6 else 1)]
            theirs_len = len(r[0][0])
            host_copy.append(statistics.median(x[1] for x in r))
            host_encode.append(statistics.median(x[2] for x in r))
            if pil_ok:
                pil_len, ms = pillow_route(r[0][3])
                pil_ms.append(ms)
            del r

        def stat(v):
            return {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "rounds_ms": [round(x, 3) for x in v]}

        k_ms = kernels_only(2 * args.reps + 1)
        hbm = frame_bytes + 2 * n_stream + 3 * (len(ours) - 75)
        row = {"size": name, "file_bytes": len(ours), "frame_bytes": frame_bytes, "filtered_stream_bytes_N": n_stream,
               "chunks": (n_stream + 32767) // 32768, "scratch_bytes": int(lib.nesr_png_scratch_bytes(h, w, c, depth)),
               "kernels_only_ms": round(k_ms, 3),
               # what the passes read and write once, from the shapes: the frame read by the filter pass (its second read and the
               # neighbours come from the caches), N written and read back by the chunk pass, each IDAT written to its slot, read
               # and written to its place by the gather pass
               "kernel_hbm_bytes": hbm, "kernel_hbm_in_units_of_N": round(hbm / n_stream, 3),
               "kernels_achieved_TB_per_s": round(hbm / (k_ms * 1e-3) / 1e12, 4),
               "device_route": {"events": stat(dev_event), "wall": stat(dev_wall), "bytes_to_host": len(ours) + 16}}
        if not args.no_host:
            host_total = [a + b for a, b in zip(host_copy, host_encode)]
            row["host_route_cv2_settings"] = {"wall": stat(host_total), "copy": stat(host_copy), "encode_one_thread": stat(host_encode),
                                              "file_bytes": theirs_len, "bytes_to_host": frame_bytes}
            d, hst = row["device_route"]["wall"], row["host_route_cv2_settings"]["wall"]
            row["device_faster_by_more_than_the_spread"] = bool(hst["median_ms"] - d["median_ms"] > max(d["spread_ms"], hst["spread_ms"]))
            row["device_file_not_larger"] = bool(len(ours) <= theirs_len)
            if pil_ok:
                row["pillow_default_encode_only"] = dict(stat(pil_ms), file_bytes=pil_len)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del frame
        torch.cuda.empty_cache()
    result = {"tool": "tools/bench_png.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
              "zlib": zlib.ZLIB_RUNTIME_VERSION, "pillow": PIL.__version__ if PIL else None, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
