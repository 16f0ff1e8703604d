"""The PNG decode of an input frame, timed as the device routes (imgproc.decode_png: the upload of the file plus csrc/png_decode.hip,
all-device for a segmented file, hybrid -- host zlib, upload of the filtered stream, device unfilter -- for a one-stream file) and as
the route they replace (Pillow's decode on one thread plus the upload of the frame), the routes alternating in one process on the same
file.  Writes profiles/png_decode/bench_png_decode.json.

    python tools/bench_png_decode.py [--rounds R] [--reps N] [--only NAME] [--routes device,hybrid,...] [--out F]

Frames (tools/bench_png.py's image): 1024 x 1024 RGB8, 3840 x 2160 RGB8 and 3840 x 2160 RGBA16 written by imgproc.encode_png (one
segment per 32 KiB chunk: all-device); the 2160p RGB8 frame written by Pillow (one stream: hybrid); the 1024 x 1024 file of ours with
its chunks merged into one stream and pushed through inflate="device" (one wave: what serial costs); and the 1024 x 1024 and 2160p RGB8
frames written by zlib with Z_FULL_FLUSH every S bytes for a sweep of S, each through inflate="device" and inflate="host", to place
imgproc.PNG_DEVICE_SEGMENT_MAX.  Routes: `device` (inflate="device"), `hybrid` (inflate="host"), `pillow` (where Pillow holds the kind:
not 16-bit RGBA) and `zlib`: stdlib zlib's inflate of the file's stream plus the upload of what it gives, with no filter undone -- a floor
under every host decoder, and the host baseline of the 16-bit RGBA frame.
Per file and route: the median over `rounds` rounds of the round's median over its reps and the spread of the round medians (largest -
smallest), host clock around the call with a device synchronisation at both ends.  Every device frame is compared with the host's.
`device_wins`: the device route is faster than the fastest other route by more than both spreads.  `sweep` in the file: per frame, the
largest compressed segment of every swept file and whether the device route won there; `segment_max_measured` is the largest such
segment up to which it won without a gap (0: it never did), which is what PNG_DEVICE_SEGMENT_MAX should not exceed.

--routes device runs the device route alone (for a profiler run: rocprofv3 --kernel-trace --stats -- python tools/bench_png_decode.py
--routes device --only 3840x2160-rgb8-ours --rounds 1 --out F)."""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_png import bench_image, idat_stream       # noqa: E402


def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def file_of(h, w, c, depth, parts):
    ihdr = struct.pack(">IIBBBBB", w, h, depth, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b"")


def flushed(stream, every):
    """zlib level 1 with Z_FULL_FLUSH after every `every` bytes: one IDAT per part"""
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8)
    parts = [co.compress(stream[at:at + every]) + co.flush(zlib.Z_FULL_FLUSH) for at in range(0, len(stream), every)]
    return parts + [co.flush()]


def timed(fn, reps, sync):
    out = []
    for _ in range(reps):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def main():
    import numpy as np
    import torch
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--routes", default=None, help="comma-separated subset of device,hybrid,pillow,zlib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode", "bench_png_decode.json"))
    args = ap.parse_args()
    device = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(device)        # noqa: E731
    try:
        from PIL import Image
    except ImportError:
        Image = None

    def pillow_route(data):
        arr = np.asarray(Image.open(io.BytesIO(data)))
        return torch.from_numpy(np.ascontiguousarray(arr if arr.dtype == np.uint8 else arr.view(np.int16))).to(device)

    def zlib_route(data):
        return torch.from_numpy(np.frombuffer(zlib.decompress(idat_stream(data)), np.uint8).copy()).to(device)

    files = []                                            # (name, bytes, {route: kwargs})
    frames = {}
    for name, h, w, c, depth in [("1024x1024-rgb8", 1024, 1024, 3, 8), ("3840x2160-rgb8", 2160, 3840, 3, 8), ("3840x2160-rgba16", 2160, 3840, 4, 16)]:
        frame = bench_image(h, w, c, depth, device)
        frames[name] = frame
        files.append((name + "-ours", imgproc.encode_png(frame, order="rgb"), {"device": {"inflate": "device"}, "hybrid": {"inflate": "host"}}))
    if Image is not None:
        buf = io.BytesIO()
        Image.fromarray(frames["3840x2160-rgb8"].cpu().numpy()).save(buf, format="PNG")
        files.append(("3840x2160-rgb8-pillow", buf.getvalue(), {"hybrid": {}}))
    ours = files[0][1]
    stream = zlib.decompress(idat_stream(ours))
    files.append(("1024x1024-rgb8-one-stream", file_of(1024, 1024, 3, 8, [zlib.compress(stream, 1)]), {"device": {"inflate": "device"}, "hybrid": {"inflate": "host"}}))
    big = zlib.decompress(idat_stream(files[1][1]))
    for frame_name, (h, w), raw in (("1024x1024-rgb8", (1024, 1024), stream), ("3840x2160-rgb8", (2160, 3840), big)):
        for every in (8192, 32768, 131072, 524288):
            files.append((f"{frame_name}-flush{every}", file_of(h, w, 3, 8, flushed(raw, every)),
                          {"device": {"inflate": "device"}, "hybrid": {"inflate": "host"}}))
    only_routes = set(args.routes.split(",")) if args.routes else None
    results = []
    for name, data, routes in files:
        if args.only and args.only not in name:
            continue
        want = imgproc.decode_png(data, device=device, inflate="host")
        fns = {r: (lambda kw=kw: imgproc.decode_png(data, device=device, **kw)) for r, kw in routes.items()}
        if Image is not None and "rgba16" not in name:    # Pillow holds no 16-bit RGBA
            fns["pillow"] = lambda: pillow_route(data)
        fns["zlib"] = lambda: zlib_route(data)
        if only_routes is not None:
            fns = {r: fn for r, fn in fns.items() if r in only_routes}
        for r, fn in fns.items():
            got = fn()
            if r != "zlib":
                assert torch.equal(got.reshape(want.shape).view(want.dtype), want), (name, r)
        rounds = {r: [] for r in fns}
        for _ in range(args.rounds):
            for r, fn in fns.items():                     # the routes alternate inside a round
                rounds[r].append(timed(fn, args.reps, sync))
        _, segs = _lib.png_parse(data)
        row = {"file": name, "bytes": len(data), "frame_bytes": int(want.numel() * want.element_size()), "segments": len(segs),
               "largest_segment_bytes": max(int(s.bytes) for s in segs)}
        for r, v in rounds.items():
            row[r + "_ms"] = round(statistics.median(v), 3)
            row[r + "_spread_ms"] = round(max(v) - min(v), 3)
        others = [r for r in rounds if r not in ("device", "zlib")]       # zlib alone decodes no frame
        if "device" in rounds and others:
            best = min(others, key=lambda r: row[r + "_ms"])
            row["device_wins"] = row["device_ms"] + row["device_spread_ms"] + row[best + "_spread_ms"] < row[best + "_ms"]
        print(json.dumps(row), flush=True)
        results.append(row)
    sweep, measured = {}, None
    for row in results:
        if "-flush" in row["file"] and "device_wins" in row:
            sweep.setdefault(row["file"].split("-flush")[0], []).append((row["largest_segment_bytes"], row["device_wins"]))
    for frame_name, points in sweep.items():
        upto = 0
        for largest, wins in sorted(points):
            if not wins:
                break
            upto = largest
        measured = upto if measured is None else min(measured, upto)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"rounds": args.rounds, "reps": args.reps, "segment_max": imgproc.PNG_DEVICE_SEGMENT_MAX, "segment_max_measured": measured,
                   "sweep": {k: sorted(v) for k, v in sweep.items()}, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
