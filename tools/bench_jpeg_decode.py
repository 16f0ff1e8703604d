"""The JPEG decode of an input frame, timed as the device route (imgproc.decode_jpeg_u8: the file's bytes go up, nesr_jpeg_parse on
the host, csrc/jpeg_decode.hip, the 4-byte status comes back) and as the route it replaces (Pillow's libjpeg-turbo on one thread --
what cv2.imread runs -- then the upload of the decoded frame), the two alternating in one process on the same file, with the two
frames compared pixel for pixel.  Writes profiles/jpeg/bench_jpeg_decode.json.

    python tools/bench_jpeg_decode.py [--rounds R] [--reps N] [--only NAME] [--out F]

Files: the reference's asset (tests/golden/jpeg_decode/reference_test.jpeg: 512 x 512, DRI = 32, the restart-interval path) and
3840 x 2160 and 7680 x 4320 frames written by this project's encoder at quality 95 (no restart markers: the self-synchronising
path; the image is tools/bench_jpeg.py's).  Per file and route: the median over `rounds` rounds of the round's median over its
reps and the spread of the round medians (largest - smallest).  kernels_only_ms: nesr_jpeg_decode_u8 alone (events; file, scratch
and destination allocated once), with the launches of the synchronisation sequence, the kernel launches, the bytes each pass moves
through HBM counted from the shapes, and the share of the 8 TB/s HBM bound those bytes over that time come to."""
from __future__ import annotations

import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 8.0e12
FILES = [("reference-512x512-dri32", None), ("own-3840x2160", (2160, 3840)), ("own-7680x4320", (4320, 7680))]


def pass_bytes(info, file_bytes):
    """Bytes each pass reads and writes once, from the shapes (n: the scan; the unstuffed stream is counted as n too)."""
    n = int(info.scan_bytes)
    per = 1 if info.C == 1 else info.hs * info.vs + 2
    blocks = info.mcus_x * info.mcus_y * per
    planes = info.mcus_x * info.mcus_y * 64 * per
    frame = info.H * info.W * info.C
    dri = info.restart_interval > 0
    rows = {"upload": file_bytes, "clear (stream, coefficients)": n + 128 * blocks, "count": n, "compact": 2 * n,
            "entropy": (n + 128 * blocks) if dri else (2 * n + n + 128 * blocks), "dc prefix sum": 0 if dri else 3 * 32 * blocks,
            "idct": 128 * blocks + planes, "colour": planes + frame}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg", "bench_jpeg_decode.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode.py needs the GPU (ROCm device); there is no CPU measurement")
    import PIL
    from PIL import Image, features
    from bench_jpeg import bench_image
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    from neural_enhanced_super_resolution_amd._contexts import device_call
    Image.MAX_IMAGE_PIXELS = None
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rows = []
    for name, size in FILES:
        if args.only and args.only != name:
            continue
        if size is None:
            with open(os.path.join(ROOT, "tests", "golden", "jpeg_decode", "reference_test.jpeg"), "rb") as f:
                data = f.read()
        else:
            data = imgproc.encode_jpeg_u8(bench_image(size[0], size[1], dev), 95)
            torch.cuda.empty_cache()
        info = _lib.jpeg_parse(data)
        h, w, c = info.H, info.W, info.C

        def device_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frame = imgproc.decode_jpeg_u8(data, device=dev, use_hip=True)       # waits for the status word
            return frame, (time.perf_counter() - t0) * 1e3

        def host_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arr = np.asarray(Image.open(io.BytesIO(data)))
            t1 = time.perf_counter()
            frame = torch.from_numpy(arr).to(dev)                                 # the full-frame upload the host decode needs
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            return frame, (t1 - t0) * 1e3, (t2 - t1) * 1e3

        def kernels_only(reps):
            need = int(lib.nesr_jpeg_decode_scratch_bytes(ctypes.byref(info)))
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
            out = torch.empty((h, w, c), dtype=torch.uint8, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            file_dev = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
            p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
            times = []
            for _ in range(reps + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                device_call("nesr_jpeg_decode_u8", dev, p(file_dev), len(data), ctypes.byref(info), p(out), w * c, _lib.ORDER_RGB, p(scratch), need, p(status))
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            assert int(status.item()) == 0
            rounds, launches = ctypes.c_int(-1), ctypes.c_int(-1)
            lib.nesr_jpeg_decode_last_launches(ctypes.byref(rounds), ctypes.byref(launches))
            return statistics.median(times[1:]), rounds.value, launches.value, need

        ours, _ = device_route()                                         # warm-up of both, and the check that they are one frame
        theirs = host_route()[0]
        if ours.shape[-1] == 1:
            ours = ours[:, :, 0]
        if not torch.equal(ours, theirs):
            raise SystemExit(f"{name}: the device's frame is not Pillow's")
        del ours, theirs
        dev_wall, host_decode, host_copy = [], [], []
        for _ in range(args.rounds):                                     # alternating: device, host, device, host ...
            dev_wall.append(statistics.median(device_route()[1] for _ in range(args.reps)))
            r = [host_route()[1:] for _ in range(args.reps)]
            host_decode.append(statistics.median(x[0] for x in r))
            host_copy.append(statistics.median(x[1] for x in r))
        host_total = [a + b for a, b in zip(host_decode, host_copy)]

        def stat(v):
            return {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "rounds_ms": [round(x, 3) for x in v]}

        k_ms, sync_rounds, launches, scratch_bytes = kernels_only(2 * args.reps + 1)
        moved = pass_bytes(info, len(data))
        kernel_bytes = sum(v for k, v in moved.items() if k != "upload")
        row = {"file": name, "file_bytes": len(data), "frame_bytes": h * w * c, "shape": [h, w, c], "restart_interval": info.restart_interval,
               "frames_equal": True, "scratch_bytes": scratch_bytes, "kernels_only_ms": round(k_ms, 3), "sync_rounds": sync_rounds, "launches": launches,
               "pass_bytes": moved, "kernel_hbm_bytes": kernel_bytes, "share_of_hbm_bound": round(kernel_bytes / HBM_BYTES_PER_S / (k_ms * 1e-3), 4),
               "device_route": {"wall": stat(dev_wall), "bytes_to_device": len(data)},
               "host_route": {"wall": stat(host_total), "decode_one_thread": stat(host_decode), "upload": stat(host_copy), "bytes_to_device": h * w * c}}
        d, hst = row["device_route"]["wall"], row["host_route"]["wall"]
        row["device_faster_by_more_than_the_spread"] = bool(hst["median_ms"] - d["median_ms"] > max(d["spread_ms"], hst["spread_ms"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    result = {"tool": "tools/bench_jpeg_decode.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
              "pillow": {"version": PIL.__version__, "jpeg": features.version("jpg"), "turbo": bool(features.check_feature("libjpeg_turbo"))},
              "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
