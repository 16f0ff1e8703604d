"""The JPEG encoder's options (4:4:4, optimised Huffman tables, a restart interval of one MCU row), measured after
tools/bench_jpeg.py's protocol: the routes of a comparison alternate in one process on the same pixels, 3 rounds, the median of
the round medians and their spread (largest - smallest).  Writes profiles/jpeg/bench_jpeg_options.json.

    python tools/bench_jpeg_options.py [--rounds R] [--reps N] [--parent-lib path/to/the/parent/commit's/libnesr_hip.so] [--out F]

  (a) default options, this tree against the parent commit's library (--parent-lib; left out without it): nesr_jpeg_encode_u8's
      launches alone (events, buffers allocated once) at 1024 x 1024 and 7680 x 4320, the two libraries alternating call by call.
  (b) device route (imgproc.encode_jpeg_u8 with the option, then the copy of the length words and of the file) against the host
      route (the copy of the frame, then Pillow with the same option on one thread) at 7680 x 4320, for 4:4:4, optimize and a
      restart interval of one MCU row; the two files are compared byte for byte.  A round is the median of `reps` device runs and
      ONE host run (100 to 400 ms each), so the host column is the median and spread of single runs.
  (c) the file's size with optimised against standard tables, per layout, on the benchmark's frame.
  (d) the read-back of our own 7680 x 4320 file with and without a restart interval: nesr_jpeg_decode_last_launches' sync rounds and
      the event time of imgproc.decode_jpeg_u8 on bytes that are already in host memory (tools/bench_jpeg_decode.py's device route).
"""
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


def stat(v):
    return {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "rounds_ms": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg", "bench_jpeg_options.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_options.py needs the GPU (ROCm device); there is no CPU measurement")
    import PIL
    from PIL import Image, features
    from bench_jpeg import bench_image
    from neural_enhanced_super_resolution_amd import _lib, imgproc
    Image.MAX_IMAGE_PIXELS = None
    dev = torch.device("cuda:0")
    lib = _lib.load()
    q = args.quality
    result = {"tool": "tools/bench_jpeg_options.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "quality": q,
              "pillow": {"version": PIL.__version__, "jpeg": features.version("jpg"), "turbo": bool(features.check_feature("libjpeg_turbo"))}}

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return out, a.elapsed_time(b)

    # ---------------------------------------------------------------- (a) default options: this tree against the parent commit
    rows = []
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("nesr_jpeg_scratch_bytes", "nesr_jpeg_encode_u8"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        for name, h, w in (("1024x1024", 1024, 1024), ("7680x4320", 4320, 7680)):
            frame = bench_image(h, w, dev)
            need = int(lib.nesr_jpeg_scratch_bytes(h, w, 3))
            assert need == int(parent.nesr_jpeg_scratch_bytes(h, w, 3))
            cap = h * w * 3 // 2 + 4096
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
            outs = {k: torch.zeros(cap, dtype=torch.uint8, device=dev) for k in ("tree", "parent")}
            words = torch.zeros(2, dtype=torch.int64, device=dev)
            p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def run(which):
                handle = lib if which == "tree" else parent
                rc = handle.nesr_jpeg_encode_u8(0, p(frame), w * 3, h, w, 3, _lib.ORDER_RGB, q, p(scratch), need, p(outs[which]), cap, p(words), stream)
                assert rc == 0, rc

            for which in ("tree", "parent"):
                event_ms(lambda: run(which))
            n = int(words.cpu()[0])
            assert torch.equal(outs["tree"][:n], outs["parent"][:n]), "the default file changed"
            times = {"tree": [], "parent": []}
            for _ in range(args.rounds):
                r = {"tree": [], "parent": []}
                for _ in range(4 * args.reps):                 # alternating call by call
                    for which in ("tree", "parent"):
                        r[which].append(event_ms(lambda: run(which))[1])
                for which in r:
                    times[which].append(statistics.median(r[which]))
            row = {"size": name, "file_bytes": n, "files_equal": True, "tree": stat(times["tree"]), "parent": stat(times["parent"])}
            margin = max(row["tree"]["spread_ms"], row["parent"]["spread_ms"])
            row["tree_minus_parent_ms"] = round(row["tree"]["median_ms"] - row["parent"]["median_ms"], 3)
            row["not_slower_by_more_than_the_larger_spread"] = bool(row["tree_minus_parent_ms"] <= margin)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del frame, scratch, outs
            torch.cuda.empty_cache()
    result["default_options_against_parent"] = rows if args.parent_lib else "not taken: no --parent-lib"

    # ---------------------------------------------------------------- (b) device against host, (c) sizes, (d) read-back at 7680 x 4320
    h, w = 4320, 7680
    frame = bench_image(h, w, dev)
    torch.cuda.synchronize()
    options = {"default": {}, "4:4:4": {"sampling": "4:4:4"}, "optimize": {"optimize": True}, "restart_row": {"restart_interval": (w + 15) // 16},
               "4:4:4+optimize+restart_row": {"sampling": "4:4:4", "optimize": True, "restart_interval": (w + 7) // 8}}
    pillow_kw = {"sampling": "subsampling", "optimize": "optimize", "restart_interval": "restart_marker_blocks"}
    rows, files = [], {}
    for name, kw in options.items():
        def device_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data, ev = event_ms(lambda: imgproc.encode_jpeg_u8(frame, q, **kw))
            return data, ev, (time.perf_counter() - t0) * 1e3

        def host_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = frame.cpu().numpy()
            t1 = time.perf_counter()
            buf = io.BytesIO()
            Image.fromarray(host).save(buf, format="JPEG", quality=q, **{pillow_kw[k]: v for k, v in kw.items()})
            return buf.getvalue(), (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        ours = device_route()[0]
        theirs = host_route()[0]
        if ours != theirs:
            raise SystemExit(f"{name}: the device's file ({len(ours)} bytes) is not Pillow's ({len(theirs)} bytes)")
        files[name] = ours
        dev_event, dev_wall, host_copy, host_encode = [], [], [], []
        for _ in range(args.rounds):
            r = [device_route()[1:] for _ in range(args.reps)]
            dev_event.append(statistics.median(x[0] for x in r))
            dev_wall.append(statistics.median(x[1] for x in r))
            r = [host_route()[1:]]
            host_copy.append(r[0][0])
            host_encode.append(r[0][1])
        row = {"options": name, "size": "7680x4320", "file_bytes": len(ours), "files_equal": True,
               "device_route": {"events": stat(dev_event), "wall": stat(dev_wall)},
               "host_route": {"wall": stat([a + b for a, b in zip(host_copy, host_encode)]), "copy": stat(host_copy), "encode_one_thread": stat(host_encode)}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    result["device_against_host_7680x4320"] = rows

    sizes = []
    for sampling in ("4:2:0", "4:2:2", "4:4:4"):
        std = len(files["default"] if sampling == "4:2:0" else files["4:4:4"] if sampling == "4:4:4" else imgproc.encode_jpeg_u8(frame, q, sampling=sampling))
        opt = len(files["optimize"] if sampling == "4:2:0" else imgproc.encode_jpeg_u8(frame, q, sampling=sampling, optimize=True))
        sizes.append({"sampling": sampling, "standard_tables_bytes": std, "optimised_tables_bytes": opt, "saved_percent": round(100.0 * (std - opt) / std, 2)})
    result["file_sizes_7680x4320"] = sizes
    print(json.dumps(sizes), flush=True)

    rows = []
    rounds_, launches_ = ctypes.c_int(-1), ctypes.c_int(-1)
    for name in ("default", "restart_row"):
        data = files[name]
        want = imgproc.decode_jpeg_u8(data, device=dev, use_hip=True)
        assert lib.nesr_jpeg_decode_last_launches(ctypes.byref(rounds_), ctypes.byref(launches_)) == 0
        times = []
        for _ in range(args.rounds):
            r = []
            for _ in range(args.reps):
                got, ev = event_ms(lambda: imgproc.decode_jpeg_u8(data, device=dev, use_hip=True))
                r.append(ev)
            assert torch.equal(got, want)
            times.append(statistics.median(r))
        rows.append({"file": name, "file_bytes": len(data), "sync_rounds": rounds_.value, "launches": launches_.value, "decode_events": stat(times)})
        print(json.dumps(rows[-1]), flush=True)
    assert torch.equal(imgproc.decode_jpeg_u8(files["default"], device=dev, use_hip=True), imgproc.decode_jpeg_u8(files["restart_row"], device=dev, use_hip=True))
    result["read_back_7680x4320"] = rows

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
