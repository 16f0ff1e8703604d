"""CPU: which files imgproc.decode_png(inflate=None) sends to the device inflater, held to the measurement it was derived from
(profiles/png_decode/bench_png_decode.json, written by tools/bench_png_decode.py).  The rule may leave a file on the hybrid route that
the device would have decoded faster; it must not choose the device inflater for a measured file on which that route did not beat the
fastest host route by more than both spreads."""
import json
import os
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows():
    with open(os.path.join(ROOT, "profiles", "png_decode", "bench_png_decode.json")) as f:
        return [r for r in json.load(f)["results"] if "device_wins" in r]


def _chosen(imgproc, nbytes, n_segments, largest, contiguous=1):
    info = SimpleNamespace(contiguous=contiguous, n_segments=n_segments)
    segs = [SimpleNamespace(bytes=largest)] + [SimpleNamespace(bytes=1)] * (n_segments - 1)
    return imgproc._png_default_on_device(info, segs, nbytes)


def test_the_default_route_follows_the_measurement():
    from neural_enhanced_super_resolution_amd import imgproc
    rows = _rows()
    assert len(rows) >= 12 and any(r["device_wins"] for r in rows) and any(not r["device_wins"] for r in rows)
    chosen = [r["file"] for r in rows if _chosen(imgproc, r["bytes"], r["segments"], r["largest_segment_bytes"])]
    assert all(r["device_wins"] for r in rows if r["file"] in chosen), chosen
    # encode_png's own 2160p files are why the route exists: they stay on it
    assert {"3840x2160-rgb8-ours", "3840x2160-rgba16-ours"} <= set(chosen) and "1024x1024-rgb8-ours" not in chosen


def test_plans_the_device_inflater_never_gets_by_default():
    from neural_enhanced_super_resolution_amd import imgproc
    big = 64 << 20
    assert _chosen(imgproc, big, 2000, 20000)
    assert not _chosen(imgproc, big, 2000, 20000, contiguous=0)
    assert not _chosen(imgproc, big, 1, 20000)
    assert not _chosen(imgproc, big, 2000, imgproc.PNG_DEVICE_SEGMENT_MAX + 1)
    assert _chosen(imgproc, imgproc.PNG_DEVICE_MIN_RATIO * 20000, 2000, 20000)
    assert not _chosen(imgproc, imgproc.PNG_DEVICE_MIN_RATIO * 20000 - 1, 2000, 20000)
