"""Writes tests/golden/jpeg_options: Pillow's (libjpeg-turbo's) files for a subset of the option grid of tests/jpeg_options_cases.py,
and length_limit.json, the length and sha256 of Pillow's files of the two 512 x 512 length-limit frames.
tests/test_jpeg_options_spec.py compares the specification with them, so that check needs no Pillow.

    python -m tests.make_jpeg_options_golden
"""
import hashlib
import io
import json
import os

import numpy as np
from PIL import Image

from tests import jpeg_options_cases as cases


def pillow_bytes(img, quality, order="rgb", sampling="4:2:0", optimize=False, restart_interval=0):
    """PIL.Image.save(format="JPEG") with the options; a gray frame is saved without `subsampling`, which it ignores."""
    if img.ndim == 3 and order == "bgr":
        img = img[:, :, ::-1]
    kw = {"subsampling": sampling} if img.ndim == 3 else {}
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img)).save(buf, format="JPEG", quality=quality, optimize=bool(optimize), restart_marker_blocks=int(restart_interval), **kw)
    return buf.getvalue()


def pillow_file(f):
    kind, h, w, layout, q, opt, ri = f
    return pillow_bytes(cases.image(kind, h, w, layout), q, "rgb", "4:2:0" if layout == "gray" else layout, opt, ri)


def main():
    os.makedirs(cases.GOLDEN, exist_ok=True)
    for f in cases.GOLDEN_FILES:
        data = pillow_file(f)
        with open(cases.golden_path(f), "wb") as out:
            out.write(data)
        print(f"{cases.golden_path(f)}: {len(data)} bytes")
    digests = {}
    for q, sampling in cases.LENGTH_LIMIT:
        data = pillow_bytes(cases.length_limit_image(), q, "rgb", sampling, True, 0)
        digests[f"q{q}_{sampling}"] = {"length": len(data), "sha256": hashlib.sha256(data).hexdigest()}
    with open(cases.length_limit_digest_path(), "w") as out:
        json.dump(digests, out, indent=1, sort_keys=True)
        out.write("\n")
    print(digests)


if __name__ == "__main__":
    main()
