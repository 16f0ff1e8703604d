"""Writes tests/golden/jpeg/*.jpg: Pillow's (libjpeg-turbo's) files for a subset of the JPEG grid, from the seeded images of
tests/jpeg_cases.py.  tests/test_jpeg_spec.py compares the specification with them, so that check needs no Pillow.

    python -m tests.make_jpeg_golden
"""
import io
import os

import numpy as np
from PIL import Image

from tests import jpeg_cases


def pillow_bytes(img, quality, order="rgb"):
    """PIL.Image.save(format="JPEG", quality=q): 4:2:0, baseline, standard tables -- cv2.imwrite's defaults at quality 95."""
    if img.ndim == 3 and order == "bgr":
        img = img[:, :, ::-1]
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img)).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def main():
    os.makedirs(os.path.join(jpeg_cases.GOLDEN, "jpeg"), exist_ok=True)
    for kind, h, w, c, quality in jpeg_cases.GOLDEN_FILES:
        img, order = jpeg_cases.image(kind, h, w, c)
        data = pillow_bytes(img, quality, order)
        path = jpeg_cases.golden_path(kind, h, w, c, quality)
        with open(path, "wb") as f:
            f.write(data)
        print(f"{path}: {len(data)} bytes")


if __name__ == "__main__":
    main()
