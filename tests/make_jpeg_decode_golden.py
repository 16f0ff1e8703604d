"""Writes tests/golden/jpeg_decode: the files of jpeg_decode_cases.GOLDEN_FILES as Pillow writes them, and Pillow's decode of each as
.npy (RGB order, or gray).  Run once with Pillow installed: python -m tests.make_jpeg_decode_golden.  reference_test.jpeg, the
reference's images/test.jpeg, is committed beside them as it is; its pixels are tests/golden/test_jpeg_full.npz['input_bgr']."""
import io
import os

import numpy as np

from tests import jpeg_decode_cases as dc


def pillow_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def main():
    os.makedirs(dc.GOLDEN, exist_ok=True)
    for entry in dc.GOLDEN_FILES:
        data = dc.write_file(*entry)
        name = dc.golden_name(*entry)
        with open(name + ".jpg", "wb") as f:
            f.write(data)
        np.save(name + ".npy", pillow_pixels(data))
        print(name, len(data))


if __name__ == "__main__":
    main()
