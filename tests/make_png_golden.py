"""Writes the committed files of tests/golden/png from the specification (tests/png_ref.py): python -m tests.make_png_golden.
They pin the specification against edits: tests/test_png_spec.py compares them byte for byte."""
import os

from tests import png_cases


def main():
    os.makedirs(os.path.join(png_cases.GOLDEN, "png"), exist_ok=True)
    for entry in png_cases.GOLDEN_FILES:
        data = png_cases.spec(*entry)[0]
        with open(png_cases.golden_path(*entry), "wb") as f:
            f.write(data)
        print(png_cases.golden_path(*entry), len(data))


if __name__ == "__main__":
    main()
