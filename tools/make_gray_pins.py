"""Writes tests/golden/gray_pins.npz: Pillow's outputs for the grey tests (tests/gray_ref.pin_keys), so that the GPU tests
need no Pillow. Needs Pillow on libjpeg-turbo. Run from the repository root: python tools/make_gray_pins.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import gray_ref  # noqa: E402


def main():
    import PIL

    files = gray_ref.files()
    pins = {key: gray_ref.to_pin(make()) for key, make in gray_ref.pin_keys(files)}
    pins["pillow_version"] = np.frombuffer(PIL.__version__.encode(), np.uint8)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gray_pins.npz")
    np.savez_compressed(out, **pins)
    print("%s: %d arrays, %d bytes" % (out, len(pins), os.path.getsize(out)))


if __name__ == "__main__":
    main()
