"""Writes tests/golden/truncated_pins.npz: the small files of the truncation tests (tests/truncated_ref.files, which Pillow
writes) and the SHA-256 of Pillow's RGB -- np.asarray(Image.open(f).convert("RGB")) with ImageFile.LOAD_TRUNCATED_IMAGES set --
at the pinned cuts of each (tests/truncated_ref.pin_cuts), so that the GPU tests need no Pillow. Needs Pillow on
libjpeg-turbo. Run from the repository root: python tools/make_truncated_pins.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import truncated_ref  # noqa: E402


def main():
    import PIL

    pins = {}
    for name, data in truncated_ref.files().items():
        cuts = truncated_ref.pin_cuts(data)
        pins["jpeg/" + name] = np.frombuffer(data, np.uint8)
        pins["cuts/" + name] = np.asarray(cuts, np.int32)
        pins["sha/" + name] = np.asarray([truncated_ref.sha(truncated_ref.pillow_rgb(data[:c])) for c in cuts])
    pins["pillow_version"] = np.frombuffer(PIL.__version__.encode(), np.uint8)
    np.savez_compressed(truncated_ref.PINS, **pins)
    print("%s: %d files, %d cuts, %d bytes" % (truncated_ref.PINS, len(truncated_ref.files()), sum(len(pins[k]) for k in pins if k.startswith("cuts/")),
                                                os.path.getsize(truncated_ref.PINS)))


if __name__ == "__main__":
    main()
