#!/usr/bin/env python3
"""Writes tests/golden/encode_fit_pins.npz: for every case of tests/encode_fit_ref.cases() the lengths of the files Pillow (on
libjpeg-turbo) writes at every quality 1..100 -- Image.fromarray(a).save(f, "JPEG", quality=, subsampling=,
restart_marker_blocks=, optimize=) -- and, for the budgets encode_fit_ref.budgets() places on that table within the case's
range, the quality the rule of jpeggpu_ext_encode_fit_batch picks (encode_fit_ref.choose), and length and SHA-256 of its
file. Chosen files of up to WHOLE_FILE_LIMIT bytes are stored whole, once per case and quality. The tests read the pins and
never import Pillow.

The rule is a bisection and Pillow's sizes are not monotone in the quality, so its answer is not always the largest quality
that fits. The pins are only written if at least MIN_DIFFERENT cases hold a budget for which the two differ: the tests rely
on the list to tell the two apart.

    python tools/make_encode_fit_pins.py
"""
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WHOLE_FILE_LIMIT = 4096
MAX_DIPS = 6  # budgets in dips per case
MIN_DIFFERENT = 5
PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def main():
    import PIL
    from PIL import Image, ImageFile, features

    from tests import encode_fit_ref as F

    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the pins are libjpeg-turbo's: this Pillow is built on another libjpeg")
    if sys.argv[1:]:
        raise SystemExit(__doc__)
    ImageFile.MAXBLOCK = 1 << 24  # optimize=True: the whole file leaves libjpeg at once (make_encode_opt_pins.py)
    versions = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"))
    out, index, different = {}, [], []
    for case in F.cases():
        im = Image.fromarray(F.image(case))
        files = {}
        for q in range(1, 101):
            f = io.BytesIO()
            im.save(f, "JPEG", quality=q, subsampling=PILLOW_SUBSAMPLING[case["subsampling"]], restart_marker_blocks=case["restart_interval"],
                    optimize=case["optimize"])
            files[q] = f.getvalue()
        table = {q: len(files[q]) for q in files}
        lo, hi = case["lo"], case["hi"]
        entries, whole, differs = [], set(), False
        for budget in F.budgets(table, lo, hi, MAX_DIPS):
            q = F.choose(table.__getitem__, lo, hi, budget)
            differs |= q != F.largest_fitting(table.__getitem__, lo, hi, budget)
            if q is None:
                entries.append(dict(budget=budget, quality=-1, length=table[lo], sha256=""))
                continue
            entries.append(dict(budget=budget, quality=q, length=table[q], sha256=hashlib.sha256(files[q]).hexdigest()))
            if table[q] <= WHOLE_FILE_LIMIT:
                whole.add(q)
        if differs:
            different.append(case["name"])
        out["sizes_" + case["name"]] = np.asarray([table[q] for q in range(1, 101)], np.int32)
        for q in sorted(whole):
            out["file_%s_q%d" % (case["name"], q)] = np.frombuffer(files[q], np.uint8)
        index.append(dict(name=case["name"], budgets=entries, whole=sorted(whole)))
    if len(different) < MIN_DIFFERENT:
        raise SystemExit("only %d cases hold a budget where the rule's answer is not the largest quality that fits (%s): %d are needed"
                         % (len(different), ", ".join(different), MIN_DIFFERENT))
    out["meta"] = np.frombuffer(json.dumps(dict(versions, cases=index, different=different)).encode(), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "encode_fit_pins.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d budgets, %d whole files, %d cases where the rule differs from the largest fitting quality, %d bytes"
          % (path, len(index), sum(len(e["budgets"]) for e in index), sum(len(e["whole"]) for e in index), len(different), os.path.getsize(path)))


if __name__ == "__main__":
    main()
