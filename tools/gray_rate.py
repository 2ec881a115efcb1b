"""What grey output saves, in one process, grey and RGB alternating round by round:
  * a 64-image batch of BASELINE.json configs[2] (4032 x 3024 4:2:0, tools/jpegsynth) through jpeggpu_ext_decode_batch,
    luma-only (Decoder.set_luma_only) against ordinary: ms of the decode call from device events and of its IDCT stage
    from the batch's stage timing, with the reference transform and with ISLOW;
  * decode_resized(..., 224, mode="L") against mode="RGB" on that batch with the same seeded RandomResizedCrop
    rectangles: ms of the whole call on the host's clock (it parses, decodes, resizes and synchronises), and of the resize
    call alone (jpeggpu_ext_resize_view_to_gray_tensor against jpeggpu_ext_resize_to_rgb_cs) from device events, with the
    scratch bytes of both.
Nothing is asserted. Not bench.py: that one measures the flagship workload in RGB and stays as it is.

    python tools/gray_rate.py [--rounds 7] [--iters 5] [--out gray_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.crop_rate import _summary, _time, random_resized_crop  # noqa: E402


def run(rounds, iters):
    import numpy as np
    import torch

    import jpeggpu_amd
    from jpeggpu_amd.api import BatchDecode, resize_scratch_size, resize_to_gray, resize_to_rgb
    from tools import jpegsynth

    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    datas = [cfg[i % 8] for i in range(64)]
    rng = np.random.default_rng(2024)
    rects = [random_resized_crop(rng, 4032, 3024) for _ in range(64)]

    batches = {"%s_%s" % (idct, kind): BatchDecode(datas, idct=idct, progressive=False, luma_only=kind == "luma")
               for idct in ("reference", "islow") for kind in ("ordinary", "luma")}
    cropped = {kind: BatchDecode(datas, crops=rects, luma_only=kind == "L") for kind in ("RGB", "L")}
    for bd in list(batches.values()) + list(cropped.values()):
        bd.decode()
    torch.cuda.synchronize()
    resize = {
        "RGB": lambda: resize_to_rgb(cropped["RGB"].planes, cropped["RGB"].infos, 224, cropped["RGB"].crop_infos, colors=cropped["RGB"].colors),
        "L": lambda: resize_to_gray(cropped["L"].planes, cropped["L"].infos, 224, cropped["L"].crop_infos, colors=cropped["L"].colors),
    }
    pipeline = {mode: (lambda mode=mode: jpeggpu_amd.decode_resized(datas, 224, crops=rects, mode=mode)) for mode in ("RGB", "L")}
    for fn in list(resize.values()) + list(pipeline.values()):
        fn()
    torch.cuda.synchronize()

    res = {"decode_ms": {k: [] for k in batches}, "idct_ms": {k: [] for k in batches}, "resize_ms": {k: [] for k in resize},
           "decode_resized_ms": {k: [] for k in pipeline}}
    for _ in range(rounds):
        for k, bd in batches.items():  # luma-only and ordinary alternate inside every round
            res["decode_ms"][k].append(_time(torch, bd.decode, iters))
            bd.batch.set_profiling(True)
            for _ in range(3):
                bd.decode()
            torch.cuda.synchronize()
            res["idct_ms"][k].append(bd.batch.stage_ms()["idct"])
            bd.batch.set_profiling(False)
        for k, fn in resize.items():
            res["resize_ms"][k].append(_time(torch, fn, iters))
        for k, fn in pipeline.items():
            t0 = time.perf_counter()
            fn()
            res["decode_resized_ms"][k].append((time.perf_counter() - t0) * 1e3)
    out = {what: {k: _summary(v, 3) for k, v in by.items()} for what, by in res.items()}
    out["resize_scratch_bytes"] = {
        "RGB": resize_scratch_size(cropped["RGB"].planes, cropped["RGB"].infos, 224, cropped["RGB"].crop_infos, colors=cropped["RGB"].colors),
        "L": _gray_scratch(cropped["L"]),
    }
    out["rounds"], out["iters"], out["device"] = rounds, iters, torch.cuda.get_device_name(0)
    for bd in list(batches.values()) + list(cropped.values()):
        bd.close()
    return out


def _gray_scratch(bd):
    from jpeggpu_amd.api import FILTERS, _color_array, _resize_items, lib

    n = len(bd.planes)
    items, _keep = _resize_items(bd.planes, bd.infos, bd.crop_infos)
    return lib().jpeggpu_ext_resize_view_to_gray_scratch_size(items, _color_array(bd.colors, n), None, None, n, 224, 224, FILTERS["bilinear"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run(a.rounds, a.iters)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
