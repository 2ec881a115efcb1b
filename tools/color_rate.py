"""What the colour-aware RGB calls (jpeggpu_ext_*_cs) cost, in one process, the variants alternating round by round. A
64-image batch of BASELINE.json configs[2] (4032 x 3024 4:2:0, tools/jpegsynth) to RGB -- one jpeggpu_ext_decode_batch call
with the ISLOW IDCT, then one conversion call per image:
  1. "old_ycbcr": jpeggpu_ext_planes_to_rgbi_fancy, the entry point without a colour model;
  2. "cs_ycbcr": jpeggpu_ext_planes_to_rgbi_fancy_cs with JPEGGPU_EXT_COLOR_YCBCR on the same planes -- the same kernel
     instantiation, so it must be no slower than 1 by more than the run's spread (the condition, "holds");
  3. "cs_ycck": a YCCK batch of the same geometry (a fourth component at the luma's full size, an Adobe segment with
     transform 2) through jpeggpu_ext_planes_to_rgbi_fancy_cs: the four-tile instantiation and a fourth plane's bytes. Only
     recorded.
Milliseconds per call sequence from device events, medians of the rounds with their spread (max - min).
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/color_rate.py [--rounds 7] [--iters 10] [--images 64] [--out color_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.crop_rate import _time  # noqa: E402
from tools.draft_rate import _setup, _spread  # noqa: E402

ADOBE_YCCK = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x02"  # APP14, transform 2


def _rgb_cs(v, color):
    """The conversion of a _setup batch through the colour-aware entry point."""
    from jpeggpu_amd.api import lib

    L = lib()
    _planes, infos, cis = v["resize"]
    srcs, outs = v["srcs"], v["outs"]

    def rgb():
        for info, ci, src, out in zip(infos, cis, srcs, outs):
            st = L.jpeggpu_ext_planes_to_rgbi_fancy_cs(C.byref(info), color, C.byref(src), out.data_ptr(), 3 * ci.width, ci.width, ci.height, None)
            assert st == 0

    return rgb


def run(rounds, iters, images):
    import torch

    import jpeggpu_amd
    from tools import jpegsynth

    w, h = 4032, 3024
    ycc = [jpegsynth.config(2, seed=100 + s) for s in range(4)]
    four = [jpegsynth.encode(w, h, ((2, 2), (1, 1), (1, 1), (2, 2)), True, (w + 15) // 16, quality=88, noise=9, seed=200 + s) for s in range(4)]
    four = [f[:2] + ADOBE_YCCK + f[2:] for f in four]
    a = _setup(torch, [ycc[i % 4] for i in range(images)], 1, "uniform", images)
    b = _setup(torch, [four[i % 4] for i in range(images)], 1, "uniform", images)
    dec = jpeggpu_amd.Decoder()
    dec.parse_header(four[0])
    assert dec.color_space() == jpeggpu_amd.ColorSpace.YCCK
    dec.cleanup()
    CS = jpeggpu_amd.ColorSpace
    variants = {"old_ycbcr": (a["decode"], a["rgb"]), "cs_ycbcr": (a["decode"], _rgb_cs(a, int(CS.YCBCR))), "cs_ycck": (b["decode"], _rgb_cs(b, int(CS.YCCK)))}
    res = {k: {"to_rgb_ms": [], "rgb_ms": []} for k in variants}
    for decode, rgb in variants.values():  # warm-up
        decode()
        rgb()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, (decode, rgb) in variants.items():  # the variants alternate inside every round

            def both():
                decode()
                rgb()

            res[k]["to_rgb_ms"].append(_time(torch, both, iters))
            res[k]["rgb_ms"].append(_time(torch, rgb, iters))
    out = []
    old = {m: _spread(v) for m, v in res["old_ycbcr"].items()}
    for k, r in res.items():
        row = {"workload": "batch%d" % images, "images": images, "variant": k}
        row.update({m: _spread(v) for m, v in r.items()})
        if k == "cs_ycbcr":  # the condition: no slower than the old entry point by more than that run's spread
            row["vs_old"] = {m: {"old_median": old[m]["median"], "spread": max(old[m]["spread"], row[m]["spread"]),
                                 "holds": bool(row[m]["median"] <= old[m]["median"] + max(old[m]["spread"], row[m]["spread"]))} for m in old}
        out.append(row)
    out.append({"rounds": rounds, "iters": iters})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run(a.rounds, a.iters, a.images)
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
