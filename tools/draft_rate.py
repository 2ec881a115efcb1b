"""What libjpeg's scale mode (jpeggpu_ext_set_scale_mode, JPEGGPU_EXT_SCALE_LIBJPEG) costs and saves, in one process, the
variants alternating round by round. To RGB -- one jpeggpu_ext_decode_batch call, then one conversion call per image --
for the reference photo alone and for a 64-image batch of BASELINE.json configs[2] (4032 x 3024 4:2:0, tools/jpegsynth),
at d = 2, 4, 8:
  1. "libjpeg": the new mode at 1/d (per-component IDCT sizes) + jpeggpu_ext_planes_to_rgbi_fancy (a 4:2:0 file has no
     subsampling left at any reduced scale: the call copies and converts);
  2. "full_islow": the ISLOW IDCT at full size + jpeggpu_ext_planes_to_rgbi_fancy -- the only route to Pillow's pixels
     without the mode, before the caller shrinks the image on its own; the same work at every d;
  3. "uniform": the uniform scaled decode at 1/d + jpeggpu_ext_planes_to_rgbi_fancy (the pixel count of 1, not Pillow's
     pixels): what the 8 x 8 chroma costs and what the missing upsampling saves.
Milliseconds per call sequence from device events, the `idct` stage's ms from the batch's stage timing, medians of the
rounds with their spread (max - min). Then the RandomResizedCrop batch of tools/resize_rate.py through decode + resize,
at scale 1 and at the scale draft_scale picks for each crop.
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/draft_rate.py [--rounds 7] [--iters 10] [--out draft_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.crop_rate import _time, random_resized_crop  # noqa: E402

SCALES = (2, 4, 8)


def _setup(torch, datas, scale, mode, hint, crops=None):
    """A batch of decoders at one scale (or one per image) and mode, transferred, with their planes: decode(), rgb() and
    what the resize takes; "srcs" and "outs" are rgb()'s Img and output of every image (tools/color_rate.py)."""
    import jpeggpu_amd
    from jpeggpu_amd.api import _img, lib

    scales = list(scale) if isinstance(scale, (list, tuple)) else [scale] * len(datas)
    bd = jpeggpu_amd.BatchDecode(datas, hint=hint, progressive=False, scales=scales, scale_mode=mode, crops=crops)
    infos, cis = bd.infos, [dec.crop_info() for dec in bd.decoders]  # (without a crop: the whole image at the scale)
    srcs = [_img(planes) for planes in bd.planes]
    outs = [torch.empty((ci.height, ci.width, 3), dtype=torch.uint8, device="cuda:0") if crops is None else None for ci in cis]
    L = lib()

    def rgb():
        for info, ci, src, out in zip(infos, cis, srcs, outs):
            st = L.jpeggpu_ext_planes_to_rgbi_fancy(C.byref(info), C.byref(src), out.data_ptr(), 3 * ci.width, ci.width, ci.height, None)
            assert st == 0

    return {"decode": bd.decode, "rgb": rgb, "batch": bd.batch, "keep": bd, "srcs": srcs, "outs": outs, "resize": (bd.planes, infos, cis),
            "n": len(datas)}


def _spread(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread": round(max(v) - min(v), digits)}


def run(rounds, iters, size=224):
    import numpy as np
    import torch

    import jpeggpu_amd
    from jpeggpu_amd.api import FILTERS, LAYOUTS, _resize_items, lib
    from tools import jpegsynth

    photo = open(os.path.join(ROOT, "tests", "golden", "IMG_6510.JPG"), "rb").read()
    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    work = {"photo": ([photo], 0), "batch64": ([cfg[i % 8] for i in range(64)], 64)}
    out = []
    for wname, (datas, hint) in work.items():
        variants = {("full_islow", 1): _setup(torch, datas, 1, "uniform", hint)}
        for d in SCALES:
            variants[("libjpeg", d)] = _setup(torch, datas, d, "libjpeg", hint)
            variants[("uniform", d)] = _setup(torch, datas, d, "uniform", hint)
        res = {k: {"to_rgb_ms": [], "decode_ms": [], "rgb_ms": [], "idct_ms": []} for k in variants}
        for v in variants.values():  # warm-up
            v["decode"]()
            v["rgb"]()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, v in variants.items():  # the variants alternate inside every round

                def both():
                    v["decode"]()
                    v["rgb"]()

                res[k]["to_rgb_ms"].append(_time(torch, both, iters))
                res[k]["decode_ms"].append(_time(torch, v["decode"], iters))
                res[k]["rgb_ms"].append(_time(torch, v["rgb"], iters))
                v["batch"].set_profiling(True)  # (a new measurement window)
                for _ in range(3):
                    v["decode"]()
                torch.cuda.synchronize()
                res[k]["idct_ms"].append(v["batch"].stage_ms()["idct"])
                v["batch"].set_profiling(False)
        full = _spread(res[("full_islow", 1)]["to_rgb_ms"])
        for (mode, d), r in res.items():
            row = {"workload": wname, "images": len(datas), "variant": mode, "scale": d}
            row.update({k: _spread(v) for k, v in r.items()})
            if mode == "libjpeg":  # the condition: no slower than the full-size route by more than that route's own spread
                row["vs_full_islow"] = {"full_islow_median": full["median"], "full_islow_spread": full["spread"],
                                        "holds": bool(row["to_rgb_ms"]["median"] <= full["median"] + full["spread"])}
            out.append(row)
        del variants
        torch.cuda.empty_cache()

    # RandomResizedCrop: decode + resize to size x size, at scale 1 and at draft_scale's choice for each crop
    L = lib()
    datas = work["batch64"][0]
    rng = np.random.default_rng(2024)
    rects = [random_resized_crop(rng, 4032, 3024) for _ in range(64)]
    scales = [jpeggpu_amd.draft_scale(w, h, (size, size)) for _, _, w, h in rects]
    groups = {"scale_1": ([1] * 64, rects),
              "draft_scale": (scales, [(x // d, y // d, max(1, w // d), max(1, h // d)) for (x, y, w, h), d in zip(rects, scales)])}
    calls = {}
    for gname, (sc, rc) in groups.items():
        s = _setup(torch, datas, sc, "libjpeg", 64, rc)  # any mix of scales in ONE batch
        decode = s["decode"]
        items, items_keep = _resize_items(*s["resize"])
        need = L.jpeggpu_ext_resize_scratch_size(items, 64, size, size, FILTERS["bilinear"])
        rscratch = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda:0")
        dst = torch.empty((64, size, size, 3), dtype=torch.uint8, device="cuda:0")

        def both(decode=decode, items=items, need=need, rscratch=rscratch, dst=dst):
            decode()
            st = L.jpeggpu_ext_resize_to_rgb(items, 64, size, size, FILTERS["bilinear"], LAYOUTS["NHWC"], dst.data_ptr(), rscratch.data_ptr(), need, None)
            assert st == 0, jpeggpu_amd.status_string(st)

        both()
        calls[gname] = (both, (s, items_keep, rscratch, dst))
    torch.cuda.synchronize()
    rr = {g: [] for g in calls}
    for _ in range(rounds):
        for g, (fn, _keep) in calls.items():
            rr[g].append(_time(torch, fn, iters))
    row = {"workload": "random_resized_crop_64", "out": [size, size], "scales_picked": {str(d): scales.count(d) for d in (1, 2, 4, 8)}}
    row.update({g + "_ms": _spread(v) for g, v in rr.items()})
    row.update({g + "_img_s": round(64 * 1000.0 / statistics.median(v), 1) for g, v in rr.items()})
    out.append(row)
    out.append({"rounds": rounds, "iters": iters})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run(a.rounds, a.iters)
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
