"""What one jpeggpu_ext_batch_to_rgb call costs against the per-image route it replaces, in one process, the variants
alternating round by round (the method of tools/orient_rate.py).

Two inputs: "photos", 64 images of BASELINE.json configs[2] (4032 x 3024 4:2:0, tools/jpegsynth, 8 different files), and
"imagenet", 256 images of about 500 x 375 (32 different files of varying size, 4:2:0 and 4:2:2). For each:

(a) the conversion alone, on planes decoded once by one jpeggpu_ext_decode_batch call:
      * "batch_hwc_1" / "batch_hwc_6": ONE jpeggpu_ext_batch_to_rgb for all images, orientation 1 / 6 for every image;
        "loop_hwc_1" / "loop_hwc_6": the same items through one jpeggpu_ext_planes_to_rgbi_oriented call per image on one
        stream -- the route of the library without the batched call;
      * "batch_chw_1": the batched call with JPEGGPU_EXT_CHW; "loop_chw_1": the per-image call and
        permute(2, 0, 1).contiguous() of each result.
(b) end to end, from file bytes: "decode_batch_to_rgb" against a loop of decode_to_rgb, in images per second of wall
    time (both synchronise before they return).
The bar, per pair: the batched variant is not slower than the per-image one by more than the spread of the rounds
("holds"). Medians of the rounds with their spread (max - min); (a) in milliseconds per call sequence from device events.
The results of each pair are compared before anything is timed. Not bench.py: that one measures the flagship workload and
stays as it is.

    python tools/batch_rgb_rate.py [--rounds 7] [--iters 10] [--inputs photos,imagenet] [--out batch_rgb_rate.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.crop_rate import _time  # noqa: E402
from tools.draft_rate import _spread  # noqa: E402


def inputs(which):
    """The files of one input, repeated to its batch size."""
    import numpy as np

    from tools import jpegsynth

    if which == "photos":
        files = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
        return [files[i % 8] for i in range(64)]
    rng = np.random.default_rng(1000)
    files = []
    for s in range(32):
        w, h = 500 + int(rng.integers(-60, 61)), 375 + int(rng.integers(-50, 51))
        sampling = ((2, 2), (1, 1), (1, 1)) if s % 4 else ((2, 1), (1, 1), (1, 1))
        files.append(jpegsynth.encode(w, h, sampling, quality=85, noise=8, seed=300 + s))
    return [files[i % 32] for i in range(256)]


def _not_slower(new, old, higher_is_better=False):
    spread = max(new["spread"], old["spread"])
    ok = new["median"] + spread >= old["median"] if higher_is_better else new["median"] <= old["median"] + spread
    ratio = new["median"] / old["median"] if old["median"] else None
    return {"spread": spread, "batched_over_per_image": round(ratio, 4) if ratio is not None else None, "holds": bool(ok)}


def _decode_planes(torch, datas):
    """All files decoded by one jpeggpu_ext_decode_batch call (ISLOW): (planes_list, infos)."""
    import jpeggpu_amd

    with jpeggpu_amd.BatchDecode(datas, progressive=False) as bd:
        bd.decode()
        torch.cuda.synchronize()
        return bd.planes, bd.infos


def conversion(torch, which, datas, rounds, iters):
    import jpeggpu_amd
    from jpeggpu_amd.api import IMAGE_LAYOUTS, RgbItem, _frame_size, _resize_items

    L = jpeggpu_amd.lib()
    n = len(datas)
    planes_list, infos = _decode_planes(torch, datas)
    items, _keep = _resize_items(planes_list, infos, None)
    sizes = [_frame_size(i) for i in infos]
    YCBCR = int(jpeggpu_amd.ColorSpace.YCBCR)
    need = L.jpeggpu_ext_batch_rgb_scratch_size(n)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda:0")

    def outputs(o, layout):
        shapes = [((w, h, 3) if o >= 5 else (h, w, 3)) if layout == "HWC" else ((3, w, h) if o >= 5 else (3, h, w)) for w, h in sizes]
        return [torch.empty(s, dtype=torch.uint8, device="cuda:0") for s in shapes]

    def batched(o, layout):
        outs = outputs(o, layout)
        rgb = (RgbItem * n)()
        for i, t in enumerate(outs):
            rgb[i].info, rgb[i].crop, rgb[i].src = items[i].info, items[i].crop, items[i].src
            rgb[i].color, rgb[i].orientation, rgb[i].replicate = YCBCR, o, 0
            rgb[i].dst = t.data_ptr()
            rgb[i].dst_pitch = t.stride(0) if layout == "HWC" else t.stride(1)
            rgb[i].plane_stride = t.stride(0) if layout == "CHW" else 0

        def fn():
            assert L.jpeggpu_ext_batch_to_rgb(rgb, n, IMAGE_LAYOUTS[layout], scratch.data_ptr(), need, None) == 0

        return fn, outs

    def looped(o, layout):
        outs = outputs(o, "HWC")
        final = [None] * n

        def fn():
            for i, t in enumerate(outs):
                w, h = sizes[i]
                assert L.jpeggpu_ext_planes_to_rgbi_oriented(items[i].info, YCBCR, o, 0, items[i].src, t.data_ptr(), t.stride(0), w, h, None) == 0
                final[i] = t.permute(2, 0, 1).contiguous() if layout == "CHW" else t

        return fn, final

    pairs = {"hwc_1": (1, "HWC"), "hwc_6": (6, "HWC"), "chw_1": (1, "CHW")}
    variants = {}
    for key, (o, layout) in pairs.items():
        fb, ob = batched(o, layout)
        fl, ol = looped(o, layout)
        fb()
        fl()
        torch.cuda.synchronize()
        for i in range(n):  # the routes agree
            assert torch.equal(ob[i], ol[i]), (key, i)
        variants["batch_" + key], variants["loop_" + key] = fb, fl
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():  # the variants alternate inside every round
            res[k].append(_time(torch, fn, iters))
    r = {k: _spread(v) for k, v in res.items()}
    out = [dict(input=which, images=n, measure="conversion_ms", variant=k, ms=v) for k, v in r.items()]
    out.append({"input": which, "measure": "conversion_ms",
                **{"batch_%s_vs_loop" % key: _not_slower(r["batch_" + key], r["loop_" + key]) for key in pairs}})
    return out


def end_to_end(torch, which, datas, rounds):
    import jpeggpu_amd

    n = len(datas)

    def batched():
        return jpeggpu_amd.decode_batch_to_rgb(datas)

    def looped():
        return [jpeggpu_amd.decode_to_rgb(d) for d in datas]

    a, b = batched(), looped()
    for i in range(0, n, max(n // 16, 1)):
        assert torch.equal(a[i], b[i]), i
    del a, b
    variants = {"decode_batch_to_rgb": batched, "loop_decode_to_rgb": looped}
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[k].append(n / (time.perf_counter() - t0))
    r = {k: _spread(v, 1) for k, v in res.items()}
    out = [dict(input=which, images=n, measure="end_to_end_images_per_s", variant=k, images_per_s=v) for k, v in r.items()]
    out.append({"input": which, "measure": "end_to_end_images_per_s",
                "batch_vs_loop": _not_slower(r["decode_batch_to_rgb"], r["loop_decode_to_rgb"], higher_is_better=True)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--inputs", default="photos,imagenet")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    res = []
    for which in a.inputs.split(","):
        datas = inputs(which)
        part = conversion(torch, which, datas, a.rounds, a.iters)
        torch.cuda.empty_cache()
        part += end_to_end(torch, which, datas, a.rounds)
        torch.cuda.empty_cache()
        for r in part:
            print(json.dumps(r), flush=True)
        res += part
        if a.out:  # written after each input: a run cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res + [{"rounds": a.rounds, "iters": a.iters}], f, indent=1)


if __name__ == "__main__":
    main()
