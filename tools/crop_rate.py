"""What a crop (jpeggpu_ext_set_crop) saves, in one process, cropped and uncropped alternating round by round:
  * the reference photo decoded on its own (jpeggpu_decoder_transfer + jpeggpu_decoder_decode): ms per image from device
    events, per-stage ms from jpeggpu_ext_set_profiling, and the bytes transfer copies -- uncropped, a centre 224 x 224
    crop and a band of half the image's height;
  * a 64-image batch of BASELINE.json configs[2] (4032 x 3024 4:2:0, tools/jpegsynth) through jpeggpu_ext_decode_batch,
    uncropped and with seeded RandomResizedCrop rectangles (8 to 100 % of the area, aspect 3/4 to 4/3): images/s of the
    decode call from device events, per-stage ms from the batch's stage timing, and the bytes transferred;
  * jpeggpu_ext_crop_to_rgbi_fancy of a 224 x 224 crop against jpeggpu_ext_planes_to_rgbi_fancy of the whole image.
Not bench.py: that one measures the flagship workload uncropped and stays as it is.

    python tools/crop_rate.py [--rounds 7] [--iters 10] [--out crop_rate.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def random_resized_crop(rng, width, height, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """torchvision's RandomResizedCrop.get_params with a numpy Generator: (x, y, w, h)."""
    area = width * height
    for _ in range(10):
        target = area * rng.uniform(*scale)
        aspect = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= width and 0 < h <= height:
            return int(rng.integers(0, width - w + 1)), int(rng.integers(0, height - h + 1)), w, h
    return 0, 0, width, height  # the fallback: the whole image


def _time(torch, fn, iters):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / iters


def _lone(torch, data, crop):
    import jpeggpu_amd

    dec = jpeggpu_amd.Decoder()
    if crop is not None:
        dec.set_crop(*crop)
    info = dec.parse_header(data)
    n = dec.get_buffer_size()
    tmp = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
    base = (tmp.data_ptr() + 255) // 256 * 256
    planes = [torch.empty((info.sizes_y[c], info.sizes_x[c]), dtype=torch.uint8, device="cuda:0") for c in range(info.num_components)]
    ptrs, pitches = [p.data_ptr() for p in planes], [p.stride(0) for p in planes]

    def run():
        dec.transfer(base, n, 0)
        dec.decode(ptrs, pitches, base, n, 0)

    return dec, run, (tmp, planes), dec.layout().transferred_bytes


def _batch(torch, datas, crops):
    import jpeggpu_amd

    return jpeggpu_amd.BatchDecode(datas, idct="reference", progressive=False, crops=crops)


def _summary(v, digits):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def run(rounds, iters):
    import numpy as np
    import torch

    import jpeggpu_amd
    from jpeggpu_amd.api import _img, lib
    from tools import jpegsynth

    photo = open(os.path.join(ROOT, "tests", "golden", "IMG_6510.JPG"), "rb").read()
    probe = jpeggpu_amd.Decoder()
    probe.parse_header(photo)
    pw, ph = probe.crop_info().width, probe.crop_info().height
    probe.cleanup()
    lone = {
        "uncropped": _lone(torch, photo, None),
        "centre_224": _lone(torch, photo, ((pw - 224) // 2, (ph - 224) // 2, 224, 224)),
        "band_50pct": _lone(torch, photo, (0, ph // 4, pw, ph // 2)),
    }
    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    datas = [cfg[i % 8] for i in range(64)]
    rng = np.random.default_rng(2024)
    rects = [random_resized_crop(rng, 4032, 3024) for _ in range(64)]
    batches = {"uncropped": _batch(torch, datas, [None] * 64), "random_resized_crop": _batch(torch, datas, rects)}
    for _, fn, _, _ in lone.values():  # warm-up
        fn()
    for bd in batches.values():
        bd.decode()
    torch.cuda.synchronize()

    # RGB: a centre 224 x 224 crop of one 12 MP 4:2:0 image against the whole image
    x0, y0 = (4032 - 224) // 2, (3024 - 224) // 2
    full_planes, full_info = jpeggpu_amd.decode_to_planes(cfg[0], idct="islow")
    crop_planes, crop_info, ci = jpeggpu_amd.decode_to_planes(cfg[0], idct="islow", crop=(x0, y0, 224, 224))
    stream = torch.cuda.current_stream().cuda_stream
    srcs = {"full": _img(full_planes), "crop": _img(crop_planes)}
    rgb_full = torch.empty((3024, 4032, 3), dtype=torch.uint8, device="cuda:0")
    rgb_crop = torch.empty((224, 224, 3), dtype=torch.uint8, device="cuda:0")
    rgb_calls = {
        "planes_to_rgbi_fancy_12mp": lambda: lib().jpeggpu_ext_planes_to_rgbi_fancy(
            C.byref(full_info), C.byref(srcs["full"]), rgb_full.data_ptr(), 3 * 4032, 4032, 3024, stream),
        "crop_to_rgbi_fancy_224": lambda: lib().jpeggpu_ext_crop_to_rgbi_fancy(
            C.byref(crop_info), C.byref(ci), C.byref(srcs["crop"]), rgb_crop.data_ptr(), 3 * 224, stream),
    }
    for fn in rgb_calls.values():
        assert fn() == 0
    torch.cuda.synchronize()
    assert np.array_equal(rgb_crop.cpu().numpy(), rgb_full[y0:y0 + 224, x0:x0 + 224].cpu().numpy())

    res_lone = {k: {"ms": [], "stages": []} for k in lone}
    res_batch = {k: {"img_s": [], "stages": []} for k in batches}
    res_rgb = {k: [] for k in rgb_calls}
    for _ in range(rounds):
        for k, (dec, fn, _, _) in lone.items():  # cropped and uncropped alternate inside every round
            res_lone[k]["ms"].append(_time(torch, fn, iters))
            dec.set_profiling(True)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            res_lone[k]["stages"].append(dec.stage_ms())
            dec.set_profiling(False)
        for k, bd in batches.items():
            ms = _time(torch, bd.decode, iters)
            res_batch[k]["img_s"].append(len(bd.decoders) * 1000.0 / ms)
            bd.batch.set_profiling(True)
            for _ in range(3):
                bd.decode()
            torch.cuda.synchronize()
            res_batch[k]["stages"].append(bd.batch.stage_ms())
            bd.batch.set_profiling(False)
        for k, fn in rgb_calls.items():
            res_rgb[k].append(_time(torch, fn, iters * 10))

    def stages(rows):
        return {s: round(statistics.median(r[s] for r in rows), 4) for s in rows[0]}

    out = []
    for k, v in res_lone.items():
        out.append({"workload": "photo_alone", "crop": k, "transfer_decode_ms": _summary(v["ms"], 4),
                    "stage_ms_median": stages(v["stages"]), "transferred_bytes": lone[k][3]})
    for k, v in res_batch.items():
        out.append({"workload": "batch64_cfg2", "crop": k, "img_s": _summary(v["img_s"], 1),
                    "stage_ms_median": stages(v["stages"]), "transferred_bytes": batches[k].transferred_bytes})
    for k, v in res_rgb.items():
        out.append({"workload": "rgb", "call": k, "ms": _summary(v, 4)})
    out.append({"rounds": rounds, "iters": iters, "rects_area_share": round(sum(w * h for _, _, w, h in rects) / (64 * 4032 * 3024), 4)})
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
