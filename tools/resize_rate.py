"""What the batched resize (jpeggpu_ext_resize_to_rgb) costs and saves, in one process, the variants alternating round by
round: a 64-image batch of BASELINE.json configs[2] (4032 x 3024 4:2:0, tools/jpegsynth) with seeded RandomResizedCrop
rectangles (8 to 100 % of the area, aspect 3/4 to 4/3), decoded with the ISLOW IDCT in one jpeggpu_ext_decode_batch call,
then resized to 224 x 224 (bilinear, NHWC) by one jpeggpu_ext_resize_to_rgb call:
  * images/s of the decode alone and of decode + resize, from device events;
  * the resize call alone (its copy of descriptors and tables and its two launches), from device events, and the host's
    time to enqueue it (weight tables included);
  * the sum of 64 jpeggpu_ext_crop_to_rgbi_fancy calls on the same planes: what the unfused route costs before it has
    resized anything.
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/resize_rate.py [--rounds 7] [--iters 10] [--out resize_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.crop_rate import _summary, _time, random_resized_crop  # noqa: E402


def run(rounds, iters, size=224):
    import numpy as np
    import torch

    import jpeggpu_amd
    from jpeggpu_amd.api import FILTERS, LAYOUTS, _img, _resize_items, lib
    from tests import pillow_resample_ref as R
    from tools import jpegsynth

    L = lib()
    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    datas = [cfg[i % 8] for i in range(64)]
    rng = np.random.default_rng(2024)
    rects = [random_resized_crop(rng, 4032, 3024) for _ in range(64)]

    bd = jpeggpu_amd.BatchDecode(datas, progressive=False, crops=rects)
    planes_list, infos, cis = bd.planes, bd.infos, bd.crop_infos

    items, _items_keep = _resize_items(planes_list, infos, cis)
    need = L.jpeggpu_ext_resize_scratch_size(items, 64, size, size, FILTERS["bilinear"])
    rscratch = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    out = torch.empty((64, size, size, 3), dtype=torch.uint8, device="cuda:0")

    decode = bd.decode

    def resize():
        st = L.jpeggpu_ext_resize_to_rgb(items, 64, size, size, FILTERS["bilinear"], LAYOUTS["NHWC"], out.data_ptr(),
                                         rscratch.data_ptr(), need, None)
        assert st == 0, jpeggpu_amd.status_string(st)

    srcs = [_img(planes) for planes in planes_list]
    crops_out = [torch.empty((ci.height, ci.width, 3), dtype=torch.uint8, device="cuda:0") for ci in cis]

    def crop64():
        for i in range(64):
            st = L.jpeggpu_ext_crop_to_rgbi_fancy(C.byref(infos[i]), C.byref(cis[i]), C.byref(srcs[i]), crops_out[i].data_ptr(),
                                                  3 * cis[i].width, None)
            assert st == 0

    decode()
    resize()
    crop64()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in (0, 17, 42):  # the result is the restatement of Pillow's resize of the crop's RGB
        assert np.array_equal(got[i], R.resize(crops_out[i].cpu().numpy(), size, size, "bilinear")), i

    res = {"decode_img_s": [], "decode_resize_img_s": [], "resize_ms": [], "resize_host_ms": [], "crop_to_rgbi_fancy_x64_ms": []}
    for _ in range(rounds):
        ms = _time(torch, decode, iters)
        res["decode_img_s"].append(64 * 1000.0 / ms)

        def both():
            decode()
            resize()

        ms = _time(torch, both, iters)
        res["decode_resize_img_s"].append(64 * 1000.0 / ms)
        res["resize_ms"].append(_time(torch, resize, iters))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            resize()
        res["resize_host_ms"].append((time.perf_counter() - t0) * 1000.0 / iters)
        torch.cuda.synchronize()
        res["crop_to_rgbi_fancy_x64_ms"].append(_time(torch, crop64, iters))
    area = sum(w * h for _, _, w, h in rects)
    return [{k: _summary(v, 4 if k.endswith("ms") else 1) for k, v in res.items()},
            {"rounds": rounds, "iters": iters, "images": 64, "out": [size, size], "filter": "bilinear", "layout": "NHWC",
             "crop_megapixels_mean": round(area / 64 / 1e6, 3), "resize_scratch_bytes": need}]


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
