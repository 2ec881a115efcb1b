"""What thumbnails cost, in one process, the variants alternating inside every round (the method of tools/tensor_rate.py):
the 64 photographs of tools/resize_rate.py (BASELINE.json configs[2], 4032 x 3024 4:2:0, tools/jpegsynth) to Pillow's
thumbnail((128, 128)) -- 1/8 decode, then the resize from the box 504 x 378 -- and thumbnail((48, 48)) -- 1/8 decode, reduce
(5, 5), then the resize --, bicubic, reducing_gap 2.

  * "decode_thumbnails": the list of files to the list of thumbnail tensors (parse, transfer, one decode batch, one
    jpeggpu_ext_thumbnail_to_rgb call).
  * "thumbnail_jpeg": the same and one encode call, to the list of files' bytes on the host.
  * "decode_resized": the parent's nearest route -- decode_resized at the same scales to the thumbnail's size as a fixed
    size, which does the same decode work but resizes without the reduction and from the integer box: not Pillow's
    thumbnail.
  * "thumbnails_to_rgb_alone" / "resize_to_rgb_alone": the second step of the first and of the third route on planes that
    are already decoded (scratch allocation, tables, copy and launches).
  * "pillow": im.thumbnail(...) of every file on one CPU thread ("pillow_jpeg": and im.save(..., "JPEG", quality=75)),
    by the wall clock; left out where Pillow does not import.
Medians of the rounds with their spread (max - min), in milliseconds per call over all 64 files, from device events (the
calls synchronise themselves, so the host's share is inside). Before anything is timed the first thumbnails are compared with
Pillow's where it imports.
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/thumbnail_rate.py [--rounds 7] [--iters 3] [--out thumbnail_rate.json]
"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.crop_rate import _time  # noqa: E402
from tools.draft_rate import _spread  # noqa: E402

REQUESTS = ((128, 128), (48, 48))
FILTER, GAP, QUALITY = "bicubic", 2.0, 75


def _wall(fn, iters):
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) * 1e3 / iters


def run(rounds, iters, n=64):
    import numpy as np
    import torch

    import jpeggpu_amd
    from tools import jpegsynth

    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    datas = [cfg[i % 8] for i in range(n)]
    W, H = 4032, 3024
    try:
        from PIL import Image
    except ImportError:
        Image = None

    def pillow(req, save):
        for d in datas:
            im = Image.open(io.BytesIO(d))
            im.thumbnail(req, Image.Resampling.BICUBIC, reducing_gap=GAP)
            if save:
                im.save(io.BytesIO(), "JPEG", quality=QUALITY)

    variants, plans = {}, {}
    for req in REQUESTS:
        p = plans[req] = jpeggpu_amd.thumbnail_plan(W, H, req, FILTER, GAP)
        tag = "%dx%d" % req
        variants["decode_thumbnails_" + tag] = (_time, lambda req=req: jpeggpu_amd.decode_thumbnails(datas, req, FILTER, GAP))
        variants["thumbnail_jpeg_" + tag] = (_time, lambda req=req: jpeggpu_amd.thumbnail_jpeg(datas, req, FILTER, GAP, quality=QUALITY))
        variants["decode_resized_" + tag] = (_time, lambda p=p: jpeggpu_amd.decode_resized(datas, (p.out_h, p.out_w), filt=FILTER, scales=[p.scale] * n))
        if Image is not None:
            variants["pillow_" + tag] = (_wall, lambda req=req: pillow(req, False))
            variants["pillow_jpeg_" + tag] = (_wall, lambda req=req: pillow(req, True))
            got = jpeggpu_amd.decode_thumbnails(datas[:8], req, FILTER, GAP)
            for d, g in zip(datas[:8], got):
                im = Image.open(io.BytesIO(d))
                im.thumbnail(req, Image.Resampling.BICUBIC, reducing_gap=GAP)
                assert np.array_equal(g.cpu().numpy(), np.asarray(im)), "a thumbnail differs from Pillow's"
    # the second step alone, on planes that are already decoded: the thumbnail call against the resize call it stands beside
    keep = []
    for req in REQUESTS:
        p, tag = plans[req], "%dx%d" % req
        bd = jpeggpu_amd.BatchDecode(datas, scales=[p.scale] * n)
        bd.decode()
        keep.append(bd)
        ps = [jpeggpu_amd.thumbnail_plan(W, H, req, FILTER, GAP) for _ in range(n)]
        variants["thumbnails_to_rgb_alone_" + tag] = (_time, lambda bd=bd, ps=ps, p=p: jpeggpu_amd.thumbnails_to_rgb(
            bd.planes, bd.infos, ps, (p.out_h, p.out_w), FILTER, bd.colors))
        variants["resize_to_rgb_alone_" + tag] = (_time, lambda bd=bd, p=p: jpeggpu_amd.resize_to_rgb(
            bd.planes, bd.infos, (p.out_h, p.out_w), None, FILTER, colors=bd.colors))
    for timer, fn in variants.values():  # warm up: allocator, staging ring, code objects
        if timer is _time:
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (timer, fn) in variants.items():  # the variants alternate inside every round
            res[k].append(timer(torch, fn, iters) if timer is _time else timer(fn, 1))
    out = [dict(variant=k, ms=_spread(v), images_per_s=round(n * 1e3 / _spread(v)["median"], 1)) for k, v in res.items()]
    for req, p in plans.items():
        out.append({"request": list(req), "scale": p.scale, "decoded": [p.dec_w, p.dec_h], "factors": [p.fx, p.fy], "reduced": [p.red_w, p.red_h],
                    "thumbnail": [p.out_w, p.out_h]})
    out.append({"rounds": rounds, "iters": iters, "images": n, "filter": FILTER, "reducing_gap": GAP, "quality": QUALITY, "pillow": Image is not None})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run(a.rounds, a.iters)
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
