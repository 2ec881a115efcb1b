"""What applying the EXIF orientation on the GPU costs and saves, in one process, the variants alternating round by round.

1. One BASELINE.json configs[2] image (4032 x 3024 4:2:0, tools/jpegsynth), decoded once with the ISLOW IDCT, to DISPLAYED RGB:
     * "old_1" / "new_1": jpeggpu_ext_planes_to_rgbi_fancy against jpeggpu_ext_planes_to_rgbi_oriented with orientation 1 --
       the same kernel, so equal within the spread;
     * "new_3", "new_6": the oriented call; "two_step_3", "two_step_6": what a user of the library without it does --
       jpeggpu_ext_planes_to_rgbi_fancy, then torch.flip / torch.rot90(...).contiguous() of the 36 MB result. The bar: the
       oriented call is faster by more than the run's spread ("holds"); it writes the image once, not twice.
2. The 64-image RandomResizedCrop batch of tools/resize_rate.py to 224 x 224 with every image at orientation 6 (the crops
   drawn in displayed coordinates and mapped by jpeggpu_ext_orient_rect): "oriented_6" is one
   jpeggpu_ext_resize_to_rgb_oriented call; "oriented_1" and "cs_1" the same stored rectangles without orientation, through
   the new and the old entry point; "unfused_6" the route without the call: 64 jpeggpu_ext_crop_to_rgbi_fancy, torch.rot90
   (...).contiguous() and torch's antialiased bilinear interpolation of each -- which is not Pillow's arithmetic. Recorded,
   no bar.
Milliseconds per call sequence from device events, medians of the rounds with their spread (max - min). The results of
the variants that must agree are compared before anything is timed. Not bench.py: that one measures the flagship
workload and stays as it is.

    python tools/orient_rate.py [--rounds 7] [--iters 10] [--out orient_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.crop_rate import _time, random_resized_crop  # noqa: E402
from tools.draft_rate import _spread  # noqa: E402


def _rounds(torch, variants, rounds, iters):
    res = {k: [] for k in variants}
    for fn in variants.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in variants.items():  # the variants alternate inside every round
            res[k].append(_time(torch, fn, iters))
    return {k: _spread(v) for k, v in res.items()}


def _faster(new, old):
    spread = max(new["spread"], old["spread"])
    return {"spread": spread, "holds": bool(new["median"] + spread < old["median"])}


def photo(rounds, iters):
    import torch

    import jpeggpu_amd
    from jpeggpu_amd.api import _img
    from tools import jpegsynth

    L = jpeggpu_amd.lib()
    w, h = 4032, 3024
    planes, info = jpeggpu_amd.decode_to_planes(jpegsynth.config(2, seed=100), idct="islow")
    src = _img(planes)
    stored = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0")
    upright = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0")
    turned = torch.empty((w, h, 3), dtype=torch.uint8, device="cuda:0")
    YCBCR = int(jpeggpu_amd.ColorSpace.YCBCR)

    def old():
        assert L.jpeggpu_ext_planes_to_rgbi_fancy(C.byref(info), C.byref(src), stored.data_ptr(), 3 * w, w, h, None) == 0

    def new(o):
        out = turned if o >= 5 else upright

        def fn():
            assert L.jpeggpu_ext_planes_to_rgbi_oriented(C.byref(info), YCBCR, o, 0, C.byref(src), out.data_ptr(), out.stride(0), w, h, None) == 0

        return fn

    keep = {}

    def two_step_3():
        old()
        keep[3] = torch.flip(stored, (0, 1))  # a copy: flip never returns a view

    def two_step_6():
        old()
        keep[6] = torch.rot90(stored, -1, (0, 1)).contiguous()

    for o, two in ((3, two_step_3), (6, two_step_6)):  # the routes agree
        new(o)()
        two()
        torch.cuda.synchronize()
        assert torch.equal(keep[o], turned if o >= 5 else upright), o
    variants = {"old_1": old, "new_1": new(1), "new_3": new(3), "two_step_3": two_step_3, "new_6": new(6), "two_step_6": two_step_6}
    r = _rounds(torch, variants, rounds, iters)
    out = [dict(workload="photo_12mp_420_to_displayed_rgb", variant=k, ms=v) for k, v in r.items()]
    s = max(r["old_1"]["spread"], r["new_1"]["spread"])
    out.append({"new_1_vs_old_1": {"spread": s, "equal_within_spread": bool(abs(r["new_1"]["median"] - r["old_1"]["median"]) <= s)},
                "new_3_faster_than_two_step_3": _faster(r["new_3"], r["two_step_3"]),
                "new_6_faster_than_two_step_6": _faster(r["new_6"], r["two_step_6"])})
    return out


def batch(rounds, iters, size=224):
    import numpy as np
    import torch

    import jpeggpu_amd
    from jpeggpu_amd.api import FILTERS, LAYOUTS, _color_array, _img, _resize_items
    from tools import jpegsynth

    L = jpeggpu_amd.lib()
    n, w, h = 64, 4032, 3024
    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    rng = np.random.default_rng(2024)
    shown = [random_resized_crop(rng, h, w) for _ in range(n)]  # in the displayed image of orientation 6: 3024 x 4032
    rects = [jpeggpu_amd.orient_rect(6, w, h, r) for r in shown]
    bd = jpeggpu_amd.BatchDecode([cfg[i % 8] for i in range(n)], progressive=False, crops=rects)
    bd.decode()
    torch.cuda.synchronize()
    planes_list, infos, cis = bd.planes, bd.infos, bd.crop_infos

    items, _keep = _resize_items(planes_list, infos, cis)
    colors = _color_array([jpeggpu_amd.ColorSpace.YCBCR] * n, n)
    F = FILTERS["bilinear"]
    outs = {k: torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda:0") for k in ("oriented_6", "oriented_1", "cs_1")}

    def oriented(o, key):
        os_ = _color_array([o] * n, n)
        need = L.jpeggpu_ext_resize_scratch_size_oriented(items, colors, os_, n, size, size, F)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda:0")

        def fn():
            assert L.jpeggpu_ext_resize_to_rgb_oriented(items, colors, os_, n, size, size, F, LAYOUTS["NHWC"], outs[key].data_ptr(),
                                                        scratch.data_ptr(), need, None) == 0

        return fn

    need_cs = L.jpeggpu_ext_resize_scratch_size_cs(items, colors, n, size, size, F)
    scratch_cs = torch.empty(need_cs, dtype=torch.uint8, device="cuda:0")

    def cs():
        assert L.jpeggpu_ext_resize_to_rgb_cs(items, colors, n, size, size, F, LAYOUTS["NHWC"], outs["cs_1"].data_ptr(), scratch_cs.data_ptr(),
                                              need_cs, None) == 0

    srcs = [_img(p) for p in planes_list]
    crops = [torch.empty((ci.height, ci.width, 3), dtype=torch.uint8, device="cuda:0") for ci in cis]
    unfused_out = torch.empty((n, 3, size, size), dtype=torch.float32, device="cuda:0")

    def unfused():
        for i in range(n):
            assert L.jpeggpu_ext_crop_to_rgbi_fancy(C.byref(infos[i]), C.byref(cis[i]), C.byref(srcs[i]), crops[i].data_ptr(), 3 * cis[i].width, None) == 0
            t = torch.rot90(crops[i], -1, (0, 1)).contiguous()
            unfused_out[i] = torch.nn.functional.interpolate(t.permute(2, 0, 1)[None].float(), (size, size), mode="bilinear", antialias=True)[0]

    variants = {"oriented_6": oriented(6, "oriented_6"), "oriented_1": oriented(1, "oriented_1"), "cs_1": cs, "unfused_6": unfused}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    assert torch.equal(outs["oriented_1"], outs["cs_1"])
    from tests import pillow_resample_ref as R

    for i in (0, 17, 42):  # Pillow's resize of the displayed crop
        want = R.resize(torch.rot90(crops[i], -1, (0, 1)).contiguous().cpu().numpy(), size, size, "bilinear")
        assert np.array_equal(outs["oriented_6"][i].cpu().numpy(), want), i
    r = _rounds(torch, variants, rounds, iters)
    area = sum(r_[2] * r_[3] for r_ in rects)
    return [dict(workload="batch64_random_resized_crop_to_224", variant=k, ms=v) for k, v in r.items()] + [
        {"images": n, "crop_megapixels_mean": round(area / n / 1e6, 3)}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = photo(a.rounds, a.iters) + batch(a.rounds, a.iters) + [{"rounds": a.rounds, "iters": a.iters}]
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
