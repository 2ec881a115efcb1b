"""What Resize + CenterCrop through jpeggpu_ext_resize_view_to_tensor costs against the route there was without it, in one
process, the variants alternating inside every round (the method of tools/tensor_rate.py): 64 images of BASELINE.json
configs[2] (4032 x 3024 4:2:0, tools/jpegsynth) to Resize(256) + CenterCrop(224), bilinear, NCHW float16 with the ImageNet
mean and std.

  * "view": ONE jpeggpu_ext_resize_view_to_tensor call on planes of a CROPPED decode (each file's resize_view_rect).
  * "parent": the yardstick -- 64 single-item jpeggpu_ext_resize_to_tensor calls at each item's own (rw, rh) on WHOLE
    decoded planes, each into its own rh x rw tensor. "parent_sliced": the same followed by the copy of the centre windows
    into one batch tensor, which a loader needs as well.
The bar: "view" is not slower than "parent" by more than the spread of the rounds ("holds"). Medians of the rounds with
their spread (max - min), in milliseconds per call sequence from device events. Before anything is timed the results are
compared bit for bit.
  * the decode batch (transfer + jpeggpu_ext_decode_batch) with and without the rectangles, at scale 1 and at the scale
    Pillow's draft() would pick for the resized size (draft_scale): ms per batch and the bytes transferred.
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/center_crop_rate.py [--rounds 7] [--iters 10] [--out center_crop_rate.json]
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
from tools.draft_rate import _spread  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RESIZE, CROP = 256, 224


def _not_slower(view, parent):
    spread = max(view["spread"], parent["spread"])
    return {"spread": spread, "view_over_parent": round(view["median"] / parent["median"], 4),
            "holds": bool(view["median"] <= parent["median"] + spread)}


def _decoders(torch, datas, scale, rects):
    """One decoder per file (ISLOW, the libjpeg scale mode below 1, the rectangle if any), parsed, with its buffers: what a
    decode batch needs, and the bytes its transfers copy."""
    import jpeggpu_amd

    bd = jpeggpu_amd.BatchDecode(datas, progressive=False, scales=[scale] * len(datas), crops=rects)

    def decode():
        bd.transfer()
        bd.decode()

    return dict(decode=decode, planes=bd.planes, infos=bd.infos, cis=bd.crop_infos, bytes=bd.transferred_bytes, keep=bd)


def run(rounds, iters, n=64):
    import torch

    import jpeggpu_amd
    from jpeggpu_amd.api import FILTERS, LAYOUTS, TENSOR_TYPES, ResizeView, TensorSpec, _resize_items, lib
    from tools import jpegsynth

    L = lib()
    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    datas = [cfg[i % 8] for i in range(n)]
    W, H = 4032, 3024
    filt, layout, dtype = "bilinear", "NCHW", torch.float16
    sets = {}
    for scale in (1, jpeggpu_amd.draft_scale(W, H, jpeggpu_amd.resized_size(W, H, RESIZE))):
        w, h = -(-W // scale), -(-H // scale)
        rw, rh = jpeggpu_amd.resized_size(w, h, RESIZE)
        view = (rw, rh) + jpeggpu_amd.center_crop_window(rw, rh, CROP)
        rect = jpeggpu_amd.resize_view_rect(w, h, view, CROP, filt)
        sets[scale] = dict(view=view, rect=rect, size=(w, h), whole=_decoders(torch, datas, scale, [None] * n),
                           cropped=_decoders(torch, datas, scale, [rect] * n))
        for k in ("whole", "cropped"):
            sets[scale][k]["decode"]()
    torch.cuda.synchronize()

    s1 = sets[1]
    rw, rh, vx, vy = s1["view"]
    spec = TensorSpec()
    spec.type = TENSOR_TYPES[dtype]
    spec.mean[:], spec.std[:] = MEAN, STD
    # the view call, on the cropped planes
    c_items, _keep_c = _resize_items(s1["cropped"]["planes"], s1["cropped"]["infos"], s1["cropped"]["cis"])
    views = (ResizeView * n)(*[ResizeView(rw, rh, vx, vy, 0) for _ in range(n)])
    need_v = L.jpeggpu_ext_resize_view_scratch_size(c_items, None, None, views, n, CROP, CROP, FILTERS[filt])
    scratch_v = torch.empty(need_v, dtype=torch.uint8, device="cuda:0")
    out_v = torch.empty((n, 3, CROP, CROP), dtype=dtype, device="cuda:0")

    def view_call():
        st = L.jpeggpu_ext_resize_view_to_tensor(c_items, None, None, views, n, CROP, CROP, FILTERS[filt], LAYOUTS[layout], C.byref(spec),
                                                 out_v.data_ptr(), scratch_v.data_ptr(), need_v, None)
        assert st == 0, jpeggpu_amd.status_string(st)

    # the parent's route, on the whole planes: one call per image at its own (rw, rh)
    singles = []
    for i in range(n):
        it, keep = _resize_items([s1["whole"]["planes"][i]], [s1["whole"]["infos"][i]], None)
        need = L.jpeggpu_ext_resize_scratch_size(it, 1, rw, rh, FILTERS[filt])
        singles.append((it, keep, need, torch.empty(need, dtype=torch.uint8, device="cuda:0"),
                        torch.empty((1, 3, rh, rw), dtype=dtype, device="cuda:0")))
    out_p = torch.empty((n, 3, CROP, CROP), dtype=dtype, device="cuda:0")

    def parent_calls():
        for it, _, need, scratch, out in singles:
            st = L.jpeggpu_ext_resize_to_tensor(it, None, None, 1, rw, rh, FILTERS[filt], LAYOUTS[layout], C.byref(spec), out.data_ptr(),
                                                scratch.data_ptr(), need, None)
            assert st == 0, jpeggpu_amd.status_string(st)

    def parent_sliced():
        parent_calls()
        for i, s in enumerate(singles):
            out_p[i].copy_(s[4][0, :, vy:vy + CROP, vx:vx + CROP])

    view_call()
    parent_sliced()
    torch.cuda.synchronize()
    assert torch.equal(out_v.view(torch.int16), out_p.view(torch.int16)), "the view call and the per-image route differ"

    variants = {"view": view_call, "parent": parent_calls, "parent_sliced": parent_sliced}
    for scale, s in sets.items():
        variants["decode_whole_1_%d" % scale] = s["whole"]["decode"]
        variants["decode_rect_1_%d" % scale] = s["cropped"]["decode"]
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():  # the variants alternate inside every round
            res[k].append(_time(torch, fn, iters))
    r = {k: _spread(v) for k, v in res.items()}
    out = [dict(variant=k, ms=v) for k, v in r.items()]
    out.append({"view_vs_parent": _not_slower(r["view"], r["parent"]), "view_vs_parent_sliced": _not_slower(r["view"], r["parent_sliced"])})
    for scale, s in sets.items():
        w, h = s["size"]
        out.append({"scale": scale, "image": [w, h], "view": list(s["view"]), "rect": list(s["rect"]),
                    "rect_area_share": round(s["rect"][2] * s["rect"][3] / (w * h), 4),
                    "transferred_bytes_whole": s["whole"]["bytes"], "transferred_bytes_rect": s["cropped"]["bytes"]})
    out.append({"rounds": rounds, "iters": iters, "images": n, "resize": RESIZE, "crop": CROP, "filter": filt, "layout": layout, "dtype": "float16"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
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
