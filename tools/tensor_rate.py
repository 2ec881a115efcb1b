"""What jpeggpu_ext_resize_to_tensor costs against the route it replaces, in one process, the variants alternating inside
every round (the method of tools/batch_rgb_rate.py): the 64-image RandomResizedCrop batch of tools/resize_rate.py
(BASELINE.json configs[2], 4032 x 3024 4:2:0, seeded rectangles), decoded once, to 224 x 224, bilinear, half of the items
flipped.

  * "fused_f32" / "fused_f16": ONE jpeggpu_ext_resize_to_tensor call to float32 / float16 NCHW with the ImageNet mean and
    std and the flips; "parent_f32" / "parent_f16": jpeggpu_ext_resize_to_rgb_oriented to uint8 NCHW, then torch on the
    device and the same stream: .float().div(255), sub, div, the cast for the half, and torch.where over a flipped copy
    for the items to flip -- what a loader does with the library without the call.
  * "fused_u8": the call to uint8 NHWC with the flips; "parent_u8": the uint8 call and the torch.where flip alone.
The bar, per pair: the fused call is not slower than the parent route by more than the spread of the rounds ("holds").
Medians of the rounds with their spread (max - min), in milliseconds per call sequence from device events.
Before anything is timed the results are compared: the bytes exactly; the floats of the two routes within a few units in the
last place (torch's division by a scalar on the device multiplies by a reciprocal, so its last bits are not ToTensor's on
the CPU), and the fused float results bit for bit against torch on the CPU.
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/tensor_rate.py [--rounds 7] [--iters 10] [--out tensor_rate.json]
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

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _not_slower(fused, parent):
    spread = max(fused["spread"], parent["spread"])
    return {"spread": spread, "fused_over_parent": round(fused["median"] / parent["median"], 4),
            "holds": bool(fused["median"] <= parent["median"] + spread)}


def _decode(torch, datas, rects):
    """The files' rectangles decoded by one jpeggpu_ext_decode_batch call (ISLOW): (planes_list, infos, crop infos)."""
    import jpeggpu_amd

    with jpeggpu_amd.BatchDecode(datas, progressive=False, crops=rects) as bd:
        bd.decode()
        torch.cuda.synchronize()
        return bd.planes, bd.infos, bd.crop_infos


def run(rounds, iters, size=224, n=64):
    import numpy as np
    import torch

    import jpeggpu_amd
    from jpeggpu_amd.api import FILTERS, LAYOUTS, TENSOR_TYPES, TensorSpec, _color_array, _resize_items, lib
    from tools import jpegsynth

    L = lib()
    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    datas = [cfg[i % 8] for i in range(n)]
    rng = np.random.default_rng(2024)
    rects = [random_resized_crop(rng, 4032, 3024) for _ in range(n)]
    flips = [int(v) for v in np.random.default_rng(7).permutation(n) < n // 2]  # half of the items, seeded
    planes_list, infos, cis = _decode(torch, datas, rects)
    items, _keep = _resize_items(planes_list, infos, cis)
    cs, os_ = _color_array([jpeggpu_amd.ColorSpace.YCBCR] * n, n), _color_array([1] * n, n)
    need = L.jpeggpu_ext_resize_scratch_size_oriented(items, cs, os_, n, size, size, FILTERS["bilinear"])
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    flip_bytes = (C.c_ubyte * n)(*flips)
    mask = torch.tensor(flips, dtype=torch.bool, device="cuda:0").view(n, 1, 1, 1)
    mean_d = torch.tensor(MEAN, dtype=torch.float32, device="cuda:0").view(1, 3, 1, 1)
    std_d = torch.tensor(STD, dtype=torch.float32, device="cuda:0").view(1, 3, 1, 1)

    def fused(dtype, layout):
        out = torch.empty((n, 3, size, size) if layout == "NCHW" else (n, size, size, 3), dtype=dtype, device="cuda:0")
        spec = TensorSpec()
        spec.type = TENSOR_TYPES[dtype]
        spec.mean[:], spec.std[:] = MEAN, STD
        spec.flips = C.cast(flip_bytes, C.POINTER(C.c_ubyte))

        def fn():
            st = L.jpeggpu_ext_resize_to_tensor(items, cs, os_, n, size, size, FILTERS["bilinear"], LAYOUTS[layout], C.byref(spec), out.data_ptr(),
                                                scratch.data_ptr(), need, None)
            assert st == 0, jpeggpu_amd.status_string(st)

        return fn, lambda: out

    def parent(dtype, layout):
        u8 = torch.empty((n, 3, size, size) if layout == "NCHW" else (n, size, size, 3), dtype=torch.uint8, device="cuda:0")
        res = [None]

        def fn():
            st = L.jpeggpu_ext_resize_to_rgb_oriented(items, cs, os_, n, size, size, FILTERS["bilinear"], LAYOUTS[layout], u8.data_ptr(),
                                                      scratch.data_ptr(), need, None)
            assert st == 0, jpeggpu_amd.status_string(st)
            x = u8
            if dtype != torch.uint8:
                x = u8.float().div(255).sub(mean_d).div(std_d)
                if dtype != torch.float32:
                    x = x.to(dtype)
            res[0] = torch.where(mask, x.flip(3 if layout == "NCHW" else 2), x)

        return fn, lambda: res[0]

    pairs = {"f32": (torch.float32, "NCHW"), "f16": (torch.float16, "NCHW"), "u8": (torch.uint8, "NHWC")}
    variants = {}
    for key, (dtype, layout) in pairs.items():
        ff, fo = fused(dtype, layout)
        pf, po = parent(dtype, layout)
        ff()
        pf()
        torch.cuda.synchronize()
        a, b = fo(), po()
        assert a.dtype == b.dtype == dtype and a.shape == b.shape, key
        if dtype == torch.uint8:
            assert torch.equal(a, b), key
        else:
            # the routes differ where torch's device kernels round differently: u * (1 / 255) is off by up to 1.5 * 2^-24,
            # the subtraction adds 2^-25, the division by std >= 0.224 multiplies both by up to 4.5 -- 2.2 * 2^-22 -- and each
            # route rounds its result (|y| < 4: 2^-22 a unit): four units for float32; for the half, one of ITS units (2^-9)
            # where that difference changes the rounding, and as much again
            tol = 4 * 2.0 ** -22 if dtype == torch.float32 else 2 * 2.0 ** -9
            assert float((a.float() - b.float()).abs().max()) <= tol, (key, float((a.float() - b.float()).abs().max()))
        variants["fused_" + key], variants["parent_" + key] = ff, pf
    # the fused float results against torch on the CPU, from the uint8 call's own bytes
    uf, uo = parent(torch.uint8, "NCHW")
    uf()
    torch.cuda.synchronize()
    u8 = uo().cpu()  # flipped already
    want = u8.to(torch.float32).div(255).sub(torch.tensor(MEAN).view(1, 3, 1, 1)).div(torch.tensor(STD).view(1, 3, 1, 1))
    for key in ("f32", "f16"):
        ff, fo = fused(*pairs[key])
        ff()
        torch.cuda.synchronize()
        got, w = fo().cpu(), want.to(pairs[key][0])
        view = torch.int32 if key == "f32" else torch.int16
        assert torch.equal(got.view(view), w.view(view)), key

    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():  # the variants alternate inside every round
            res[k].append(_time(torch, fn, iters))
    r = {k: _spread(v) for k, v in res.items()}
    out = [dict(variant=k, ms=v) for k, v in r.items()]
    out.append({"fused_%s_vs_parent" % key: _not_slower(r["fused_" + key], r["parent_" + key]) for key in pairs})
    out.append({"rounds": rounds, "iters": iters, "images": n, "out": [size, size], "filter": "bilinear", "flipped": sum(flips)})
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
