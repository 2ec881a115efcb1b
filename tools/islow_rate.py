"""Decode rate of the two full-size IDCT methods (jpeggpu_ext_set_idct) and the time of the two RGB kernels, in one
process, the methods alternating round by round:
  * the reference photo decoded on its own, and a 64-image batch of BASELINE.json configs[2] (4032 x 3024 4:2:0,
    tools/jpegsynth) through jpeggpu_ext_decode_batch: images/s from device events and the `idct` stage's ms from the
    batch's stage timing;
  * jpeggpu_ext_planes_to_rgbi (the reference's helper) and jpeggpu_ext_planes_to_rgbi_fancy on the planes of one 12 MP
    image: ms per call from device events, and the bytes each moves (planes read, RGB written) against HBM peak.
Not bench.py: that one measures the flagship workload with the default IDCT and stays as it is.

    python tools/islow_rate.py [--rounds 7] [--iters 10] [--out islow_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, GB/s
METHODS = ("reference", "islow")


def _setup(torch, datas, method, hint):
    import jpeggpu_amd

    return jpeggpu_amd.BatchDecode(datas, hint=hint, idct=method, progressive=False)


def _time(torch, fn, iters):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / iters


def run(rounds, iters):
    import torch

    import jpeggpu_amd
    from jpeggpu_amd.api import _img, lib
    from tools import jpegsynth

    photo = open(os.path.join(ROOT, "tests", "golden", "IMG_6510.JPG"), "rb").read()
    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    setups = {}
    for m in METHODS:
        setups[("photo", m)] = _setup(torch, [photo], m, 0)
        setups[("batch64", m)] = _setup(torch, [cfg[i % 8] for i in range(64)], m, 64)
    results = {k: {"img_s": [], "idct_ms": []} for k in setups}
    for bd in setups.values():  # warm-up
        bd.decode()
    torch.cuda.synchronize()

    # the RGB kernels on the planes of one 12 MP 4:2:0 image
    planes, info = jpeggpu_amd.decode_to_planes(cfg[0], idct="islow")
    width, height = info.sizes_x[0], info.sizes_y[0]
    src = _img(planes)
    rgb = torch.empty((height, width, 3), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    kernels = {"rgbi_kernel": lib().jpeggpu_ext_planes_to_rgbi, "fancy_rgbi_kernel": lib().jpeggpu_ext_planes_to_rgbi_fancy}
    rgb_ms = {k: [] for k in kernels}

    def rgb_call(fn):
        return lambda: fn(C.byref(info), C.byref(src), rgb.data_ptr(), 3 * width, width, height, stream)

    for fn in kernels.values():
        assert rgb_call(fn)() == 0
    for _ in range(rounds):
        for name in ("photo", "batch64"):
            for m in METHODS:  # the methods alternate inside every round
                bd = setups[(name, m)]
                ms = _time(torch, bd.decode, iters)
                results[(name, m)]["img_s"].append(len(bd.decoders) * 1000.0 / ms)
                bd.batch.set_profiling(True)  # (a new measurement window)
                for _ in range(3):
                    bd.decode()
                torch.cuda.synchronize()
                results[(name, m)]["idct_ms"].append(bd.batch.stage_ms()["idct"])
                bd.batch.set_profiling(False)
        for k, fn in kernels.items():
            rgb_ms[k].append(_time(torch, rgb_call(fn), iters * 10))
    out = []
    for (name, m), v in results.items():
        out.append({
            "workload": name, "idct": m, "images": len(setups[(name, m)].decoders),
            "img_s_median": round(statistics.median(v["img_s"]), 1), "img_s_min": round(min(v["img_s"]), 1), "img_s_max": round(max(v["img_s"]), 1),
            "idct_ms_median": round(statistics.median(v["idct_ms"]), 4), "idct_ms_min": round(min(v["idct_ms"]), 4), "idct_ms_max": round(max(v["idct_ms"]), 4),
        })
    nbytes = sum(p.numel() for p in planes) + rgb.numel()
    for k, v in rgb_ms.items():
        ms = statistics.median(v)
        out.append({
            "workload": "rgb_12mp_420", "kernel": k, "ms_median": round(ms, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "bytes": nbytes, "gb_s": round(nbytes / (ms * 1e6), 1), "hbm_share": round(nbytes / (ms * 1e6) / HBM_PEAK_GBS, 4),
        })
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
