"""What encode_jpeg costs against the route a caller takes without it, in one process, the variants alternating inside every
round (the method of tools/tensor_rate.py). Two workloads:

  * "photos":  64 images of 4032 x 3024 RGB (BASELINE.json configs[2], decoded by this library), quality 75, 4:2:0, no restarts
  * "resized": 256 images of 224 x 224 (decode_resized's output), quality 90, 4:2:0

  * "device": jpeggpu_amd.encode_jpeg on the device tensors -- one jpeggpu_ext_encode_batch call, one synchronisation, the
    files copied to the host;
  * "host": the batch copied to the host and each image saved by Pillow on 16 threads -- what a caller does today. Without
    Pillow: torchvision.io.encode_jpeg on the CPU tensors; without either the device numbers stand alone and no bar is drawn.
Both are WALL time per call, the copy to the host included, medians of the rounds with their spread (max - min) in
milliseconds. The bar: the device route is not slower than the host route by more than the two spreads. Before anything is
timed the files of both routes are compared (Pillow: byte for byte).
`--once WORKLOAD` runs a single device call and nothing else: the process to put under a kernel trace.
`--optimize` measures optimised Huffman tables instead: encode_jpeg(optimize=True) against Pillow's optimize=True, by the same
method and with the same bar; each entry also records what the files save against the standard tables.
`--progressive` measures progressive files: encode_jpeg(progressive=True) against Pillow's progressive=True, and beside them
the same call with optimize=True ("device_optimize"), the nearest thing the encoder did before; `--no-host` leaves the host
route out (Pillow needs seconds per call for the photographs). `--flat` times the one call whose end-of-band runs are the
longest: a flat 1456 x 1456 grey image, progressive.
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/encode_rate.py [--optimize | --progressive [--no-host] | --flat] [--rounds 7] [--iters 10] [--out encode_rate.json] [--once photos|resized]
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

from tools.draft_rate import _spread  # noqa: E402

THREADS = 16
PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def _workload(torch, name):
    import jpeggpu_amd
    from tools import jpegsynth

    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    if name == "photos":
        images = jpeggpu_amd.decode_batch_to_rgb([cfg[i % 8] for i in range(64)])
        return [x.clone() for x in images], dict(quality=75, subsampling="4:2:0", restart_interval=0)
    small = jpeggpu_amd.decode_resized([cfg[i % 8] for i in range(64)], 224)
    batch = torch.cat([torch.roll(small, shifts=(7 * k, 11 * k), dims=(1, 2)) for k in range(4)])  # 256 different images
    return batch.contiguous(), dict(quality=90, subsampling="4:2:0", restart_interval=0)


def _host_route(torch, params):
    """(name, fn(images) -> list of bytes) of the yardstick this machine has, or (None, None)."""
    from concurrent.futures import ThreadPoolExecutor

    pool = ThreadPoolExecutor(THREADS)
    try:
        from PIL import Image, ImageFile

        optimize, progressive = bool(params.get("optimize")), bool(params.get("progressive"))
        if optimize or progressive:  # the whole file leaves libjpeg at once then, and Pillow's default buffer is too small for some files
            ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 26)

        def save(a):
            f = io.BytesIO()
            Image.fromarray(a).save(f, "JPEG", quality=params["quality"], subsampling=PILLOW_SUBSAMPLING[params["subsampling"]],
                                    restart_marker_blocks=params["restart_interval"], optimize=optimize, progressive=progressive)
            return f.getvalue()

        def fn(images):
            host = [x.cpu().numpy() for x in images] if isinstance(images, list) else list(images.cpu().numpy())
            return list(pool.map(save, host))

        return "pillow", fn
    except ImportError:
        pass
    if params.get("optimize") or params.get("progressive"):  # torchvision's encoder has no such switch: no yardstick
        return None, None
    try:
        import torchvision.io as tio

        def fn(images):
            host = [x.cpu() for x in images] if isinstance(images, list) else list(images.cpu())
            return list(pool.map(lambda x: tio.encode_jpeg(x.permute(2, 0, 1).contiguous(), quality=params["quality"]).numpy().tobytes(), host))

        return "torchvision", fn
    except ImportError:
        return None, None


def _wall(torch, fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1000 / iters


def run(rounds, iters, optimize=False, progressive=False, host=True):
    import torch

    import jpeggpu_amd

    out = []
    for name in ("photos", "resized"):
        images, params = _workload(torch, name)
        n = len(images)
        standard_bytes = sum(len(f) for f in jpeggpu_amd.encode_jpeg(images, **params)) if optimize or progressive else None
        plain = dict(params)
        if optimize:
            params["optimize"] = True
        if progressive:
            params["progressive"] = True
        device = lambda: jpeggpu_amd.encode_jpeg(images, **params)  # noqa: E731
        files = device()
        route, host_fn = _host_route(torch, params) if host else (None, None)
        variants = {"device": device}
        if progressive:
            variants["device_optimize"] = lambda: jpeggpu_amd.encode_jpeg(images, optimize=True, **plain)
        if route:
            theirs = host_fn(images)
            if route == "pillow":
                assert theirs == files, "the device's files are not Pillow's"
            variants["host_" + route] = lambda: host_fn(images)
        res = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():  # the variants alternate inside every round
                res[k].append(_wall(torch, fn, iters))
        r = {k: _spread(v) for k, v in res.items()}
        entry = dict(workload=name, images=n, params=params, file_bytes=sum(len(f) for f in files), ms=r, yardstick=route, rounds=rounds, iters=iters)
        if optimize or progressive:
            entry["standard_file_bytes"] = standard_bytes
            entry["saving"] = round(1 - entry["file_bytes"] / standard_bytes, 4)
        if route:
            d, h = r["device"], r["host_" + route]
            entry["bar"] = {"spreads": round(d["spread"] + h["spread"], 4), "device_over_host": round(d["median"] / h["median"], 4),
                            "holds": bool(d["median"] <= h["median"] + d["spread"] + h["spread"])}
        out.append(entry)
        del images, files
        torch.cuda.empty_cache()
    return out


def flat(rounds, iters):
    """The longest walk of prog_runs: 33 124 blocks of one value, four AC scans, each one lane from end to end."""
    import torch

    import jpeggpu_amd

    x = torch.full((1456, 1456), 128, dtype=torch.uint8, device="cuda:0")
    files = jpeggpu_amd.encode_jpeg([x], quality=75, subsampling="4:4:4", progressive=True)
    res = [_wall(torch, lambda: jpeggpu_amd.encode_jpeg([x], quality=75, subsampling="4:4:4", progressive=True), iters) for _ in range(rounds)]
    opt = [_wall(torch, lambda: jpeggpu_amd.encode_jpeg([x], quality=75, subsampling="4:4:4", optimize=True), iters) for _ in range(rounds)]
    return [dict(workload="flat_1456_grey", file_bytes=len(files[0]), ms=dict(device=_spread(res), device_optimize=_spread(opt)), rounds=rounds, iters=iters)]


def once(name, optimize=False, progressive=False):
    import torch

    import jpeggpu_amd

    images, params = _workload(torch, name)
    if optimize:
        params["optimize"] = True
    if progressive:
        params["progressive"] = True
    files = jpeggpu_amd.encode_jpeg(images, **params)
    torch.cuda.synchronize()
    print(json.dumps(dict(workload=name, images=len(files), file_bytes=sum(len(f) for f in files))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", default=None, choices=("photos", "resized"))
    ap.add_argument("--optimize", action="store_true")
    ap.add_argument("--progressive", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--flat", action="store_true")
    a = ap.parse_args()
    if a.once:
        return once(a.once, a.optimize, a.progressive)
    res = flat(a.rounds, a.iters) if a.flat else run(a.rounds, a.iters, a.optimize, a.progressive, not a.no_host)
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
