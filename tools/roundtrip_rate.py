"""What one jpeg_roundtrip call costs against the route it replaces, in one process, the variants alternating round by
round (the method of tools/batch_rgb_rate.py).

Two inputs, RGB, 4:2:0, a quality per image from 30..95: "augment", 64 images of 224 x 224 (an augmentation batch), and
"photos", 8 images of 4032 x 3024. For each:

  * "roundtrip": jpeg_roundtrip on the device tensors -- one jpeggpu_ext_roundtrip_batch call, two launches, no
    synchronisation;
  * "chain": the route of the library without that call -- encode_jpeg_to_device, the copy of the files to the host (the
    decoder parses there), decode_batch_to_rgb.

Both give the same tensors: that is compared before anything is timed, and the tool exits with status 1 if they differ.
Milliseconds per call from device events, medians of the rounds with their spread (max - min). The bar: "roundtrip" is
faster than "chain" by more than the larger of the two spreads ("holds"). Also reported: the bytes the new call has to move
-- 3 B/pixel read, the component planes written and read (1.5 B/pixel each for 4:2:0), 3 B/pixel written -- over its time.
Which of the two launches takes how long is not measured here: a kernel trace of a run with --only roundtrip shows it. Not
bench.py: that one measures the flagship workload and stays as it is.

    python tools/roundtrip_rate.py [--rounds 7] [--iters 10] [--inputs augment,photos] [--only roundtrip] [--out roundtrip_rate.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.crop_rate import _time  # noqa: E402
from tools.draft_rate import _spread  # noqa: E402


def inputs(which):
    """(images as uint8 H x W x 3 arrays, qualities): smooth colour fields with noise on top, a different one per image."""
    import numpy as np

    n, w, h = (64, 224, 224) if which == "augment" else (8, 4032, 3024)
    rng = np.random.default_rng(2024 if which == "augment" else 2025)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    images = []
    for i in range(n):
        f = rng.uniform(2.0, 9.0, (3, 2)) * np.pi / max(w, h)
        field = np.stack([127.0 + 90.0 * np.sin(f[c, 0] * x + i) * np.cos(f[c, 1] * y + c) for c in range(3)], axis=-1)
        images.append(np.clip(field + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8))
    return images, [int(q) for q in rng.integers(30, 96, n)]


def measure(torch, which, rounds, iters, only):
    import jpeggpu_amd

    arrays, qualities = inputs(which)
    xs = [torch.from_numpy(a).to("cuda:0") for a in arrays]
    pixels = sum(a.shape[0] * a.shape[1] for a in arrays)

    def roundtrip():
        return jpeggpu_amd.jpeg_roundtrip(xs, quality=qualities, subsampling="4:2:0")

    def chain():
        buf, offsets, sizes = jpeggpu_amd.encode_jpeg_to_device(xs, quality=qualities, subsampling="4:2:0")
        host = torch.cat([buf[o:o + s] for o, s in zip(offsets, sizes)]).cpu().numpy().tobytes()
        files, p = [], 0
        for s in sizes:
            files.append(host[p:p + s])
            p += s
        return jpeggpu_amd.decode_batch_to_rgb(files)

    a, b = roundtrip(), chain()
    torch.cuda.synchronize()
    differ = [i for i in range(len(xs)) if not torch.equal(a[i], b[i])]
    if differ:
        print(json.dumps({"input": which, "error": "roundtrip and chain differ", "images": differ}), flush=True)
        return None
    del a, b
    variants = {"roundtrip": roundtrip, "chain": chain}
    if only:
        variants = {only: variants[only]}
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():  # the variants alternate inside every round
            res[k].append(_time(torch, fn, iters))
    r = {k: _spread(v) for k, v in res.items()}
    out = [dict(input=which, images=len(xs), pixels=pixels, variant=k, ms=v) for k, v in r.items()]
    if "roundtrip" in r:
        moved = 9.0 * pixels  # 3 read, 1.5 + 1.5 planes written and read, 3 written
        out.append({"input": which, "roundtrip_bytes_moved": int(moved), "roundtrip_GB_per_s": round(moved / (r["roundtrip"]["median"] * 1e-3) / 1e9, 1)})
    if len(r) == 2:
        spread = max(r["roundtrip"]["spread"], r["chain"]["spread"])
        out.append({"input": which, "spread": spread, "chain_over_roundtrip": round(r["chain"]["median"] / r["roundtrip"]["median"], 2),
                    "holds": bool(r["roundtrip"]["median"] + spread < r["chain"]["median"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--inputs", default="augment,photos")
    ap.add_argument("--only", default=None, choices=["roundtrip", "chain"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    res = []
    for which in a.inputs.split(","):
        part = measure(torch, which, a.rounds, a.iters, a.only)
        if part is None:
            sys.exit(1)
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
