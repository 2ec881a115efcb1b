"""What transcode_jpeg costs against the pixel round trip that did the same job before it, in one process, the variants
alternating inside every round (the method of tools/encode_rate.py). The workload: 64 files of 4032 x 3024, 4:2:0
(BASELINE.json configs[2]), from bytes on the host to bytes on the host.

  * "transcode_optimize", "transcode_progressive": jpeggpu_amd.transcode_jpeg(optimize=True / progressive=True) -- a batched
    decode that stops in front of the IDCT, one jpeggpu_ext_transcode_batch call, one synchronisation;
  * "pixels_optimize", "pixels_progressive": decode_batch_to_rgb, then encode_jpeg(quality=75, subsampling="4:2:0") with the
    same flag -- lossy, and an IDCT, a colour conversion, an FDCT and a quantiser more.
WALL time per call in milliseconds, medians of the rounds with their spread (max - min). Before anything is timed the
transcoded files are decoded again and compared with the sources' pixels.
Both routes spend most of that on the host (parsing, the copies in and out), so the same four follow with everything
RESIDENT ("resident_*"): the files parsed and transferred once, the output slots allocated once, and a timed call is the
decode batch plus jpeggpu_ext_transcode_batch, or the decode batch, jpeggpu_ext_batch_to_rgb and jpeggpu_ext_encode_batch,
up to the synchronisation -- what the device does for either route.
`--once optimize|progressive` runs a single transcode call and nothing else: the process to put under a kernel trace, which
gives gather_blocks its own time (it writes 36 MB of coefficients per image); `--orientation N` turns every file of that
call (transcode_jpeg's `orientation`), which launches the gather's other instantiation.
`--crop` cuts the centred rectangle of a quarter of the area out of every file (transcode_jpeg's `crops`: 2016 x 1512 at
1008, 752). With `--once` the call is then made of its parts, so that `--no-window` can leave the decode window off (the
whole file is transferred and entropy-decoded, and only the gather and what follows see the rectangle); the line printed
holds the bytes transferred. Without `--once`, `--crop` times three calls against each other, alternating inside every
round, wall time from bytes on the host to bytes on the host: the uncropped transcode, the cropped one on whole decodes,
and the cropped one with the decode narrowed to the restart segments that hold the rectangle.
The files carry a restart interval of one MCU row (252 MCUs), which is what the narrowed decode cuts by.

    python tools/transcode_rate.py [--rounds 7] [--iters 3] [--images 64] [--out transcode_rate.json] [--crop]
                                   [--once optimize|progressive [--orientation N] [--crop [--no-window]]]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.draft_rate import _spread  # noqa: E402


CROP = (1008, 752, 2016, 1512)  # of 4032 x 3024: a quarter of the area, about the centre, on iMCU boundaries


def _sources(n):
    from tools import jpegsynth

    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    return [cfg[i % 8] for i in range(n)]


def _cropped_call(torch, jpeggpu_amd, datas, flag, crop, window):
    """transcode_jpeg(crops=) made of its parts: the batched decode, whole or (`window`) narrowed as transcode_jpeg narrows it,
    one jpeggpu_ext_transcode_batch call, the files' bytes to the host. Returns (files, bytes transferred to the device)."""
    n = len(datas)
    hooks = jpeggpu_amd.api._transcode_windows(n, None, False, False, crop, False) if crop and window else None
    with jpeggpu_amd.BatchDecode(datas, "cuda:0", coefficients_only=True, crop_hooks=hooks) as bd:
        bd.decode()
        slots = torch.empty((n, max(len(d) for d in datas) + 4096), dtype=torch.uint8, device="cuda:0")
        sizes, status = jpeggpu_amd.transcode_into(bd, list(slots), crops=crop, **{flag: True})
        sizes, status = sizes.cpu().tolist(), status.cpu().tolist()
        assert not any(status), status
        host = torch.cat([slots[i, :s] for i, s in enumerate(sizes)]).cpu().numpy().tobytes()
        moved = bd.transferred_bytes
    out, p = [], 0
    for s in sizes:
        out.append(host[p:p + s])
        p += s
    return out, moved


def crop_rate(rounds, iters, n):
    import torch

    import jpeggpu_amd

    datas = _sources(n)
    variants = {"uncropped": (None, False), "cropped_whole_decode": (CROP, False), "cropped_narrowed_decode": (CROP, True)}
    moved, sizes = {}, {}
    for k, (crop, window) in variants.items():
        files, moved[k] = _cropped_call(torch, jpeggpu_amd, datas, "optimize", crop, window)
        sizes[k] = sum(len(f) for f in files)
        if crop:  # lossless, and the same file either way
            assert files == jpeggpu_amd.transcode_jpeg(datas, optimize=True, crops=crop), k
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (crop, window) in variants.items():
            res[k].append(_wall(torch, lambda: _cropped_call(torch, jpeggpu_amd, datas, "optimize", crop, window), iters))
    return dict(workload="configs[2] 4032x3024 4:2:0, crop %r" % (CROP,), images=n, source_bytes=sum(len(d) for d in datas), transferred_bytes=moved,
                file_bytes=sizes, ms={k: _spread(v) for k, v in res.items()}, rounds=rounds, iters=iters)


def _wall(torch, fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1000 / iters


def run(rounds, iters, n):
    import torch

    import jpeggpu_amd

    datas = _sources(n)
    pixels = lambda **flag: jpeggpu_amd.encode_jpeg(jpeggpu_amd.decode_batch_to_rgb(datas), quality=75, subsampling="4:2:0", **flag)  # noqa: E731
    variants = {
        "transcode_optimize": lambda: jpeggpu_amd.transcode_jpeg(datas, optimize=True),
        "transcode_progressive": lambda: jpeggpu_amd.transcode_jpeg(datas, progressive=True),
        "pixels_optimize": lambda: pixels(optimize=True),
        "pixels_progressive": lambda: pixels(progressive=True),
    }
    sizes = {}
    for k in ("transcode_optimize", "transcode_progressive"):  # lossless: the same pixels from the new file
        files = variants[k]()
        sizes[k] = sum(len(f) for f in files)
        for i in (0, n - 1):
            assert bool((jpeggpu_amd.decode_to_rgb(files[i]) == jpeggpu_amd.decode_to_rgb(datas[i])).all()), k
        del files
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():  # the variants alternate inside every round
            res[k].append(_wall(torch, fn, iters))
    res.update(_resident(torch, jpeggpu_amd, datas, rounds, iters))
    ms = {k: _spread(v) for k, v in res.items()}
    out = dict(workload="configs[2] 4032x3024 4:2:0", images=n, source_bytes=sum(len(d) for d in datas), file_bytes=sizes, ms=ms, rounds=rounds, iters=iters)
    for flag in ("optimize", "progressive"):
        for pre in ("", "resident_"):
            t, p = ms[pre + "transcode_" + flag], ms[pre + "pixels_" + flag]
            out[pre + "transcode_over_pixels_" + flag] = round(t["median"] / p["median"], 4)
    return out


def _resident(torch, jpeggpu_amd, datas, rounds, iters):
    """The four routes on files that are parsed and transferred, into slots that exist: rounds of `iters` calls each."""
    n = len(datas)
    slots = [torch.empty(2 * len(d) + 4096, dtype=torch.uint8, device="cuda:0") for d in datas]
    with jpeggpu_amd.BatchDecode(datas, "cuda:0", coefficients_only=True) as bt, jpeggpu_amd.BatchDecode(datas, "cuda:0") as bp:
        def transcode(flag):
            bt.decode()
            return jpeggpu_amd.transcode_into(bt, slots, **{flag: True})

        def pixels(flag):
            bp.decode()
            rgb = jpeggpu_amd.api.batch_to_rgb(bp.planes, bp.infos, bp.crop_infos, bp.colors, [1] * n, bp.replicates, "HWC")
            return jpeggpu_amd.encode_into(rgb, slots, quality=75, subsampling="4:2:0", **{flag: True})

        variants = {"resident_%s_%s" % (name, flag): (lambda fn=fn, flag=flag: fn(flag)) for flag in ("optimize", "progressive")
                    for name, fn in (("transcode", transcode), ("pixels", pixels))}
        for k, fn in variants.items():
            assert not bool(fn()[1].any()), k  # every file fits its slot
        res = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():
                res[k].append(_wall(torch, fn, iters))
    return res


def once(flag, n, orientation=None, crop=False, window=True):
    import torch

    import jpeggpu_amd

    if crop:
        files, moved = _cropped_call(torch, jpeggpu_amd, _sources(n), flag, CROP, window)
        torch.cuda.synchronize()
        print(json.dumps(dict(images=len(files), file_bytes=sum(len(f) for f in files), transferred_bytes=moved)))
        return
    more = dict(orientation=orientation) if orientation else {}  # (4032 x 3024 is whole iMCUs both ways: every orientation is exact)
    files = jpeggpu_amd.transcode_jpeg(_sources(n), **{flag: True}, **more)
    torch.cuda.synchronize()
    print(json.dumps(dict(images=len(files), file_bytes=sum(len(f) for f in files))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", default=None, choices=("optimize", "progressive"))
    ap.add_argument("--orientation", type=int, default=None, help="with --once: transcode_jpeg's orientation, 1..8")
    ap.add_argument("--crop", action="store_true", help="the centred rectangle of a quarter of the area (see above)")
    ap.add_argument("--no-window", action="store_true", help="with --once --crop: the decode is not narrowed to the rectangle")
    a = ap.parse_args()
    if a.once:
        return once(a.once, a.images, a.orientation, a.crop, not a.no_window)
    res = crop_rate(a.rounds, a.iters, a.images) if a.crop else run(a.rounds, a.iters, a.images)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
