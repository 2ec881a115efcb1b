#!/usr/bin/env python3
"""bench.py -- images/s of the baseline-JPEG decode hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--full]

One "step" = `--rounds` passes of the hot path (destuff -> Huffman sync / write -> IDCT, through
jpeggpu_ext_decode_batch by default or the drop-in jpeggpu_decoder_decode with --mode streams) over the rank's
batch of 12 MP 4:2:0 restart-interval JPEGs (BASELINE.json configs[1]; with N > 1 the images are sharded by
rank as in configs[2], no data-path collective in the timed region, weak scaling). The defaults make a step
2048 images, so the timed region is about 1.5 s.

`value` is the rate with inputs (entropy-coded bytes + table blobs) resident in HBM when the timed region
starts. Rank 0 prints ONE JSON line; DESIGN.md section 4 defines every field. `ms_per_step` is the wall time of one
timed step. A plain run does only what these need: set-up, the warm-up and timed steps, --dump-outputs, the line.

`--dump-outputs DIR` writes what the timed path decoded in its last step -- the planes of every image of the batch, a
fixed seeded sample of each -- to DIR/plane<c>.npy (float32, at most 64 MB; `dump_outputs`). The inputs are seeded, so
two builds run with the same arguments can be compared array for array.

`--full` adds everything else the line can carry (every leg runs after the timed steps but the CPU baseline, first):
`value_full_path`, the rate of the whole boundary protocol from pinned host memory (parse_header + transfer +
decode), which the boundary hands over -- never `value`; `verified`, the planes of every distinct image compared
with the CPU oracle after the timed loop; and the legs below.

`roofline` is the destuff+Huffman PASS the north star names: SURVEY.md 8(d)'s algorithmic bytes of that pass
(B_dh = stuffed scan bytes + 128 B per data unit) x the images of one launch / the SUM of the average durations of
the pass's kernels, measured in this run from serialized launches with HIP events on the launch stream, over the
HBM peak. `kernels` lists every kernel with the bytes it really has to move. `cpu_baseline` is libjpeg-turbo on this
box's host cores, timed BEFORE this process touches the GPU (its worker processes are spawned, not forked).

For N > 1 the driver launches this file with torch.distributed.run, one rank per GPU (RCCL); with --full the line then
also carries `gather`: BASELINE.json configs[2] itself -- 64 images sharded over the ranks, decoded, and collected
on rank 0, the gather of round k on a side stream while round k + 1 decodes.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
SIMDS, VALU_CYCLES, SHADER_HZ = 1024, 4, 2.4e9  # 256 CUs x 4 SIMDs; a wave64 VALU instruction issues over 4 cycles
KERNEL_NAMES = {"front": "front_count+front_prefix+front_marks+front_plan", "destuff": "destuff_kernel",
                "sync_intra": "huff_sync_intra", "sync_inter": "huff_sync_tail", "tails": "huff_seq_tails",
                "write": "huff_write", "idct": "idct_kernel"}
PASS_STAGES = ("front", "destuff", "sync_intra", "sync_inter", "tails", "write")  # "front" only with the device scan
PHOTO = os.path.join(ROOT, "tests", "golden", "IMG_6510.JPG")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="images per GPU per round (4 groups of 64: one launch per stage and group; BASELINE configs[2] is a batch of 64)")
    ap.add_argument("--rounds", type=int, default=8, help="passes over the batch per step (a step = batch * rounds images)")
    ap.add_argument("--mode", default="batch", choices=["batch", "streams"],
                    help="batch: jpeggpu_ext_decode_batch, one launch per stage per group of images; "
                         "streams: the drop-in jpeggpu_decoder_decode, one image per call")
    ap.add_argument("--streams", type=int, default=0,
                    help="HIP streams (batch mode: groups of images, default 4; streams mode: default 16)")
    ap.add_argument("--unique", type=int, default=16, help="distinct synthetic images per rank (seeded)")
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "photo"])
    ap.add_argument("--subseq-bytes", type=int, default=0, help="0 = the library's choice for the call type (jpeggpu_ext.h)")
    ap.add_argument("--overlap", type=int, default=1,
                    help="jpeggpu_ext_batch_set_overlap: concurrent parts per batch call (for --streams 1)")
    ap.add_argument("--sync-iters", type=int, default=0,
                    help="flow iterations inside the sequence kernel in batch mode (0 = library default, 1)")
    ap.add_argument("--gather-rounds", type=int, default=10,
                    help="N > 1: rounds of the configs[2] leg (64 images over the ranks + RCCL gather to rank 0); 0 = skip")
    ap.add_argument("--segment-shard-rounds", type=int, default=5,
                    help="N > 1: rounds of the restart-interval-sharding leg (ONE 39 MP image, every rank decodes its share of "
                         "the restart segments, bands gathered on rank 0); 0 = skip")
    ap.add_argument("--latency-iters", type=int, default=200,
                    help="iterations of the reference's own protocol (1 warm-up + 200, benchmark_common.hpp:39); 0 = skip")
    ap.add_argument("--device-scan", type=int, default=0,
                    help="1: the images of the timed batch use jpeggpu_ext_set_device_scan (marker scan inside the timed region)")
    ap.add_argument("--roofline-launches", type=int, default=6,
                    help="serialized launches (one stream, nothing else on the chip) the roofline figures are averaged over; 0 = skip")
    ap.add_argument("--other-configs", type=int, default=200,
                    help="iterations of the latency protocol on BASELINE.json configs[0] (the reference's photo), [3] and [4]; 0 = skip")
    ap.add_argument("--photo-steps", type=int, default=3,
                    help="N = 1: steps of the batched protocol of `value` on the reference's photo (other_configs...batch_images_per_s); 0 = skip")
    ap.add_argument("--cpu-seconds", type=float, default=6.0, help="budget of each leg of the CPU baseline")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--e2e-rounds", type=int, default=16,
                    help="rounds of the full-path measurement (parse + transfer + decode from pinned host memory); 0 = skip")
    ap.add_argument("--host-threads", type=int, default=6, help="threads of jpeggpu_ext_parse_headers in that measurement")
    ap.add_argument("--curve-iters", type=int, default=30,
                    help="N = 1: calls per point of `batch_curve` (one batched call of 1 .. 64 images, device time per image); 0 = skip")
    ap.add_argument("--shard-iters", type=int, default=200,
                    help="N = 1: iterations of `config3_rank_shard` (BASELINE configs[2]'s per-rank 8 images through the whole protocol); 0 = skip")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the planes the last step decoded to DIR/plane<c>.npy (float32, a fixed "
                         "seeded sample of every image of the batch, at most 64 MB in all; see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beyond the headline figure: CPU baseline, oracle check, roofline, latency, "
                         "full path, other configurations, batch curve, rank shard, and for N > 1 gather and segment shard; "
                         "without it the options of those legs have no effect")
    args = ap.parse_args(argv)
    if not args.full:
        lean(args)
    return args


# the options of the legs a plain run skips: 0 skips each of them
EXTRA_LEGS = ("gather_rounds", "segment_shard_rounds", "latency_iters", "roofline_launches", "other_configs", "photo_steps",
              "e2e_rounds", "curve_iters", "shard_iters")


def lean(args):
    """A plain run (no --full) does only what `value` and `ms_per_step` need: it sets up, warms up, times the steps,
    writes --dump-outputs and prints the line. The CPU baseline, the oracle check and every other leg are off, and their
    fields are absent or null as when each is switched off on its own."""
    args.no_cpu = args.no_verify = True
    for k in EXTRA_LEGS:
        setattr(args, k, 0)


def make_images(args, rank, world):
    """Synthetic 12 MP 4:2:0 JPEGs (DRI = one MCU row). Image i of the global batch has seed i mod
    (unique * world) and is decoded by rank i mod world (jpeggpu_amd.shard), so a rank needs only the
    `unique` seeds of its own shard."""
    if args.workload == "photo":
        with open(PHOTO, "rb") as f:
            return [f.read()]
    from jpeggpu_amd import shard

    seeds = shard.shard_indices(args.unique * world, rank, world)
    # one image takes seconds of a core to encode: the rank's share of the host's cores encodes them side by side, in
    # spawned processes (nothing here has touched the GPU yet, and the children never do)
    procs = min(len(seeds), max(1, usable_cores() // world))
    if procs <= 1:
        return [_synth_cfg2(s) for s in seeds]
    import multiprocessing as mp

    with mp.get_context("spawn").Pool(procs) as pool:
        return pool.map(_synth_cfg2, seeds, chunksize=1)


def _synth_cfg2(seed):
    from tools import jpegsynth

    return jpegsynth.config(2, seed=seed)


class Slot:
    """One image in flight: its decoder, its temporary device memory and its output planes."""

    def __init__(self, torch, jp, data, device, subseq_bytes, planes_flat=None, planes_off=0, device_scan=False, batched=False):
        self.dec = jp.Decoder(subseq_bytes or None)
        if batched:
            # how many images share a call: the library plans for that (subsequence size, speculation, sync kernel)
            self.dec.set_batch_hint(int(batched))
        if device_scan:
            self.dec.set_device_scan(True)
        self.data = data
        self.info = self.dec.parse_header(data)
        self.tmp_size = self.dec.get_buffer_size()
        self.tmp = torch.empty(self.tmp_size + 256, dtype=torch.uint8, device=device)
        self.base = (self.tmp.data_ptr() + 255) // 256 * 256
        nc = self.info.num_components
        sizes = [(self.info.sizes_y[c], self.info.sizes_x[c]) for c in range(nc)]
        self.plane_bytes = sum(h * w for h, w in sizes)
        if planes_flat is None:
            planes_flat = torch.empty(self.plane_bytes, dtype=torch.uint8, device=device)
            planes_off = 0
        self.planes, o = [], planes_off
        for h, w in sizes:
            self.planes.append(planes_flat[o:o + h * w].view(h, w))
            o += h * w
        self.ptrs = [p.data_ptr() for p in self.planes]
        self.pitches = [p.stride(0) for p in self.planes]
        self.layout = self.dec.layout()

    def transfer(self, stream):
        self.dec.transfer(self.base, self.tmp_size, stream)

    def decode(self, stream):
        self.dec.decode(self.ptrs, self.pitches, self.base, self.tmp_size, stream)

    def stream_entries(self, torch):
        """16-bit entries of the symbol stream the write pass emitted for this image (sum of the data-unit table's
        counts, read back after a decode): what huff_write really stores and idct_kernel really gathers."""
        total = 0
        off0 = self.base - self.tmp.data_ptr()
        for s in range(self.layout.num_scans):
            sc = self.layout.scans[s]
            raw = self.tmp[off0 + sc.off_du_table: off0 + sc.off_du_table + 8 * sc.num_data_units]
            total += int((raw.view(torch.int32).view(-1, 2)[:, 1] & 0x7F).sum().item())
        return total


class BatchSet:
    """`batch` images of a rank, resident in HBM, in `nstreams` groups: each group is one jpeggpu_ext_decode_batch call
    per round on its own stream (--mode streams: the drop-in call, one image per call)."""

    def __init__(self, args, torch, jp, images, device, streams, batch):
        self.args, self.streams = args, streams
        nstreams = len(streams)
        batched = max(1, batch // nstreams) if args.mode == "batch" else 0  # images per jpeggpu_ext_decode_batch call
        probe = Slot(torch, jp, images[0], device, args.subseq_bytes, device_scan=bool(args.device_scan), batched=batched)
        self.per_image = probe.plane_bytes
        probe.dec.cleanup()
        # all planes of the rank's batch live in one flat tensor so that a gather is one collective
        self.planes_flat = torch.empty(self.per_image * batch, dtype=torch.uint8, device=device)
        self.slots = [Slot(torch, jp, images[i % len(images)], device, args.subseq_bytes, self.planes_flat, i * self.per_image,
                           device_scan=bool(args.device_scan), batched=batched) for i in range(batch)]
        for i, s in enumerate(self.slots):
            s.transfer(streams[i % nstreams].cuda_stream)
        torch.cuda.synchronize()
        self.groups = []
        if batched:
            for g in range(nstreams):
                mine = self.slots[g::nstreams]
                bt = jp.Batch(sum(s.layout.num_scans for s in mine))
                scratch = torch.empty(bt.scratch_size, dtype=torch.uint8, device=device)
                bt.set_items([(s.dec, s.ptrs, s.pitches, s.base, s.tmp_size) for s in mine])
                if args.sync_iters > 0:
                    bt.set_sync_iterations(args.sync_iters)
                bt.set_overlap(args.overlap)
                self.groups.append((bt, scratch, streams[g], len(mine)))

    def one_round(self):
        if self.groups:
            for bt, scratch, st, _ in self.groups:
                bt.decode(scratch.data_ptr(), st.cuda_stream)
        else:
            for i, s in enumerate(self.slots):
                s.decode(self.streams[i % len(self.streams)].cuda_stream)

    def step(self):
        for _ in range(self.args.rounds):
            self.one_round()

    def destroy(self):
        for bt, _, _, _ in self.groups:
            bt.destroy()
        for s in self.slots:
            s.dec.cleanup()


def algorithmic_bytes(slot, entries):
    """destuff+Huffman pass B_dh = stuffed scan bytes + 128 B per data unit; end-to-end B_e2e =
    stuffed scan bytes + plane bytes. And per kernel the bytes it has to move in THIS design:
    `entries` 16-bit symbol-stream entries per image (measured), an 8-byte record per data unit."""
    lay = slot.layout
    stuffed = lay.transferred_bytes
    ndu = sum(lay.scans[s].num_data_units for s in range(lay.num_scans))
    nsub = sum(lay.scans[s].num_subsequences for s in range(lay.num_scans))
    sb = lay.subsequence_bytes
    return {
        "stuffed": stuffed,
        "b_dh": stuffed + 128 * ndu,
        "b_e2e": stuffed + slot.plane_bytes,
        "front": stuffed,
        # stuffed bytes in, padded rows (own words + 3 mirrored ones) and the subsequence -> segment map out
        "destuff": stuffed + nsub * (sb + 12) + nsub * 4,
        # sync_intra: destuffed bytes read once + subsequence->segment map read + 21 B of state written
        "sync_intra": nsub * sb + nsub * 4 + nsub * 21,
        # sync_tail: about one subsequence of bitstream per subsequence (the live flows decay
        # geometrically, summing to ~0.9 lane-passes) + state read and written
        "sync_inter": nsub * sb + nsub * 40,
        "tails": nsub * 16,
        # write pass: destuffed bytes + state in, symbol stream + data-unit table out
        "write": nsub * sb + nsub * 24 + 2 * entries + 8 * ndu,
        # IDCT: symbol stream + data-unit table in, planes out
        "idct": 2 * entries + 8 * ndu + slot.plane_bytes,
    }


# ---- CPU baseline: runs before this process touches the GPU ---------------------------------------------------------

def _pillow_decode(data):
    import io

    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    im.load()


_TJ = None


def _turbojpeg():
    """libturbojpeg's planes-only decode (tjDecompressToYUVPlanes: entropy decode + IDCT, no upsampling, no colour
    conversion -- the closest CPU counterpart of this path), bound with ctypes; None when the library is not installed."""
    global _TJ
    if _TJ is not None:
        return _TJ or None
    import ctypes as C

    _TJ = False
    for name in ("libturbojpeg.so.0", "libturbojpeg.so"):
        try:
            L = C.CDLL(name)
        except OSError:
            continue
        try:
            L.tjInitDecompress.restype = C.c_void_p
            L.tjDecompressHeader3.argtypes = [C.c_void_p, C.c_char_p, C.c_ulong] + [C.POINTER(C.c_int)] * 4
            L.tjDecompressToYUVPlanes.argtypes = [C.c_void_p, C.c_char_p, C.c_ulong, C.POINTER(C.c_void_p), C.c_int,
                                                  C.POINTER(C.c_int), C.c_int, C.c_int]
            L.tjPlaneWidth.argtypes = L.tjPlaneHeight.argtypes = [C.c_int, C.c_int, C.c_int]
            handle = L.tjInitDecompress()
            if handle:
                _TJ = (L, handle)
                break
        except AttributeError:
            continue
    return _TJ or None


def _tj_decode(data, state={}):
    import ctypes as C

    L, h = _turbojpeg()
    w, hgt, ss, cs = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    if L.tjDecompressHeader3(h, data, len(data), C.byref(w), C.byref(hgt), C.byref(ss), C.byref(cs)) != 0:
        raise RuntimeError("tjDecompressHeader3 failed")
    key = (w.value, hgt.value, ss.value)
    if key not in state:
        bufs = [C.create_string_buffer(L.tjPlaneWidth(c, w.value, ss.value) * L.tjPlaneHeight(c, hgt.value, ss.value)) for c in range(3)]
        state.clear()
        state[key] = (bufs, (C.c_void_p * 3)(*[C.cast(b, C.c_void_p) for b in bufs]))
    _, planes = state[key]
    if L.tjDecompressToYUVPlanes(h, data, len(data), planes, w.value, None, hgt.value, 0) != 0:
        raise RuntimeError("tjDecompressToYUVPlanes failed")


def _turbo_backend():
    """(name, decode function, version) of the libjpeg-turbo decode available on this box, or None. Probe order of
    SURVEY.md 8(d): the TurboJPEG API's planes-only decode, then Pillow (libjpeg-turbo inside, YCbCr draft mode:
    planes at full resolution, i.e. including its chroma upsampling)."""
    if _turbojpeg():
        return "libturbojpeg tjDecompressToYUVPlanes (planes only)", _tj_decode, "turbojpeg"
    try:
        from PIL import features

        ver = features.version_feature("libjpeg_turbo")
        if ver:
            return "Pillow draft('YCbCr') on libjpeg-turbo %s (planes incl. chroma upsampling)" % ver, _pillow_decode, ver
    except Exception:
        pass
    return None


def _turbo_worker(job):
    data, seconds = job
    _, fn, _ = _turbo_backend()
    fn(data)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds and n < 256:
        fn(data)
        n += 1
    return n, time.perf_counter() - t0


def usable_cores():
    """Host cores this process may really use: the affinity mask, cut to the cgroup's CPU quota (a GPU box hands a
    one-GPU job a share of a big host) and to 64."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 64))


def cpu_baseline(args, data):
    """CPU decodes of the same 12 MP image on this box's host cores, bounded samples. `value` is libjpeg-turbo on ONE
    core (`kind` names the entry point that was found); `all_cores_value` the same on every core this process may use,
    one image stream per spawned worker process; `port_value` the oracle (scalar C restatement of the reference's
    arithmetic, oracle/jpeg_oracle.c) on one core -- also the fallback for `value` when no libjpeg-turbo is installed."""
    from oracle import oracle

    oracle.decode(data)  # warm (page in the library)
    n, t0 = 0, time.perf_counter()
    while True:
        oracle.decode(data)
        n += 1
        dt = time.perf_counter() - t0
        if dt >= args.cpu_seconds or n >= 64:
            break
    port = {"value": n / dt, "sample": "%d sequential decodes of one 12 MP image by oracle/jpeg_oracle.c, %.1f s" % (n, dt)}
    out = {"value": port["value"], "unit": "images/s", "cores": 1, "kind": "port", "sample": port["sample"],
           "port_value": port["value"]}
    try:
        backend = _turbo_backend()
        if backend:
            name, _, ver = backend
            budget = min(4.0, args.cpu_seconds)
            m, dt1 = _turbo_worker((data, budget))
            out.update({"value": m / dt1, "kind": "libjpeg-turbo: " + name, "version": ver,
                        "sample": "%d decodes of the same 12 MP image on one core, %.1f s" % (m, dt1)})
            cores = usable_cores()
            import multiprocessing as mp

            # spawned, not forked: the children never inherit anything of a GPU runtime (and this runs before the
            # parent has one)
            with mp.get_context("spawn").Pool(cores) as pool:
                t1 = time.perf_counter()
                res = pool.map(_turbo_worker, [(data, budget)] * cores)
                wall = time.perf_counter() - t1
            total = sum(r[0] for r in res)
            rate = sum(r[0] / r[1] for r in res)  # per-worker rates: the pool's start-up is not decode time
            out["all_cores_value"] = rate
            out["all_cores"] = cores
            out["all_cores_sample"] = "%d spawned processes, one image stream each, %d decodes, %.1f s wall incl. start-up" % (cores, total, wall)
    except Exception as e:  # libjpeg-turbo is optional on the box
        out["libjpeg_turbo_error"] = repr(e)
    return out


def pcie_inclusive(args, torch, jp, slots, groups, nstreams):
    """Full path from pinned host memory: per group of the batch, parse the headers on a pool of host threads
    (jpeggpu_ext_parse_headers), enqueue the two H2D copies of every image and one batched decode on the
    group's stream, and go on to the next group while that runs. Images/s over `--e2e-rounds` rounds."""
    pinned = []
    for s in slots:
        t = torch.empty(len(s.data), dtype=torch.uint8).pin_memory()
        t.numpy()[:] = memoryview(s.data)
        pinned.append(t)
    per_group = [list(range(g, len(slots), nstreams)) for g in range(nstreams)]
    copied = [torch.cuda.Event() for _ in groups]

    def one_round():
        for g, (bt, scratch, st, _) in enumerate(groups):
            copied[g].synchronize()  # the group's previous copies have executed: its decoders' pinned tables are free again
            idx = per_group[g]
            jp.parse_headers([slots[i].dec for i in idx], [pinned[i] for i in idx], num_threads=args.host_threads)
            for i in idx:
                slots[i].dec.transfer(slots[i].base, slots[i].tmp_size, st.cuda_stream)
            copied[g].record(st)
            bt.decode(scratch.data_ptr(), st.cuda_stream)

    one_round()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.e2e_rounds):
        one_round()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nbytes = sum(len(s.data) for s in slots)
    return {"value": args.e2e_rounds * len(slots) / dt, "unit": "images/s", "host_threads": args.host_threads,
            "rounds": args.e2e_rounds, "seconds": dt,
            "h2d_GBs": args.e2e_rounds * sum(s.layout.transferred_bytes for s in slots) / dt / 1e9,
            "file_bytes_per_image": nbytes // len(slots),
            "protocol": "pinned host JPEGs -> parse_headers (thread pool) -> transfer -> decode_batch, %d groups in flight" % nstreams}


def latency_probe(args, torch, jp, data, device, stream, device_scan):
    """The reference's own protocol (benchmark/benchmark_jpeggpu.hpp:69-108): per image parse_header +
    get_buffer_size + transfer + decode + stream sync, wall clock, pinned input, one warm-up. Library defaults
    unless `device_scan`."""
    s0 = Slot(torch, jp, data, device, 0, device_scan=device_scan)
    pinned = torch.empty(len(data), dtype=torch.uint8).pin_memory()
    pinned.numpy()[:] = memoryview(data)
    host_ptr, host_n = pinned.data_ptr(), pinned.numel()
    lat, lat_parse, lat_enqueue, lat_xfer = [], [], [], []
    warm = 3
    for it in range(args.latency_iters + warm):
        t1 = time.perf_counter()
        s0.dec.parse_header(host_ptr, host_n)
        n = s0.dec.get_buffer_size()
        t2 = time.perf_counter()
        s0.dec.transfer(s0.base, n, stream.cuda_stream)
        t2b = time.perf_counter()
        s0.dec.decode(s0.ptrs, s0.pitches, s0.base, n, stream.cuda_stream)
        t3 = time.perf_counter()
        stream.synchronize()
        if it >= warm:
            lat.append((time.perf_counter() - t1) * 1e3)
            lat_parse.append((t2 - t1) * 1e3)
            lat_xfer.append((t2b - t2) * 1e3)
            lat_enqueue.append((t3 - t2) * 1e3)
    worst = max(range(len(lat)), key=lambda i: lat[i])
    # device-only time of one decode, nothing else running
    s0.dec.set_profiling(True)
    for _ in range(10):
        s0.decode(stream.cuda_stream)
    stream.synchronize()
    solo = {k: v * 1e3 for k, v in s0.dec.stage_ms().items()}  # us, mean of 10 single-image decodes
    out = {"protocol": "parse+size+transfer+decode+sync, 1 image, 1 stream, pinned input (reference benchmark_jpeggpu.hpp:69-108)",
           "subsequence_bytes": s0.layout.subsequence_bytes, "device_scan": bool(s0.layout.scans[s0.layout.num_scans - 1].device_scan),
           "p50": statistics.median(lat), "mean": statistics.fmean(lat), "max": max(lat),
           "p99": sorted(lat)[min(len(lat) - 1, int(0.99 * len(lat)))],
           # where the slowest iteration spent its time (host calls; the rest is waiting for the stream)
           "slowest": {"iteration": worst, "total": lat[worst], "parse_header": lat_parse[worst], "transfer_call": lat_xfer[worst],
                       "decode_call": lat_enqueue[worst] - lat_xfer[worst], "synchronize": lat[worst] - lat_parse[worst] - lat_enqueue[worst]},
           "p50_host_parse": statistics.median(lat_parse), "p50_host_enqueue": statistics.median(lat_enqueue),
           "iters": len(lat), "images_per_s_single_stream": 1e3 / statistics.fmean(lat), "stage_us_device": solo}
    s0.dec.cleanup()
    return out


def _percentile(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def batch_point(args, torch, jp, images, device, stream, nb, iters, subseq_bytes=0, sync_iters=0, hint=None, overlap=1, stages=False):
    """Device time of ONE jpeggpu_ext_decode_batch call over `nb` images (inputs resident, one stream, nothing else on
    the chip): HIP events on the launch stream around the call, median over `iters` calls. The decoders are told how many
    images share a call (jpeggpu_ext_set_batched(decoder, nb)) and the library plans for that; `subseq_bytes`,
    `sync_iters` override the plan (sweeps: tools/probe/batch_curve.py)."""
    slots = []
    for i in range(nb):
        s = Slot(torch, jp, images[i % len(images)], device, subseq_bytes, batched=(nb if hint is None else hint))
        s.transfer(stream.cuda_stream)
        slots.append(s)
    bt = jp.Batch(sum(s.layout.num_scans for s in slots))
    scratch = torch.empty(bt.scratch_size, dtype=torch.uint8, device=device)
    bt.set_items([(s.dec, s.ptrs, s.pitches, s.base, s.tmp_size) for s in slots])
    if sync_iters > 0:
        bt.set_sync_iterations(sync_iters)
    bt.set_overlap(overlap)
    for _ in range(3):
        bt.decode(scratch.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    us = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        bt.decode(scratch.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        stream.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    lay = slots[0].layout
    out = {"images": nb, "device_us": statistics.median(us), "device_us_per_image": statistics.median(us) / nb,
           "device_us_p99": _percentile(us, 0.99), "subsequence_bytes": lay.subsequence_bytes,
           "subsequences_per_sequence": lay.subsequences_per_sequence, "hypotheses": lay.scans[0].hypotheses, "iters": iters}
    if stages:
        try:
            bt.set_profiling(True)
            for _ in range(5):
                bt.decode(scratch.data_ptr(), stream.cuda_stream)
                stream.synchronize()
            out["stage_us"] = {k: v * 1e3 for k, v in bt.stage_ms().items()}
        except jp.JpegGpuError:  # a call the library decodes image by image (lone plans): the decoders' own stage timing applies
            out["stage_us"] = {}
    bt.destroy()
    for s in slots:
        s.dec.cleanup()
    return out


def batch_curve(args, torch, jp, images, device, stream):
    """`batch_curve`: device time per image of one batched call of 1 / 2 / 4 / 8 / 16 / 32 / 64 cfg-2 images with the plan
    the library picks for that many (what a service that cannot wait for 64 images sees)."""
    return [batch_point(args, torch, jp, images, device, stream, nb, args.curve_iters) for nb in (1, 2, 4, 8, 16, 32, 64)]


def rank_shard(args, torch, jp, images, device, stream):
    """BASELINE.json configs[2]'s PER-RANK unit of work on one GPU: the 8 images a rank of an 8-GPU node decodes (cfg 2,
    seeds 0..7) through the whole boundary protocol -- jpeggpu_ext_parse_headers on a host thread pool, the two H2D copies
    of every image, ONE jpeggpu_ext_decode_batch, stream sync -- from pinned host memory, wall clock, `--shard-iters`
    iterations after 3 warm-ups; the device part of the same iterations from HIP events around the batched call."""
    nb = 8
    mine = [images[i % len(images)] for i in range(nb)]
    slots = [Slot(torch, jp, d, device, args.subseq_bytes, batched=nb) for d in mine]
    pinned = []
    for d in mine:
        t = torch.empty(len(d), dtype=torch.uint8).pin_memory()
        t.numpy()[:] = memoryview(d)
        pinned.append(t)
    # d_tmp must hold whatever plan parse_header picks in the loop: it is the same plan as the probe's (same bytes, same hint)
    bt = jp.Batch(sum(s.layout.num_scans for s in slots))
    scratch = torch.empty(bt.scratch_size, dtype=torch.uint8, device=device)
    bt.set_items([(s.dec, s.ptrs, s.pitches, s.base, s.tmp_size) for s in slots])
    bt.set_overlap(2)  # one caller stream: two parts hide each other's synchronisation tail (jpeggpu_ext.h)
    wall, dev, parse = [], [], []
    for it in range(args.shard_iters + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        jp.parse_headers([s.dec for s in slots], pinned, num_threads=min(nb, args.host_threads))
        t1 = time.perf_counter()
        for s in slots:
            s.dec.transfer(s.base, s.tmp_size, stream.cuda_stream)
        e0.record(stream)
        bt.decode(scratch.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        stream.synchronize()
        t2 = time.perf_counter()
        if it >= 3:
            wall.append((t2 - t0) * 1e3)
            parse.append((t1 - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
    ok = None
    if not args.no_verify:
        _, bad = verify(slots[:2], torch)
        ok = not bad
    lay = slots[0].layout
    out = {"what": "BASELINE.json configs[2], one rank's share on one GPU: 8 x cfg 2 (seeds 0..7) per call; parse_headers (%d host "
                   "threads) -> transfer -> decode_batch (2 overlapping parts) -> sync, pinned input" % min(nb, args.host_threads),
           "images_per_call": nb, "iters": len(wall), "p50_ms": statistics.median(wall), "p99_ms": _percentile(wall, 0.99),
           "device_p50_ms": statistics.median(dev), "device_p99_ms": _percentile(dev, 0.99), "host_parse_p50_ms": statistics.median(parse),
           "images_per_s": nb * len(wall) / (sum(wall) * 1e-3), "device_images_per_s": nb / (statistics.median(dev) * 1e-3),
           "subsequence_bytes": lay.subsequence_bytes, "verified": ok}
    bt.destroy()
    for s in slots:
        s.dec.cleanup()
    return out


def verify(slots, torch):
    """Planes of one slot per distinct image against the CPU oracle, after the timed loop: the timed launches
    did the work the number claims."""
    from oracle import oracle

    seen, bad = {}, []
    for s in slots:
        key = id(s.data)
        if key in seen:
            continue
        seen[key] = True
        ref = oracle.decode(s.data)
        for c in range(ref.ncomp):
            got = s.planes[c].cpu().numpy()
            if got.shape != ref.planes[c].shape or hashlib.sha256(got.tobytes()).digest() != hashlib.sha256(ref.planes[c].tobytes()).digest():
                bad.append((len(seen) - 1, c))
    return len(seen), bad


def timed_steps(torch, bset, steps, warmup, barrier):
    """W untimed steps, then K steps bracketed by barrier + synchronize on both sides; seconds of the K steps."""
    for p in bset.planes_flat.split(1 << 30):
        p.zero_()  # the planes hold nothing a previous run could have left behind
    for _ in range(warmup):
        bset.step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        bset.step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


DUMP_BYTES = 60 << 20  # --dump-outputs: values of all ranks together (64 MB less room for the .npy headers)
DUMP_SEED = 20261015


def dump_outputs(torch, bset, out_dir, rank, world):
    """--dump-outputs: what the timed path handed its caller in the last step -- the planes of every image of the rank's batch
    -- as DIR/plane<c>.npy (DIR/rank<r>_plane<c>.npy for N > 1), float32 [batch, m_c]: row i holds component c of image i at
    m_c positions of its plane (row-major flat indices). Where the whole batch fits in the budget that is every sample in
    order; otherwise each image gets its own positions, drawn once from numpy.random.default_rng(DUMP_SEED + rank) and
    sorted, m_c in proportion to the plane's size. Same arguments, same inputs, same positions: two builds compare
    file for file."""
    import numpy as np

    slots = bset.slots
    sizes = [p.numel() for p in slots[0].planes]
    nb = len(slots)
    per_image = max(len(sizes), DUMP_BYTES // 4 // world // nb)  # float32 values per image
    rng = np.random.default_rng(DUMP_SEED + rank)
    flat = bset.planes_flat.view(nb, bset.per_image)
    os.makedirs(out_dir, exist_ok=True)
    written, off = {}, 0
    for c, n in enumerate(sizes):
        m = n if sum(sizes) <= per_image else max(1, per_image * n // sum(sizes))
        if m >= n:
            vals = flat[:, off:off + n]
        else:
            pos = np.sort(np.stack([rng.choice(n, m, replace=False) for _ in range(nb)]), axis=1)
            idx = torch.from_numpy(pos + off).to(flat.device)
            vals = torch.gather(flat, 1, idx)
        a = vals.to(torch.float32).cpu().numpy()
        name = ("rank%d_plane%d" % (rank, c)) if world > 1 else ("plane%d" % c)
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = list(a.shape)
        off += n
    return {"dir": os.path.abspath(out_dir), "arrays": written, "dtype": "float32", "seed": DUMP_SEED + rank}


def serialized_stage_us(args, bset):
    """Average duration of every stage over `--roofline-launches` launches of ONE group (64 images by default) on one
    stream with nothing else on the chip: HIP events the library records on the launch stream between its launches."""
    bt, scratch, st, images_per_launch = bset.groups[0]
    bt.set_profiling(True)
    for _ in range(args.roofline_launches):
        bt.decode(scratch.data_ptr(), st.cuda_stream)
        st.synchronize()
    us = {k: v * 1e3 for k, v in bt.stage_ms().items()}
    bt.set_profiling(False)
    return us, images_per_launch


def committed_profile(name):
    """A summary under profiles/ written by tools/summarize_profiles.py from rocprofv3 --pmc passes over the serialized
    run (counters cannot be read from inside this process); {} when it is not there."""
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            return json.load(f)
    except Exception:
        return {}


def counter_ratios(c):
    """What the committed SQ counters of a kernel say about its waves' time (profiles/pmc_counters.json: rocprofv3 --pmc
    passes over the serialized run of ANOTHER process of the same tree): per cycle a wave is resident, the share in which
    it has an instruction being issued or executed (SQ_ACTIVE_INST_ANY / SQ_WAVE_CYCLES), waits for anything
    (SQ_WAIT_ANY), waits for an instruction's operands or result (SQ_WAIT_INST_ANY); and the instruction mix. The 4-cycle
    model behind `valu_issue_util` prices vector instructions only; these ratios are counter / counter and need no model."""
    wc = c.get("SQ_WAVE_CYCLES")
    if not wc:
        return None
    out = {"active_inst_per_wave_cycle": c.get("SQ_ACTIVE_INST_ANY", 0.0) / wc, "wait_any_per_wave_cycle": c.get("SQ_WAIT_ANY", 0.0) / wc,
           "wait_inst_per_wave_cycle": c.get("SQ_WAIT_INST_ANY", 0.0) / wc}
    for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_WAVES", "SQ_BUSY_CYCLES"):
        if k in c:
            out[k] = c[k]
    return out


def roofline_report(args, slot, stage_us, images_per_launch, entries, value, world):
    """The `roofline` and `kernels` objects (module docstring)."""
    ab = algorithmic_bytes(slot, entries)
    device_scan = bool(slot.layout.scans[0].device_scan)
    stages = [k for k in stage_us if k != "front" or device_scan]  # without the device scan "front" is a 24-us descriptor copy, not a kernel
    traffic = committed_profile("pmc_traffic.json")
    counters = committed_profile("pmc_counters.json")
    # huff_tail_write (round 5): the tail kernel's parts and the write pass's sequences as one launch, reported under "write";
    # "sync_inter" and "tails" then hold only the gaps between their events (no kernel: not listed below, but counted in the pass)
    # (what the library does for a call of this size: fewer than 220 000 subsequences keep the two kernels -- jg_defs.h)
    call_subseq = images_per_launch * sum(slot.layout.scans[k].num_subsequences for k in range(slot.layout.num_scans))
    fused = os.environ.get("JPEGGPU_FUSE_TAIL_WRITE", "1") != "0" and call_subseq >= 220000 and stage_us.get("sync_inter", 1e9) < 15.0
    names = dict(KERNEL_NAMES)
    if fused:
        names["write"] = "huff_tail_write"
        ab = dict(ab)
        ab["write"] = ab["write"] + ab["sync_inter"]
    kernels = {}
    for k in stages:
        if fused and k in ("sync_inter", "tails"):
            continue
        us = stage_us[k]
        name = names[k]
        t = traffic.get(name.split("+")[0], {}).get("per_image_bytes")
        valu = counters.get(name.split("+")[0], {}).get("SQ_INSTS_VALU")
        c = counters.get(name.split("+")[0], {})
        kernels[name] = {
            "avg_launch_us": us, "own_bytes_per_launch": ab[k] * images_per_launch,
            "own_GBs": ab[k] * images_per_launch / (us * 1e-6) / 1e9 if us > 0 else None,
            "own_frac_of_hbm_peak": ab[k] * images_per_launch / (us * 1e-6) / 1e9 / HBM_PEAK_GBS if us > 0 else None,
            "traffic_bytes_per_launch": t * images_per_launch if t else None,
            # RAW value of the 4-cycle model (SQ_INSTS_VALU x 4 cycles over the SIMD-cycles of this duration): simple additions
            # and shifts issue in 2.1-2.6 cycles (profiles/r04_valu_issue_cost_by_instruction.txt), so the model overestimates
            # and a kernel made of them can come out above 1; `issue_counters` below need no model
            "valu_issue_util": valu * VALU_CYCLES / (SIMDS * SHADER_HZ * us * 1e-6) if valu and us > 0 else None,
            "valu_issue_util_note": "4-cycle model, overestimates simple two-operand instructions (measured 2.1-2.6 cycles); not capped",
            # ratios of counters of the SAME unit (per wave-resident cycle), from the committed profile, not from this run
            "issue_counters": counter_ratios(c)}
    all_pass = [k for k in stages if k in PASS_STAGES]
    in_pass = [k for k in all_pass if names[k] in kernels]  # the stages that launch a kernel
    t_pass_us = sum(stage_us[k] for k in all_pass)
    pass_traffic = [kernels[names[k]]["traffic_bytes_per_launch"] for k in in_pass]
    pass_valu = [counters.get(names[k].split("+")[0], {}).get("SQ_INSTS_VALU") for k in in_pass]
    bytes_per_launch = ab["b_dh"] * images_per_launch
    # instruction mix of the pass from the committed counters (vector / scalar / LDS + memory)
    mix = {k: sum(counters.get(names[st].split("+")[0], {}).get(k, 0.0) for st in in_pass)
           for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR")}
    tot = sum(mix.values())
    limiter = "instruction issue" if not tot else ("instruction issue (vector %.0f %%, scalar %.0f %%, LDS / memory %.0f %% of the pass's instructions; "
                                                   "profiles/pmc_counters.json)" % (100 * mix["SQ_INSTS_VALU"] / tot, 100 * mix["SQ_INSTS_SALU"] / tot,
                                                                                  100 * (tot - mix["SQ_INSTS_VALU"] - mix["SQ_INSTS_SALU"]) / tot))
    roofline = None
    if t_pass_us > 0:
        achieved = bytes_per_launch / (t_pass_us * 1e-6) / 1e9
        roofline = {
            "bound": "hbm",
            # by the counter ratios, not by the model: a wave of the pass has an instruction in issue or execution in about 0.3 of
            # its resident cycles and waits for an instruction's operands in 0.2 (issue_counters); vector instructions are 70 % of
            # what it issues
            "limiter": limiter,
            "kernel": "destuff+Huffman pass: " + " + ".join(names[k] for k in in_pass),
            "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": sum(pass_traffic) if all(pass_traffic) else None,
            "traffic_source": "profiles/pmc_traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over serialized launches of "
                              "the same shape in ANOTHER process of the same tree (counters cannot be read from inside this one), "
                              "per-shape calibration of profiles/*_fetch_calibration.json; valu_issue_util and issue_counters come "
                              "from profiles/pmc_counters.json the same way -- only the durations are measured in this run",
            "issue_counters": counter_ratios({k: sum(counters.get(names[s].split("+")[0], {}).get(k, 0.0) for s in in_pass)
                                             for k in ("SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_ANY", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_INSTS_VALU",
                                                       "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_BUSY_CYCLES")}),
            "algorithmic_bytes_per_launch": bytes_per_launch, "algorithmic_bytes_per_image": ab["b_dh"],
            "avg_launch_us": t_pass_us, "images_per_launch": images_per_launch,
            "valu_issue_util": (sum(pass_valu) * VALU_CYCLES / (SIMDS * SHADER_HZ * t_pass_us * 1e-6)) if all(pass_valu) else None,
            "frac_at_throughput": ab["b_dh"] * value / world / 1e9 / HBM_PEAK_GBS,
            "what": "B_dh = stuffed scan bytes + 128 B per data unit (SURVEY.md 8d) x images per launch / SUM of the serialized "
                    "average durations of the pass's kernels / HBM peak; the kernels are bound by vector-instruction issue "
                    "(valu_issue_util: SQ_INSTS_VALU of profiles/pmc_counters.json x 4 cycles / (1024 SIMDs x 2.4 GHz x this time))",
            "measured": "HIP events on the launch stream, %d serialized launches of %d images, one stream"
                        % (args.roofline_launches, images_per_launch)}
    if roofline is not None:
        # the counter-derived figures belong to the committed profile's run: say how its durations compare with this run's
        prof_us = [traffic.get(names[k].split("+")[0], {}).get("profile_avg_us") for k in in_pass]
        if all(prof_us):
            ratio = t_pass_us / sum(prof_us)
            roofline["profile_pass_us"] = sum(prof_us)
            roofline["run_over_profile_duration"] = ratio
            if abs(ratio - 1.0) > 0.03:
                roofline["traffic_source"] += ("; NOTE: this run's pass took %.0f us, the profile's %.0f us (%+.1f %%): traffic, valu_issue_util and "
                                               "issue_counters are the profile's and are NOT rescaled" % (t_pass_us, sum(prof_us), 100.0 * (ratio - 1.0)))
    e2e = {"bytes_per_image": ab["b_e2e"], "throughput_GBs": ab["b_e2e"] * value / world / 1e9,
           "frac_of_hbm_peak": ab["b_e2e"] * value / world / 1e9 / HBM_PEAK_GBS}
    return roofline, kernels, e2e, ab


def gather_leg(args, torch, dist, jp, shard, bset, streams, device, rank, world, backend, barrier, max_over_ranks):
    """BASELINE.json configs[2]: 64 images over the ranks (image i -> rank i mod N), decoded, planes collected on rank 0.
    Double-buffered: round k decodes into plane buffer k % 2 on the decode stream, its gather runs on a side stream
    (RCCL's own stream behind it) while round k + 1 decodes into the other buffer. Three timings, same rounds each:
    decode alone, gather alone, the pipeline."""
    per_rank = max(1, min(64 // world, args.batch))
    per_image = bset.per_image
    # the rank's images parsed again for calls of `per_rank` images (jpeggpu_ext_set_batch_hint: the timed batch's
    # decoders were planned for 64 per call)
    mine = [Slot(torch, jp, bset.slots[i].data, device, args.subseq_bytes, batched=per_rank) for i in range(per_rank)]
    for s in mine:
        s.transfer(streams[0].cuda_stream)
    on_gpu = backend == "nccl"
    nbytes = per_rank * per_image
    bufs = [bset.planes_flat[:nbytes], torch.empty(nbytes, dtype=torch.uint8, device=device)]
    bts, scratches = [], []
    for b in range(2):
        items = []
        for i, s in enumerate(mine):
            ptrs, o = [], bufs[b].data_ptr() + i * per_image
            for p in s.planes:
                ptrs.append(o)
                o += p.numel()
            items.append((s.dec, ptrs, s.pitches, s.base, s.tmp_size))
        bt = jp.Batch(sum(s.layout.num_scans for s in mine))
        bt.set_items(items)
        bt.set_overlap(2 if per_rank >= 8 else 1)  # a rank's 8 images fill a sixth of the chip: two parts hide each other's sync tail
        bts.append(bt)
        scratches.append(torch.empty(bt.scratch_size, dtype=torch.uint8, device=device))
    gl = [None, None]
    if rank == 0:
        gl = [[torch.empty(nbytes, dtype=torch.uint8, device=device if on_gpu else "cpu") for _ in range(world)] for _ in range(2)]
    dec_st, comm_st = streams[0], streams[1 % len(streams)] if len(streams) > 1 else torch.cuda.Stream(device=device)
    decoded = [torch.cuda.Event() for _ in range(2)]
    gathered = [torch.cuda.Event() for _ in range(2)]

    def decode(b):
        bts[b].decode(scratches[b].data_ptr(), dec_st.cuda_stream)

    def gather(b):
        if on_gpu:
            with torch.cuda.stream(comm_st):
                shard.gather_planes(bufs[b], rank, world, dst=0, gather_list=gl[b])
        else:  # gloo rehearsal: the collective runs on CPU tensors
            comm_st.synchronize()
            shard.gather_planes(bufs[b].cpu(), rank, world, dst=0, gather_list=gl[b])

    def timed(fn):
        fn(0)
        torch.cuda.synchronize()
        barrier()
        t1 = time.perf_counter()
        for k in range(args.gather_rounds):
            fn(k)
        torch.cuda.synchronize()
        barrier()
        return max_over_ranks(time.perf_counter() - t1) / args.gather_rounds * 1e3

    def pipelined(k):
        b = k % 2
        dec_st.wait_event(gathered[b])  # the gather that read this buffer two rounds ago is done
        decode(b)
        decoded[b].record(dec_st)
        comm_st.wait_event(decoded[b])
        gather(b)
        gathered[b].record(comm_st)

    decode_ms = timed(lambda k: decode(k % 2))
    gather_ms = timed(lambda k: gather(k % 2))
    overlapped_ms = timed(pipelined)

    # what arrived on rank 0 is what every rank sent: 64-bit wrapping sums of the buffers, exchanged separately
    def checksum(t):
        return int(t[: t.numel() // 8 * 8].view(torch.int64).sum().item())

    ok = True
    for b in range(2):
        mine_sum = torch.tensor([checksum(bufs[b])], dtype=torch.int64, device=device if on_gpu else "cpu")
        sums = [torch.zeros_like(mine_sum) for _ in range(world)]
        dist.all_gather(sums, mine_sum)
        if rank == 0:
            ok = ok and all(checksum(gl[b][r]) == int(sums[r].item()) for r in range(world))
    for bt in bts:
        bt.destroy()
    sb = mine[0].layout.subsequence_bytes
    for s in mine:
        s.dec.cleanup()
    return {"what": "BASELINE.json configs[2]: 64 x 12 MP 4:2:0 sharded over the ranks (image i -> rank i mod N), decoded, planes "
                    "gathered on rank 0; the gather of round k overlaps the decode of round k + 1 (two plane buffers, side stream)",
            "images_per_round": per_rank * world, "rounds": args.gather_rounds,
            "value": per_rank * world / (overlapped_ms * 1e-3), "unit": "images/s",
            "decode_ms": decode_ms, "gather_ms": gather_ms, "overlapped_ms": overlapped_ms, "ms_per_round": overlapped_ms,
            "bytes_per_rank": nbytes, "backend": backend, "gathered_buffers_match_senders": ok, "subsequence_bytes": sb}


def segment_shard_leg(args, torch, dist, jp, shard, streams, device, rank, world, backend, barrier, max_over_ranks):
    """Restart-interval sharding of ONE large image (second bullet): 39 MP 4:2:0 (the size of
    BASELINE.json configs[3]) with one restart interval per MCU row; rank r decodes segments [r n / N, (r + 1) n / N)
    into its band of the planes (jpeggpu_ext_set_segment_shard), bands gathered on rank 0."""
    from tools import jpegsynth

    big = jpegsynth.encode(7216, 5408, ((2, 2), (1, 1), (1, 1)), True, (7216 + 15) // 16, quality=88, noise=9, seed=4242)
    dec = jp.Decoder()
    dec.set_batched(True)  # 256-byte subsequences: the share of a 39 MP image fills the chip
    dec.set_segment_shard(rank, world)
    info = dec.parse_header(big)
    n = dec.get_buffer_size()
    tmp = torch.empty(n + 256, dtype=torch.uint8, device=device)
    base = (tmp.data_ptr() + 255) // 256 * 256
    shapes = [(info.sizes_y[c], info.sizes_x[c]) for c in range(info.num_components)]
    full = [torch.zeros(h, w, dtype=torch.uint8, device=device) for h, w in shapes]
    rows = [dec.shard_rows(c) for c in range(info.num_components)]
    st = streams[0]
    on_gpu = backend == "nccl"
    dec.transfer(base, n, st.cuda_stream)
    all_rows = [None] * world
    dist.all_gather_object(all_rows, rows)

    def shard_round():
        with torch.cuda.stream(st):
            dec.decode([p.data_ptr() for p in full], [p.stride(0) for p in full], base, n, st.cuda_stream)
            band = torch.cat([full[c][a:a + k].reshape(-1) for c, (a, k) in enumerate(rows)])
            return shard.gather_bands(band if on_gpu else band.cpu(), rank, world, dst=0)

    bands = shard_round()
    torch.cuda.synchronize()
    barrier()
    t1 = time.perf_counter()
    for _ in range(args.segment_shard_rounds):
        bands = shard_round()
    torch.cuda.synchronize()
    barrier()
    dt = max_over_ranks(time.perf_counter() - t1)
    ok = None
    if rank == 0:  # the assembled image against this GPU's own decode of the whole file
        got = shard.assemble_bands(bands, all_rows, shapes)
        whole, _ = jp.decode_to_planes(big, device=str(device))
        ok = all(bool(torch.equal(got[c].to(device), whole[c])) for c in range(len(shapes)))
    dec.cleanup()
    return {"what": "ONE 7216x5408 4:2:0 image (39 MP, DRI = one MCU row) over the ranks by restart segments, "
                    "bands gathered on rank 0", "file_bytes": len(big), "rounds": args.segment_shard_rounds,
            "value": args.segment_shard_rounds / dt, "unit": "images/s", "ms_per_image": dt / args.segment_shard_rounds * 1e3,
            "rows_of_plane_0_per_rank": [r[0] for r in all_rows], "backend": backend,
            "assembled_equals_whole_decode": ok}


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if "WORLD_SIZE" not in os.environ and args.gpus > 1:
            # Started as the driver starts N = 1 (`python3 bench.py --gpus N ...`): this process becomes the launcher of its
            # own ranks. Nothing here has imported torch or touched the GPU yet; the ranks are a CHILD process
            # (torch.distributed.run), never an exec of this one, and its exit code is ours.
            import subprocess

            port = os.environ.get("MASTER_PORT") or str(29500 + os.getpid() % 2000)
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
                   "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
            raise SystemExit(subprocess.run(cmd).returncode)
        args.gpus = world

    images = make_images(args, rank, world)
    # CPU baseline: rank 0 at N = 1 only, and FIRST -- before this process has initialised HIP or RCCL, so that its
    # worker processes start from a parent without a GPU runtime
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu:
        cpu = cpu_baseline(args, images[0])

    import torch
    import torch.distributed as dist

    import jpeggpu_amd as jp
    from jpeggpu_amd import shard

    assert torch.cuda.is_available(), "bench.py needs a HIP device (there is no CPU fallback)"
    # JPEGGPU_BENCH_BACKEND=gloo rehearses the N > 1 control flow on a box with fewer GPUs than ranks
    # (ranks share devices, collectives on CPU tensors); the driver's runs use nccl (= RCCL).
    backend = os.environ.get("JPEGGPU_BENCH_BACKEND", "nccl")
    dev_index = local_rank % torch.cuda.device_count() if backend == "gloo" else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    if args.streams <= 0:
        args.streams = 4 if args.mode == "batch" else 16
    nstreams = max(1, min(args.streams, args.batch))
    streams = [torch.cuda.Stream(device=device) for _ in range(nstreams)]

    def barrier():
        if world > 1:
            dist.barrier()

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=device if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    bset = BatchSet(args, torch, jp, images, device, streams, args.batch)
    slots = bset.slots
    elapsed = max_over_ranks(timed_steps(torch, bset, args.steps, args.warmup, barrier))
    ms_per_step = elapsed / args.steps * 1e3
    images_per_step = world * args.batch * args.rounds
    value = images_per_step * args.steps / elapsed
    # before anything else writes into the planes (the gather leg reuses them)
    dumped = dump_outputs(torch, bset, args.dump_outputs, rank, world) if args.dump_outputs else None

    # every distinct image of the timed batch against the oracle
    verified, nverified = None, 0
    if not args.no_verify:
        nverified, bad = verify(slots, torch)
        ok = 0.0 if bad else 1.0
        if world > 1:
            ok = -max_over_ranks(-ok)  # min over ranks
        verified = ok == 1.0
        if bad:
            sys.stderr.write("bench: planes differ from the oracle: %r\n" % (bad[:8],))

    gather = None
    if world > 1 and args.gather_rounds > 0 and args.mode == "batch":
        gather = gather_leg(args, torch, dist, jp, shard, bset, streams, device, rank, world, backend, barrier, max_over_ranks)
    segment_shard = None
    if world > 1 and args.segment_shard_rounds > 0:
        segment_shard = segment_shard_leg(args, torch, dist, jp, shard, streams, device, rank, world, backend, barrier, max_over_ranks)

    out = None
    if rank == 0:
        # Roofline figures from SERIALIZED launches: one stream, one batched launch per stage, nothing else on the
        # chip -- what `rocprofv3 --kernel-trace --stats` of tools/collect_profiles.sh's serialized run reproduces
        # (profiles/). In the timed region the launches of the groups overlap and their durations say nothing
        # about a kernel alone.
        roofline, kernels, e2e, ab = None, {}, None, algorithmic_bytes(slots[0], 0)
        if args.roofline_launches > 0 and args.mode == "batch":
            stage_us, images_per_launch = serialized_stage_us(args, bset)
            entries = slots[0].stream_entries(torch)
            roofline, kernels, e2e, ab = roofline_report(args, slots[0], stage_us, images_per_launch, entries, value, world)
            # the same pass in ONE call over the rank's whole batch (256 images): what larger launches are worth -- the tail
            # kernel's latency and the last, partly filled round of workgroups are spread over four times the images
            # (`frac` stays the 64-image figure of every round so far: BASELINE configs[2] is a batch of 64)
            if roofline is not None and len(slots) > images_per_launch:
                bt = jp.Batch(sum(s.layout.num_scans for s in slots))
                scratch = torch.empty(bt.scratch_size, dtype=torch.uint8, device=device)
                bt.set_items([(s.dec, s.ptrs, s.pitches, s.base, s.tmp_size) for s in slots])
                bt.set_profiling(True)
                for _ in range(3):
                    bt.decode(scratch.data_ptr(), streams[0].cuda_stream)
                    streams[0].synchronize()
                us_all = {k: v * 1e3 for k, v in bt.stage_ms().items()}
                bt.destroy()
                t_all = sum(v for k, v in us_all.items() if k in PASS_STAGES and (k != "front" or bool(slots[0].layout.scans[0].device_scan)))
                roofline["by_images_per_launch"] = {
                    str(images_per_launch): {"pass_us": roofline["avg_launch_us"], "frac": roofline["frac"]},
                    str(len(slots)): {"pass_us": t_all, "frac": ab["b_dh"] * len(slots) / (t_all * 1e-6) / 1e9 / HBM_PEAK_GBS if t_all > 0 else None,
                                      "stage_us": us_all}}
        photo = args.workload == "photo"
        out = {
            "metric": "images/s, 12 MP 4:2:0 baseline JPEG decode, inputs resident in HBM "
                      "(value_full_path: from pinned host memory, parse + transfer + decode; latency_ms: p50 of the reference's protocol)",
            "value": value, "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,  # BASELINE.md holds no published number for this metric on this hardware
            "dtype": "int16/int32 fixed point, u8 out",
            "data": "the reference's photo (tests/golden/IMG_6510.JPG), one file repeated" if photo else "synthetic",
            "verified": verified, "verified_images": nverified,
            "config": {"workload": "cfg1 bytes: tests/golden/IMG_6510.JPG (the reference's 12 MP photo)" if photo else
                                   "cfg2: 4032x3024 4:2:0 interleaved baseline JPEG, DRI=252 (one MCU row), "
                                   "%d seeded images per rank" % len(images),
                       "images_per_gpu_per_step": args.batch * args.rounds, "images_per_step": images_per_step,
                       "batch_per_gpu": args.batch, "rounds_per_step": args.rounds,
                       "mode": args.mode, "streams": nstreams,
                       "subsequence_bytes": slots[0].layout.subsequence_bytes,
                       "device_scan": bool(slots[0].layout.scans[0].device_scan),
                       "stuffed_scan_bytes": ab["stuffed"], "parallelism": "image-sharded x%d" % world},
            "roofline": roofline,
            "roofline_e2e": e2e,
            "kernels": kernels,
        }
        if dumped is not None:
            out["dumped_outputs"] = dumped
        if gather is not None:
            out["gather"] = gather
        if segment_shard is not None:
            out["segment_shard"] = segment_shard
        if args.latency_iters > 0:
            out["latency_ms"] = latency_probe(args, torch, jp, slots[0].data, device, streams[0], device_scan=False)
            out["latency_ms_device_scan"] = latency_probe(args, torch, jp, slots[0].data, device, streams[0], device_scan=True)
        if args.mode == "batch" and args.e2e_rounds > 0:
            out["pcie_inclusive"] = pcie_inclusive(args, torch, jp, slots, bset.groups, nstreams)
            out["value_full_path"] = out["pcie_inclusive"]["value"]
    bset.destroy()
    del bset, slots
    torch.cuda.empty_cache()
    if rank == 0 and args.other_configs > 0:
        # the other BASELINE.json configurations under the per-image protocol (parity at full size: tests/), and the
        # reference's photo under the batched protocol of `value`
        from tools import jpegsynth

        saved, args.latency_iters = args.latency_iters, args.other_configs
        others = {}
        with open(PHOTO, "rb") as f:
            photo_bytes = f.read()
        for name, blob in (("config1_photo_12MP_420_dri252", photo_bytes),
                           ("config4_39MP_444_three_scans", jpegsynth.config(4)),
                           ("config5_12MP_4_components_8_tables_no_dri", jpegsynth.config(5)),
                           ("cfg2_geometry_without_restart_markers_12MP_420", jpegsynth.encode(
                               4032, 3024, ((2, 2), (1, 1), (1, 1)), True, 0, quality=88, noise=9, seed=0))):
            r = latency_probe(args, torch, jp, blob, device, streams[0], device_scan=False)
            others[name] = {"file_bytes": len(blob), "p50_ms": r["p50"], "p99_ms": r["p99"], "p50_host_parse_ms": r["p50_host_parse"],
                            "max_ms": r["max"], "slowest_ms": r["slowest"], "iters": r["iters"], "subsequence_bytes": r["subsequence_bytes"],
                            "stage_us_device": r["stage_us_device"]}
            if name.startswith("cfg2_geometry"):
                # no restart markers: with the device scan the block list of the multi-hypothesis walk is the device's too (round 5)
                r = latency_probe(args, torch, jp, blob, device, streams[0], device_scan=True)
                others[name]["with_device_scan_enabled"] = {"p50_ms": r["p50"], "p99_ms": r["p99"], "p50_host_parse_ms": r["p50_host_parse"],
                                                            "stage_us_device": r["stage_us_device"]}
            if name.startswith("config4"):
                # three scans: jpeggpu_ext_set_device_scan hands the LAST scan of such a file to the device only if it is the
                # bulk of the bytes; here it is a fifth, so the host walks all three (with the last one on the device, measured
                # in round 4: host parse 0.105 -> 0.099 ms, p50 0.58 -> 0.76 ms)
                r = latency_probe(args, torch, jp, blob, device, streams[0], device_scan=True)
                others[name]["with_device_scan_enabled"] = {"p50_ms": r["p50"], "p50_host_parse_ms": r["p50_host_parse"],
                                                            "last_scan_walked_on_device": r["device_scan"]}
        args.latency_iters = saved
        if world == 1 and args.photo_steps > 0 and args.mode == "batch" and args.workload != "photo":
            pset = BatchSet(args, torch, jp, [photo_bytes], device, streams, args.batch)
            dt = timed_steps(torch, pset, args.photo_steps, 1, lambda: None)
            p = others["config1_photo_12MP_420_dri252"]
            p["batch_images_per_s"] = args.batch * args.rounds * args.photo_steps / dt
            p["batch_protocol"] = "as `value`: %d images per round in %d groups, %d rounds per step, %d steps, inputs resident" % (
                args.batch, nstreams, args.rounds, args.photo_steps)
            p["batch_subsequence_bytes"] = pset.slots[0].layout.subsequence_bytes
            if args.roofline_launches > 0:
                us, ipl = serialized_stage_us(args, pset)
                p["batch_stage_us_serialized"] = us
                t_pass = sum(v for k, v in us.items() if k in PASS_STAGES and (k != "front" or args.device_scan))
                pab = algorithmic_bytes(pset.slots[0], 0)
                p["batch_roofline_frac"] = pab["b_dh"] * ipl / (t_pass * 1e-6) / 1e9 / HBM_PEAK_GBS if t_pass > 0 else None
            if not args.no_verify:
                _, bad = verify(pset.slots[:1], torch)
                p["batch_verified"] = not bad
            pset.destroy()
        out["other_configs"] = others
    if rank == 0 and world == 1 and args.mode == "batch":
        # what callers that cannot wait for 64 images see, and BASELINE configs[2]'s per-rank unit of work on this one GPU
        if args.curve_iters > 0:
            out["batch_curve"] = batch_curve(args, torch, jp, images, device, streams[0])
        if args.shard_iters > 0:
            out["config3_rank_shard"] = rank_shard(args, torch, jp, images, device, streams[0])
    if rank == 0:
        # The driver's record keeps `value`, `config`, `roofline` and `cpu_baseline` whole and only names the other keys:
        # the second half of BASELINE's metric (p50 latency), the PCIe-inclusive rate, the real image's fraction and the
        # small-batch figures are therefore ALSO stored inside `roofline` (copies of the keys above, nothing new).
        keep = {}
        lat = out.get("latency_ms") or {}
        if lat:
            keep["latency_p50_ms"], keep["latency_p99_ms"] = lat["p50"], lat["p99"]
            keep["latency_protocol"] = lat["protocol"]
        if out.get("latency_ms_device_scan"):
            keep["latency_p50_ms_device_scan"] = out["latency_ms_device_scan"]["p50"]
        if out.get("value_full_path") is not None:
            keep["value_full_path"] = out["value_full_path"]
        ph = (out.get("other_configs") or {}).get("config1_photo_12MP_420_dri252") or {}
        if ph.get("batch_roofline_frac") is not None:
            keep["photo_frac"] = ph["batch_roofline_frac"]
            keep["photo_images_per_s"] = ph.get("batch_images_per_s")
            keep["photo_pass_us_serialized"] = {k: v for k, v in (ph.get("batch_stage_us_serialized") or {}).items() if k in PASS_STAGES}
        if ph.get("p50_ms") is not None:
            keep["photo_latency_p50_ms"] = ph["p50_ms"]
        if out.get("batch_curve"):
            keep["batch_curve"] = [{"images": p["images"], "device_us_per_image": p["device_us_per_image"], "subsequence_bytes": p["subsequence_bytes"]}
                                   for p in out["batch_curve"]]
        if out.get("config3_rank_shard"):
            keep["config3_rank_shard"] = {k: out["config3_rank_shard"][k] for k in
                                          ("images_per_call", "iters", "p50_ms", "p99_ms", "device_p50_ms", "device_p99_ms", "images_per_s", "subsequence_bytes")}
        if out.get("roofline") is not None:
            out["roofline"].update(keep)
        else:
            out["config"].update(keep)
    if rank == 0 and cpu is not None:
        out["cpu_baseline"] = cpu
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
