"""Where an encoded file differs from the expected one: which stage of the encoder a failing comparison points at. Both files
are decoded by the CPU oracle; a coefficient that differs is encode_blocks' (colour conversion, downsampling, the forward
DCT, the quantiser, dummy blocks), equal coefficients leave the stages behind it (bit counts, the scans, packing, stuffing,
markers, the header). Called only by a comparison that has failed."""
import numpy as np

from tests.encode_ref import ZIGZAG


def byte_offset(got, want):
    n = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return "lengths %d / %d, first difference at byte %d" % (len(got), len(want), n)


def where_files_differ(got, want):
    """One line on the first difference between the device's file `got` and the expected file `want`."""
    if got is None:
        return "no file: the slot was reported too small"
    if got == want:
        return "the files are equal"
    where = byte_offset(got, want)
    try:
        from oracle import oracle

        oracle.build()
        ref = oracle.decode(want)
        try:
            dev = oracle.decode(got)
        except oracle.OracleError as e:
            return "%s; the oracle cannot read the device's stream (%s): packing, stuffing, markers or the header" % (where, e)
        if (dev.width, dev.height, dev.ncomp, dev.hs, dev.vs, dev.restart_interval) != (ref.width, ref.height, ref.ncomp, ref.hs, ref.vs, ref.restart_interval):
            return "%s; the headers describe different images" % where
        if not np.array_equal(dev.qtab, ref.qtab):
            return "%s; the quantisation tables differ" % where
        a, b = dev.stream_coef[0][:, ZIGZAG].astype(np.int64), ref.stream_coef[0][:, ZIGZAG].astype(np.int64)
        if a.shape != b.shape:
            return "%s; %d blocks were decoded where %d are expected" % (where, a.shape[0], b.shape[0])
        blocks = np.nonzero((a != b).any(1))[0]
        if len(blocks) == 0:
            return "%s; all %d blocks' coefficients are equal: the difference lies in packing, stuffing or markers, behind encode_blocks" % (where, a.shape[0])
        blk = int(blocks[0])
        k = int(np.nonzero(a[blk] != b[blk])[0][0])
        per_mcu = ref.scan_du_per_mcu[0]
        j = blk % per_mcu
        luma = ref.hs[0] * ref.vs[0] if ref.ncomp > 1 else 1
        comp = 0 if j < luma else 1 + j - luma
        return "%s; %d of %d blocks differ, the first is block %d (MCU %d, component %d) at zigzag index %d: %d where %d is expected -- encode_blocks" % (
            where, len(blocks), a.shape[0], blk, blk // per_mcu, comp, k, a[blk, k], b[blk, k])
    except Exception as e:  # the report must not hide the failure it describes
        return "%s (the oracle gave no more: %r)" % (where, e)
