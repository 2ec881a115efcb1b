// jg_decoder.cpp -- the lone decode (transfer, decode, the device's status word) and the decoder's part of the exported C
// ABI (include/jpeggpu/jpeggpu.h, jpeggpu_ext.h). The plan and the jobs are jg_plan.cpp's, the batch is jg_batch.cpp.
//
// Counterpart of the reference's src/jpeggpu.cpp:39-160 (argument checks, status strings) and
// src/decoder.cpp:67-354 (parse -> size -> transfer -> decode). Differences by design:
//   * one `plan` carves d_tmp for get_buffer_size / transfer / decode alike (the reference replays
//     decode_impl<false>, decoder.cpp:327-334);
//   * transfer ships the entropy-coded byte range plus ONE pinned table blob (2 copies instead of
//     ~10, and no post-EOI trailer; decoder.cpp:175-208);
//   * coefficients stay in stream order; there are no per-component coefficient planes, no transpose
//     pass and no DC pass (decoder.cpp:240-314).
#include "jg_decoder.hpp"
#include "jg_front.hpp"
#include "jg_kernels.hpp"
#include "jg_prog.hpp"
#include "jg_selftest_data.h"
#include "jg_stage_timer.hpp"
#include "jg_staging.hpp"
#include "jg_trunc.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <new>
#include <vector>

using jg::Decoder;

namespace {

/// A decoder as jpeggpu_decoder_startup makes it: with what needs the HIP runtime, which the Decoder only points at.
struct DeviceDecoder : jpeggpu_decoder {
    jg::StagingBuffer staging; // the table blob
    jg::StageTimer timer;
    DeviceDecoder() { d.timer = &timer; }
};

#define JG_CHECK_HIP(call)                                                                          \
    do {                                                                                            \
        const hipError_t err_ = (call);                                                             \
        if (err_ != hipSuccess) {                                                                   \
            d.logger.log("HIP error \"%s\" at: " __FILE__ ":%d\n", hipGetErrorString(err_), __LINE__); \
            return JPEGGPU_INTERNAL_ERROR;                                                          \
        }                                                                                           \
    } while (0)

jpeggpu_status do_transfer(Decoder& d, void* d_tmp, size_t tmp_size, hipStream_t stream)
{
    if (!d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    if (!d_tmp || (reinterpret_cast<uintptr_t>(d_tmp) & 255)) return JPEGGPU_INVALID_ARGUMENT;
    if (tmp_size < d.plan.total) return JPEGGPU_INTERNAL_ERROR; // reference util.hpp:66-68
    uint8_t* base = static_cast<uint8_t*>(d_tmp);
    JG_CHECK_HIP(hipMemcpyAsync(
        base + d.plan.off_bytes, d.data + d.reader.s.xfer_begin, d.plan.bytes_len, hipMemcpyHostToDevice, stream));
    JG_CHECK_HIP(hipMemcpyAsync(
        base + d.plan.off_blob, d.blob, d.plan.blob_size, hipMemcpyHostToDevice, stream));
    return JPEGGPU_SUCCESS;
}

/// The status word of the device-side front end (synchronises `stream`); SUCCESS for host-walked images.
jpeggpu_status read_device_status(Decoder& d, const void* d_tmp, hipStream_t stream, jpeggpu_status* status)
{
    *status = JPEGGPU_SUCCESS;
    const int k = device_scan_index(d);
    if (k < 0) return JPEGGPU_SUCCESS; // the host walk has already judged the stream
    uint32_t word = 0;
    const uint8_t* src = static_cast<const uint8_t*>(d_tmp) + d.plan.scan[k].d_status;
    if (hipMemcpyAsync(&word, src, sizeof(word), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return JPEGGPU_INTERNAL_ERROR;
    *status = word <= JPEGGPU_INCOMPLETE_BITSTREAM ? static_cast<jpeggpu_status>(word) : JPEGGPU_INTERNAL_ERROR;
    return JPEGGPU_SUCCESS;
}

/// The progressive part of a lone decode: the coefficient buffers zeroed, the scans level by level, the hand-over.
jpeggpu_status decode_progressive(Decoder& d, void* d_tmp, hipStream_t stream)
{
    using namespace jg;
    uint8_t* base      = static_cast<uint8_t*>(d_tmp);
    const ProgPlan& pp = d.plan.prog;
    JG_CHECK_HIP(hipMemsetAsync(base + pp.coef_begin, 0, pp.coef_bytes, stream));
    ProgExtent e;
    extend(e, *reinterpret_cast<const ProgHeader*>(d.blob + pp.blob.header));
    JG_CHECK_HIP(launch_prog(ProgImage{base, d.plan.off_blob + pp.blob.header}, e, stream));
    return JPEGGPU_SUCCESS;
}

} // namespace

jpeggpu_status jg::do_decode(Decoder& d, jpeggpu_img* img, void* d_tmp, size_t tmp_size, hipStream_t stream, bool may_block)
{
    using namespace jg;
    d.jobs.clear();
    // one image: latency matters, keep every flow inside the sequence's workgroup
    const jpeggpu_status st = build_jobs(d, img, d_tmp, tmp_size, jg::kSeqLanes, true, true, d.jobs);
    if (st != JPEGGPU_SUCCESS) return st;
    (void)d.timer->begin(stream);
    if (const int k = device_scan_index(d); k >= 0) {
        // Device-side front end for the image's last scan: its job lives in device memory, front_plan fills in its counts,
        // and the stages read it from there, with launch extents from the header's upper bounds. The scans in front of
        // it (a file of several scans) were walked on the host: their jobs travel by value, one launch per stage for all
        // of them beside the device-walked scan's.
        ScanJob* d_job = reinterpret_cast<ScanJob*>(static_cast<uint8_t*>(d_tmp) + d.plan.scan[k].d_job);
        const FrontParams P = front_params(d, d_tmp, d_job, k);
        // the job travels as a kernel argument of the first front-end kernel, which stores it to d_job
        JG_CHECK_HIP(launch_front(P, d.jobs[k], stream));
        JobExtent extent;
        extend(extent, d.jobs[k]);
        for (int stage = 0; stage < kNumStages; ++stage) {
            if (stage == kStageSyncIntra) {
                for (int i = 0; i < k; ++i)
                    if (d.jobs[i].sp.mh > 1) JG_CHECK_HIP(launch_mh(d.jobs[i], nullptr, d.plan.scan[i].max_seg_subseq, stream));
                if (d.jobs[k].sp.mh > 1) JG_CHECK_HIP(launch_mh(d.jobs[k], d_job, d.plan.scan[k].max_seg_subseq, stream));
            }
            if (k > 0) JG_CHECK_HIP(launch_stage_scans(static_cast<Stage>(stage), d.jobs.data(), k, stream));
            JG_CHECK_HIP(launch_stage_device_job(static_cast<Stage>(stage), d_job, extent, stream));
            (void)d.timer->mark(stage, stream);
        }
        if (d.device_scan == 2 && may_block) {
            // Checked mode (JPEGGPU_DEVICE_SCAN=1 / 2 / checked in the environment of a caller that knows only the drop-in API):
            // what the host walk would have reported from parse_header is known on the device only now. Wait for
            // it and return it, as such a caller cannot ask for it; nothing of the device-walked scan was written to the
            // planes if it is not success.
            jpeggpu_status dev = JPEGGPU_SUCCESS;
            const jpeggpu_status rc = read_device_status(d, d_tmp, stream, &dev);
            return rc != JPEGGPU_SUCCESS ? rc : dev;
        }
        return JPEGGPU_SUCCESS;
    }
    for (size_t i = 0; i < d.jobs.size(); ++i) {
        const ScanJob& job = d.jobs[i];
        d.logger.log(
            "scan %d: %d chunks, %d subsequences of %d bytes, %d sequences, %d segments\n",
            static_cast<int>(i), job.num_chunks, job.sp.num_subseq, d.subseq_bytes, job.num_seq, job.sp.num_segments);
    }
    // a file that ended early (jpeggpu_ext_set_truncated): three launches more for the scan it ends in (jg_trunc.hip)
    const int cut_scan = truncated_scan_index(d);
    const TruncParams cut = cut_scan >= 0 ? trunc_params(d, d_tmp) : TruncParams{};
    // every stage once, for all scans of the image at a time (they are independent: grid.y = scan)
    for (int stage = 0; stage < kNumStages; ++stage) {
        if (stage == kStageSyncIntra) {
            // multi-hypothesis speculation in front of the sequence kernel, which then starts from its table
            for (size_t i = 0; i < d.jobs.size(); ++i)
                if (d.jobs[i].sp.mh > 1) JG_CHECK_HIP(launch_mh(d.jobs[i], nullptr, d.plan.scan[i].max_seg_subseq, stream));
        }
        if (stage == kStageWrite && d.plan.prog.on) { // a progressive frame: its jobs have no other work in front of the IDCT
            const jpeggpu_status ps = decode_progressive(d, d_tmp, stream);
            if (ps != JPEGGPU_SUCCESS) return ps;
        }
        JG_CHECK_HIP(launch_stage_scans(static_cast<Stage>(stage), d.jobs.data(), static_cast<int>(d.jobs.size()), stream));
        if (cut_scan >= 0 && stage == kStageDestuff) JG_CHECK_HIP(launch_trunc_prepare(d.jobs[static_cast<size_t>(cut_scan)], cut, stream));
        if (cut_scan >= 0 && stage == kStageWrite) JG_CHECK_HIP(launch_trunc_finish(d.jobs[static_cast<size_t>(cut_scan)], cut, stream));
        (void)d.timer->mark(stage, stream);
    }
    return JPEGGPU_SUCCESS;
}

extern "C" {

const char* jpeggpu_get_status_string(enum jpeggpu_status stat)
{
    switch (stat) { // same strings as the reference, src/jpeggpu.cpp:41-60
    case JPEGGPU_SUCCESS: return "success";
    case JPEGGPU_INVALID_ARGUMENT: return "invalid argument";
    case JPEGGPU_INVALID_JPEG: return "invalid jpeg";
    case JPEGGPU_INTERNAL_ERROR: return "internal jpeggpu error";
    case JPEGGPU_NOT_SUPPORTED: return "jpeg is not supported";
    case JPEGGPU_OUT_OF_HOST_MEMORY: return "out of host memory";
    case JPEGGPU_INCOMPLETE_BITSTREAM: return "incomplete bitstream";
    }
    return "unknown status";
}

enum jpeggpu_status jpeggpu_decoder_startup(jpeggpu_decoder_t* decoder)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    *decoder = new (std::nothrow) DeviceDecoder();
    if (*decoder == nullptr) return JPEGGPU_OUT_OF_HOST_MEMORY;
    if (const char* e = std::getenv("JPEGGPU_SUBSEQ_BYTES")) {
        const int v = std::atoi(e);
        if (jg::subseq_bytes_supported(v)) (*decoder)->d.subseq_request = v;
    }
    // A caller of the drop-in API alone can opt into the device-side marker scan through the environment (jpeggpu_ext.h).
    if (const char* e = std::getenv("JPEGGPU_MULTI_HYPOTHESIS")) (*decoder)->d.mh_enabled = std::atoi(e) != 0;
    if (const char* e = std::getenv("JPEGGPU_DEVICE_SCAN")) {
        // 1, 2 and "checked": the CHECKED mode (2 of jpeggpu_ext_set_device_scan) -- a caller that knows only the drop-in
        // API cannot ask for the device's verdict, so decode waits for it and returns it; "async": mode 1, decode stays
        // asynchronous and a refused scan shows as untouched planes. (Round 3 made "1" the asynchronous mode; a caller who
        // had set it for round 2's checked mode lost the error reporting without notice: ADVICE r3.)
        const int v = std::atoi(e);
        const bool off = std::strcmp(e, "0") == 0 || std::strcmp(e, "off") == 0 || e[0] == 0;
        (*decoder)->d.device_scan = std::strcmp(e, "async") == 0 ? 1 : (v == 1 || v == 2 || std::strcmp(e, "checked") == 0) ? 2 : 0;
        // a value nobody recognises must not silently mean "off" (ADVICE r4); the mode in force is logged at parse_header
        if ((*decoder)->d.device_scan == 0 && !off)
            std::fprintf(stderr, "jpeggpu: JPEGGPU_DEVICE_SCAN=\"%s\" is not one of 0, off, 1, 2, checked, async: the device scan stays off\n", e);
    }
    // JPEGGPU_IDCT=islow: libjpeg's ISLOW IDCT at full size for a caller of the drop-in API alone (jpeggpu_ext_set_idct)
    if (const char* e = std::getenv("JPEGGPU_IDCT")) {
        if (std::strcmp(e, "islow") == 0) (*decoder)->d.idct_method_request = jg::kIdctIslow;
        else if (e[0] != 0 && std::strcmp(e, "reference") != 0)
            std::fprintf(stderr, "jpeggpu: JPEGGPU_IDCT=\"%s\" is not one of reference, islow: the reference IDCT stays in use\n", e);
    }
    // JPEGGPU_SCALE_MODE=libjpeg: libjpeg's per-component block sizes for scaled decodes (jpeggpu_ext_set_scale_mode)
    if (const char* e = std::getenv("JPEGGPU_SCALE_MODE")) {
        if (std::strcmp(e, "libjpeg") == 0) (*decoder)->d.scale_mode_request = JPEGGPU_EXT_SCALE_LIBJPEG;
        else if (e[0] != 0 && std::strcmp(e, "uniform") != 0)
            std::fprintf(stderr, "jpeggpu: JPEGGPU_SCALE_MODE=\"%s\" is not one of uniform, libjpeg: the uniform mode stays in use\n", e);
    }
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_set_logging(jpeggpu_decoder_t decoder, int do_logging)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.logger.enabled = do_logging != 0;
    return JPEGGPU_SUCCESS;
}

int is_css_444(struct jpeggpu_subsampling css, int num_components)
{
    if (num_components < 1 || num_components > JPEGGPU_MAX_COMP) return 0;
    for (int c = 0; c < num_components; ++c) {
        if (css.x[c] != 1 || css.y[c] != 1) return 0;
    }
    return 1;
}

enum jpeggpu_status jpeggpu_decoder_parse_header(
    jpeggpu_decoder_t decoder, struct jpeggpu_img_info* img_info, const uint8_t* data, size_t size)
{
    if (!decoder || !img_info || !data) return JPEGGPU_INVALID_ARGUMENT;
    Decoder& d = decoder->d;
    const jpeggpu_status st = d.plan_image(img_info, data, size);
    if (st != JPEGGPU_SUCCESS) return st;
    jg::StagingBuffer& staging = static_cast<DeviceDecoder*>(decoder)->staging;
    if (!staging.reserve(d.plan.blob_size)) return JPEGGPU_OUT_OF_HOST_MEMORY;
    d.fill_blob(staging.ptr);
    d.blob = staging.ptr;
    d.seq_subseq_used = 0;
    d.parsed = true;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_decoder_get_buffer_size(jpeggpu_decoder_t decoder, size_t* tmp_size)
{
    if (!decoder || !tmp_size) return JPEGGPU_INVALID_ARGUMENT;
    if (!decoder->d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    *tmp_size = decoder->d.plan.total;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_decoder_transfer(
    jpeggpu_decoder_t decoder, void* d_tmp, size_t tmp_size, jpeggpu_stream_t stream)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    return do_transfer(decoder->d, d_tmp, tmp_size, stream);
}

enum jpeggpu_status jpeggpu_decoder_decode(
    jpeggpu_decoder_t decoder, struct jpeggpu_img* img, void* d_tmp, size_t tmp_size, jpeggpu_stream_t stream)
{
    if (!decoder || !img) return JPEGGPU_INVALID_ARGUMENT;
    return do_decode(decoder->d, img, d_tmp, tmp_size, stream);
}

enum jpeggpu_status jpeggpu_decoder_cleanup(jpeggpu_decoder_t decoder)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    DeviceDecoder* dd = static_cast<DeviceDecoder*>(decoder); // every decoder is startup's
    dd->staging.release();
    delete dd;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_subsequence_bytes(jpeggpu_decoder_t decoder, int subseq_bytes)
{
    if (!decoder || (subseq_bytes != 0 && !jg::subseq_bytes_supported(subseq_bytes))) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.subseq_request = subseq_bytes; // 0: back to the per-image choice
    decoder->d.parsed         = false;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_batched(jpeggpu_decoder_t decoder, int batched)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    return jpeggpu_ext_set_batch_hint(decoder, batched != 0 ? jg::kBatchHintFull : 0);
}

enum jpeggpu_status jpeggpu_ext_set_batch_hint(jpeggpu_decoder_t decoder, int images_per_call)
{
    if (!decoder || images_per_call < 0) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.batch_hint = images_per_call;
    // up to kLonePlanImages images per call get the lone decode's plan (multi-hypothesis tables, 64-byte subsequences):
    // jpeggpu_ext_decode_batch then decodes them one by one, as jpeggpu_decoder_decode would (jg::lone_plan)
    decoder->d.batched = !jg::lone_plan(images_per_call);
    decoder->d.parsed  = false;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_segment_shard(jpeggpu_decoder_t decoder, int rank, int world)
{
    if (!decoder || world < 1 || rank < 0 || rank >= world) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.shard_rank  = rank;
    decoder->d.shard_world = world;
    decoder->d.parsed      = false;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_get_shard_rows(jpeggpu_decoder_t decoder, int component, int* first_row, int* num_rows)
{
    if (!decoder || !first_row || !num_rows) return JPEGGPU_INVALID_ARGUMENT;
    const Decoder& d = decoder->d;
    if (!d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    const jg::Stream& s = d.reader.s;
    if (component < 0 || component >= s.num_comp) return JPEGGPU_INVALID_ARGUMENT;
    const int size_y = d.full_y(component);
    *first_row = 0;
    *num_rows  = size_y;
    const jg::Scan& sc = s.scans[0];
    if (sc.total_segments == 0) return JPEGGPU_SUCCESS; // no shard: every row
    int v = 1;
    for (int a = 0; a < sc.num_comp; ++a)
        if (sc.comp[a].comp_idx == component) v = sc.comp[a].v;
    const int rows_per_mcu_row = d.blk(component) * v; // whole MCU rows: v blocks of the component's size at the scale each
    const int row0 = sc.first_mcu / sc.mcus_x * rows_per_mcu_row, row1 = (sc.first_mcu + sc.shard_mcus) / sc.mcus_x * rows_per_mcu_row;
    *first_row = std::min(row0, size_y);
    *num_rows  = std::min(row1, size_y) - *first_row;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_profiling(jpeggpu_decoder_t decoder, int enable)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.timer->enable(enable != 0);
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_get_stage_ms(jpeggpu_decoder_t decoder, float* ms)
{
    if (!decoder || !ms) return JPEGGPU_INVALID_ARGUMENT;
    return decoder->d.timer->mean_ms(ms);
}

enum jpeggpu_status jpeggpu_ext_get_layout(jpeggpu_decoder_t decoder, struct jpeggpu_ext_layout* out)
{
    if (!decoder || !out) return JPEGGPU_INVALID_ARGUMENT;
    const Decoder& d = decoder->d;
    if (!d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    const jg::Stream& s = d.reader.s;
    std::memset(out, 0, sizeof(*out));
    out->subsequence_bytes = d.subseq_bytes;
    // of the last decode call built from this parse, whichever call it was (jpeggpu_decoder_decode and small batches: 240, a
    // full batch: 255); before any: what a call of the kind the decoder was set up for would use
    out->subsequences_per_sequence = d.seq_subseq_used ? d.seq_subseq_used : d.batched ? jg::kSeqSubseqBatch : jg::kSeqSubseq;
    out->num_scans         = s.num_scans;
    out->transferred_bytes = d.plan.bytes_len;
    out->blob_bytes        = d.plan.blob_size;
    out->off_bytes         = d.plan.off_bytes;
    out->off_qtables       = d.plan.off_blob + d.plan.blob_qtables;
    out->shard_rank        = d.shard_rank;
    out->shard_world       = d.shard_world;
    for (int i = 0; i < s.num_scans; ++i) {
        const jg::Scan& sc         = s.scans[i];
        const jg::ScanPlan& pl     = d.plan.scan[i];
        jpeggpu_ext_scan_layout& o = out->scans[i];
        o.num_components           = sc.num_comp;
        for (int k = 0; k < sc.num_comp; ++k) o.component_idx[k] = sc.comp[k].comp_idx;
        o.off_state_dc01 = pl.st_dc01;
        o.off_state_dc23 = pl.st_dc23;
        o.num_subsequences   = sc.num_subseq;
        o.num_segments       = static_cast<int>(sc.segments.size());
        o.num_sequences      = static_cast<int>((static_cast<size_t>(sc.num_subseq) + out->subsequences_per_sequence - 1) / out->subsequences_per_sequence);
        o.num_data_units     = sc.num_du;
        o.data_units_per_mcu = sc.du_per_mcu;
        o.num_chunks         = static_cast<int>(sc.chunks.size());
        o.off_segments       = d.plan.off_blob + pl.blob_segments;
        o.off_chunks         = d.plan.off_blob + pl.blob_chunks;
        o.off_destuffed      = pl.destuffed;
        o.off_segment_index  = pl.seg_idx;
        o.off_state_p        = pl.st_p;
        o.off_state_n        = pl.st_n;
        o.off_state_cz       = pl.st_cz;
        o.off_symbols        = pl.sym;
        o.off_du_table       = pl.du_tab;
        o.symbol_region_entries = static_cast<int>(jg::sym_region_entries(d.subseq_bytes));
        o.device_scan           = sc.device_walk ? 1 : 0;
        o.hypotheses            = pl.mh;
        o.hypothesis_blocks     = pl.mh_blocks_device ? pl.mh_blocks_device : static_cast<int>(pl.mh_blocks.size());
        if (sc.device_walk) {
            o.num_segments      = sc.expect_segments;
            o.num_chunks        = sc.max_chunks;
            o.off_segments      = pl.d_segments;
            o.off_chunks        = pl.d_chunks;
            o.off_device_status = pl.d_status;
        }
    }
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_device_scan(jpeggpu_decoder_t decoder, int enable)
{
    if (!decoder || enable < 0 || enable > 2) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.device_scan = enable;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_scale(jpeggpu_decoder_t decoder, int scale_denom)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    int lg = 0;
    while (lg <= 3 && (1 << lg) != scale_denom) ++lg;
    if (lg > 3) return JPEGGPU_INVALID_ARGUMENT; // 1, 2, 4 or 8
    decoder->d.scale_log2_request = lg;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_transcode_orientation(jpeggpu_decoder_t decoder, int orientation, int trim)
{
    if (!decoder || orientation < 1 || orientation > 8 || (trim != 0 && trim != 1)) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.transcode_orientation = orientation;
    decoder->d.transcode_trim        = trim != 0;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_transcode_crop(jpeggpu_decoder_t decoder, int x, int y, int width, int height)
{
    if (!decoder || x < 0 || y < 0 || width < 0 || height < 0) return JPEGGPU_INVALID_ARGUMENT;
    if ((width == 0 || height == 0) && (x || y || width || height)) return JPEGGPU_INVALID_ARGUMENT; // all zero: no crop
    int* r = decoder->d.transcode_crop;
    r[0] = x, r[1] = y, r[2] = width, r[3] = height;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_transcode_frame(jpeggpu_decoder_t decoder, int mode)
{
    if (!decoder || (mode != JPEGGPU_EXT_TRANSCODE_FRAME_ENCODER && mode != JPEGGPU_EXT_TRANSCODE_FRAME_SOURCE)) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.transcode_frame = mode;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_scale_mode(jpeggpu_decoder_t decoder, enum jpeggpu_ext_scale_mode mode)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    const int m = static_cast<int>(mode);
    if (m != JPEGGPU_EXT_SCALE_UNIFORM && m != JPEGGPU_EXT_SCALE_LIBJPEG) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.scale_mode_request = m;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_luma_only(jpeggpu_decoder_t decoder, int enable)
{
    if (!decoder || (enable != 0 && enable != 1)) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.luma_only_request = enable != 0;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_get_scale_info(jpeggpu_decoder_t decoder, struct jpeggpu_ext_scale_info* info)
{
    if (!decoder || !info) return JPEGGPU_INVALID_ARGUMENT;
    const Decoder& d = decoder->d;
    if (!d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    std::memset(info, 0, sizeof(*info));
    info->scale_denom = 1 << d.scale_log2;
    info->mode        = d.scale_mode;
    for (int c = 0; c < d.reader.s.num_comp; ++c) info->block_size[c] = d.blk(c);
    // jdsample.c: do_fancy_upsampling && min_DCT_scaled_size > 1
    info->fancy_upsampling = !(d.scale_mode == JPEGGPU_EXT_SCALE_LIBJPEG && d.scale_log2 == 3);
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_get_color_space(jpeggpu_decoder_t decoder, enum jpeggpu_ext_color_space* color)
{
    static_assert(jg::kColorUnknown == int{JPEGGPU_EXT_COLOR_UNKNOWN} && jg::kColorGray == int{JPEGGPU_EXT_COLOR_GRAY} &&
                      jg::kColorYCbCr == int{JPEGGPU_EXT_COLOR_YCBCR} && jg::kColorRGB == int{JPEGGPU_EXT_COLOR_RGB} &&
                      jg::kColorCMYK == int{JPEGGPU_EXT_COLOR_CMYK} && jg::kColorYCCK == int{JPEGGPU_EXT_COLOR_YCCK},
                  "jg::ColorSpace is enum jpeggpu_ext_color_space");
    if (!decoder || !color) return JPEGGPU_INVALID_ARGUMENT;
    if (!decoder->d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    *color = static_cast<jpeggpu_ext_color_space>(decoder->d.reader.s.color_space);
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_get_orientation(jpeggpu_decoder_t decoder, int* orientation)
{
    if (!decoder || !orientation) return JPEGGPU_INVALID_ARGUMENT;
    if (!decoder->d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    *orientation = decoder->d.reader.s.orientation;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_progressive(jpeggpu_decoder_t decoder, int enable)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.progressive = enable != 0;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_truncated(jpeggpu_decoder_t decoder, int enable)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.truncated = enable != 0;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_get_truncated(jpeggpu_decoder_t decoder, struct jpeggpu_ext_truncated_info* info)
{
    if (!decoder || !info) return JPEGGPU_INVALID_ARGUMENT;
    if (!decoder->d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    const jg::Stream::Truncation& t = decoder->d.reader.s.trunc;
    std::memset(info, 0, sizeof(*info));
    info->truncated              = t.no_eoi ? 1 : 0;
    info->scan                   = t.scan;
    info->scan_bytes             = t.scan >= 0 ? t.scan_bytes : 0;
    info->first_missing_interval = t.first_missing_interval;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_get_progressive_info(jpeggpu_decoder_t decoder, struct jpeggpu_ext_progressive_info* info)
{
    if (!decoder || !info) return JPEGGPU_INVALID_ARGUMENT;
    const Decoder& d = decoder->d;
    if (!d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    std::memset(info, 0, sizeof(*info));
    const jg::Stream& s = d.reader.s;
    if (!s.progressive) return JPEGGPU_SUCCESS;
    info->progressive = 1;
    info->num_scans   = static_cast<int>(s.prog_scans.size());
    info->num_levels  = s.num_levels;
    for (int c = 0; c < s.num_comp; ++c) {
        info->off_coefficients[c] = d.plan.prog.coef[c];
        info->blocks_x[c] = s.prog_blocks_x[c], info->blocks_y[c] = s.prog_blocks_y[c];
        info->visible_blocks_x[c] = s.scans[c].mcus_x, info->visible_blocks_y[c] = s.scans[c].mcus_y;
    }
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_idct(jpeggpu_decoder_t decoder, enum jpeggpu_ext_idct method)
{
    if (!decoder) return JPEGGPU_INVALID_ARGUMENT;
    const int m = static_cast<int>(method);
    if (m != JPEGGPU_EXT_IDCT_REFERENCE && m != JPEGGPU_EXT_IDCT_ISLOW) return JPEGGPU_INVALID_ARGUMENT;
    decoder->d.idct_method_request = m == JPEGGPU_EXT_IDCT_ISLOW ? jg::kIdctIslow : jg::kIdctReference;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_set_crop(jpeggpu_decoder_t decoder, int x, int y, int width, int height)
{
    if (!decoder || x < 0 || y < 0 || width < 0 || height < 0 || (width == 0) != (height == 0)) return JPEGGPU_INVALID_ARGUMENT;
    int* r = decoder->d.crop_request;
    r[0] = width ? x : 0, r[1] = width ? y : 0, r[2] = width, r[3] = height; // 0 x 0: no crop
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_get_crop(jpeggpu_decoder_t decoder, struct jpeggpu_ext_crop_info* info)
{
    if (!decoder || !info) return JPEGGPU_INVALID_ARGUMENT;
    const Decoder& d = decoder->d;
    if (!d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    const jg::Stream& s = d.reader.s;
    std::memset(info, 0, sizeof(*info));
    info->x      = d.crop.on ? d.crop.x : 0;
    info->y      = d.crop.on ? d.crop.y : 0;
    info->width  = d.crop.on ? d.crop.w : d.scaled(s.size_x);
    info->height = d.crop.on ? d.crop.h : d.scaled(s.size_y);
    for (int c = 0; c < s.num_comp; ++c) {
        info->origin_x[c] = d.crop.on ? d.crop.ox[c] : 0;
        info->origin_y[c] = d.crop.on ? d.crop.oy[c] : 0;
        info->full_x[c]   = d.full_x(c);
        info->full_y[c]   = d.full_y(c);
    }
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_get_device_status(
    jpeggpu_decoder_t decoder, const void* d_tmp, jpeggpu_stream_t stream, enum jpeggpu_status* status)
{
    if (!decoder || !d_tmp || !status) return JPEGGPU_INVALID_ARGUMENT;
    Decoder& d = decoder->d;
    if (!d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    return read_device_status(d, d_tmp, stream, status);
}

enum jpeggpu_status jpeggpu_ext_self_test(jpeggpu_stream_t stream)
{
    // One small decode through the public calls, planes hashed against constants. The write pass refills its bit window
    // with a counted wait the compiler knows nothing about (jg_kernels.hip, RowWindow; the build checks the generated code,
    // jpeggpu_amd/build.py): this is the same question asked of the running system -- driver, firmware, device.
    jpeggpu_decoder_t dec = nullptr;
    if (jpeggpu_decoder_startup(&dec) != JPEGGPU_SUCCESS) return JPEGGPU_OUT_OF_HOST_MEMORY;
    jpeggpu_status result = JPEGGPU_INTERNAL_ERROR;
    void* d_tmp           = nullptr;
    uint8_t* d_planes     = nullptr;
    std::vector<uint8_t> host;
    do {
        jpeggpu_img_info info;
        if (jpeggpu_decoder_parse_header(dec, &info, jg::kSelfTestJpeg, sizeof(jg::kSelfTestJpeg)) != JPEGGPU_SUCCESS) break;
        size_t tmp_size = 0, total = 0, off[3];
        if (jpeggpu_decoder_get_buffer_size(dec, &tmp_size) != JPEGGPU_SUCCESS || info.num_components != 3) break;
        for (int c = 0; c < 3; ++c) {
            if (info.sizes_x[c] != jg::kSelfTestW[c] || info.sizes_y[c] != jg::kSelfTestH[c]) break;
            off[c] = total;
            total += static_cast<size_t>(jg::kSelfTestW[c]) * jg::kSelfTestH[c];
        }
        if (total != 96u * 80u + 2u * 48u * 40u) break;
        if (hipMalloc(&d_tmp, tmp_size) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&d_planes), total) != hipSuccess) break;
        jpeggpu_img img{};
        for (int c = 0; c < 3; ++c) {
            img.image[c] = d_planes + off[c];
            img.pitch[c] = jg::kSelfTestW[c];
        }
        if (jpeggpu_decoder_transfer(dec, d_tmp, tmp_size, stream) != JPEGGPU_SUCCESS) break;
        if (jpeggpu_decoder_decode(dec, &img, d_tmp, tmp_size, stream) != JPEGGPU_SUCCESS) break;
        try {
            host.resize(total);
        } catch (const std::bad_alloc&) {
            result = JPEGGPU_OUT_OF_HOST_MEMORY;
            break;
        }
        if (hipMemcpyAsync(host.data(), d_planes, total, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            break;
        bool same = true;
        for (int c = 0; c < 3; ++c) {
            uint64_t h = 0xcbf29ce484222325ull; // FNV-1a
            for (size_t i = 0, n = static_cast<size_t>(jg::kSelfTestW[c]) * jg::kSelfTestH[c]; i < n; ++i) h = (h ^ host[off[c] + i]) * 0x100000001b3ull;
            same = same && h == jg::kSelfTestHash[c];
        }
        result = same ? JPEGGPU_SUCCESS : JPEGGPU_INTERNAL_ERROR;
    } while (false);
    (void)hipGetLastError();
    if (d_tmp) (void)hipFree(d_tmp);
    if (d_planes) (void)hipFree(d_planes);
    (void)jpeggpu_decoder_cleanup(dec);
    return result;
}

enum jpeggpu_status jpeggpu_ext_parse_headers(
    const struct jpeggpu_ext_parse_item* items, int num_items, int num_threads, enum jpeggpu_status* statuses)
{
    if (!items || num_items < 0 || !statuses) return JPEGGPU_INVALID_ARGUMENT;
    for (int i = 0; i < num_items; ++i) {
        statuses[i] = JPEGGPU_INVALID_ARGUMENT;
        for (int j = 0; j < i; ++j) // one decoder must not be used concurrently
            if (items[i].decoder && items[i].decoder == items[j].decoder) return JPEGGPU_INVALID_ARGUMENT;
    }
    if (num_threads < 1) num_threads = 1;
    if (num_threads > num_items) num_threads = num_items;
    std::atomic<int> next{0};
    const auto work = [&]() {
        for (int i = next.fetch_add(1); i < num_items; i = next.fetch_add(1)) {
            const jpeggpu_ext_parse_item& it = items[i];
            statuses[i] = jpeggpu_decoder_parse_header(it.decoder, it.img_info, it.data, it.size);
        }
    };
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < num_threads; ++t) pool.emplace_back(work);
    } catch (...) {
        // fewer threads than asked for: the calling thread picks up the rest
    }
    work();
    for (std::thread& t : pool) t.join();
    for (int i = 0; i < num_items; ++i)
        if (statuses[i] != JPEGGPU_SUCCESS) return statuses[i];
    return JPEGGPU_SUCCESS;
}

} // extern "C"
