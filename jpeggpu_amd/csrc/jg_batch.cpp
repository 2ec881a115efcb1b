// jg_batch.cpp -- jpeggpu_ext_decode_batch: many images, one launch per stage and part (jpeggpu_ext.h). The jobs of all
// items are built on the host (jg_plan.cpp), travel to the device in one copy and are decoded with the batch variants of
// the kernels; a call planned as lone decodes goes through the lone decode instead (jg_decoder.cpp, do_decode).
#include "jg_decoder.hpp"
#include "jg_front.hpp"
#include "jg_kernels.hpp"
#include "jg_prog.hpp"
#include "jg_stage_timer.hpp"
#include "jg_trunc.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

using jg::Decoder;

struct jpeggpu_batch {
    static constexpr int kRing = 4;
    int max_jobs = 0;
    uint8_t* staging[kRing]     = {}; // ScanJob[n], then FrontParams[device-scanned images]
    hipEvent_t copied[kRing]    = {};
    bool in_use[kRing]          = {};
    int next                    = 0;
    // Flow iterations inside the sequence kernel of a batch. One: speculate + verify there, the rest in the tail kernel. More
    // were measured with the survivors re-packed into one wave per workgroup (round 4): 2 / 3 / 8 iterations take the tail
    // kernel from 364 to 204 / 70 / 14 us per 64 images and the sequence kernel from 680 to 937 / 1109 / 1138 -- a
    // workgroup keeps its 22 KB of tables in LDS while one of its four waves works, and LDS is what bounds the kernel.
    int sync_iters              = 1;
    bool sync_iters_set         = false; // jpeggpu_ext_batch_set_sync_iterations was called: the caller's cap, whatever the call's size
    // Calls of fewer subsequences than this keep every flow in the sequence kernel (decode_batch_impl).
    long long keep_flows_below  = jg::kKeepFlowsBelowSubseq;
    // Full batches: the tail kernel's parts and the write pass's sequences as one launch (jg_kernels.hip: huff_tail_write).
    bool fuse_tail_write        = true;
    // Consecutive subsequences a lane of the batched sequence kernel owns (jg_sync_runs.h): 1, 2 or 4. Runs apply where a
    // call takes huff_sync_intra_batch with its single iteration: not to calls that keep every flow in the sequence kernel,
    // not under a caller's jpeggpu_ext_batch_set_sync_iterations. Two: every run of `value` above every run with 1 on the
    // same card, +2.5 %; four is slower than one (EXPERIMENTS.md: the fetch pattern costs more than the decodes save).
    int sync_run                = 2;
    // jpeggpu_ext_batch_set_coefficients_only: the calls stop in front of the IDCT stage (a transcode reads the entropy
    // stage's output in d_tmp, never the planes) and their items' plane pointers may be NULL.
    bool coefficients_only      = false;
    // A caller with ONE stream leaves the GPU idle while the latency-bound tail kernel runs (a fifth of a
    // batch's time). With overlap > 1 the jobs are split into that many parts, part 0 on the caller's
    // stream and the others on internal streams forked from and joined back into it with events.
    static constexpr int kMaxOverlap = 4;
    int overlap                 = 1;
    hipStream_t aux[kMaxOverlap - 1] = {};
    hipEvent_t joined[kMaxOverlap - 1] = {};
    std::vector<jg::ScanJob> jobs;
    std::vector<jg::FrontParams> fronts;
    std::vector<jg::ProgImage> progs;    // the progressive items of the call (jg_prog.hpp), and their launch extents
    jg::ProgExtent prog_extent;
    std::vector<jg::TruncRef> truncs;    // the scans of the call whose file ended early (jg_trunc.hpp), in job order,
    std::vector<int> trunc_job;          // ... and the index of each one's job
    hipEvent_t prog_done        = nullptr; // overlap > 1: the other streams' IDCT waits for the progressive launches
    std::vector<int> order, group_begin; // scratch of decode_batch: items by subsequence size, job ranges of the sizes
    struct Part {                        // ... and the parts of the job array, one launch per stage each
        int begin, end, way;
        jg::JobExtent extent;
    };
    std::vector<Part> parts;
    jg::StageTimer timer; // optional stage timing, same contract as the decoder's: kNumStages + 1 events per call
};

namespace {

/// One call of jpeggpu_ext_decode_batch, for the steps it is made of.
struct Call {
    const jpeggpu_ext_batch_item* items;
    int num_items;
    uint8_t* d_scratch; // ScanJob[n], FrontParams[nf], ProgImage[np], TruncRef[nt]
    hipStream_t stream;
    bool keep_flows        = false;
    uint32_t front_windows = 0; // most windows of a device-scanned item
    size_t jbytes = 0, fbytes = 0, pbytes = 0, tbytes = 0;
    int ring = 0; // the staging buffer and the `copied` event of the call
    hipStream_t part_stream[jpeggpu_batch::kMaxOverlap];
};

/// Order and group the items. One kernel variant per launch: the items are taken in the order of their subsequence size
/// (chosen per image at parse_header unless the caller fixed it), and every size is a group of launches of its own. Fills
/// the batch's jobs, front-end parameters, progressive descriptors and group_begin.
jpeggpu_status gather_jobs(jpeggpu_batch& b, Call& c)
{
    jg::ScanJob* d_jobs_rw = reinterpret_cast<jg::ScanJob*>(c.d_scratch);
    std::vector<int>& order = b.order;
    order.resize(static_cast<size_t>(c.num_items));
    for (int i = 0; i < c.num_items; ++i) order[static_cast<size_t>(i)] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return c.items[x].decoder->d.subseq_bytes > c.items[y].decoder->d.subseq_bytes; });
    std::vector<int>& group_begin = b.group_begin; // job index at which each size group starts, plus the end
    group_begin.clear();
    int subseq_bytes = 0;
    for (int k = 0; k < c.num_items; ++k) {
        const jpeggpu_ext_batch_item& it = c.items[order[static_cast<size_t>(k)]];
        if (it.decoder->d.subseq_bytes != subseq_bytes) {
            subseq_bytes = it.decoder->d.subseq_bytes;
            group_begin.push_back(static_cast<int>(b.jobs.size()));
        }
        const size_t first_job = b.jobs.size();
        const jpeggpu_status st = jg::build_jobs(it.decoder->d, it.img, it.d_tmp, it.tmp_size, b.sync_iters, false, c.keep_flows, b.jobs, !b.coefficients_only);
        if (st != JPEGGPU_SUCCESS) return st;
        if (const int dk = jg::device_scan_index(it.decoder->d); dk >= 0) {
            // device-side front end (jpeggpu_ext_set_device_scan): the counts of this job are filled in on the device
            b.fronts.push_back(jg::front_params(it.decoder->d, it.d_tmp, d_jobs_rw + first_job + static_cast<size_t>(dk), dk));
            c.front_windows = std::max(c.front_windows, b.fronts.back().num_windows);
        }
        if (const int tk = jg::truncated_scan_index(it.decoder->d); tk >= 0) {
            b.truncs.push_back(jg::TruncRef{d_jobs_rw + first_job + static_cast<size_t>(tk), jg::trunc_params(it.decoder->d, it.d_tmp)});
            b.trunc_job.push_back(static_cast<int>(first_job) + tk);
        }
        if (const Decoder& pd = it.decoder->d; pd.plan.prog.on) {
            b.progs.push_back(jg::ProgImage{static_cast<uint8_t*>(it.d_tmp), pd.plan.off_blob + pd.plan.prog.blob.header});
            jg::extend(b.prog_extent, *reinterpret_cast<const jg::ProgHeader*>(pd.blob + pd.plan.prog.blob.header));
        }
    }
    group_begin.push_back(static_cast<int>(b.jobs.size()));
    return JPEGGPU_SUCCESS;
}

/// Stage and copy the job array: into the next staging buffer of the ring, from there to d_scratch on the caller's stream,
/// where the device-side front end of the device-scanned items then completes their jobs.
jpeggpu_status stage_jobs(jpeggpu_batch& b, Call& c, size_t scratch_size)
{
    const size_t n = b.jobs.size(), nf = b.fronts.size(), np = b.progs.size(), nt = b.truncs.size();
    c.jbytes = sizeof(jg::ScanJob) * n, c.fbytes = sizeof(jg::FrontParams) * nf, c.pbytes = sizeof(jg::ProgImage) * np, c.tbytes = sizeof(jg::TruncRef) * nt;
    if (static_cast<int>(n) > b.max_jobs || scratch_size < c.jbytes + c.fbytes + c.pbytes + c.tbytes) return JPEGGPU_INVALID_ARGUMENT;
    const int r = c.ring = b.next;
    b.next      = (r + 1) % jpeggpu_batch::kRing;
    // the staging buffer may still be the source of a copy enqueued kRing batches ago
    if (b.in_use[r] && hipEventSynchronize(b.copied[r]) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    std::memcpy(b.staging[r], b.jobs.data(), c.jbytes);
    if (nf) std::memcpy(b.staging[r] + c.jbytes, b.fronts.data(), c.fbytes);
    if (np) std::memcpy(b.staging[r] + c.jbytes + c.fbytes, b.progs.data(), c.pbytes);
    if (nt) std::memcpy(b.staging[r] + c.jbytes + c.fbytes + c.pbytes, b.truncs.data(), c.tbytes);
    if (!b.timer.begin(c.stream, static_cast<size_t>(jg::kNumStages) + 1)) return JPEGGPU_INTERNAL_ERROR;
    if (hipMemcpyAsync(c.d_scratch, b.staging[r], c.jbytes + c.fbytes + c.pbytes + c.tbytes, hipMemcpyHostToDevice, c.stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    if (nf && jg::launch_front_batch(reinterpret_cast<const jg::FrontParams*>(c.d_scratch + c.jbytes), static_cast<int>(nf), c.front_windows, c.stream) != hipSuccess) {
        (void)hipGetLastError();
        return JPEGGPU_INTERNAL_ERROR;
    }
    // the staging buffer is free again, and the parts may start: the job array is complete
    if (hipEventRecord(b.copied[r], c.stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    b.in_use[r] = true;
    return JPEGGPU_SUCCESS;
}

/// Cut the parts of the job array: every size group into up to `overlap` contiguous parts of at least 4 jobs each, part w
/// of every group on stream w -- the caller's, or an internal one forked from it behind the copy.
jpeggpu_status cut_parts(jpeggpu_batch& b, Call& c)
{
    const int ways   = b.overlap;
    c.part_stream[0] = c.stream;
    for (int w = 1; w < ways; ++w) {
        if (!b.aux[w - 1]) {
            if (hipStreamCreateWithFlags(&b.aux[w - 1], hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&b.joined[w - 1], hipEventDisableTiming) != hipSuccess)
                return JPEGGPU_INTERNAL_ERROR;
        }
        c.part_stream[w] = b.aux[w - 1];
        if (hipStreamWaitEvent(c.part_stream[w], b.copied[c.ring], 0) != hipSuccess) return JPEGGPU_INTERNAL_ERROR; // fork
    }
    typedef jpeggpu_batch::Part Part;
    b.parts.clear();
    for (size_t g = 0; g + 1 < b.group_begin.size(); ++g) {
        const int lo = b.group_begin[g], hi = b.group_begin[g + 1];
        int gw = ways;
        while (gw > 1 && (hi - lo) / gw < 4) --gw;
        for (int w = 0; w < gw; ++w) {
            Part p{lo + static_cast<int>(static_cast<long long>(hi - lo) * w / gw), lo + static_cast<int>(static_cast<long long>(hi - lo) * (w + 1) / gw), w, jg::JobExtent{}};
            for (int j = p.begin; j < p.end; ++j) jg::extend(p.extent, b.jobs[static_cast<size_t>(j)]);
            p.extent.repack_flows = c.keep_flows;
            p.extent.fuse_tail_write = b.fuse_tail_write && !b.sync_iters_set;
            p.extent.sync_run = c.keep_flows || b.sync_iters_set ? 1 : b.sync_run;
            if (p.end > p.begin) b.parts.push_back(p);
        }
    }
    return JPEGGPU_SUCCESS;
}

/// The progressive items of the call, once for all of them: their coefficient buffers zeroed, one launch per level, the
/// hand-over; on the caller's stream, and the IDCT of the other streams' parts waits for it.
jpeggpu_status run_progressive(jpeggpu_batch& b, const Call& c)
{
    for (int k = 0; k < c.num_items; ++k) {
        const Decoder& pd = c.items[k].decoder->d;
        if (pd.plan.prog.on && hipMemsetAsync(static_cast<uint8_t*>(c.items[k].d_tmp) + pd.plan.prog.coef_begin, 0, pd.plan.prog.coef_bytes, c.stream) != hipSuccess)
            return JPEGGPU_INTERNAL_ERROR;
    }
    const jg::ProgImage* d_progs = reinterpret_cast<const jg::ProgImage*>(c.d_scratch + c.jbytes + c.fbytes);
    if (jg::launch_prog_batch(d_progs, static_cast<int>(b.progs.size()), b.prog_extent, c.stream) != hipSuccess) {
        (void)hipGetLastError();
        return JPEGGPU_INTERNAL_ERROR;
    }
    if (b.overlap > 1) {
        if (!b.prog_done && hipEventCreateWithFlags(&b.prog_done, hipEventDisableTiming) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
        if (hipEventRecord(b.prog_done, c.stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
        for (int w = 1; w < b.overlap; ++w)
            if (hipStreamWaitEvent(c.part_stream[w], b.prog_done, 0) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    }
    return JPEGGPU_SUCCESS;
}

/// Run the stages: each one for every part, then the join of the internal streams.
jpeggpu_status run_stages(jpeggpu_batch& b, const Call& c)
{
    const jg::ScanJob* d_jobs = reinterpret_cast<const jg::ScanJob*>(c.d_scratch);
    for (int stage = 0; stage < jg::kNumStages; ++stage) {
        const bool skip = stage == jg::kStageIdct && b.coefficients_only; // a coefficients-only call has no IDCT stage, wherever it stands
        if (stage == jg::kStageWrite && !b.progs.empty()) {
            const jpeggpu_status st = run_progressive(b, c);
            if (st != JPEGGPU_SUCCESS) return st;
        }
        for (const jpeggpu_batch::Part& p : b.parts) {
            if (skip) break; // (the stage's mark below is kept: the timer counts kNumStages + 1 events per call)
            if (jg::launch_stage_batch(static_cast<jg::Stage>(stage), d_jobs + p.begin, p.end - p.begin, p.extent, c.part_stream[p.way]) != hipSuccess) {
                (void)hipGetLastError();
                return JPEGGPU_INTERNAL_ERROR;
            }
            if ((stage == jg::kStageDestuff || stage == jg::kStageWrite) && !b.truncs.empty()) {
                // the part's scans whose file ended early (jg_trunc.hpp): a run of the references, which are in job order
                const auto lo = std::lower_bound(b.trunc_job.begin(), b.trunc_job.end(), p.begin) - b.trunc_job.begin();
                const auto hi = std::lower_bound(b.trunc_job.begin(), b.trunc_job.end(), p.end) - b.trunc_job.begin();
                const jg::TruncRef* d_refs = reinterpret_cast<const jg::TruncRef*>(c.d_scratch + c.jbytes + c.fbytes + c.pbytes) + lo;
                if (hi > lo && (stage == jg::kStageDestuff ? jg::launch_trunc_prepare_batch(d_refs, static_cast<int>(hi - lo), c.part_stream[p.way])
                                                           : jg::launch_trunc_finish_batch(d_refs, static_cast<int>(hi - lo), c.part_stream[p.way])) != hipSuccess) {
                    (void)hipGetLastError();
                    return JPEGGPU_INTERNAL_ERROR;
                }
            }
        }
        (void)b.timer.mark(stage, c.stream); // stage times are those of the caller's stream
    }
    for (int w = 1; w < b.overlap; ++w) { // join: the caller's stream completes when every part has
        if (hipEventRecord(b.joined[w - 1], c.part_stream[w]) != hipSuccess ||
            hipStreamWaitEvent(c.stream, b.joined[w - 1], 0) != hipSuccess)
            return JPEGGPU_INTERNAL_ERROR;
    }
    return JPEGGPU_SUCCESS;
}

jpeggpu_status decode_batch_impl(
    jpeggpu_batch_t batch, const jpeggpu_ext_batch_item* items, int num_items, void* d_scratch, size_t scratch_size, jpeggpu_stream_t stream)
{
    if (!batch || !items || num_items < 0 || !d_scratch) return JPEGGPU_INVALID_ARGUMENT;
    if (num_items == 0) return JPEGGPU_SUCCESS;
    batch->jobs.clear();
    batch->fronts.clear();
    batch->progs.clear();
    batch->truncs.clear();
    batch->trunc_job.clear();
    batch->prog_extent = jg::ProgExtent{};
    for (int i = 0; i < num_items; ++i)
        if (!items[i].decoder || !items[i].img) return JPEGGPU_INVALID_ARGUMENT;
    // A call of one or two images planned as lone decodes (jpeggpu_ext_set_batch_hint): decoded one by one with the lone
    // decode's kernels, multi-hypothesis speculation included -- the chip is empty either way.
    {
        // (with the batch's stage timing on, the call takes the batch's kernels: its events sit between THOSE launches)
        bool all_lone = num_items <= jg::kLonePlanImages && !batch->timer.enabled() && !batch->coefficients_only;
        for (int i = 0; i < num_items && all_lone; ++i) all_lone = !items[i].decoder->d.batched;
        if (all_lone) {
            for (int i = 0; i < num_items; ++i) {
                const jpeggpu_status st = jg::do_decode(items[i].decoder->d, items[i].img, items[i].d_tmp, items[i].tmp_size, stream, false);
                if (st != JPEGGPU_SUCCESS) return st;
            }
            return JPEGGPU_SUCCESS;
        }
    }
    Call c{items, num_items, static_cast<uint8_t*>(d_scratch), stream};
    // Does the call fill the chip? A launch of fewer than kKeepFlowsBelowSubseq subsequences does not: its sequence kernel
    // keeps every flow in the workgroup (the lone decode's kernel, one job per blockIdx.y) and the tail kernel has only
    // the sequence boundaries to look at; a full batch runs one flow iteration there and leaves the rest to the tail kernel,
    // whose latency other launches hide.
    {
        long long total_subseq = 0;
        for (int i = 0; i < num_items; ++i) {
            const jg::Stream& s = items[i].decoder->d.reader.s;
            if (!items[i].decoder->d.parsed) return JPEGGPU_INVALID_ARGUMENT;
            for (int k = 0; k < s.num_scans; ++k) total_subseq += s.scans[k].num_subseq;
        }
        c.keep_flows = batch->sync_iters_set ? false : total_subseq < batch->keep_flows_below;
    }
    jpeggpu_status st = gather_jobs(*batch, c);
    if (st == JPEGGPU_SUCCESS) st = stage_jobs(*batch, c, scratch_size);
    if (st == JPEGGPU_SUCCESS) st = cut_parts(*batch, c);
    if (st == JPEGGPU_SUCCESS) st = run_stages(*batch, c);
    return st;
}

} // namespace

extern "C" {

size_t jpeggpu_ext_batch_scratch_size(int max_scans)
{
    // (a progressive item's descriptor lies behind the jobs and front-end parameters; such an item has a job per component
    // and no front-end parameters, so the same bound holds)
    static_assert(sizeof(jg::ProgImage) <= sizeof(jg::FrontParams), "a progressive item takes the place of front-end parameters");
    // (so does the one scan a truncated item ends in: such a scan is walked on the host)
    static_assert(sizeof(jg::TruncRef) <= sizeof(jg::FrontParams), "a truncated item's scan takes the place of front-end parameters");
    return static_cast<size_t>(max_scans > 0 ? max_scans : 0) * (sizeof(jg::ScanJob) + sizeof(jg::FrontParams));
}

enum jpeggpu_status jpeggpu_ext_batch_create(jpeggpu_batch_t* batch, int max_scans)
{
    if (!batch || max_scans <= 0) return JPEGGPU_INVALID_ARGUMENT;
    jpeggpu_batch* b = new (std::nothrow) jpeggpu_batch();
    if (!b) return JPEGGPU_OUT_OF_HOST_MEMORY;
    b->max_jobs = max_scans;
    if (const char* e = std::getenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW")) b->keep_flows_below = std::atoll(e); // experiments (tools/probe/batch_curve.py)
    if (const char* e = std::getenv("JPEGGPU_FUSE_TAIL_WRITE")) b->fuse_tail_write = std::atoi(e) != 0;
    if (const char* e = std::getenv("JPEGGPU_SYNC_RUN")) {
        const int r = std::atoi(e);
        if (r == 1 || r == 2 || r == 4) b->sync_run = r; // (anything else: the default)
    }
    for (int r = 0; r < jpeggpu_batch::kRing; ++r) {
        void* p = nullptr;
        if (hipHostMalloc(&p, jpeggpu_ext_batch_scratch_size(max_scans), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&b->copied[r], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            jpeggpu_ext_batch_destroy(b);
            return JPEGGPU_INTERNAL_ERROR; // the batch path needs a device: no fallback
        }
        b->staging[r] = static_cast<uint8_t*>(p);
    }
    *batch = b;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_batch_destroy(jpeggpu_batch_t batch)
{
    if (!batch) return JPEGGPU_INVALID_ARGUMENT;
    for (int w = 0; w < jpeggpu_batch::kMaxOverlap - 1; ++w) {
        if (batch->aux[w]) {
            (void)hipStreamSynchronize(batch->aux[w]);
            (void)hipStreamDestroy(batch->aux[w]);
        }
        if (batch->joined[w]) (void)hipEventDestroy(batch->joined[w]);
    }
    for (int r = 0; r < jpeggpu_batch::kRing; ++r) {
        if (batch->staging[r]) (void)hipHostFree(batch->staging[r]);
        if (batch->copied[r]) (void)hipEventDestroy(batch->copied[r]);
    }
    if (batch->prog_done) (void)hipEventDestroy(batch->prog_done);
    delete batch;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_decode_batch(
    jpeggpu_batch_t batch,
    const struct jpeggpu_ext_batch_item* items,
    int num_items,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream)
{
    try { // the scratch vectors of the batch grow with its first calls: no exception crosses the C ABI
        return decode_batch_impl(batch, items, num_items, d_scratch, scratch_size, stream);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
}

enum jpeggpu_status jpeggpu_ext_batch_set_overlap(jpeggpu_batch_t batch, int parts)
{
    if (!batch || parts < 1 || parts > jpeggpu_batch::kMaxOverlap) return JPEGGPU_INVALID_ARGUMENT;
    batch->overlap = parts;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_batch_set_fused_tail(jpeggpu_batch_t batch, int enable)
{
    if (!batch) return JPEGGPU_INVALID_ARGUMENT;
    batch->fuse_tail_write = enable != 0;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_fused_tail_timeouts(unsigned int* count)
{
    if (!count) return JPEGGPU_INVALID_ARGUMENT;
    return jg::read_fuse_timeouts(count) == hipSuccess ? JPEGGPU_SUCCESS : JPEGGPU_INTERNAL_ERROR;
}

enum jpeggpu_status jpeggpu_ext_batch_set_sync_iterations(jpeggpu_batch_t batch, int iterations)
{
    if (!batch || iterations < 1) return JPEGGPU_INVALID_ARGUMENT; // the first flow iteration supplies n and the DC sums
    batch->sync_iters     = iterations;
    batch->sync_iters_set = true;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_batch_set_coefficients_only(jpeggpu_batch_t batch, int enable)
{
    if (!batch) return JPEGGPU_INVALID_ARGUMENT;
    batch->coefficients_only = enable != 0;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_batch_set_sync_run(jpeggpu_batch_t batch, int r)
{
    if (!batch || (r != 1 && r != 2 && r != 4)) return JPEGGPU_INVALID_ARGUMENT;
    batch->sync_run = r;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_batch_set_profiling(jpeggpu_batch_t batch, int enable)
{
    if (!batch) return JPEGGPU_INVALID_ARGUMENT;
    batch->timer.enable(enable != 0);
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_batch_get_stage_ms(jpeggpu_batch_t batch, float* ms)
{
    if (!batch || !ms) return JPEGGPU_INVALID_ARGUMENT;
    return batch->timer.mean_ms(ms);
}

} // extern "C"
