// plan_check_main.cpp -- the plan of jg_plan.cpp under AddressSanitizer + UBSan, without a device: where sizes read from a
// file become device addresses. Built by tests/test_plan_host.py from this file, jg_reader.cpp and jg_plan.cpp alone.
//
//   plan_check_main file.jpg [file.jpg ...] [--progressive file.jpg ...]
//
// Every file is planned under every setting below (files behind --progressive with progressive reading on), the way
// jpeggpu_decoder_parse_header does it (Decoder::plan_image); a setting the parse refuses for a file is skipped. Then
//   * the blob is filled into a heap buffer of exactly plan.blob_size bytes: an overrun is a sanitizer report;
//   * region bounds: every region make_plan carved (PlanTrace) starts 256-byte aligned, lies inside the blob / inside
//     [0, plan.total), and ends in front of the next one;
//   * pointer bounds: the jobs (and the front-end parameters of a device-walked scan) are built against a fake base; every
//     pointer of theirs lies in [base, base + plan.total) and, but for `bytes`, at the start of a carved region; the plane
//     pointers are the image's;
//   * determinism: building the jobs twice gives the same bytes.
// Prints what it checked; the exit status is the number of the check that failed (see fail()).
#include "jg_decoder.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

namespace {

const char* g_file = "";
int g_setting      = 0;

[[noreturn]] void fail(int code, const char* what)
{
    std::fprintf(stderr, "plan check: %s, setting %d: %s\n", g_file, g_setting, what);
    std::exit(code);
}

uint8_t* const kBase   = reinterpret_cast<uint8_t*>(uintptr_t{0x7000} << 24); // never dereferenced
uint8_t* const kPlanes = reinterpret_cast<uint8_t*>(uintptr_t{0x3000} << 24);

void check_regions(const std::vector<jg::PlanTrace::Region>& r, size_t total)
{
    for (size_t i = 0; i < r.size(); ++i) {
        if (r[i].offset % 256) fail(10, "a region does not start 256-byte aligned");
        if (r[i].offset > total || r[i].bytes > total - r[i].offset) fail(11, "a region does not lie inside its buffer");
        if (i + 1 < r.size() && r[i].offset + r[i].bytes > r[i + 1].offset) fail(12, "two regions overlap");
    }
}

struct Pointers {
    const jg::Plan& plan;
    std::set<uintptr_t> starts; // of the carved regions
    void check(const void* p, bool at_start = true) const
    {
        if (!p) return;
        const uintptr_t v = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(kBase);
        if (v < b || v >= b + plan.total) fail(20, "a pointer lies outside d_tmp");
        if (at_start && !starts.count(v)) fail(21, "a pointer does not point at a carved region");
    }
};

void check_job(const Pointers& P, const jg::ScanJob& j)
{
    P.check(j.bytes, false); // (a device-walked scan's start inside the transferred bytes)
    const void* const all[] = {j.chunks,  j.segments,  j.tables,     j.tables_sync, j.qtables,    j.destuffed, j.seg_idx,     j.st_p,
                               j.st_n,    j.st_cz,     j.st_dc01,    j.st_dc23,     j.pending,    j.flow_list, j.tail_parts,  j.fuse_ctl,
                               j.tails_n, j.tails_dc01, j.tails_dc23, j.mh_p,        j.mh_cz,      j.mh_link,   j.mh_pool,     j.mh_known,
                               j.mh_blocks, j.mh_blk_exit, j.mh_blk_entry, j.sym,    j.du_tab,     j.bnd_p,     j.bnd_cz};
    for (const void* p : all) P.check(p);
}

void check_front(const Pointers& P, const jg::FrontParams& f)
{
    P.check(f.bytes, false);
    const void* const all[] = {f.win_data, f.win_nmark, f.win_bad, f.win_prefix, f.mark_off, f.mk_pos,    f.mk_g,
                               f.seg_cnt,  f.seg_nch,   f.segments, f.chunks,    f.tail_parts, f.mh_blocks, f.job, f.status};
    for (const void* p : all) P.check(p);
}

struct Counts {
    int checked = 0, skipped = 0, mh = 0, mh_blocks = 0, device_walked = 0, progressive = 0;
};

/// One (file, setting) pair; false if the parse refuses it.
bool check_one(jg::Decoder& d, const std::vector<uint8_t>& file, Counts& n)
{
    jg::PlanTrace trace;
    jpeggpu_img_info info;
    if (d.plan_image(&info, file.data(), file.size(), &trace) != JPEGGPU_SUCCESS) return false;
    const jg::Plan& plan = d.plan;
    const jg::Stream& s  = d.reader.s;
    uint8_t* blob        = static_cast<uint8_t*>(std::malloc(plan.blob_size)); // exactly: one byte too far is a report
    if (!blob) fail(2, "out of memory");
    d.fill_blob(blob);
    d.blob   = blob;
    d.parsed = true;

    check_regions(trace.blob, plan.blob_size);
    check_regions(trace.tmp, plan.total);
    if (trace.tmp.size() < 2 || trace.tmp[1].offset != plan.off_blob || trace.tmp[1].bytes != plan.blob_size) fail(13, "the blob is not the second region of d_tmp");
    Pointers P{plan, {}};
    for (const auto& r : trace.tmp) P.starts.insert(reinterpret_cast<uintptr_t>(kBase + r.offset));
    for (const auto& r : trace.blob) P.starts.insert(reinterpret_cast<uintptr_t>(kBase + plan.off_blob + r.offset));

    jpeggpu_img img{};
    for (int c = 0; c < s.num_comp; ++c) img.image[c] = kPlanes + (static_cast<size_t>(c) << 20), img.pitch[c] = d.plane_x(c);
    std::vector<jg::ScanJob> jobs[2];
    for (std::vector<jg::ScanJob>& j : jobs) { // as a lone decode builds them, or a full batch
        const jpeggpu_status st = d.batched ? jg::build_jobs(d, &img, kBase, plan.total, 1, false, false, j)
                                            : jg::build_jobs(d, &img, kBase, plan.total, jg::kSeqLanes, true, true, j);
        if (st != JPEGGPU_SUCCESS) fail(22, "build_jobs refuses its own plan");
    }
    if (jobs[0].size() != static_cast<size_t>(s.num_scans) || jobs[1].size() != jobs[0].size()) fail(23, "not one job per scan");
    if (std::memcmp(jobs[0].data(), jobs[1].data(), jobs[0].size() * sizeof(jg::ScanJob)) != 0) fail(30, "the jobs differ between two builds");
    bool mh = false, mh_blocks = false;
    for (int i = 0; i < s.num_scans; ++i) {
        check_job(P, jobs[0][static_cast<size_t>(i)]);
        for (int a = 0; a < s.scans[i].num_comp; ++a)
            if (jobs[0][static_cast<size_t>(i)].ip.plane[a] != img.image[s.scans[i].comp[a].comp_idx]) fail(24, "a plane pointer is not the image's");
        mh        = mh || plan.scan[i].mh > 1;
        mh_blocks = mh_blocks || !plan.scan[i].mh_blocks.empty();
    }
    n.mh += mh, n.mh_blocks += mh_blocks;
    if (const int k = jg::device_scan_index(d); k >= 0) {
        jg::ScanJob* d_job = reinterpret_cast<jg::ScanJob*>(kBase + plan.scan[k].d_job);
        check_front(P, jg::front_params(d, kBase, d_job, k));
        ++n.device_walked;
    }
    n.progressive += plan.prog.on;
    std::free(blob);
    d.blob = nullptr;
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    Counts n;
    int files = 0;
    bool progressive = false;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "--progressive") == 0) {
            progressive = true;
            continue;
        }
        g_file  = argv[i];
        FILE* f = std::fopen(argv[i], "rb");
        if (!f) return 2;
        std::fseek(f, 0, SEEK_END);
        const long len = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        std::vector<uint8_t> file(static_cast<size_t>(len)); // an exact-size heap copy
        if (std::fread(file.data(), 1, file.size(), f) != file.size()) return 2;
        std::fclose(f);
        ++files;
        g_setting = 0;
        // scale 1 and 8 x both scale modes x {no crop, (1, 1, 3, 3), the whole image, no crop and shard 1 of 2} x device
        // scan off / on x batched off / on, set the way the setters of jpeggpu_ext.h set them
        for (int scale_log2 = 0; scale_log2 <= 3; scale_log2 += 3)
            for (int mode = JPEGGPU_EXT_SCALE_UNIFORM; mode <= JPEGGPU_EXT_SCALE_LIBJPEG; ++mode)
                for (int window = 0; window < 4; ++window)
                    for (int device_scan = 0; device_scan < 2; ++device_scan)
                        for (int batched = 0; batched < 2; ++batched, ++g_setting) {
                            jg::Decoder d;
                            d.progressive        = progressive;
                            d.scale_log2_request = scale_log2;
                            d.scale_mode_request = mode;
                            d.device_scan        = device_scan;
                            d.batch_hint         = batched ? jg::kBatchHintFull : 0;
                            d.batched            = !jg::lone_plan(d.batch_hint);
                            if (window == 3) d.shard_rank = 1, d.shard_world = 2;
                            if (window == 1) d.crop_request[0] = d.crop_request[1] = 1, d.crop_request[2] = d.crop_request[3] = 3;
                            if (window == 2) { // the size at the scale is known after a parse
                                jpeggpu_img_info info;
                                if (d.plan_image(&info, file.data(), file.size()) != JPEGGPU_SUCCESS) {
                                    ++n.skipped;
                                    continue;
                                }
                                d.crop_request[2] = d.scaled(d.reader.s.size_x), d.crop_request[3] = d.scaled(d.reader.s.size_y);
                            }
                            if (check_one(d, file, n)) ++n.checked;
                            else ++n.skipped;
                        }
    }
    std::printf("plan check: %d files, %d pairs checked, %d skipped, %d plans with mh > 1, %d with mh_blocks, %d device-walked, %d progressive\n",
                files, n.checked, n.skipped, n.mh, n.mh_blocks, n.device_walked, n.progressive);
    return 0;
}
