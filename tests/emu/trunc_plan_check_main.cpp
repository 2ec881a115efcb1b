// trunc_plan_check_main.cpp -- the host side of truncated decoding (jpeggpu_ext_set_truncated) under AddressSanitizer + UBSan,
// without a device: jg_reader.cpp's walk of a file that ends early and jg_plan.cpp's plan of it. Built by
// tests/test_truncated_host.py from this file, jg_reader.cpp and jg_plan.cpp alone.
//
//   trunc_plan_check_main file.jpg [file.jpg ...]
//
// Every file is cut at every length from the end of its first SOS header to its whole length; each prefix is copied into a
// heap buffer of exactly that length (a read past the cut is a sanitizer report) and planned with the flag set, as a lone
// and as a batched image, without and with a crop. Then
//   * the blob is filled into a heap buffer of exactly plan.blob_size bytes;
//   * the segment table is contiguous and adds up to the scan's subsequences; every chunk lies inside the transferred bytes,
//     and what it writes, zero padding included, inside its segment's subsequences;
//   * the truncation parameters name segments of the table; the cut segment keeps Scan::trunc_tail_bytes of zeros behind its
//     data, the all-zero segment is that long; the state words lie at a carved region of d_tmp;
//   * the whole file gives no truncation at all, and the plan it gives without the flag.
// Prints what it checked; the exit status is the number of the check that failed.
#include "jg_decoder.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

const char* g_file = "";
size_t g_cut       = 0;

[[noreturn]] void fail(int code, const char* what)
{
    std::fprintf(stderr, "truncated plan check: %s cut at %zu: %s\n", g_file, g_cut, what);
    std::exit(code);
}

uint8_t* const kBase = reinterpret_cast<uint8_t*>(uintptr_t{0x7000} << 24); // never dereferenced

size_t scan_begin(const std::vector<uint8_t>& f)
{
    size_t i = 2;
    while (i + 4 <= f.size()) {
        const uint8_t m  = f[i + 1];
        const size_t len = static_cast<size_t>(f[i + 2]) << 8 | f[i + 3];
        i += 2 + len;
        if (m == 0xDA) return i;
    }
    fail(3, "no SOS");
}

struct Counts {
    long plans = 0, cut_scans = 0, zero_segments = 0, no_data = 0;
};

void check_one(jg::Decoder& d, const uint8_t* data, size_t size, bool whole, Counts& n)
{
    jg::PlanTrace trace;
    jpeggpu_img_info info;
    if (d.plan_image(&info, data, size, &trace) != JPEGGPU_SUCCESS) fail(10, "a file cut behind its first SOS header is refused");
    const jg::Plan& plan = d.plan;
    const jg::Stream& s  = d.reader.s;
    uint8_t* blob        = static_cast<uint8_t*>(std::malloc(plan.blob_size));
    if (!blob) fail(2, "out of memory");
    d.fill_blob(blob);
    d.blob   = blob;
    d.parsed = true;
    ++n.plans;
    const size_t B = static_cast<size_t>(d.subseq_bytes);
    for (int i = 0; i < s.num_scans; ++i) {
        const jg::Scan& sc = s.scans[i];
        int at             = 0;
        for (const jg::Segment& g : sc.segments) {
            if (g.subseq_offset != at || g.subseq_count <= 0) fail(20, "the segment table is not contiguous");
            at += g.subseq_count;
        }
        if (at != sc.num_subseq) fail(21, "the segments do not add up to the scan's subsequences");
        for (const jg::DestuffChunk& c : sc.chunks) {
            if (c.begin > c.end || c.end > plan.bytes_len || c.begin < c.win_off || c.end > c.win_off + jg::kDestuffWin) fail(22, "a chunk leaves the transferred bytes or its window");
            if (c.seg < 0 || static_cast<size_t>(c.seg) >= sc.segments.size()) fail(23, "a chunk names no segment");
            const jg::Segment& g = sc.segments[static_cast<size_t>(c.seg)];
            const size_t lo = static_cast<size_t>(g.subseq_offset) * B, hi = lo + static_cast<size_t>(g.subseq_count) * B;
            // (what a chunk writes: its bytes that are not FF -- the zero of a stuffed pair stands for the FF in front of it)
            size_t written = 0;
            for (uint32_t b = c.begin; b < c.end; ++b) written += data[s.xfer_begin + b] != 0xFF;
            if (c.dst_off < lo || c.dst_off + written > hi || (c.pad_end && (c.pad_end < c.dst_off + written || c.pad_end > hi))) fail(24, "a chunk writes outside its segment");
        }
    }
    const jg::Stream::Truncation& t = s.trunc;
    if (whole) {
        if (t.no_eoi || t.scan >= 0) fail(30, "the whole file counts as truncated");
    } else {
        if (!t.no_eoi) fail(31, "a cut file does not count as truncated");
        if (t.scan >= 0) {
            ++n.cut_scans;
            const jg::Scan& sc = s.scans[t.scan];
            const size_t tail  = static_cast<size_t>(sc.trunc_tail_bytes);
            if (sc.trunc_tail_bytes < 16 || sc.trunc_tail_bytes > jg::truncation_tail_bytes(sc.du_per_mcu)) fail(39, "the tail of zeros is not what the tables ask for");
            if (t.cut_segment < 0 || static_cast<size_t>(t.cut_segment) >= sc.segments.size()) fail(32, "the cut segment is not in the table");
            const jg::Segment& g = sc.segments[static_cast<size_t>(t.cut_segment)];
            if (t.end_bit % 8 || t.end_bit / 8 + tail > static_cast<size_t>(g.subseq_count) * B) fail(33, "the cut segment lacks its zeros");
            if (t.end_bit == 0) ++n.no_data;
            if (t.zero_segment >= 0) {
                ++n.zero_segments;
                if (t.zero_segment != t.cut_segment + 1 || static_cast<size_t>(t.zero_segment) >= sc.segments.size()) fail(34, "the all-zero segment is not the next one");
                if (tail > static_cast<size_t>(sc.segments[static_cast<size_t>(t.zero_segment)].subseq_count) * B) fail(35, "the all-zero segment is too short");
            }
            if (static_cast<size_t>(sc.segments.size()) > static_cast<size_t>((sc.mcus_x * sc.mcus_y + sc.mcus_per_segment - 1) / sc.mcus_per_segment))
                fail(36, "more segments than restart intervals");
            const jg::TruncParams tp = jg::trunc_params(d, kBase);
            bool carved              = false;
            for (const auto& r : trace.tmp) carved = carved || (kBase + r.offset == reinterpret_cast<uint8_t*>(tp.state) && r.bytes >= 8);
            if (!carved || tp.cut_segment != t.cut_segment || tp.end_bit != t.end_bit || tp.zero_segment != t.zero_segment) fail(37, "the kernels' parameters are not the walk's");
            if (t.scan_bytes != size - sc.begin) fail(38, "scan_bytes is not what the file holds of the scan");
        }
    }
    jpeggpu_img img{};
    for (int c = 0; c < s.num_comp; ++c) img.image[c] = kBase, img.pitch[c] = d.plane_x(c);
    std::vector<jg::ScanJob> jobs;
    if ((d.batched ? jg::build_jobs(d, &img, kBase, plan.total, 1, false, false, jobs) : jg::build_jobs(d, &img, kBase, plan.total, jg::kSeqLanes, true, true, jobs)) != JPEGGPU_SUCCESS)
        fail(40, "build_jobs refuses its own plan");
    for (const jg::ScanJob& j : jobs)
        if (j.ip.num_du <= 0 || j.sp.num_segments <= 0) fail(41, "a job without data units or segments");
    std::free(blob);
    d.blob = nullptr;
}

} // namespace

int main(int argc, char** argv)
{
    Counts n;
    int files = 0;
    for (int i = 1; i < argc; ++i) {
        g_file  = argv[i];
        FILE* f = std::fopen(argv[i], "rb");
        if (!f) return 2;
        std::fseek(f, 0, SEEK_END);
        const long len = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        std::vector<uint8_t> file(static_cast<size_t>(len));
        if (std::fread(file.data(), 1, file.size(), f) != file.size()) return 2;
        std::fclose(f);
        ++files;
        for (g_cut = scan_begin(file); g_cut <= file.size(); ++g_cut) {
            uint8_t* prefix = static_cast<uint8_t*>(std::malloc(g_cut)); // exactly: one byte too far is a report
            if (!prefix) return 2;
            std::memcpy(prefix, file.data(), g_cut);
            for (int setting = 0; setting < 4; ++setting) {
                jg::Decoder d;
                d.truncated  = true;
                d.batch_hint = setting & 1 ? jg::kBatchHintFull : 0;
                d.batched    = !jg::lone_plan(d.batch_hint);
                if (setting & 2) d.crop_request[0] = d.crop_request[1] = 1, d.crop_request[2] = d.crop_request[3] = 3;
                check_one(d, prefix, g_cut, g_cut == file.size(), n);
            }
            std::free(prefix);
        }
        { // the whole file plans the same with and without the flag
            jg::Decoder a, b;
            b.truncated = true;
            jpeggpu_img_info ia, ib;
            if (a.plan_image(&ia, file.data(), file.size()) != JPEGGPU_SUCCESS || b.plan_image(&ib, file.data(), file.size()) != JPEGGPU_SUCCESS) fail(50, "the whole file is refused");
            if (a.plan.total != b.plan.total || a.plan.blob_size != b.plan.blob_size || a.reader.s.scans[0].num_subseq != b.reader.s.scans[0].num_subseq)
                fail(51, "the flag changes the plan of a whole file");
        }
    }
    std::printf("truncated plan check: %d files, %ld plans, %ld cut scans, %ld with an all-zero segment, %ld without data\n", files, n.plans, n.cut_scans,
                n.zero_segments, n.no_data);
    return 0;
}
