// jg_plan.cpp -- from a parsed image to device addresses, on the host alone: the geometry of the image at its scale and
// crop, the plan (where every buffer lies in d_tmp and in the table blob), the blob's content, and the ScanJob /
// FrontParams that bind the plan's offsets to a caller's d_tmp.
//
// This is where sizes read from an untrusted file become device addresses, so nothing here needs the HIP runtime: the
// file compiles with a plain C++ compiler and is checked under ASan and UBSan in a stand-alone program
// (tests/emu/plan_check_main.cpp). Counterpart of the reference's src/decoder.cpp:116-155; one `plan` carves d_tmp for
// get_buffer_size / transfer / decode alike (the reference replays decode_impl<false>, decoder.cpp:327-334).
//
// A buffer is added in two places: its size in make_plan's carve, its pointer in build_jobs or front_params.
#include "jg_decoder.hpp"

#include <algorithm>
#include <cstring>
#include <new>

namespace jg {

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/// Hands out a buffer piece by piece: operator() takes a byte count and returns the piece's offset; every piece starts
/// 256-byte aligned.
struct Carve {
    size_t at = 0;
    std::vector<PlanTrace::Region>* trace = nullptr;
    size_t operator()(size_t bytes)
    {
        const size_t o = at;
        at += align_up(bytes, 256);
        if (trace) trace->push_back({o, bytes});
        return o;
    }
};

/// The plan's offset `off` behind `base`, as a pointer to T.
template <typename T>
T* at(uint8_t* base, size_t off)
{
    return reinterpret_cast<T*>(base + off);
}

} // namespace

/// Each component's block size for the parsed image. JPEGGPU_EXT_SCALE_LIBJPEG at a scale below 1: jdmaster.c's rule -- from
/// S_min = 8 / d, a component's size doubles while it stays below 8 and the doubled block still divides what the largest
/// sampling factors span, in both directions. Where that leaves every component at S_min (4:4:4, grey, 4:2:2 and the like)
/// the image is decoded as in JPEGGPU_EXT_SCALE_UNIFORM mode: the planes are the same.
void Decoder::set_block_sizes()
{
    const Stream& s = reader.s;
    const int mn    = 8 >> scale_log2;
    draft           = false;
    for (int c = 0; c < s.num_comp; ++c) {
        int size = mn;
        if (scale_mode == JPEGGPU_EXT_SCALE_LIBJPEG)
            while (size < 8 && (s.hs_max * mn) % (s.comp[c].hs * size * 2) == 0 && (s.vs_max * mn) % (s.comp[c].vs * size * 2) == 0) size *= 2;
        blk_lg[c] = size == 8 ? 0 : size == 4 ? 1 : size == 2 ? 2 : 3;
        if (size != mn) draft = true;
    }
}

/// The windows of a crop (jpeggpu_ext.h, jpeggpu_ext_set_crop) from the request and the parsed frame; false if the
/// rectangle does not lie inside the image at the scale.
bool Decoder::set_crop_window()
{
    const Stream& s = reader.s;
    Crop c;
    c.on = true;
    c.x = crop_request[0], c.y = crop_request[1], c.w = crop_request[2], c.h = crop_request[3];
    if (c.x + static_cast<long long>(c.w) > scaled(s.size_x) || c.y + static_cast<long long>(c.h) > scaled(s.size_y)) return false;
    int lo_x[kMaxComp], hi_x[kMaxComp], lo_y[kMaxComp], hi_y[kMaxComp];
    c.mx0 = c.my0 = 1 << 30;
    for (int k = 0; k < s.num_comp; ++k) {
        const Component& fc = s.comp[k];
        // samples per block side at the scale (draft mode: the component's own), and the sampling factors its plane has
        // there (eff_hs: what is left of h_max / h_c once the IDCT has done its part)
        const int n = blk(k), hs = eff_hs(k), vs = eff_vs(k);
        // samples of the rectangle, plus the one-sample halo of the upsamplers, clipped to the plane
        lo_x[k] = std::max(static_cast<int>(static_cast<long long>(c.x) * hs / s.hs_max) - 1, 0);
        hi_x[k] = std::min(static_cast<int>(static_cast<long long>(c.x + c.w - 1) * hs / s.hs_max) + 1, full_x(k) - 1);
        lo_y[k] = std::max(static_cast<int>(static_cast<long long>(c.y) * vs / s.vs_max) - 1, 0);
        hi_y[k] = std::min(static_cast<int>(static_cast<long long>(c.y + c.h - 1) * vs / s.vs_max) + 1, full_y(k) - 1);
        c.mx0 = std::min(c.mx0, lo_x[k] / (n * fc.hs)), c.mx1 = std::max(c.mx1, hi_x[k] / (n * fc.hs) + 1);
        c.my0 = std::min(c.my0, lo_y[k] / (n * fc.vs)), c.my1 = std::max(c.my1, hi_y[k] / (n * fc.vs) + 1);
    }
    for (int k = 0; k < s.num_comp; ++k) {
        const Component& fc = s.comp[k];
        const int n = blk(k);
        c.ox[k] = c.mx0 * n * fc.hs, c.oy[k] = c.my0 * n * fc.vs;
        c.wx[k] = hi_x[k] + 1 - c.ox[k], c.wy[k] = hi_y[k] + 1 - c.oy[k];
    }
    crop = c;
    return true;
}

/// The IDCT window of one scan of a cropped image (IdctWindow): the frame's MCU window for an interleaved scan, the block
/// window that holds the component's window for a non-interleaved one. Zero without a crop.
IdctWindow Decoder::scan_window(const Scan& sc) const
{
    IdctWindow w{};
    if (!crop.on) return w;
    if (sc.num_comp > 1) {
        w.mx0 = crop.mx0, w.my0 = crop.my0, w.mcus_x = crop.mx1 - crop.mx0, w.mcus_y = crop.my1 - crop.my0;
    } else {
        const int c = sc.comp[0].comp_idx, n = blk(c);
        w.mx0 = crop.ox[c] / n, w.my0 = crop.oy[c] / n;
        w.mcus_x = (crop.ox[c] + crop.wx[c] + n - 1) / n - w.mx0, w.mcus_y = (crop.oy[c] + crop.wy[c] + n - 1) / n - w.my0;
    }
    const MagicDiv m = magic_div(static_cast<uint32_t>(w.mcus_x));
    w.mcus_x_mul = m.mul, w.mcus_x_shift = m.shift;
    return w;
}

void Decoder::make_plan(PlanTrace* trace)
{
    const Stream& s = reader.s;
    Plan p;
    // table blob
    Carve blob{0, trace ? &trace->blob : nullptr};
    p.blob_qtables = blob(sizeof(s.qtable));
    for (int i = 0; i < s.num_scans; ++i) {
        const Scan& sc      = s.scans[i];
        ScanPlan& sp        = p.scan[i];
        sp.blob_tables      = blob(sc.table_pack.size());
        sp.blob_tables_sync = blob(sc.table_pack_sync.size());
        sp.blob_segments    = blob(sc.segments.size() * sizeof(Segment));
        sp.blob_chunks      = blob(sc.chunks.size() * sizeof(DestuffChunk));
        sp.blob_parts       = blob(sc.tail_parts.size() * sizeof(int));
        // Multi-hypothesis speculation (jg_defs.h) for an image decoded on its own: several data units per MCU. Segments
        // the chain walk can hold in LDS are walked whole; longer ones (a scan without restart markers is one segment) in
        // blocks whose descriptors travel with the blob.
        sp.mh = 0;
        sp.mh_blocks.clear();
        // What the speculation buys depends on how long a decoder that is off by some data units stays undetected: as long
        // as the units it confuses share their code tables. `run` = the longest run of consecutive data units of the MCU
        // with the same tables: 4 for 4:2:0 (Y Y Y Y), 2 for 4:2:2 (Y Y | Cb Cr) and 4:4:4 (Cb Cr). Sync stage of one 12 MP
        // image, speculation on / off (us, round 4): 4:2:0 with restart markers 137 / 294, without (block-wise walk)
        // 186 / 278; 4:2:2 117 / 138 and 161 / 133; 4:4:4 95 / 62 and 133 / 75; BASELINE configs[4] (4 components, runs of
        // 2, no restart markers) 204 / 140. So: runs of three and more always; runs of two only in the cheaper whole-segment
        // form and only with four units or more per MCU.
        int run = 1;
        {
            int du_tabs[2 * kMaxDuPerMcu], m = 0;
            for (int rep = 0; rep < 2; ++rep)
                for (int a = 0; a < sc.num_comp; ++a)
                    for (int k = 0; k < sc.comp[a].h * sc.comp[a].v && m < 2 * kMaxDuPerMcu; ++k) du_tabs[m++] = sc.comp[a].dc_id * 4 + sc.comp[a].ac_id;
            for (int i = 1, cur = 1; i < m; ++i) {
                cur = du_tabs[i] == du_tabs[i - 1] ? cur + 1 : 1;
                run = std::max(run, std::min(cur, sc.du_per_mcu));
            }
        }
        if (!batched && sc.du_per_mcu >= 2 && sc.du_per_mcu <= kMhMaxHyp && mh_enabled && run >= 2) {
            int longest = sc.device_walk ? kMhMaxSegSubseq : 0; // the device finds the segments: it falls back where one is longer
            for (const Segment& g : sc.segments) longest = std::max(longest, g.subseq_count);
            // a device-scanned scan without restart markers is ONE segment whose length the host can only bound: the
            // device builds the block list from what it finds (jg_front.hip, front_plan), sized here from the bound
            const bool device_blocks = sc.device_walk && s.restart_interval == 0;
            if (device_blocks) longest = std::max(sc.num_subseq, kMhMaxSegSubseq + 1);
            if (longest <= kMhMaxSegSubseq && run < 3 && sc.du_per_mcu < 4) longest = -1; // (runs of two: four units and more)
            if (longest > kMhMaxSegSubseq && run < 3) longest = -1;                       // (block-wise: runs of three and more)
            sp.mh_blocks_device = 0;
            if (longest < 0) {
            } else if (longest <= kMhMaxSegSubseq) {
                sp.mh             = sc.du_per_mcu;
                sp.max_seg_subseq = longest;
            } else if (device_blocks) {
                const int nb = (sc.num_subseq + kMhMaxSegSubseq - 1) / kMhMaxSegSubseq;
                if (nb <= kMhMaxBlocks) {
                    sp.mh               = sc.du_per_mcu;
                    sp.max_seg_subseq   = kMhMaxSegSubseq;
                    sp.mh_blocks_device = nb;
                }
            } else if (!sc.device_walk) {
                for (const Segment& g : sc.segments) {
                    for (int r = 0; r < g.subseq_count; r += kMhMaxSegSubseq)
                        sp.mh_blocks.push_back(MhBlock{g.subseq_offset + r, std::min(kMhMaxSegSubseq, g.subseq_count - r),
                                                       g.subseq_offset + g.subseq_count, r == 0 ? 1 : 0});
                }
                if (sp.mh_blocks.size() <= static_cast<size_t>(kMhMaxBlocks)) {
                    sp.mh             = sc.du_per_mcu;
                    sp.max_seg_subseq = kMhMaxSegSubseq;
                    sp.blob_mh_blocks = blob(sp.mh_blocks.size() * sizeof(MhBlock));
                } else {
                    sp.mh_blocks.clear();
                }
            }
        }
    }
    if (s.progressive) { // its descriptors (jg_prog_plan.hpp carves them): one region of the trace
        const size_t begin = blob.at;
        p.prog.on = true;
        prog_plan_blob(s, p.prog.blob, blob.at);
        if (trace) trace->blob.push_back({begin, blob.at - begin});
    }
    p.blob_size = blob.at;

    // device carve: transferred region first, at fixed places (reference decoder.cpp:116-155)
    Carve tmp{0, trace ? &trace->tmp : nullptr};
    p.bytes_len = s.xfer_end - s.xfer_begin;
    p.off_bytes = tmp(align_up(p.bytes_len, kDestuffWin) + kDestuffWin); // whole windows are loaded
    p.off_blob  = tmp(p.blob_size);
    for (int i = 0; i < s.num_scans; ++i) {
        const Scan& sc = s.scans[i];
        ScanPlan& sp   = p.scan[i];
        const size_t S = static_cast<size_t>(sc.num_subseq);
        sp.num_seq     = static_cast<int>((S + kSeqSubseq - 1) / kSeqSubseq);
        const size_t Q = static_cast<size_t>(sp.num_seq);
        sp.destuffed   = tmp(tiled_buffer_bytes(static_cast<uint32_t>(S), subseq_bytes, 96) + 256); // whole tiles of padded rows, 96 rows spare
        sp.seg_idx     = tmp(S * 4);
        sp.st_p        = tmp(S * 4);
        sp.st_n        = tmp(S * 4);
        sp.st_cz       = tmp(S * 4);
        sp.st_dc01     = tmp(S * 4);
        sp.st_dc23     = tmp(S * 4);
        sp.pending     = tmp(S);
        sp.flow_list   = tmp(S * 4);
        sp.tails_n     = tmp(Q * 4);
        sp.tails_dc01  = tmp(Q * 4);
        sp.tails_dc23  = tmp(Q * 4);
        sp.bnd_p       = tmp(Q * 4);
        sp.bnd_cz      = tmp(Q * 4);
        sp.fuse_ctl    = tmp(fuse_ctl_words(Q) * 4); // control words of huff_tail_write
        if (sp.mh > 1) { // multi-hypothesis speculation (decided with the blob, above)
            const size_t N = S * static_cast<size_t>(sp.mh);
            sp.mh_p        = tmp(N * 4);
            sp.mh_cz       = tmp(N * 4);
            sp.mh_link     = tmp(N * 4);
            sp.mh_pool     = tmp((1 + static_cast<size_t>(mh_pool_entries(static_cast<uint32_t>(S)))) * sizeof(uint2_t));
            sp.mh_known    = tmp(S);
            const size_t nblocks = sp.mh_blocks_device ? static_cast<size_t>(sp.mh_blocks_device) : sp.mh_blocks.size();
            if (nblocks) {
                sp.mh_blk_exit  = tmp(nblocks * 64 * sizeof(uint16_t));
                sp.mh_blk_entry = tmp(nblocks * sizeof(uint16_t));
            }
            if (sp.mh_blocks_device) sp.d_mh_blocks = tmp(nblocks * sizeof(MhBlock));
        }
        if (sc.device_walk) {
            const size_t E  = static_cast<size_t>(sc.expect_segments);
            sp.num_windows  = static_cast<uint32_t>(align_up(p.bytes_len, kDestuffWin) / kDestuffWin) - sc.front_win0;
            const size_t Wn = sp.num_windows;
            sp.d_segments   = tmp(E * sizeof(Segment));
            sp.d_chunks     = tmp(static_cast<size_t>(sc.max_chunks) * sizeof(DestuffChunk));
            sp.d_parts      = tmp(static_cast<size_t>(sc.max_tail_parts) * sizeof(int));
            sp.d_win_data   = tmp(Wn * 4);
            sp.d_win_nmark  = tmp(Wn * 4);
            sp.d_win_bad    = tmp(Wn * 4);
            sp.d_win_prefix = tmp((Wn + 1) * 4);
            sp.d_mark_off   = tmp((Wn + 1) * 4);
            sp.d_mk_pos     = tmp((E + 1) * 4);
            sp.d_mk_g       = tmp((E + 1) * 4);
            sp.d_seg_cnt    = tmp((E + 1) * 4);
            sp.d_seg_nch    = tmp((E + 1) * 4);
            sp.d_job        = tmp(sizeof(ScanJob));
            sp.d_status     = tmp(32);
        }
        if (s.trunc.scan == i) sp.trunc_state = tmp(2 * sizeof(uint32_t));
    }
    for (int i = 0; i < s.num_scans; ++i) {
        p.scan[i].sym    = tmp(sym_buffer_entries(sym_regions(i), sym_region()) * 2 + 256); // symbol stream: a fixed region per subsequence
        p.scan[i].du_tab = tmp(static_cast<size_t>(s.scans[i].num_du) * sizeof(uint2_t));
    }
    if (s.progressive) { // the coefficient buffers, one after the other: one memset zeroes them
        p.prog.coef_begin = tmp.at;
        for (int c = 0; c < s.num_comp; ++c)
            p.prog.coef[c] = tmp(static_cast<size_t>(s.prog_blocks_x[c]) * static_cast<size_t>(s.prog_blocks_y[c]) * 64 * sizeof(int16_t));
        p.prog.coef_bytes = tmp.at - p.prog.coef_begin;
    }
    p.total = tmp.at;
    plan    = p;
}

/// What jpeggpu_decoder_parse_header does on the host alone: parse the file under the settings asked for, set the geometry,
/// fill `img_info`, make the plan. The blob is then filled by the caller, who also sets `parsed`.
jpeggpu_status Decoder::plan_image(jpeggpu_img_info* img_info, const uint8_t* data, size_t size, PlanTrace* trace)
{
    parsed      = false;
    scale_log2  = scale_log2_request;
    idct_method = idct_method_request;
    scale_mode  = scale_mode_request;
    draft       = false;
    crop.on     = false;
    const bool want_crop = crop_request[2] > 0;
    if (want_crop && shard_world > 1) {
        logger.log("a crop and a segment shard do not go together\n");
        return JPEGGPU_NOT_SUPPORTED;
    }
    jpeggpu_status st;
    try {
        const int ask = subseq_request > 0 ? subseq_request : -batch_hint; // 0 / -N: chosen per image for N images per call
        st = reader.parse(data, size, ask, logger, device_scan != 0, shard_rank, shard_world, progressive, truncated);
        subseq_bytes = reader.subseq_bytes();
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    if (st != JPEGGPU_SUCCESS) return st;
    const Stream& s = reader.s;
    luma_only = false;
    if (luma_only_request) { // libjpeg's out_color_space = JCS_GRAYSCALE: grey and RGB-coded files need every component
        if (s.color_space != kColorGray && s.color_space != kColorYCbCr && s.color_space != kColorRGB) {
            logger.log("luma-only decoding: colour model %d has no grey\n", s.color_space);
            return JPEGGPU_NOT_SUPPORTED;
        }
        luma_only = s.color_space == kColorYCbCr;
    }
    set_block_sizes();
    if (want_crop) {
        if (!set_crop_window()) {
            logger.log("crop %d,%d %dx%d does not lie inside the image\n", crop_request[0], crop_request[1], crop_request[2], crop_request[3]);
            return JPEGGPU_INVALID_ARGUMENT;
        }
        // one host-walked scan with restart markers: keep only the segments that hold the window's MCUs
        const Scan& sc = s.scans[0];
        // (not the scan a truncated file ends in: its segment table ends with the data, and jg_trunc.hip counts from MCU 0)
        if (s.num_scans == 1 && s.restart_interval > 0 && !sc.device_walk && !sc.segments.empty() && s.trunc.scan < 0) {
            const IdctWindow w = scan_window(sc);
            const int m0 = w.my0 * sc.mcus_x + w.mx0, m1 = (w.my0 + w.mcus_y - 1) * sc.mcus_x + w.mx0 + w.mcus_x - 1;
            reader.cut_segments(m0 / sc.mcus_per_segment, m1 / sc.mcus_per_segment + 1);
        }
    }
    if (device_scan)
        logger.log("device-side marker scan: %s (jpeggpu_ext_set_device_scan / JPEGGPU_DEVICE_SCAN)\n",
                   device_scan == 2 ? "checked -- jpeggpu_decoder_decode waits for the stream and returns the device's status" : "asynchronous");
    std::memset(img_info, 0, sizeof(*img_info));
    img_info->num_components = s.num_comp;
    for (int c = 0; c < s.num_comp; ++c) {
        img_info->sizes_x[c]       = plane_x(c); // libjpeg's downsampled_width at the scale (cropped: the window's)
        img_info->sizes_y[c]       = plane_y(c);
        img_info->subsampling.x[c] = eff_hs(c); // (draft mode: the factors the planes have, h_c S_c / S_min)
        img_info->subsampling.y[c] = eff_vs(c);
    }
    this->data = data;
    data_size  = size;
    // The IDCT addresses the 16-bit symbol stream with 32-bit BYTE offsets and the data-unit table holds 32-bit
    // entry indices (jg_idct.hip, entry_at / prefetch): a scan whose stream would not fit them (from about
    // 400 MB of entropy-coded data at 64-byte subsequences) is refused here instead of gathering from wrapped offsets.
    for (int i = 0; i < s.num_scans; ++i) {
        const uint64_t entries = sym_buffer_entries(sym_regions(i), sym_region());
        if (entries * 2u >= (1ull << 32)) {
            logger.log("scan %d: %d subsequences of %d bytes need a symbol stream of %llu bytes (32-bit offsets)\n", i,
                       s.scans[i].num_subseq, subseq_bytes, static_cast<unsigned long long>(entries * 2u));
            return JPEGGPU_NOT_SUPPORTED;
        }
    }
    try {
        make_plan(trace);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    // the descriptors of a progressive image hold 32-bit offsets of the blob inside d_tmp
    if (plan.prog.on && plan.off_blob + plan.blob_size >= (1ull << 32)) return JPEGGPU_NOT_SUPPORTED;
    return JPEGGPU_SUCCESS;
}

void Decoder::fill_blob(uint8_t* dst) const
{
    const Stream& s = reader.s;
    std::memset(dst, 0, plan.blob_size);
    std::memcpy(dst + plan.blob_qtables, s.qtable, sizeof(s.qtable));
    for (int i = 0; i < s.num_scans; ++i) {
        const Scan& sc     = s.scans[i];
        const ScanPlan& sp = plan.scan[i];
        if (!sc.table_pack.empty()) std::memcpy(dst + sp.blob_tables, sc.table_pack.data(), sc.table_pack.size());
        if (!sc.table_pack_sync.empty()) std::memcpy(dst + sp.blob_tables_sync, sc.table_pack_sync.data(), sc.table_pack_sync.size());
        if (!sc.segments.empty()) std::memcpy(dst + sp.blob_segments, sc.segments.data(), sc.segments.size() * sizeof(Segment));
        if (!sc.chunks.empty()) std::memcpy(dst + sp.blob_chunks, sc.chunks.data(), sc.chunks.size() * sizeof(DestuffChunk));
        if (!sc.tail_parts.empty()) std::memcpy(dst + sp.blob_parts, sc.tail_parts.data(), sc.tail_parts.size() * sizeof(int));
        if (!sp.mh_blocks.empty()) std::memcpy(dst + sp.blob_mh_blocks, sp.mh_blocks.data(), sp.mh_blocks.size() * sizeof(MhBlock));
    }
    if (!plan.prog.on) return;
    const ProgPlan& pp = plan.prog; // a progressive image's descriptors say where the rest of it lies in d_tmp
    ProgPlacement at{};
    at.blob_in_tmp = plan.off_blob;
    at.bytes_off = plan.off_bytes, at.bytes_len = plan.bytes_len;
    at.coef_begin = pp.coef_begin, at.coef_bytes = pp.coef_bytes;
    for (int c = 0; c < s.num_comp; ++c) at.coef[c] = pp.coef[c], at.sym[c] = plan.scan[c].sym, at.du_tab[c] = plan.scan[c].du_tab;
    prog_fill_blob(s, pp.blob, at, dst);
}

jpeggpu_status build_jobs(
    Decoder& d, const jpeggpu_img* img, void* d_tmp, size_t tmp_size, int max_intra_iters, bool lone, bool keep_flows, std::vector<ScanJob>& jobs, bool planes)
{
    if (!d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    const Stream& s = d.reader.s;
    for (int c = 0; c < s.num_comp && planes; ++c) {
        if (c > 0 && d.luma_only) break; // never written: the pointers may be NULL
        if (!img->image[c] || img->pitch[c] < d.plane_x(c)) return JPEGGPU_INVALID_ARGUMENT;
    }
    if (!d_tmp || (reinterpret_cast<uintptr_t>(d_tmp) & 255)) return JPEGGPU_INVALID_ARGUMENT;
    if (tmp_size < d.plan.total) return JPEGGPU_INTERNAL_ERROR;
    uint8_t* base    = static_cast<uint8_t*>(d_tmp);
    const Plan& plan = d.plan;
    uint8_t* blob    = base + plan.off_blob;

    for (int i = 0; i < s.num_scans; ++i) {
        const Scan& sc     = s.scans[i];
        const ScanPlan& pl = plan.scan[i];
        ScanJob job{};
        ScanParams& sp      = job.sp;
        sp.num_subseq       = sc.num_subseq;
        sp.num_segments     = static_cast<int>(sc.segments.size());
        sp.du_per_mcu       = sc.du_per_mcu;
        sp.num_comp         = sc.num_comp;
        sp.mcus_per_segment = sc.mcus_per_segment;
        sp.total_mcus       = sc.shard_mcus ? sc.shard_mcus : sc.mcus_x * sc.mcus_y; // of this decoder's share
        sp.subseq_words     = d.subseq_bytes / 4;
        sp.tab_bytes        = static_cast<uint32_t>(sc.table_pack.size());
        sp.max_intra_iters  = keep_flows ? kSeqLanes : max_intra_iters;
        sp.tail_marks       = keep_flows ? 0 : 1;
        sp.cursor_off       = sc.cursor_off;
        sp.tab_bytes_sync   = static_cast<uint32_t>(sc.table_pack_sync.size());
        sp.cursor_off_sync  = sc.cursor_off_sync;
        sp.mh               = lone ? pl.mh : 0; // the multi-hypothesis kernels run in front of a lone decode's sequence kernel only
        // a full batch's sequences are longer: one overlap lane (jg_defs.h); where every flow stays in the workgroup the 16
        // overlap lanes are what keeps the sequence boundaries from starting tail flows
        sp.seq_subseq       = keep_flows ? kSeqSubseq : kSeqSubseqBatch;
        d.seq_subseq_used   = sp.seq_subseq;
        job.mh_p            = at<int>(base, pl.mh_p);
        job.mh_cz           = at<int>(base, pl.mh_cz);
        job.mh_link         = at<uint32_t>(base, pl.mh_link);
        job.mh_pool         = at<uint2_t>(base, pl.mh_pool);
        job.mh_known        = at<uint8_t>(base, pl.mh_known);
        job.num_mh_blocks   = lone ? static_cast<int>(pl.mh_blocks.size()) : 0;
        job.mh_blocks       = job.num_mh_blocks ? at<const MhBlock>(blob, pl.blob_mh_blocks) : nullptr;
        if (lone && pl.mh_blocks_device) { // the list the device builds (capacity here, the real count in its copy of the job)
            job.num_mh_blocks = pl.mh_blocks_device;
            job.mh_blocks     = at<const MhBlock>(base, pl.d_mh_blocks);
        }
        job.mh_blk_exit     = at<uint16_t>(base, pl.mh_blk_exit);
        job.mh_blk_entry    = at<uint16_t>(base, pl.mh_blk_entry);
        IdctParams& ip = job.ip;
        ip.num_du      = sc.num_du;
        ip.du_per_mcu  = sc.du_per_mcu;
        ip.mcus_x      = sc.mcus_x;
        ip.first_mcu   = sc.first_mcu;
        // a luma-only job lists its units by block size as a draft job does: no kernel of the other jobs takes it
        ip.scale_log2  = static_cast<uint8_t>(d.draft || d.luma_only ? kDraftScale | d.scale_log2 : d.scale_log2);
        ip.idct_method = d.scale_log2 == 0 ? d.idct_method : kIdctReference;
        {
            const MagicDiv a = magic_div(static_cast<uint32_t>(sc.du_per_mcu)), b = magic_div(static_cast<uint32_t>(sc.mcus_x));
            ip.du_per_mcu_mul = a.mul, ip.du_per_mcu_shift = a.shift;
            ip.mcus_x_mul = b.mul, ip.mcus_x_shift = b.shift;
        }
        int du         = 0;
        for (int a = 0; a < sc.num_comp; ++a) {
            const ScanComponent& c = sc.comp[a];
            for (int y = 0; y < c.v; ++y) {
                for (int x = 0; x < c.h; ++x) { // row-major inside the MCU (T.81 A.2.3)
                    ip.du_comp[du] = static_cast<uint8_t>(a);
                    ip.du_dx[du]   = static_cast<uint8_t>(x);
                    ip.du_dy[du]   = static_cast<uint8_t>(y);
                    ++du;
                }
            }
            const Component& fc = s.comp[c.comp_idx];
            ip.comp_h[a]        = c.h;
            ip.comp_v[a]        = c.v;
            ip.size_x[a]        = d.plane_x(c.comp_idx); // (cropped: the window, and the window's units below)
            ip.size_y[a]        = d.plane_y(c.comp_idx);
            ip.pitch[a]         = img->pitch[c.comp_idx];
            ip.qidx[a]          = fc.qidx;
            ip.plane[a]         = img->image[c.comp_idx];
        }
        if (d.draft || d.luma_only) { // the units of the MCU by block size (IdctDraft); luma only: those of component 0
            IdctDraft& dr = job.draft;
            // 8x8 blocks of kDraftOn jobs take the ISLOW arithmetic; a full-size luma-only job of the reference IDCT is a
            // class of its own
            dr.on = d.luma_only && !d.draft && d.scale_log2 == 0 && d.idct_method == kIdctReference ? kDraftLumaReference : kDraftOn;
            for (int k = 0; k < sc.du_per_mcu; ++k) {
                const int comp_idx             = sc.comp[ip.du_comp[k]].comp_idx;
                const int lg                   = d.blk_lg[comp_idx];
                dr.comp_lg[ip.du_comp[k]]      = static_cast<uint8_t>(lg);
                if (d.luma_only && comp_idx != 0) continue; // component_needed = FALSE (jdmaster.c): no IDCT
                dr.k[lg][dr.n[lg]++]           = static_cast<uint8_t>(k);
            }
            for (int lg = 0; lg < 4; ++lg) {
                const MagicDiv m = magic_div(dr.n[lg]);
                dr.mul[lg] = m.mul, dr.shift[lg] = m.shift;
            }
        }
        job.win = d.scan_window(sc);
        if (job.win.mcus_x) ip.num_du = job.win.mcus_x * job.win.mcus_y * sc.du_per_mcu;
        job.bytes      = at<uint8_t>(base, plan.off_bytes);
        job.chunks     = at<const DestuffChunk>(blob, pl.blob_chunks);
        job.segments   = at<const Segment>(blob, pl.blob_segments);
        job.tables     = at<uint8_t>(blob, pl.blob_tables);
        job.tables_sync = at<uint8_t>(blob, pl.blob_tables_sync);
        job.qtables    = at<const uint16_t>(blob, plan.blob_qtables);
        job.destuffed  = at<uint8_t>(base, pl.destuffed);
        job.seg_idx    = at<int>(base, pl.seg_idx);
        job.st_p       = at<int>(base, pl.st_p);
        job.st_n       = at<int>(base, pl.st_n);
        job.st_cz      = at<int>(base, pl.st_cz);
        job.st_dc01    = at<uint32_t>(base, pl.st_dc01);
        job.st_dc23    = at<uint32_t>(base, pl.st_dc23);
        job.pending    = at<uint8_t>(base, pl.pending);
        job.bnd_p      = at<int>(base, pl.bnd_p);
        job.bnd_cz     = at<int>(base, pl.bnd_cz);
        job.flow_list  = at<int>(base, pl.flow_list);
        job.tail_parts = at<const int>(blob, pl.blob_parts);
        job.num_tail_parts = static_cast<int>(sc.tail_parts.size()) - 1;
        job.max_tail_part  = 0;
        job.fuse_ctl       = at<uint32_t>(base, pl.fuse_ctl);
        for (size_t k = 0; k + 1 < sc.tail_parts.size(); ++k)
            job.max_tail_part = std::max(job.max_tail_part, sc.tail_parts[k + 1] - sc.tail_parts[k]);
        job.tails_n    = at<int>(base, pl.tails_n);
        job.tails_dc01 = at<uint32_t>(base, pl.tails_dc01);
        job.tails_dc23 = at<uint32_t>(base, pl.tails_dc23);
        job.sym         = at<uint16_t>(base, pl.sym);
        job.du_tab      = at<uint2_t>(base, pl.du_tab);
        job.sym_region  = d.sym_region();
        job.sym_entries = sym_buffer_entries(d.sym_regions(i), job.sym_region);
        job.num_chunks = static_cast<int>(sc.chunks.size());
        job.num_seq    = static_cast<int>((static_cast<size_t>(sc.num_subseq) + sp.seq_subseq - 1) / sp.seq_subseq); // <= pl.num_seq, what the arrays are sized for
        if (sc.device_walk) {
            // tables built by jg_front.hip in device memory; the counts below are capacities (launch extents),
            // the device writes the real ones into its copy of the job
            job.chunks         = at<const DestuffChunk>(base, pl.d_chunks);
            job.segments       = at<const Segment>(base, pl.d_segments);
            job.tail_parts     = at<const int>(base, pl.d_parts);
            job.num_chunks     = sc.max_chunks;
            job.num_tail_parts = sc.max_tail_parts - 1;
            job.max_tail_part  = s.restart_interval ? kTailPartSubseq : (1 << 30); // lanes of the tail kernel
            sp.num_segments    = sc.expect_segments;
            // the device's tables count from the window that holds this scan's first byte (earlier scans lie in front)
            job.bytes          = base + plan.off_bytes + static_cast<size_t>(sc.front_win0) * kDestuffWin;
        }
        jobs.push_back(job);
    }
    return JPEGGPU_SUCCESS;
}

int truncated_scan_index(const Decoder& d) { return d.reader.s.trunc.scan; }

TruncParams trunc_params(const Decoder& d, void* d_tmp)
{
    const Stream::Truncation& t = d.reader.s.trunc;
    TruncParams tp{};
    tp.cut_segment  = t.cut_segment;
    tp.end_bit      = t.end_bit;
    tp.zero_segment = t.zero_segment;
    tp.state        = at<uint32_t>(static_cast<uint8_t*>(d_tmp), d.plan.scan[t.scan].trunc_state);
    return tp;
}

int device_scan_index(const Decoder& d)
{
    const Stream& s = d.reader.s;
    return s.num_scans > 0 && s.scans[s.num_scans - 1].device_walk ? s.num_scans - 1 : -1;
}

FrontParams front_params(const Decoder& d, void* d_tmp, ScanJob* d_job, int k)
{
    const Scan& sc     = d.reader.s.scans[k];
    const ScanPlan& pl = d.plan.scan[k];
    uint8_t* base      = static_cast<uint8_t*>(d_tmp);
    const size_t skip  = static_cast<size_t>(sc.front_win0) * kDestuffWin; // whole windows of earlier scans' bytes
    FrontParams P{};
    P.bytes           = base + d.plan.off_bytes + skip;
    P.bytes_len       = static_cast<uint32_t>(d.plan.bytes_len - skip);
    P.scan_begin      = static_cast<uint32_t>(sc.begin - d.reader.s.xfer_begin - skip);
    P.num_windows     = pl.num_windows;
    P.expect_segments = static_cast<uint32_t>(sc.expect_segments);
    P.subseq_bytes    = static_cast<uint32_t>(d.subseq_bytes);
    P.max_subseq      = static_cast<uint32_t>(sc.num_subseq);
    P.max_chunks      = static_cast<uint32_t>(sc.max_chunks);
    P.max_parts       = static_cast<uint32_t>(sc.max_tail_parts);
    P.win_data   = at<uint32_t>(base, pl.d_win_data);
    P.win_nmark  = at<uint32_t>(base, pl.d_win_nmark);
    P.win_bad    = at<uint32_t>(base, pl.d_win_bad);
    P.win_prefix = at<uint32_t>(base, pl.d_win_prefix);
    P.mark_off   = at<uint32_t>(base, pl.d_mark_off);
    P.mk_pos     = at<uint32_t>(base, pl.d_mk_pos);
    P.mk_g       = at<uint32_t>(base, pl.d_mk_g);
    P.seg_cnt    = at<uint32_t>(base, pl.d_seg_cnt);
    P.seg_nch    = at<uint32_t>(base, pl.d_seg_nch);
    P.segments   = at<Segment>(base, pl.d_segments);
    P.chunks     = at<DestuffChunk>(base, pl.d_chunks);
    P.tail_parts = at<int>(base, pl.d_parts);
    P.job        = d_job;
    P.status     = at<uint32_t>(base, pl.d_status);
    P.mh_blocks     = pl.mh_blocks_device ? at<MhBlock>(base, pl.d_mh_blocks) : nullptr;
    P.max_mh_blocks = static_cast<uint32_t>(pl.mh_blocks_device);
    return P;
}

} // namespace jg
