// jg_decoder.hpp -- the decoder's state and its plan, shared by the sources of the host side: jg_plan.cpp (geometry, plan,
// jobs: host only), jg_decoder.cpp (the lone decode and the decoder's C ABI) and jg_batch.cpp (jpeggpu_ext_decode_batch).
//
// Nothing here needs the HIP runtime: jg_plan.cpp compiles with a plain C++ compiler and runs without a device
// (tests/test_plan_host.py). What does need it -- the pinned copy of the table blob, the stage timer -- belongs to
// jg_decoder.cpp, and the Decoder only points at it.
#ifndef JG_DECODER_HPP_
#define JG_DECODER_HPP_

#include "jg_prog_plan.hpp"
#include "jg_reader.hpp"

#include <jpeggpu/jpeggpu.h>
#include <jpeggpu/jpeggpu_ext.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace jg {

class StageTimer; // jg_stage_timer.hpp

struct ScanPlan {
    // offsets inside the blob (and, shifted by off_blob, inside d_tmp)
    size_t blob_tables = 0, blob_tables_sync = 0, blob_segments = 0, blob_chunks = 0, blob_parts = 0;
    // offsets inside d_tmp
    size_t destuffed = 0, seg_idx = 0, st_p = 0, st_n = 0, st_cz = 0, st_dc01 = 0, st_dc23 = 0;
    size_t tails_n = 0, tails_dc01 = 0, tails_dc23 = 0, pending = 0, flow_list = 0, bnd_p = 0, bnd_cz = 0, fuse_ctl = 0;
    size_t sym = 0, du_tab = 0;
    size_t mh_p = 0, mh_cz = 0, mh_link = 0, mh_pool = 0, mh_known = 0; // multi-hypothesis speculation (jg_defs.h), if mh > 1
    size_t blob_mh_blocks = 0, mh_blk_exit = 0, mh_blk_entry = 0;        // its block-wise chain walk, if mh_blocks is not empty
    std::vector<jg::MhBlock> mh_blocks;
    int mh_blocks_device = 0;           // device-scanned scan without restart markers: capacity of the list jg_front.hip builds
    size_t d_mh_blocks = 0;             //   ... and where it sits in d_tmp
    int mh = 0, max_seg_subseq = 0;
    int num_seq = 0;
    // device-side front end (jg_front.hip): tables built on the device, scratch, the job and the status word
    size_t d_segments = 0, d_chunks = 0, d_parts = 0;
    size_t d_win_data = 0, d_win_nmark = 0, d_win_bad = 0, d_win_prefix = 0, d_mark_off = 0;
    size_t d_mk_pos = 0, d_mk_g = 0, d_seg_cnt = 0, d_seg_nch = 0, d_job = 0, d_status = 0;
    uint32_t num_windows = 0;
    size_t trunc_state = 0; // the scan a truncated file ends in: two words of jg_trunc.hip (TruncParams::state); else not carved
};

/// A progressive image's part of the plan (jg_prog_core.h): its descriptors in the blob, its coefficient buffers in d_tmp.
struct ProgPlan {
    bool on = false;
    ProgBlobLayout blob;                                        // jg_prog_plan.hpp: offsets inside the blob, the work list
    size_t coef[kMaxComp] = {}, coef_begin = 0, coef_bytes = 0; // offsets inside d_tmp
};

struct Plan {
    size_t off_bytes = 0, bytes_len = 0;
    size_t off_blob = 0, blob_size = 0;
    size_t blob_qtables = 0;
    size_t total = 0;
    ScanPlan scan[kMaxScans];
    ProgPlan prog;
};

/// What make_plan carved, in the order of the carve, for a check of the plan: {offset, bytes asked for} inside the blob
/// and inside d_tmp.
struct PlanTrace {
    struct Region {
        size_t offset, bytes;
    };
    std::vector<Region> blob, tmp;
};

// What one source of the library defines for the others is not among the symbols the library exports.
#define JG_LOCAL __attribute__((visibility("hidden")))

struct Decoder {
    Reader reader;
    Logger logger;
    Plan plan;
    // The table blob as fill_blob wrote it, plan.blob_size bytes of host memory (page-locked where there is a device: the
    // copy that transfer enqueues is asynchronous), and the stage timer of jpeggpu_ext_set_profiling: both the library's.
    const uint8_t* blob = nullptr;
    StageTimer* timer   = nullptr;
    const uint8_t* data = nullptr;
    size_t data_size    = 0;
    // Subsequence size: chosen PER IMAGE at parse_header (jg_reader.hpp, choose_subseq_bytes) from the scan's size, its
    // restart density and the call type -- `batched`: the decoder's images share their launches with others
    // (jpeggpu_ext_set_batched; jpeggpu_ext_decode_batch accepts any mix of sizes) -- unless the caller fixed one
    // (jpeggpu_ext_set_subsequence_bytes, JPEGGPU_SUBSEQ_BYTES). `subseq_bytes` is the size of the last parsed image.
    int subseq_request  = 0;     // 0: choose per image; else 32 / 64 / 128 / 256
    // About how many images of this kind share one jpeggpu_ext_decode_batch call (jpeggpu_ext_set_batch_hint; 0: decoded on
    // its own, jpeggpu_ext_set_batched(1): kBatchHintFull). `batched`: the plan is a batch's (no multi-hypothesis tables).
    int batch_hint      = 0;
    bool batched        = false;
    int seq_subseq_used = 0;     // subsequences per sequence of the last decode call built from this parse (0: none yet)
    bool mh_enabled     = true;  // JPEGGPU_MULTI_HYPOTHESIS=0 at startup: plain speculation for lone decodes as well
    int subseq_bytes    = 64;
    bool parsed         = false;
    int shard_rank = 0, shard_world = 1; // jpeggpu_ext_set_segment_shard
    bool progressive    = false; // jpeggpu_ext_set_progressive: SOF2 frames are read, from the next parse_header on
    bool truncated      = false; // jpeggpu_ext_set_truncated: files that end early are read, from the next parse_header on
    int device_scan     = 0;     // jpeggpu_ext_set_device_scan: 0 off, 1 on (status via jpeggpu_ext_get_device_status), 2 on and checked by decode
    // jpeggpu_ext_set_scale: planes at 1 / 2^scale_log2. The request takes effect at the next parse_header (`scale_log2`:
    // that of the parsed image); it changes the plane sizes and the IDCT stage only, never the plan or the Huffman path.
    int scale_log2_request = 0;
    int scale_log2         = 0;
    int scaled(int size) const { return (size + (1 << scale_log2) - 1) >> scale_log2; } // ceil(size / 2^scale_log2)
    // jpeggpu_ext_set_scale_mode (or JPEGGPU_SCALE_MODE at startup), taking effect at the next parse_header like the scale.
    // `draft`: the parsed image is decoded in JPEGGPU_EXT_SCALE_LIBJPEG mode at a scale below 1: component c has blocks of
    // 8 >> blk_lg[c] samples (jdmaster.c's DCT_scaled_size, set_block_sizes). Otherwise blk_lg[c] == scale_log2 for all.
    int scale_mode_request = 0;
    int scale_mode         = 0;
    bool draft             = false;
    int blk_lg[kMaxComp]   = {0, 0, 0, 0};
    JG_LOCAL void set_block_sizes();
    int blk(int c) const { return 8 >> blk_lg[c]; }                                           // samples per block side
    int eff_hs(int c) const { return reader.s.comp[c].hs << (scale_log2 - blk_lg[c]); }      // h_c S_c / S_min: the sampling
    int eff_vs(int c) const { return reader.s.comp[c].vs << (scale_log2 - blk_lg[c]); }      //   factor the planes really have
    // the component's whole plane at the scale: ceil(W h_c S_c / (8 h_max)) in draft mode, ceil(plane / d) otherwise
    int full_x(int c) const
    {
        const Stream& s = reader.s;
        if (!draft) return scaled(s.comp[c].size_x);
        const long long den = 8ll * s.hs_max;
        return static_cast<int>((static_cast<long long>(s.size_x) * s.comp[c].hs * blk(c) + den - 1) / den);
    }
    int full_y(int c) const
    {
        const Stream& s = reader.s;
        if (!draft) return scaled(s.comp[c].size_y);
        const long long den = 8ll * s.vs_max;
        return static_cast<int>((static_cast<long long>(s.size_y) * s.comp[c].vs * blk(c) + den - 1) / den);
    }
    // jpeggpu_ext_set_idct (or JPEGGPU_IDCT at startup): the full-size IDCT, taking effect at the next parse_header like the
    // scale. It changes the IDCT stage only, and only at scale 1 (the reduced IDCTs are libjpeg's already).
    uint8_t idct_method_request = kIdctReference;
    uint8_t idct_method         = kIdctReference;
    // jpeggpu_ext_set_crop: the rectangle {x, y, width, height} asked for (width 0: none), taking effect at the next
    // parse_header like the scale; `crop`: what the parsed image got. The decoder writes a WINDOW of each plane (jpeggpu_ext.h).
    int crop_request[4] = {0, 0, 0, 0};
    struct Crop {
        bool on = false;
        int x = 0, y = 0, w = 0, h = 0;       // the rectangle, in pixels of the image at the scale
        int mx0 = 0, my0 = 0, mx1 = 0, my1 = 0; // the frame MCUs the windows start in / end behind
        int ox[kMaxComp]{}, oy[kMaxComp]{};   // window origin in the component's plane
        int wx[kMaxComp]{}, wy[kMaxComp]{};   // window size
    } crop;
    // jpeggpu_ext_set_transcode_orientation: read by the jpeggpu_ext_transcode_* calls only (jg_transcode.cpp), when they run
    int transcode_orientation = 1;
    bool transcode_trim       = false;
    // jpeggpu_ext_set_transcode_crop: {x, y, width, height} in pixels of the image the transcode would write without it
    // (width 0: none), read by the same calls
    int transcode_crop[4] = {0, 0, 0, 0};
    // jpeggpu_ext_set_transcode_frame: the new file keeps the source's frame layout (1) or must have the encoder's (0)
    int transcode_frame = 0;
    // jpeggpu_ext_set_luma_only, taking effect at the next parse_header like the scale. `luma_only`: the parsed image is a
    // YCbCr one whose IDCT stage transforms component 0 alone (build_jobs lists only its units, IdctDraft); the planes of the
    // other components are neither asked for nor written. Grey and RGB-coded images are decoded as ever.
    bool luma_only_request = false;
    bool luma_only         = false;
    int plane_x(int c) const { return crop.on ? crop.wx[c] : full_x(c); } // what decode writes
    int plane_y(int c) const { return crop.on ? crop.wy[c] : full_y(c); }
    JG_LOCAL bool set_crop_window();
    JG_LOCAL IdctWindow scan_window(const Scan& sc) const;

    std::vector<ScanJob> jobs; // scratch of the last decode

    /// The plan of the parsed image, from the reader's stream and the settings above (jg_plan.cpp).
    JG_LOCAL void make_plan(PlanTrace* trace = nullptr);
    /// jpeggpu_decoder_parse_header without the blob: parse, geometry, `img_info`, plan.
    JG_LOCAL jpeggpu_status plan_image(jpeggpu_img_info* img_info, const uint8_t* data, size_t size, PlanTrace* trace = nullptr);
    /// The table blob of the plan: plan.blob_size bytes at `dst`.
    JG_LOCAL void fill_blob(uint8_t* dst) const;
    /// Entries of scan i's symbol stream: a region per subsequence, or per data unit for a component of a progressive frame.
    uint32_t sym_regions(int i) const { return static_cast<uint32_t>(reader.s.progressive ? reader.s.scans[i].prog_regions : reader.s.scans[i].num_subseq); }
    uint32_t sym_region() const { return reader.s.progressive ? kProgRegionEntries : sym_region_entries(subseq_bytes); }
};

#pragma GCC visibility push(hidden)
/// Validate the arguments of a decode and describe every scan of the image as a ScanJob, appended to `jobs` (jg_plan.cpp).
/// `lone`: jpeggpu_decoder_decode (multi-hypothesis tables where the plan has them). `keep_flows`: every flow stays in its
/// sequence's workgroup (huff_sync_intra with re-packed flows; the tail kernel looks at sequence boundaries only) -- lone
/// decodes and batches too small to fill the chip; else the sequence kernel runs `max_intra_iters` iterations and marks
/// the rest for the tail kernel. `planes` false: the jobs stop in front of the IDCT stage, and img's planes are not looked at.
jpeggpu_status build_jobs(
    Decoder& d, const jpeggpu_img* img, void* d_tmp, size_t tmp_size, int max_intra_iters, bool lone, bool keep_flows, std::vector<ScanJob>& jobs,
    bool planes = true);
/// Index of the scan a parsed truncated file ends in, whose job needs the kernels of jg_trunc.hip, or -1 (a whole file, a
/// file that lacks only what lies behind its last scan); `tp`: their parameters for that scan's job in `d_tmp`.
int truncated_scan_index(const Decoder& d);
TruncParams trunc_params(const Decoder& d, void* d_tmp);
/// Index of the scan of a parsed image that the device walks (its last one), or -1.
int device_scan_index(const Decoder& d);
/// Parameters of the device-side front end for the device-walked scan `k` of a parsed image; `d_job` is the device copy
/// of its job.
FrontParams front_params(const Decoder& d, void* d_tmp, ScanJob* d_job, int k);

/// One image on its own, with the lone decode's kernels (jg_decoder.cpp). `may_block`: the checked mode of the device scan
/// may wait for the stream (jpeggpu_decoder_decode); an item of a batch is never waited for (jpeggpu_ext.h).
jpeggpu_status do_decode(Decoder& d, jpeggpu_img* img, void* d_tmp, size_t tmp_size, jpeggpu_stream_t stream, bool may_block = true);

#pragma GCC visibility pop

} // namespace jg

struct jpeggpu_decoder {
    jg::Decoder d;
};

#endif // JG_DECODER_HPP_
