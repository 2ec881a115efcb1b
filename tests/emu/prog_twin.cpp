// prog_twin.cpp -- host twin of the progressive kernels (jpeggpu_amd/csrc/jg_prog.hip): the product's parser and
// jg_prog_core.h compiled as they are, driven the way the kernels drive them -- every (scan, restart segment) of a level
// before the next level, then the hand-over of every visible block -- plus the way back from the symbol stream by the
// rules of jg_defs.h. tests/test_progressive_host.py binds it; tests/emu/prog_fuzz_main.cpp runs it under sanitizers.
#include "jg_prog_plan.hpp"

#include <cstring>
#include <vector>

using namespace jg;

extern "C" {

struct ProgTwinInfo {
    int num_comp, num_scans, num_levels, color_space;
    int size_x[4], size_y[4];       // plane sizes
    int blocks_x[4], blocks_y[4];   // MCU-padded grid
    int vis_x[4], vis_y[4];         // ceil(size / 8)
    int scan_level[kMaxProgScans];
    int scan_segments[kMaxProgScans];
};

/// Parse `data` (SOF2 accepted iff `progressive`), and, for a progressive frame and non-null buffers, decode it:
/// coef[c]: int16[blocks_y][blocks_x][64] (the coefficient buffer); back[c]: int16[vis_y][vis_x][64], each visible block
/// packed into the symbol stream and read back from it. Returns the parser's status.
int prog_twin_run(const uint8_t* data, size_t size, int progressive, int shard_world, ProgTwinInfo* info, int16_t* const* coef, int16_t* const* back)
{
    Reader r;
    Logger log;
    const jpeggpu_status st = r.parse(data, size, 64, log, false, 0, shard_world, progressive != 0);
    if (st != JPEGGPU_SUCCESS) return st;
    const Stream& s = r.s;
    std::memset(info, 0, sizeof(*info));
    info->num_comp    = s.num_comp;
    info->color_space = s.color_space;
    for (int c = 0; c < s.num_comp; ++c) info->size_x[c] = s.comp[c].size_x, info->size_y[c] = s.comp[c].size_y;
    if (!s.progressive) return st;
    info->num_scans  = static_cast<int>(s.prog_scans.size());
    info->num_levels = s.num_levels;
    for (int c = 0; c < s.num_comp; ++c) {
        info->blocks_x[c] = s.prog_blocks_x[c], info->blocks_y[c] = s.prog_blocks_y[c];
        info->vis_x[c] = s.scans[c].mcus_x, info->vis_y[c] = s.scans[c].mcus_y;
    }
    for (size_t k = 0; k < s.prog_scans.size(); ++k) {
        info->scan_level[k]    = s.prog_scans[k].level;
        info->scan_segments[k] = static_cast<int>(s.prog_scans[k].segments.size());
    }
    if (!coef) return st;

    // The image's memory, laid out as d_tmp is: transferred bytes | table blob | coefficient buffers. The blob is the
    // decoder's (jg_prog_plan.hpp), and what follows reads it the way the kernels do: ProgHeader, the work list of each
    // level lane by lane (prog_scan_kernel), idle items included.
    const size_t bytes_len = s.xfer_end - s.xfer_begin;
    const auto up          = [](size_t v) { return (v + 255) / 256 * 256; };
    ProgBlobLayout lay;
    size_t blob_size = 0;
    prog_plan_blob(s, lay, blob_size);
    ProgPlacement at{};
    at.bytes_off = 0, at.bytes_len = bytes_len;
    at.blob_in_tmp = up(bytes_len);
    size_t o       = at.blob_in_tmp + up(blob_size);
    at.coef_begin  = o;
    size_t coef_at[kMaxComp] = {};
    for (int c = 0; c < s.num_comp; ++c) {
        coef_at[c] = at.coef[c] = o;
        o += up(static_cast<size_t>(s.prog_blocks_x[c]) * s.prog_blocks_y[c] * 128);
    }
    at.coef_bytes = o - at.coef_begin;
    std::vector<uint8_t> mem(o, 0);
    uint8_t* tmp = mem.data();
    std::memcpy(tmp, data + s.xfer_begin, bytes_len);
    prog_fill_blob(s, lay, at, tmp + at.blob_in_tmp);
    const ProgHeader& H = *reinterpret_cast<const ProgHeader*>(tmp + at.blob_in_tmp + lay.header);
    for (uint32_t level = 0; level < H.num_levels; ++level) {
        const uint32_t first = H.level_item[level], count = H.level_item[level + 1] - first;
        for (uint32_t i = count; i-- > 0;) { // (any order inside a level: its scans write disjoint coefficients)
            const ProgItem item = reinterpret_cast<const ProgItem*>(tmp + H.items_off)[first + i];
            if (item.scan >= H.num_scans) continue;
            const ProgScanDesc& sd = reinterpret_cast<const ProgScanDesc*>(tmp + H.scans_off)[item.scan];
            if (sd.level != level || item.seg >= static_cast<uint32_t>(sd.num_segments)) return JPEGGPU_INTERNAL_ERROR;
            const uint2_t range = reinterpret_cast<const uint2_t*>(tmp + sd.seg_off)[item.seg];
            ProgLane L;
            prog_lane_init(sd, tmp + H.bytes_off, H.bytes_len, range, static_cast<int>(item.seg), L);
            for (int64_t left = prog_max_steps(sd, L); left > 0 && prog_step(sd, tmp, L); --left) {
            }
        }
    }
    for (int c = 0; c < s.num_comp; ++c)
        std::memcpy(coef[c], tmp + coef_at[c], static_cast<size_t>(s.prog_blocks_x[c]) * s.prog_blocks_y[c] * 128);
    if (!back) return st;
    // the hand-over, and the way back: DC first, then value << 6 | zig-zag index, an escape behind a value of 10 bits and more
    constexpr int kNat[64] = JG_ORDER_NATURAL;
    for (int c = 0; c < s.num_comp; ++c) {
        const uint32_t units = static_cast<uint32_t>(s.scans[c].num_du);
        std::vector<uint16_t> sym(sym_buffer_entries(units, kProgRegionEntries), 0xDEADu);
        std::vector<uint2_t> du_tab(units);
        const int vx = s.scans[c].mcus_x;
        for (uint32_t w = 0; w < units; ++w) {
            const int16_t* blk = reinterpret_cast<const int16_t*>(tmp + coef_at[c]) + (static_cast<size_t>(w / vx) * s.prog_blocks_x[c] + w % vx) * 64;
            du_tab[w] = prog_pack_block(blk, sym_region_base(w, kProgRegionEntries), [&](uint32_t at, uint16_t e) { sym.at(at) = e; });
        }
        for (uint32_t w = 0; w < units; ++w) {
            int16_t* out = back[c] + static_cast<size_t>(w) * 64;
            std::memset(out, 0, 128);
            const uint32_t cnt = du_tab[w].y & 0x7Fu;
            for (uint32_t i = 0; i < cnt; ++i) {
                const uint32_t e = sym.at(sym_advance(du_tab[w].x, i));
                if (i == 0) {
                    out[0] = static_cast<int16_t>(e);
                } else if (sym_entry_index(e) != 0) {
                    const uint32_t next = i + 1 < cnt ? sym.at(sym_advance(du_tab[w].x, i + 1)) : 1u;
                    const bool esc      = (du_tab[w].y & kUnitHasEscape) && sym_entry_index(next) == 0;
                    out[kNat[sym_entry_index(e)]] = static_cast<int16_t>(esc ? sym_entry_value(e, next) : sym_entry_value(e));
                }
            }
        }
    }
    return st;
}

/// The work list of a progressive file as the device reads it: the ProgItem array and level_item, copied out of the blob
/// that prog_fill_blob wrote (not out of the planner's vectors). items: up to `cap` (scan, segment) pairs; level_item:
/// kMaxProgScans + 1 entries. Returns the number of items of the list (which may exceed cap), or -1 - status if the
/// parser refuses the file or it is not progressive.
int prog_twin_work(const uint8_t* data, size_t size, uint32_t* items, int cap, uint32_t* level_item)
{
    Reader r;
    Logger log;
    const jpeggpu_status st = r.parse(data, size, 64, log, false, 0, 1, true);
    if (st != JPEGGPU_SUCCESS) return -1 - static_cast<int>(st);
    const Stream& s = r.s;
    if (!s.progressive) return -1;
    ProgBlobLayout lay;
    size_t blob_size = 0;
    prog_plan_blob(s, lay, blob_size);
    ProgPlacement at{};
    at.bytes_len = s.xfer_end - s.xfer_begin;
    std::vector<uint8_t> blob(blob_size, 0);
    prog_fill_blob(s, lay, at, blob.data());
    const ProgHeader& H = *reinterpret_cast<const ProgHeader*>(blob.data() + lay.header);
    std::memcpy(level_item, H.level_item, sizeof(H.level_item));
    const uint32_t n     = H.level_item[H.num_levels];
    const ProgItem* list = reinterpret_cast<const ProgItem*>(blob.data() + H.items_off); // (blob_in_tmp is 0 here)
    for (uint32_t i = 0; i < n && i < static_cast<uint32_t>(cap); ++i) items[2 * i] = list[i].scan, items[2 * i + 1] = list[i].seg;
    return static_cast<int>(n);
}

} // extern "C"
