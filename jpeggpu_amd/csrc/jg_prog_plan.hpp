// jg_prog_plan.hpp -- host side of a progressive image's part of the table blob (jg_prog_core.h): where the header, the
// scan descriptors, their tables, the segment lists and the work list lie, and their content. One routine for the
// decoder's plan (jg_plan.cpp) and for the host twin of the kernels (tests/emu), which therefore reads what the device reads.
#ifndef JG_PROG_PLAN_HPP_
#define JG_PROG_PLAN_HPP_

#include "jg_prog_core.h"
#include "jg_reader.hpp"

#include <cstring>
#include <vector>

namespace jg {

struct ProgBlobLayout {
    size_t header = 0, scans = 0, tables = 0, segments = 0, items = 0; // offsets inside the blob
    std::vector<ProgItem> work;                                       // the lanes' work, level by level
    uint32_t level_item[kMaxProgScans + 1] = {};
};

/// Where the rest of the image lies in d_tmp.
struct ProgPlacement {
    size_t blob_in_tmp;          // blob offsets + this = d_tmp offsets
    size_t bytes_off, bytes_len; // transferred entropy-coded bytes
    size_t coef_begin, coef_bytes;
    size_t coef[kMaxComp], sym[kMaxComp], du_tab[kMaxComp];
};

/// Carve the blob from offset `b` on (256-byte pieces) and build the work list: per level, the (scan, segment) pairs one
/// lane each takes. A scan of kProgLaneGroup segments or more starts a wave of its own (idle items pad the one in front);
/// the scans below that are grouped by kind, since the kinds diverge.
inline void prog_plan_blob(const Stream& s, ProgBlobLayout& L, size_t& b)
{
    const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    L.header = b;
    b += up(sizeof(ProgHeader));
    L.scans = b;
    b += up(s.prog_scans.size() * sizeof(ProgScanDesc));
    size_t tables = 0, segments = 0;
    for (const ProgScan& ps : s.prog_scans) {
        if (ps.kind != kProgDcRefine) tables += static_cast<size_t>(ps.num_comp);
        segments += ps.segments.size();
    }
    L.tables = b;
    b += up(tables * sizeof(ProgTable));
    L.segments = b;
    b += up(segments * sizeof(uint2_t));
    L.work.clear();
    for (int level = 0; level < s.num_levels; ++level) {
        const size_t first  = L.work.size();
        L.level_item[level] = static_cast<uint32_t>(first);
        const auto add      = [&](size_t k) {
            for (size_t g = 0; g < s.prog_scans[k].segments.size(); ++g) L.work.push_back(ProgItem{static_cast<uint32_t>(k), static_cast<uint32_t>(g)});
        };
        const auto large = [&](size_t k) { return s.prog_scans[k].segments.size() >= static_cast<size_t>(kProgLaneGroup); };
        for (size_t k = 0; k < s.prog_scans.size(); ++k) {
            if (s.prog_scans[k].level != level || !large(k)) continue;
            while ((L.work.size() - first) % kProgLaneGroup) L.work.push_back(ProgItem{kProgNoScan, 0u});
            add(k);
        }
        for (int kind = kProgDcFirst; kind <= kProgAcRefine; ++kind)
            for (size_t k = 0; k < s.prog_scans.size(); ++k)
                if (s.prog_scans[k].level == level && s.prog_scans[k].kind == kind && !large(k)) add(k);
    }
    L.level_item[s.num_levels] = static_cast<uint32_t>(L.work.size());
    L.items                    = b;
    b += up(L.work.size() * sizeof(ProgItem));
}

/// Fill the (zeroed) blob at `blob`.
inline void prog_fill_blob(const Stream& s, const ProgBlobLayout& L, const ProgPlacement& at, uint8_t* blob)
{
    const size_t B = at.blob_in_tmp;
    ProgHeader& H  = *reinterpret_cast<ProgHeader*>(blob + L.header);
    H.bytes_off  = static_cast<uint32_t>(at.bytes_off);
    H.bytes_len  = static_cast<uint32_t>(at.bytes_len);
    H.num_scans  = static_cast<uint32_t>(s.prog_scans.size());
    H.num_levels = static_cast<uint32_t>(s.num_levels);
    H.num_comp   = static_cast<uint32_t>(s.num_comp);
    H.scans_off  = static_cast<uint32_t>(B + L.scans);
    H.items_off  = static_cast<uint32_t>(B + L.items);
    H.coef_off   = at.coef_begin;
    H.coef_bytes = at.coef_bytes;
    std::memcpy(H.level_item, L.level_item, sizeof(H.level_item));
    uint32_t unit0 = 0;
    for (int c = 0; c < s.num_comp; ++c) {
        ProgComp& pc  = H.comp[c];
        pc.coef_off   = at.coef[c];
        pc.sym_off    = at.sym[c];
        pc.du_tab_off = at.du_tab[c];
        pc.blocks_x = s.prog_blocks_x[c], pc.blocks_y = s.prog_blocks_y[c];
        pc.vis_x = s.scans[c].mcus_x, pc.vis_y = s.scans[c].mcus_y;
        pc.unit0 = unit0;
        unit0 += static_cast<uint32_t>(s.scans[c].num_du);
    }
    H.pack_units = unit0;
    if (!L.work.empty()) std::memcpy(blob + L.items, L.work.data(), L.work.size() * sizeof(ProgItem));
    size_t tab = L.tables, seg = L.segments;
    for (size_t k = 0; k < s.prog_scans.size(); ++k) {
        const ProgScan& ps = s.prog_scans[k];
        ProgScanDesc& sd   = reinterpret_cast<ProgScanDesc*>(blob + L.scans)[k];
        sd.kind = static_cast<uint8_t>(ps.kind), sd.num_comp = static_cast<uint8_t>(ps.num_comp);
        sd.ss = static_cast<uint8_t>(ps.ss), sd.se = static_cast<uint8_t>(ps.se), sd.al = static_cast<uint8_t>(ps.al);
        sd.level = static_cast<uint8_t>(ps.level), sd.du_per_mcu = static_cast<uint8_t>(ps.du_per_mcu);
        int du = 0;
        for (int a = 0; a < ps.num_comp; ++a) {
            const ScanComponent& c = ps.comp[a];
            for (int y = 0; y < c.v; ++y)
                for (int x = 0; x < c.h; ++x, ++du) // row-major inside the MCU (T.81 A.2.3)
                    sd.du_comp[du] = static_cast<uint8_t>(a), sd.du_dx[du] = static_cast<uint8_t>(x), sd.du_dy[du] = static_cast<uint8_t>(y);
            sd.h[a] = static_cast<uint8_t>(c.h), sd.v[a] = static_cast<uint8_t>(c.v);
            sd.coef_off[a] = at.coef[c.comp_idx];
            sd.blocks_x[a] = s.prog_blocks_x[c.comp_idx];
            if (ps.kind != kProgDcRefine) {
                sd.tab_off[a] = static_cast<uint32_t>(B + tab);
                std::memcpy(blob + tab, &ps.table[a], sizeof(ProgTable));
                tab += sizeof(ProgTable);
            }
        }
        sd.mcus_x = ps.mcus_x, sd.mcus_y = ps.mcus_y, sd.mcus_per_segment = ps.mcus_per_segment;
        sd.num_segments = static_cast<int32_t>(ps.segments.size());
        sd.seg_off      = static_cast<uint32_t>(B + seg);
        if (!ps.segments.empty()) std::memcpy(blob + seg, ps.segments.data(), ps.segments.size() * sizeof(uint2_t));
        seg += ps.segments.size() * sizeof(uint2_t);
    }
}

} // namespace jg

#endif // JG_PROG_PLAN_HPP_
