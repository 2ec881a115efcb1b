// jg_prog_core.h -- progressive (SOF2) entropy decoding, shared by the gfx950 kernels (jg_prog.hip) and their host twin
// (tests/emu): the descriptors that travel in the table blob, the bit reader that destuffs while it refills, the Huffman
// symbol step and the four scan bodies of T.81 Annex G (the arithmetic of libjpeg's jdphuff.c), and the routine that
// turns a finished block into the symbol stream the IDCT stage reads (jg_defs.h).
//
// The unit of work is one restart segment of one scan: an AC refinement scan cannot be entered anywhere else (how many
// correction bits a block takes depends on which of its coefficients earlier scans made non-zero), and the scans of one
// image depend on each other through the coefficient buffer. Scans get LEVELS at parse time (jg_reader.cpp): scans of
// one level write disjoint coefficients, so one launch decodes all of them and stream order carries the rest.
#ifndef JG_PROG_CORE_H_
#define JG_PROG_CORE_H_

#include "jg_defs.h"
#include "jg_huff_core.h"

namespace jg {

constexpr int kMaxProgScans  = 64;
constexpr int kProgLaneGroup = 64; // lanes of a wave: a scan of that many segments starts a wave of its own (ProgItem list)

/// Scan kinds; lanes of different kinds diverge, so the work list of a level is ordered by kind.
enum ProgKind : uint8_t { kProgDcFirst = 0, kProgDcRefine = 1, kProgAcFirst = 2, kProgAcRefine = 3 };

/// Huffman table of a progressive scan. The symbol semantics differ from baseline's (an AC symbol with s == 0 and r < 15
/// is an end-of-band RUN), so there is no pre-digested zig-zag advance: a first-level look-up on kProgLookBits bits gives
/// {code length << 8 | symbol}, 0 for a longer code, and the canonical walk of T.81 F.2.2.3 -- as left-aligned limits, the
/// form of jg_defs.h's lim16 -- stands behind it.
constexpr int kProgLookBits = 9;
struct ProgTable {
    uint16_t look[1 << kProgLookBits];
    uint32_t lim[17];    // [l]: first 16-bit window value NOT covered by codes of length <= l (up to 0x10000)
    int32_t valoff[17];  // [l]: huffval index of the first code of length l minus that code
    uint8_t huffval[256];
    uint8_t pad_[8];
};
static_assert(sizeof(ProgTable) % 16 == 0, "tables follow each other in the blob");

/// One scan of a progressive image, as the device reads it from the image's table blob. Offsets are byte offsets inside
/// the image's d_tmp (ProgHeader below says where that starts).
struct ProgScanDesc {
    uint8_t kind;     // ProgKind
    uint8_t num_comp; // 1..4 (more than one: an interleaved DC scan)
    uint8_t ss, se, al;
    uint8_t level;
    uint8_t du_per_mcu;
    uint8_t pad_;
    uint8_t du_comp[kMaxDuPerMcu]; // scan-component index, block column and block row of each data unit of the MCU
    uint8_t du_dx[kMaxDuPerMcu];
    uint8_t du_dy[kMaxDuPerMcu];
    uint8_t pad2_[2];
    uint8_t h[kMaxComp], v[kMaxComp]; // blocks per MCU of each scan component (1, 1 when not interleaved)
    uint32_t tab_off[kMaxComp];       // the component's ProgTable for this scan (DC scans: DC table, AC scans: AC table; DC refinement: none)
    uint64_t coef_off[kMaxComp];      // the component's coefficient buffer
    int32_t blocks_x[kMaxComp];       // its row length in blocks (the MCU-padded grid)
    int32_t mcus_x, mcus_y;           // MCUs of this scan (not interleaved: the component's ceil(size / 8) blocks)
    int32_t mcus_per_segment;         // restart interval, or all MCUs
    int32_t num_segments;
    uint32_t seg_off;                 // uint2_t[num_segments]: first byte / one past the last byte of each segment, in the transferred bytes
    uint32_t pad3_;
};
static_assert(sizeof(ProgScanDesc) % 8 == 0, "an array in the blob");

/// One lane's work: restart segment `seg` of scan `scan` (kProgNoScan: an idle lane that pads a wave).
struct ProgItem {
    uint32_t scan;
    uint32_t seg;
};
constexpr uint32_t kProgNoScan = 0xFFFFFFFFu;

/// The hand-over (jg_defs.h: symbol stream and data-unit table): every visible block of a component is one data unit of a
/// non-interleaved baseline scan and gets a region of its own, kProgRegionEntries entries -- the most a unit can hold
/// (kMaxUnitEntries) rounded up to whole sectors. 256 bytes of stream plus 8 of table per visible block; a unit never
/// spans regions because every region holds exactly one.
constexpr uint32_t kProgRegionEntries = (kMaxUnitEntries + kSymSectorEntries - 1) / kSymSectorEntries * kSymSectorEntries;
static_assert(kProgRegionEntries == 128, "eight sectors");

struct ProgComp {
    uint64_t coef_off;   // int16[blocks_y][blocks_x][64], natural order inside a block
    uint64_t sym_off;    // the symbol stream and the data-unit table of the component's job
    uint64_t du_tab_off;
    int32_t blocks_x, blocks_y; // MCU-padded grid
    int32_t vis_x, vis_y;       // ceil(size / 8)
    uint32_t unit0;             // first pack unit of the component (units are counted over all components)
    uint32_t pad_;
};

/// Head of a progressive image's part of the table blob.
struct ProgHeader {
    uint32_t bytes_off, bytes_len; // transferred entropy-coded bytes
    uint32_t num_scans, num_levels, num_comp;
    uint32_t scans_off;            // ProgScanDesc[num_scans]
    uint32_t items_off;            // ProgItem[level_item[num_levels]], level by level
    uint32_t pack_units;           // visible blocks of all components
    uint64_t coef_off, coef_bytes; // all coefficient buffers, zeroed at the start of every decode
    uint32_t level_item[kMaxProgScans + 1];
    uint32_t pad_;
    ProgComp comp[kMaxComp];
};
static_assert(sizeof(ProgHeader) % 8 == 0, "holds 64-bit offsets");

/// What a launch gets per image: its d_tmp and where the header sits in it.
struct ProgImage {
    uint8_t* tmp;
    uint64_t hdr_off;
};

/// Build a ProgTable from a DHT payload (16 counts, then the values).
inline void build_prog_table(ProgTable& t, const uint8_t* counts, const uint8_t* vals, int nvals)
{
    t = ProgTable{};
    for (int i = 0; i < nvals && i < 256; ++i) t.huffval[i] = vals[i];
    uint32_t code = 0;
    int idx       = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = idx - static_cast<int32_t>(code);
        for (int i = 0; i < counts[l - 1] && idx < 256; ++i, ++idx, ++code) {
            if (l <= kProgLookBits) {
                const uint32_t lo = code << (kProgLookBits - l);
                for (uint32_t j = 0; j < (1u << (kProgLookBits - l)); ++j)
                    t.look[(lo + j) & ((1u << kProgLookBits) - 1u)] = static_cast<uint16_t>(l << 8 | t.huffval[idx]);
            }
        }
        const uint32_t left = code << (16 - l);
        t.lim[l]            = left > 0x10000u ? 0x10000u : left;
        code <<= 1;
    }
}

/// Bit reader over one restart segment's bytes [p, end): 64-bit window, most significant bit first; destuffs while it
/// refills (a 0x00 behind 0xFF is dropped); a marker, or the end of the segment, ends the data and zero bits follow.
struct ProgBits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t win;
    int cnt; // valid bits at the top of win
    JG_HD inline void init(const uint8_t* b, const uint8_t* e)
    {
        p = b, end = e, win = 0, cnt = 0;
    }
    JG_HD inline void refill()
    {
        while (cnt <= 56) {
            uint32_t b = 0;
            if (p < end) {
                b = *p++;
                if (b == 0xFFu) {
                    if (p < end && *p == 0) ++p;
                    else b = 0, p = end; // a marker (or a lone FF at the end): nothing behind it is data
                }
            }
            win |= static_cast<uint64_t>(b) << (56 - cnt);
            cnt += 8;
        }
    }
    JG_HD inline void need(int n)
    {
        if (cnt < n) refill();
    }
    JG_HD inline uint32_t peek(int n) const { return static_cast<uint32_t>(win >> (64 - n)); } // 1 <= n <= 32
    JG_HD inline void skip(int n)
    {
        win <<= n;
        cnt -= n;
    }
    JG_HD inline uint32_t bit()
    {
        need(1);
        const uint32_t b = static_cast<uint32_t>(win >> 63);
        skip(1);
        return b;
    }
    /// n bits, 0 <= n <= 16, of a window that holds them (need(32) in front of a symbol covers code + magnitude)
    JG_HD inline uint32_t take(int n)
    {
        const uint32_t v = n ? static_cast<uint32_t>(win >> (64 - n)) : 0u;
        skip(n);
        return v;
    }
};

/// One Huffman symbol (the window holds 16 bits). A window no code matches is taken as a 16-bit code of symbol 0.
JG_HD inline uint32_t prog_symbol(ProgBits& br, const ProgTable* t)
{
    const uint32_t e = t->look[br.peek(kProgLookBits)];
    if (e != 0) {
        br.skip(static_cast<int>(e >> 8));
        return e & 0xFFu;
    }
    const uint32_t v = br.peek(16);
    for (int l = kProgLookBits + 1; l <= 16; ++l) {
        if (v < t->lim[l]) {
            br.skip(l);
            return t->huffval[static_cast<uint32_t>(t->valoff[l] + static_cast<int32_t>(v >> (16 - l))) & 255u];
        }
    }
    br.skip(16);
    return 0;
}

/// T.81 F.2.2.1 EXTEND of an s-bit magnitude.
JG_HD inline int prog_extend(uint32_t v, int s) { return s && v < (1u << (s - 1)) ? static_cast<int>(v) - (1 << s) + 1 : static_cast<int>(v); }

/// Per-lane state of a segment's decode: where it is in the segment's blocks, and what the format carries across blocks.
struct ProgLane {
    ProgBits br;
    int mcu, mcu_end; // MCU at hand, one past the segment's last
    int mx, my;       // its column and row in the scan's MCU grid
    int j;            // data unit inside the MCU (interleaved DC scans)
    int k;            // zig-zag index inside the band (AC scans)
    int eobrun;       // blocks an end-of-band run still covers, the one at hand included
    int pred0, pred1, pred2, pred3; // DC predictors per scan component (scalars: an indexed array would live in scratch memory)
};

JG_HD inline int16_t* prog_block(const ProgScanDesc& sd, uint8_t* tmp, const ProgLane& L, int a, int dx, int dy)
{
    const int64_t bx = static_cast<int64_t>(L.mx) * sd.h[a] + dx, by = static_cast<int64_t>(L.my) * sd.v[a] + dy;
    return reinterpret_cast<int16_t*>(tmp + sd.coef_off[a]) + (by * sd.blocks_x[a] + bx) * 64;
}

/// The next data unit: the next one of the MCU, or the first of the next MCU (raster order over the scan's grid).
JG_HD inline void prog_next_unit(const ProgScanDesc& sd, ProgLane& L)
{
    if (++L.j < sd.du_per_mcu) return;
    L.j = 0;
    ++L.mcu;
    if (++L.mx == sd.mcus_x) L.mx = 0, ++L.my;
}

JG_HD inline void prog_lane_init(const ProgScanDesc& sd, const uint8_t* bytes, uint32_t bytes_len, uint2_t range, int seg, ProgLane& L)
{
    // (a range outside the transferred bytes cannot come from the parser; a lane must not follow one all the same)
    const uint32_t b = range.x < bytes_len ? range.x : bytes_len, e = range.y < bytes_len ? range.y : bytes_len;
    L.br.init(bytes + b, bytes + (e > b ? e : b));
    const int total = sd.mcus_x * sd.mcus_y;
    L.mcu           = seg * sd.mcus_per_segment;
    if (L.mcu > total) L.mcu = total;
    L.mcu_end = L.mcu + sd.mcus_per_segment;
    if (L.mcu_end > total || L.mcu_end < L.mcu) L.mcu_end = total;
    L.my = L.mcu / sd.mcus_x, L.mx = L.mcu - L.my * sd.mcus_x;
    L.j = 0, L.k = sd.ss, L.eobrun = 0;
    L.pred0 = L.pred1 = L.pred2 = L.pred3 = 0;
}

/// ONE step of a lane: a block of a DC scan, a symbol (or a block inside an end-of-band run) of an AC scan. Returns false
/// when the segment's blocks are done. Every step either finishes a block or moves k forward, so a segment of n blocks
/// takes at most 65 n steps whatever its bits are; k never passes Se, and a block index never leaves the segment.
JG_HD inline bool prog_step(const ProgScanDesc& sd, uint8_t* tmp, ProgLane& L)
{
    if (L.mcu >= L.mcu_end) return false;
    ProgBits& br = L.br;
    const int a  = sd.du_comp[L.j];
    int16_t* blk = prog_block(sd, tmp, L, a, sd.du_dx[L.j], sd.du_dy[L.j]);
    const int al = sd.al;
    constexpr int kNat[64] = JG_ORDER_NATURAL;
    switch (sd.kind) {
    case kProgDcFirst: {
        br.need(32);
        const int s    = static_cast<int>(prog_symbol(br, reinterpret_cast<const ProgTable*>(tmp + sd.tab_off[a])) & 15u);
        const int diff = prog_extend(br.take(s), s);
        int pred       = a == 0 ? L.pred0 : a == 1 ? L.pred1 : a == 2 ? L.pred2 : L.pred3;
        pred += diff;
        if (a == 0) L.pred0 = pred;
        else if (a == 1) L.pred1 = pred;
        else if (a == 2) L.pred2 = pred;
        else L.pred3 = pred;
        blk[0] = static_cast<int16_t>(static_cast<uint32_t>(pred) << al);
        prog_next_unit(sd, L);
        return true;
    }
    case kProgDcRefine:
        if (br.bit()) blk[0] = static_cast<int16_t>(blk[0] | (1 << al));
        prog_next_unit(sd, L);
        return true;
    case kProgAcFirst: {
        if (L.eobrun > 0) { // the rest of this block's band stays zero
            --L.eobrun;
            L.k = sd.ss;
            prog_next_unit(sd, L);
            return true;
        }
        br.need(32);
        const uint32_t sym = prog_symbol(br, reinterpret_cast<const ProgTable*>(tmp + sd.tab_off[0]));
        const int r = static_cast<int>(sym >> 4), s = static_cast<int>(sym & 15u);
        if (s) {
            L.k += r;
            const int v = prog_extend(br.take(s), s);
            if (L.k <= sd.se) blk[kNat[L.k]] = static_cast<int16_t>(static_cast<uint32_t>(v) << al);
            ++L.k;
        } else if (r == 15) {
            L.k += 16;
        } else { // EOBr: this block and (1 << r) + bits - 1 more; a run never crosses a restart
            L.eobrun = (1 << r) + static_cast<int>(br.take(r));
            const int left = L.mcu_end - L.mcu;
            if (L.eobrun > left) L.eobrun = left;
            return true;
        }
        if (L.k > sd.se) {
            L.k = sd.ss;
            prog_next_unit(sd, L);
        }
        return true;
    }
    default: { // kProgAcRefine
        const int p1 = 1 << al, m1 = -(1 << al);
        // a correction bit moves an already non-zero coefficient away from zero by p1, if that bit of it is still clear
        const auto correct = [&](int16_t* c) {
            if (br.bit() && (*c & p1) == 0) *c = static_cast<int16_t>(*c + (*c >= 0 ? p1 : m1));
        };
        if (L.eobrun > 0) { // every non-zero coefficient in the rest of the band takes a correction bit
            for (; L.k <= sd.se; ++L.k) {
                int16_t* c = blk + kNat[L.k];
                if (*c != 0) correct(c);
            }
            --L.eobrun;
            L.k = sd.ss;
            prog_next_unit(sd, L);
            return true;
        }
        br.need(32);
        const uint32_t sym = prog_symbol(br, reinterpret_cast<const ProgTable*>(tmp + sd.tab_off[0]));
        int r = static_cast<int>(sym >> 4), s = static_cast<int>(sym & 15u);
        if (s) {
            s = br.bit() ? p1 : m1; // the new coefficient's sign, read BEFORE the run is skipped (a size other than 1 is corrupt data)
        } else if (r != 15) {
            L.eobrun = (1 << r) + static_cast<int>(br.take(r));
            const int left = L.mcu_end - L.mcu;
            if (L.eobrun > left) L.eobrun = left;
            return true; // the next step finishes this block's band inside the run
        }
        // pass r coefficients with a zero history (ZRL: 16 of them); every non-zero one on the way is corrected
        for (; L.k <= sd.se; ++L.k) {
            int16_t* c = blk + kNat[L.k];
            if (*c != 0) correct(c);
            else if (--r < 0) break;
        }
        if (s && L.k <= sd.se) blk[kNat[L.k]] = static_cast<int16_t>(s);
        ++L.k;
        if (L.k > sd.se) {
            L.k = sd.ss;
            prog_next_unit(sd, L);
        }
        return true;
    }
    }
}

/// Upper bound of the steps of a segment (prog_step): the loop that drives a lane stops there whatever the data says.
JG_HD inline int64_t prog_max_steps(const ProgScanDesc& sd, const ProgLane& L)
{
    return static_cast<int64_t>(L.mcu_end - L.mcu) * sd.du_per_mcu * 66 + 1;
}

/// The symbol stream of one finished block (jg_defs.h): DC first, absolute; one entry per non-zero AC coefficient, an
/// escape entry behind one that does not fit ten bits. Writes at most kMaxUnitEntries entries of the region that starts
/// at physical index `base` and returns the data-unit record.
template <class Store>
JG_HD inline uint2_t prog_pack_block(const int16_t* blk, uint32_t base, Store&& store)
{
    constexpr int kNat[64] = JG_ORDER_NATURAL;
    uint32_t n = 0, esc = 0;
    store(sym_at(base, n++), static_cast<uint16_t>(blk[0]));
    for (int z = 1; z < 64; ++z) {
        const int v = blk[kNat[z]];
        if (v == 0) continue;
        store(sym_at(base, n++), static_cast<uint16_t>(sym_entry_ac(z, v)));
        if (sym_needs_escape(v)) {
            store(sym_at(base, n++), static_cast<uint16_t>(sym_entry_escape(v)));
            esc = kUnitHasEscape;
        }
    }
    return uint2_t{base, n | esc};
}

} // namespace jg

#endif // JG_PROG_CORE_H_
