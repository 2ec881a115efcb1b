// syncprobe.cpp -- host-only probe of the SYNC pack (jg_defs.h) for CPU tests: the widened first level of a code table
// as the product's own builder makes it (jg_reader.cpp: build_huff_table + widen_huff_table), and the number of steps
// the state-only symbol loop (jg_huff_core.h, decode_subsequence) takes over a scan with it. Compiled with g++ from the
// product's sources the way tests/emu is.
//
// Two things here are restatements and not the product's code, and each is checked against it:
//   * strict_high_halves: the rule the multi-symbol entries were built by before their last symbol was allowed to end
//     behind the index bits (every symbol wholly inside the index), from the low halves alone -- the yardstick the
//     step counts of the relaxed rule are compared with;
//   * count_subsequence: decode_subsequence's two loops with counters in place of the sums. Every subsequence is also
//     decoded by decode_subsequence itself, and probe_count_steps reports how many exit states differed (none may).
#include "jg_huff_core.h"
#include "jg_reader.hpp"

#include <cstring>
#include <vector>

using namespace jg;

namespace {

struct HostFetch { // the segment's destuffed bytes, linear; zero outside (as tests/emu)
    const uint8_t* seg;
    int seg_words;
    typedef int Pos;
    Pos start(int w) const { return w; }
    void advance(Pos& q) const { ++q; }
    uint32_t load(const Pos& w) const
    {
        if (w < 0 || w >= seg_words) return 0;
        const uint8_t* p = seg + static_cast<size_t>(w) * 4;
        return static_cast<uint32_t>(p[0]) << 24 | p[1] << 16 | p[2] << 8 | p[3];
    }
    uint32_t cook(uint32_t v, const Pos&) const { return v; }
};

/// High halves of an AC first level by the STRICT rule: as many symbols as lie, code and magnitude bits, inside the index.
void strict_high_halves(uint32_t* wide)
{
    const uint32_t lb = kLutBitsAc, n = 1u << lb;
    for (uint32_t idx = 0; idx < n; ++idx) {
        const uint32_t single = wide[idx] & 0xFFFFu;
        uint32_t multi        = single;
        if ((single & 31u) != 0) {
            uint32_t bits = 0, pre = 0, total_adv = 0;
            int count = 0;
            while (true) {
                const uint32_t e   = wide[(idx << bits) & (n - 1u)] & 0xFFFFu;
                const uint32_t len = e & 31u, adv = e >> 9;
                if (len == 0 || bits + len > lb) break;
                if (count > 0 && total_adv > static_cast<uint32_t>(kMultiMaxPre)) break;
                pre = total_adv;
                total_adv += adv;
                bits += len;
                ++count;
                if (adv == kEobAdvance) break;
            }
            if (count >= 2) multi = bits | pre << 5 | total_adv << 9;
        }
        wide[idx] = single | multi << 16;
    }
}

struct Counts {
    long long steps, main_steps, multi_steps;
};

/// decode_subsequence (SpecSink: states only) with counters. `single_only`: every step takes the low half, so steps == symbols.
void count_subsequence(LaneState& st, const HostFetch& fetch, int end_bit, const uint8_t* tabs, const ScanParams& sp, bool single_only, Counts& k)
{
    BitWindow<HostFetch> bw;
    bw.seek(st.p, fetch);
    CursorEntry cur = *reinterpret_cast<const CursorEntry*>(tabs + sp.cursor_off + 16u * static_cast<uint32_t>(st.c));
    int p = st.p, zm = st.z - 1;
    bool is_dc = st.z == 0;
    uint32_t peek = 0, e = 0;
    const auto commit = [&]() {
        const int total = e & 31;
        bw.skip(total);
        p += total;
        const int zp      = zm + static_cast<int>(e >> 9);
        const bool du_end = zp >= 63;
        zm                = du_end ? -1 : zp;
        cur               = *reinterpret_cast<const CursorEntry*>(tabs + (du_end ? cur.next : cur.self));
        is_dc             = du_end;
    };
    while (end_bit - p >= 31) {
        peek               = bw.peek(fetch);
        const uint8_t* tab = tabs + (is_dc ? (cur.tabs & 0xFFFFu) : (cur.tabs >> 16));
        const uint32_t idx = peek >> (is_dc ? 32 - kLutBitsDc : 32 - kLutBitsAc);
        const uint32_t e32 = ld_u32(tab + kSyncEntryBytes * idx);
        const uint32_t one = e32 & 0xFFFFu, m = e32 >> 16;
        const bool high    = !single_only && zm + static_cast<int>((m >> 5) & 15u) < 63;
        e                  = high ? m : one;
        if ((one & 31u) == 0) e = huff_second_level<kSyncEntryBytes>(tab, one, peek, is_dc);
        ++k.steps;
        ++k.main_steps;
        k.multi_steps += high && m != one;
        commit();
    }
    const auto lookup = [&]() {
        peek               = bw.peek(fetch);
        const uint8_t* tab = tabs + (is_dc ? (cur.tabs & 0xFFFFu) : (cur.tabs >> 16));
        const uint32_t idx = peek >> (is_dc ? 32 - kLutBitsDc : 32 - kLutBitsAc);
        e                  = ld_u16(tab + kSyncEntryBytes * idx);
        if ((e & 31u) == 0) e = huff_second_level<kSyncEntryBytes>(tab, e, peek, is_dc);
    };
    lookup();
    while (p + static_cast<int>(e & 31u) <= end_bit) {
        ++k.steps;
        commit();
        lookup();
    }
    st.p = p;
    st.z = zm + 1;
    st.c = (cur.meta >> 8) & 0xFF;
}

void destuff(const uint8_t* bytes, const Scan& sc, int subseq_bytes, std::vector<uint8_t>& dst)
{
    dst.assign(static_cast<size_t>(sc.num_subseq) * subseq_bytes + 256, 0);
    for (const DestuffChunk& ck : sc.chunks) {
        uint32_t o = ck.dst_off;
        for (uint32_t pos = ck.begin; pos < ck.end; ++pos) {
            uint32_t p = pos > 0 ? bytes[pos - 1] : 0;
            if (ck.first && pos == ck.begin) p = 0;
            const uint32_t b = bytes[pos];
            if (p == 0xFF && b == 0) dst[o++] = 0xFF;
            else if (p != 0xFF && b != 0xFF) dst[o++] = static_cast<uint8_t>(b);
        }
    }
}

} // namespace

extern "C" {

int probe_lut_entries(int is_dc) { return 1 << (is_dc ? kLutBitsDc : kLutBitsAc); }

/// The 32-bit first-level entries of the sync-pack form of the table of a DHT payload (`bits`: 16 counts, `vals`: `count`
/// values), built by the product; `strict` != 0: with the high halves of the strict rule (AC tables).
int probe_widen(const uint8_t* bits, const uint8_t* vals, int count, int is_dc, int strict, uint32_t* out)
{
    uint8_t nc[16];
    std::memcpy(nc, bits, 16);
    std::vector<uint8_t> t, wide;
    build_huff_table(t, nc, vals, count, is_dc != 0);
    widen_huff_table(t, is_dc != 0, wide);
    std::memcpy(out, wide.data(), sizeof(uint32_t) * static_cast<size_t>(probe_lut_entries(is_dc)));
    if (strict && !is_dc) strict_high_halves(out);
    return 0;
}

/// Steps of the state-only loop over the first `max_segments` restart segments (0: all) of scan 0 of a file, every
/// subsequence decoded from its predecessor's true exit state as a flow does. out[0..2]: steps / main-loop steps /
/// steps that took a multi-symbol entry with the product's tables; [3..5] the same with the strict rule's; [6] symbols
/// (steps of a walk that takes single entries only); [7] subsequences walked; [8] exit states that differ between
/// decode_subsequence and any of the three counting walks (must be 0); [9] the largest total length of a multi-symbol
/// entry of the product's pack. Returns a jpeggpu_status.
int probe_count_steps(const uint8_t* data, size_t size, int subseq_bytes, int max_segments, long long* out)
{
    Reader rd;
    Logger log;
    const jpeggpu_status stat = rd.parse(data, size, subseq_bytes, log);
    if (stat != JPEGGPU_SUCCESS) return stat;
    const Stream& s = rd.s;
    const Scan& sc  = s.scans[0];
    std::vector<uint8_t> bytes(s.xfer_end - s.xfer_begin + 2 * kDestuffWin, 0);
    std::memcpy(bytes.data(), data + s.xfer_begin, s.xfer_end - s.xfer_begin);
    std::vector<uint8_t> dst;
    destuff(bytes.data(), sc, subseq_bytes, dst);

    ScanParams sp{};
    sp.du_per_mcu      = sc.du_per_mcu;
    sp.num_comp        = sc.num_comp;
    sp.subseq_words    = subseq_bytes / 4;
    sp.tab_bytes_sync  = static_cast<uint32_t>(sc.table_pack_sync.size());
    sp.cursor_off_sync = sc.cursor_off_sync;
    sp.use_sync_pack();
    const std::vector<uint8_t>& relaxed = sc.table_pack_sync;
    std::vector<uint8_t> strict         = relaxed;
    long long longest = 0;
    {
        const CursorEntry* ring = reinterpret_cast<const CursorEntry*>(relaxed.data() + sp.cursor_off);
        std::vector<uint32_t> done;
        for (int d = 0; d < sc.du_per_mcu; ++d) {
            const uint32_t off = ring[d].tabs >> 16;
            bool seen = false;
            for (uint32_t o : done) seen |= o == off;
            if (seen) continue;
            done.push_back(off);
            strict_high_halves(reinterpret_cast<uint32_t*>(strict.data() + off));
            const uint32_t* w = reinterpret_cast<const uint32_t*>(relaxed.data() + off);
            for (uint32_t i = 0; i < (1u << kLutBitsAc); ++i)
                if ((w[i] >> 16) != (w[i] & 0xFFFFu) && ((w[i] >> 16) & 31u) > longest) longest = (w[i] >> 16) & 31u;
        }
    }
    Counts kr{}, ks{}, k1{};
    long long subs = 0, bad = 0;
    const int bits = subseq_bytes * 8, W = subseq_bytes / 4;
    const int G = static_cast<int>(sc.segments.size());
    for (int g = 0; g < G && (max_segments <= 0 || g < max_segments); ++g) {
        const Segment seg = sc.segments[g];
        HostFetch f{dst.data() + static_cast<size_t>(seg.subseq_offset) * subseq_bytes, seg.subseq_count * W};
        LaneState ref{};
        for (int rel = 0; rel < seg.subseq_count; ++rel, ++subs) {
            LaneState a = ref, b = ref, c = ref;
            BitWindow<HostFetch> bw;
            bw.seek(ref.p, f);
            SpecSink sink;
            decode_subsequence(ref, bw, f, (rel + 1) * bits, relaxed.data(), sp, sink);
            count_subsequence(a, f, (rel + 1) * bits, relaxed.data(), sp, false, kr);
            count_subsequence(b, f, (rel + 1) * bits, strict.data(), sp, false, ks);
            count_subsequence(c, f, (rel + 1) * bits, relaxed.data(), sp, true, k1);
            for (const LaneState* x : {&a, &b, &c}) bad += x->p != ref.p || x->c != ref.c || x->z != ref.z;
        }
    }
    out[0] = kr.steps, out[1] = kr.main_steps, out[2] = kr.multi_steps;
    out[3] = ks.steps, out[4] = ks.main_steps, out[5] = ks.multi_steps;
    out[6] = k1.steps, out[7] = subs, out[8] = bad, out[9] = longest;
    return JPEGGPU_SUCCESS;
}

} // extern "C"
