// jg_encode_prog.hip -- progressive JPEG encoding for gfx950 (jcphuff.c on libjpeg's jpeg_simple_progression script): ELEVEN
// launches for all scans of all progressive items of a call, behind the encode_blocks launch that the call runs anyway,
// whatever the number of items, their sizes and the number of their scans.
//
//   P1  prog_facts        one lane per scan block (jg_encode_prog.hpp): does the block code a newly non-zero coefficient
//                         of its scan's band, does the band end in an end-of-band run, how many correction bits trail;
//                         one byte. It zeroes the run length of every block, and the item's first tile its symbol counts.
//   P2  prog_runs         the one thing that crosses blocks. A run begins where a block joins and no run is pending, and
//                         ends before the next block with a new coefficient, at the segment's end, at 0x7FFF blocks or at
//                         more than 937 pending correction bits. The lane of each block that has a new coefficient or
//                         opens a segment walks the facts up to the next such block, eight blocks a step where nothing
//                         happens, and leaves at every block that OPENS a run the run's length.
//   P3  prog_symbols      one lane per scan block: its symbols, the EOBn of a run it opens included, into a histogram of
//                         the tile in LDS and from there into the counts of the scan's table
//   P4  build_prog_tables (jg_encode.hip) one wave per item and table: jpeg_gen_optimal_table, codes and the DHT segment
//   P5  prog_count_bits   one lane per scan block: its bit count, and the tile's cursor function
//   P6  scan<Cursor>      (jg_encode.hip)
//   P7  clear_streams     (jg_encode.hip)
//   P8  prog_pack         one lane per scan block: its codes at its bit offset -- coefficient symbols, then the EOBn symbol
//                         of the run it opens, then its own trailing correction bits, so that the bits of a run's later
//                         blocks follow in place. Leaves the byte at which each scan begins.
//   P9  count_bytes       (jg_encode.hip)
//   P10 scan<Count>       (jg_encode.hip)
//   P11 prog_write_files  sizes and the capacity test first; then SOI .. SOF2, and per scan its DHTs and SOS (the DRI before
//                         the first SOS) in front of its stuffed bytes; RSTn counted from 0 in every scan; EOI
//
// P3, P5 and P8 run ONE coder (code_block) on three sinks, so what is counted is what is written.
//
// The small device functions of the cursor algebra, the bit writer and the byte stages are restated from jg_encode.hip,
// whose kernels stay as they are.
#include "jg_encode_prog.hpp"

#include <hip/hip_runtime.h>

namespace jg {
namespace enc {
namespace {

__device__ inline uint32_t roundup8(uint32_t x) { return (x + 7u) & ~7u; }
__device__ inline uint32_t apply(Cursor f, uint32_t x)
{
    return f.kind == kAdd ? x + f.a : f.kind == kRound ? roundup8(x + f.a) + f.b : f.b;
}
__device__ inline Cursor compose(Cursor f, Cursor g)
{
    if (g.kind == kConst) return g;
    if (f.kind == kConst) return Cursor{kConst, 0u, apply(g, f.b)};
    if (g.kind == kAdd) return f.kind == kAdd ? Cursor{kAdd, f.a + g.a, 0u} : Cursor{kRound, f.a, f.b + g.a};
    if (f.kind == kAdd) return Cursor{kRound, f.a + g.a, g.b};
    return Cursor{kRound, f.a, roundup8(f.b + g.a) + g.b};
}
__device__ inline Count compose(Count f, Count g)
{
    return g.reset ? g : Count{f.reset, f.ff + g.ff, f.starts + g.starts};
}
__device__ inline int item_of_tile(const Item* items, int n, uint32_t tile)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].tile_start <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ inline int item_of_chunk(const Item* items, int n, uint32_t chunk)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].chunk_start <= chunk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ inline uint32_t stream_bytes(const Item* items, int i, const Cursor* tile_sum, const Cursor* tile_before)
{
    const uint32_t last = items[i + 1].tile_start - 1;
    return (apply(compose(tile_before[last], tile_sum[last]), 0u) + 7u) >> 3;
}
__device__ inline int category(int v) { return 32 - __clz(abs(v)); }

__device__ inline Cursor scan_cursors(Cursor* lds, Cursor mine)
{
    lds[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < kTileBlocks; off <<= 1) {
        Cursor v = lds[threadIdx.x];
        if (int(threadIdx.x) >= off) v = compose(lds[threadIdx.x - off], v);
        __syncthreads();
        lds[threadIdx.x] = v;
        __syncthreads();
    }
    return lds[threadIdx.x];
}

struct BitWriter {
    uint32_t* word;
    uint64_t acc;
    int n;
    bool first;
    __device__ void put(uint32_t value, int len) // len <= 32, value < 2^len
    {
        acc = acc << len | value;
        n += len;
        if (n >= 32) {
            n -= 32;
            flush(uint32_t(acc >> n));
            acc &= (uint64_t(1) << n) - 1;
        }
    }
    __device__ void flush(uint32_t v)
    {
        v = __builtin_bswap32(v);
        if (first) {
            if (v) atomicOr(word, v);
        } else *word = v;
        first = false;
        ++word;
    }
    /// (The stream was cleared, so zeros need no write: the blocks inside an end-of-band run add no bits, thousands of them
    /// stand at ONE bit position, and their atomics on that dword would queue behind each other.)
    __device__ void finish()
    {
        if (n && acc) atomicOr(word, __builtin_bswap32(uint32_t(acc << (32 - n))));
    }
};

// ------------------------------------------------------------------------------------------------
// where a scan block lies
// ------------------------------------------------------------------------------------------------

constexpr int kLdsRow = 33; // dwords per block in LDS, as in jg_encode.hip

struct Where {
    const ProgScan* sc;
    int s, q;                         // the scan, and the block's number in it
    int b;                            // the block's coefficients: its place in the item's MCU stream
    bool segment_first, segment_last; // of a restart segment of THIS scan (or the scan)
    int table;                        // 0 luma, 1 chroma
    int pred;                         // DC scans: the previous block of its component in the segment, -1: none
};

/// p: the scan block's number in its item.
__device__ inline Where where_of(const ProgItem& pi, const Item& it, int p)
{
    Where w;
    w.s = 0;
    while (w.s + 1 < int(pi.scans_n) && pi.scans[w.s + 1].first <= uint32_t(p)) ++w.s;
    const ProgScan& sc = pi.scans[w.s];
    w.sc               = &sc;
    w.q                = p - int(sc.first);
    const int ri = it.restart_interval, bpm = it.blocks_per_mcu, luma = it.hs * it.vs;
    if (sc.comp < 0) { // MCU order over the padded grid, as jg_encode.hip's place_of
        const int mcu = w.q / bpm, j = w.q - mcu * bpm;
        const bool first_mcu = ri ? mcu % ri == 0 : mcu == 0;
        w.b             = w.q;
        w.segment_first = first_mcu && j == 0;
        w.segment_last  = w.q == sc.blocks - 1 || (ri && j == bpm - 1 && (mcu + 1) % ri == 0);
        if (it.hs == 0) { // the item's own frame (jg_encode.hpp: Frame), as place_of reads it
            const uint32_t m = uint32_t(it.frame.map >> (6 * j)) & 63u;
            w.table          = it.frame.select >> (m & 3u) & 1;
            w.pred           = m >> 2 ? w.b - 1 : first_mcu ? -1 : w.b - bpm + (int(it.frame.last >> (4 * j)) & 15);
            return w;
        }
        w.table         = j >= luma;
        if (j < luma && j > 0) w.pred = w.b - 1;
        else if (first_mcu) w.pred = -1;
        else w.pred = j < luma ? w.b - bpm + luma - 1 : w.b - bpm;
        return w;
    }
    // the component's real blocks row by row; an MCU of the scan is one block
    w.segment_first = ri ? w.q % ri == 0 : w.q == 0;
    w.segment_last  = w.q == sc.blocks - 1 || (ri && (w.q + 1) % ri == 0);
    w.table         = sc.comp > 0;
    if (it.hs == 0) { // the component's h x v blocks of an MCU begin at k0 (a single component's DC scans: b is q)
        const int by = w.q / sc.blocks_x, bx = w.q - by * sc.blocks_x;
        const int my = by / sc.v, mx = bx / sc.h;
        w.b     = (my * it.mcus_x + mx) * bpm + sc.k0 + (by - my * sc.v) * sc.h + (bx - mx * sc.h);
        w.table = it.frame.select >> sc.comp & 1;
    } else if (sc.comp == 0) {
        const int by = w.q / sc.blocks_x, bx = w.q - by * sc.blocks_x;
        w.b = ((by / it.vs) * it.mcus_x + bx / it.hs) * bpm + (by % it.vs) * it.hs + bx % it.hs;
    } else {
        w.b = w.q * bpm + luma + sc.comp - 1;
    }
    w.pred = w.segment_first ? -1 : w.b - 1; // (a DC scan of one component is a grey item's: b is q)
    return w;
}

/// The lane's block into its row of LDS: the 16-byte pieces that hold the scan's band. A DC scan reads nothing here.
__device__ inline void load_band(uint32_t* row, const uint8_t* scratch, const Item& it, const Where& w)
{
    if (w.sc->ss == 0) return;
    const uint4* src = reinterpret_cast<const uint4*>(scratch + it.coef_off) + size_t(w.b) * 8;
    for (int piece = w.sc->ss >> 3; piece <= w.sc->se >> 3; ++piece) {
        const uint4 v      = src[piece];
        row[4 * piece]     = v.x;
        row[4 * piece + 1] = v.y;
        row[4 * piece + 2] = v.z;
        row[4 * piece + 3] = v.w;
    }
}

// ------------------------------------------------------------------------------------------------
// the coder: jcphuff.c's four block routines on a sink
// ------------------------------------------------------------------------------------------------

/// Correction bits of a block that wait for its next symbol: at most 63.
struct Pending {
    uint64_t bits = 0;
    int n         = 0;
    template <class Sink>
    __device__ void emit(Sink& out)
    {
        if (n > 32) out.raw(uint32_t(bits >> 32), n - 32);
        if (n) out.raw(n >= 32 ? uint32_t(bits) : uint32_t(bits) & ((1u << n) - 1u), n > 32 ? 32 : n);
        bits = 0, n = 0;
    }
};

template <class Sink>
__device__ inline void emit_eobn(Sink& out, int slot, uint32_t run)
{
    const int nb = 31 - __clz(run);
    out.sym(slot, nb << 4);
    if (nb) out.raw(run & ((1u << nb) - 1u), nb);
}

/// c: the block's coefficients (AC scans); dc, dc_pred: its DC coefficient and its predecessor's (0: none), unshifted;
/// eobn: the length of the end-of-band run this block opens, 0: none.
template <class Sink>
__device__ inline void code_block(const Where& w, const int16_t* c, int dc, int dc_pred, uint32_t eobn, Sink& out)
{
    const ProgScan& sc = *w.sc;
    const int al = sc.al, slot = sc.slot;
    if (sc.ss == 0) {
        if (sc.ah) {
            out.raw(uint32_t(dc >> al) & 1u, 1);
            return;
        }
        const int diff = (dc >> al) - (dc_pred >> al); // arithmetic shifts
        const int s    = min(category(diff), 11); // (beyond 11: an uncodable transcode item, whose file is never written; its bits stay inside the bound)
        out.sym(slot + w.table, s);
        if (s) out.raw(uint32_t(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
        return;
    }
    int r = 0;
    if (sc.ah == 0) {
        for (int k = sc.ss; k <= sc.se; ++k) {
            const int v = c[k], mag = abs(v) >> al;
            if (mag == 0) {
                ++r;
                continue;
            }
            for (; r > 15; r -= 16) out.sym(slot, 0xF0);
            const int s = category(mag);
            out.sym(slot, r << 4 | s);
            out.raw(uint32_t(v < 0 ? ~mag : mag) & ((1u << s) - 1u), s);
            r = 0;
        }
        if (eobn) emit_eobn(out, slot, eobn);
        return;
    }
    int eob = 0; // the last coefficient that becomes non-zero in this scan: behind it no ZRL is sent
    for (int k = sc.ss; k <= sc.se; ++k)
        if (abs(int(c[k])) >> al == 1) eob = k;
    Pending pend;
    for (int k = sc.ss; k <= sc.se; ++k) {
        const int v = c[k], mag = abs(v) >> al;
        if (mag == 0) {
            ++r;
            continue;
        }
        while (r > 15 && k <= eob) {
            out.sym(slot, 0xF0);
            r -= 16;
            pend.emit(out);
        }
        if (mag > 1) { // already non-zero: one correction bit, behind the next symbol
            pend.bits = pend.bits << 1 | uint32_t(mag & 1);
            ++pend.n;
            continue;
        }
        out.sym(slot, r << 4 | 1);
        out.raw(v < 0 ? 0u : 1u, 1);
        pend.emit(out);
        r = 0;
    }
    if (eobn) emit_eobn(out, slot, eobn);
    pend.emit(out);
}

struct SymbolSink {
    uint32_t* hist; // [kProgSlots][256] in LDS
    __device__ void sym(int slot, int s) { atomicAdd(hist + slot * 256 + s, 1u); }
    __device__ void raw(uint32_t, int) {}
};
struct BitsSink {
    const uint32_t* tab; // [kProgSlots][256] in LDS: code << 8 | length
    uint32_t total;
    __device__ void sym(int slot, int s) { total += tab[slot * 256 + s] & 0xFFu; }
    __device__ void raw(uint32_t, int len) { total += uint32_t(len); }
};
struct PackSink {
    const uint32_t* tab;
    BitWriter bw;
    __device__ void sym(int slot, int s)
    {
        const uint32_t e = tab[slot * 256 + s];
        bw.put(e >> 8, int(e & 0xFFu));
    }
    __device__ void raw(uint32_t v, int len) { bw.put(v, len); }
};

/// What every scan-block kernel begins with.
struct Lane {
    const Item* it;
    const ProgItem* pi;
    int p;      // the scan block's number in its item
    bool valid; // the tile's last lanes may lie behind the item's scan blocks
};
__device__ inline Lane lane_of(const Item* shadow, const ProgItem* pitems, int n)
{
    const int i = item_of_tile(shadow, n, blockIdx.x);
    Lane l;
    l.it    = shadow + i;
    l.pi    = pitems + i;
    l.p     = int(blockIdx.x - shadow[i].tile_start) * kTileBlocks + int(threadIdx.x);
    const ProgScan& last = pitems[i].scans[pitems[i].scans_n - 1];
    l.valid = uint32_t(l.p) < last.first + uint32_t(last.blocks);
    return l;
}

constexpr uint8_t kFactNew = 0x80, kFactJoins = 0x40; // and the trailing correction bits below

// ------------------------------------------------------------------------------------------------
// P1 - P3
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kTileBlocks) void prog_facts(const Item* __restrict__ shadow, const ProgItem* __restrict__ pitems, int n, uint8_t* __restrict__ scratch,
                                                          uint8_t* __restrict__ facts, uint16_t* __restrict__ eobn)
{
    __shared__ uint32_t coefs[kTileBlocks * kLdsRow];
    const Lane l = lane_of(shadow, pitems, n);
    if (blockIdx.x == l.it->tile_start) {
        uint32_t* counts = &reinterpret_cast<ProgWork*>(scratch + l.pi->work_off)->counts[0][0];
        for (int i = threadIdx.x; i < int(l.pi->slots_n) * 256; i += kTileBlocks) counts[i] = 0u; // (the tables the item has)
    }
    if (!l.valid) return;
    const Where w      = where_of(*l.pi, *l.it, l.p);
    const ProgScan& sc = *w.sc;
    uint8_t fact       = 0;
    if (sc.ss) {
        uint32_t* row = coefs + threadIdx.x * kLdsRow;
        load_band(row, scratch, *l.it, w);
        const int16_t* c = reinterpret_cast<const int16_t*>(row);
        int last = 0, trailing = 0; // the last new coefficient, the already non-zero ones behind it
        for (int k = sc.ss; k <= sc.se; ++k) {
            const int mag = abs(int(c[k])) >> sc.al;
            if (sc.ah ? mag == 1 : mag != 0) last = k, trailing = 0;
            else if (sc.ah && mag > 1) ++trailing;
        }
        fact = uint8_t((last ? kFactNew : 0) | (last != sc.se ? kFactJoins : 0) | trailing);
    }
    facts[size_t(blockIdx.x) * kTileBlocks + threadIdx.x] = fact;
    eobn[size_t(blockIdx.x) * kTileBlocks + threadIdx.x]  = 0; // prog_runs marks the blocks that open a run
}

__global__ __launch_bounds__(kTileBlocks) void prog_runs(const Item* __restrict__ shadow, const ProgItem* __restrict__ pitems, int n, const uint8_t* __restrict__ facts,
                                                         uint16_t* __restrict__ eobn)
{
    const Lane l = lane_of(shadow, pitems, n);
    if (!l.valid) return;
    const Where w      = where_of(*l.pi, *l.it, l.p);
    const ProgScan& sc = *w.sc;
    const size_t at    = size_t(blockIdx.x) * kTileBlocks + threadIdx.x; // the lane's place in facts and eobn
    if (sc.ss == 0) return;
    if (!(facts[at] & kFactNew) && !w.segment_first) return; // the walker in front of it passes here
    const int ri       = l.it->restart_interval;
    const size_t first = at - size_t(w.q); // the scan's first block in facts and eobn
    uint16_t* out      = eobn + first;
    uint32_t run = 0, pending = 0;
    int opener   = 0;
    uint64_t word = 0; // the facts of eight blocks: the arrays start on a multiple of 256 bytes and are whole tiles long
    for (int q = w.q; q < sc.blocks;) {
        const size_t abs = first + size_t(q);
        if ((abs & 7u) == 0 || q == w.q) word = *reinterpret_cast<const uint64_t*>(facts + (abs & ~size_t(7)));
        // eight blocks of one segment that join with nothing new and nothing trailing, and no cap within reach: one step
        if ((abs & 7u) == 0 && q != w.q && word == 0x4040404040404040ull && q + 8 <= sc.blocks && run && run + 8 < kMaxEobRun &&
            (ri == 0 || (q % ri != 0 && q % ri + 8 <= ri))) {
            run += 8;
            q += 8;
            continue;
        }
        const uint8_t fact = uint8_t(word >> (8 * (abs & 7u)));
        if (q != w.q && ((fact & kFactNew) || (ri && q % ri == 0))) break;
        if (fact & kFactJoins) { // (only the walker's own block can be one that does not)
            if (run == 0) opener = q;
            ++run;
            pending += fact & 0x3Fu;
            if (run == kMaxEobRun || pending > kMaxPendingBits) {
                out[opener] = uint16_t(run);
                run = 0, pending = 0;
            }
        }
        ++q;
    }
    if (run) out[opener] = uint16_t(run);
}

__global__ __launch_bounds__(kTileBlocks) void prog_symbols(const Item* __restrict__ shadow, const ProgItem* __restrict__ pitems, int n, uint8_t* __restrict__ scratch,
                                                            const uint16_t* __restrict__ eobn, int slots)
{
    __shared__ uint32_t coefs[kTileBlocks * kLdsRow];
    extern __shared__ uint32_t hist[]; // [slots][256]
    const Lane l = lane_of(shadow, pitems, n);
    for (int i = threadIdx.x; i < slots * 256; i += kTileBlocks) hist[i] = 0u;
    __syncthreads();
    if (l.valid) {
        const Where w = where_of(*l.pi, *l.it, l.p);
        uint32_t* row = coefs + threadIdx.x * kLdsRow;
        load_band(row, scratch, *l.it, w);
        const int16_t* gc = reinterpret_cast<const int16_t*>(scratch + l.it->coef_off);
        SymbolSink sink{hist};
        code_block(w, reinterpret_cast<const int16_t*>(row), gc[size_t(w.b) * 64], w.pred >= 0 ? gc[size_t(w.pred) * 64] : 0,
                   eobn[size_t(blockIdx.x) * kTileBlocks + threadIdx.x], sink);
    }
    __syncthreads();
    uint32_t* counts = &reinterpret_cast<ProgWork*>(scratch + l.pi->work_off)->counts[0][0];
    for (int i = threadIdx.x; i < slots * 256; i += kTileBlocks)
        if (hist[i]) atomicAdd(counts + i, hist[i]); // integer sums: the order of the tiles does not show
}

// ------------------------------------------------------------------------------------------------
// P5, P8
// ------------------------------------------------------------------------------------------------

__device__ inline void load_codes(uint32_t* tab, const ProgItem& pi, const uint8_t* scratch)
{
    const uint32_t* codes = &reinterpret_cast<const ProgWork*>(scratch + pi.work_off)->codes[0][0];
    for (int i = threadIdx.x; i < int(pi.slots_n) * 256; i += kTileBlocks) tab[i] = codes[i];
}

__global__ __launch_bounds__(kTileBlocks) void prog_count_bits(const Item* __restrict__ shadow, const ProgItem* __restrict__ pitems, int n, const uint8_t* __restrict__ scratch,
                                                               const uint16_t* __restrict__ eobn, uint32_t* __restrict__ bits, Cursor* __restrict__ tile_sum)
{
    __shared__ uint32_t coefs[kTileBlocks * kLdsRow];
    extern __shared__ uint32_t tab[]; // [the call's most slots][256]: ProgPlan::slots
    __shared__ Cursor cursors[kTileBlocks];
    const Lane l = lane_of(shadow, pitems, n);
    load_codes(tab, *l.pi, scratch);
    __syncthreads();
    Cursor mine{kAdd, 0u, 0u};
    if (l.valid) {
        const Where w = where_of(*l.pi, *l.it, l.p);
        uint32_t* row = coefs + threadIdx.x * kLdsRow;
        load_band(row, scratch, *l.it, w);
        const int16_t* gc = reinterpret_cast<const int16_t*>(scratch + l.it->coef_off);
        BitsSink sink{tab, 0u};
        code_block(w, reinterpret_cast<const int16_t*>(row), gc[size_t(w.b) * 64], w.pred >= 0 ? gc[size_t(w.pred) * 64] : 0,
                   eobn[size_t(blockIdx.x) * kTileBlocks + threadIdx.x], sink);
        bits[size_t(blockIdx.x) * kTileBlocks + threadIdx.x] = sink.total;
        mine = w.segment_first ? Cursor{kRound, 0u, sink.total} : Cursor{kAdd, sink.total, 0u};
    }
    const Cursor incl = scan_cursors(cursors, mine);
    if (threadIdx.x == kTileBlocks - 1)
        tile_sum[blockIdx.x] = blockIdx.x == l.it->tile_start ? Cursor{kConst, 0u, apply(incl, 0u)} : incl;
}

__global__ __launch_bounds__(kTileBlocks) void prog_pack(const Item* __restrict__ shadow, const ProgItem* __restrict__ pitems, int n, uint8_t* __restrict__ scratch,
                                                         const uint16_t* __restrict__ eobn, const uint32_t* __restrict__ bits, const Cursor* __restrict__ tile_before)
{
    __shared__ uint32_t coefs[kTileBlocks * kLdsRow];
    extern __shared__ uint32_t tab[]; // [the call's most slots][256]: ProgPlan::slots
    __shared__ Cursor cursors[kTileBlocks];
    const Lane l = lane_of(shadow, pitems, n);
    load_codes(tab, *l.pi, scratch);
    Where w{};
    Cursor mine{kAdd, 0u, 0u};
    if (l.valid) {
        w                    = where_of(*l.pi, *l.it, l.p);
        const uint32_t total = bits[size_t(blockIdx.x) * kTileBlocks + threadIdx.x];
        mine                 = w.segment_first ? Cursor{kRound, 0u, total} : Cursor{kAdd, total, 0u};
    }
    const Cursor incl = scan_cursors(cursors, mine); // (its first barrier also covers the codes above)
    if (!l.valid) return;
    const Item& it          = *l.it;
    const uint32_t tile_pos = blockIdx.x == it.tile_start ? 0u : apply(tile_before[blockIdx.x], 0u);
    uint32_t pos            = threadIdx.x ? apply(cursors[threadIdx.x - 1], tile_pos) : tile_pos;
    if (w.segment_first) {
        pos = roundup8(pos);
        if (w.q) { // a restart marker goes in front of this byte
            uint32_t* starts = reinterpret_cast<uint32_t*>(scratch + it.starts_off);
            atomicOr(starts + (pos >> 8), 1u << (pos >> 3 & 31));
        } else { // the scan's tables and header do
            reinterpret_cast<ProgWork*>(scratch + l.pi->work_off)->scan_pos[w.s] = pos >> 3;
        }
    }
    uint32_t* row = coefs + threadIdx.x * kLdsRow;
    load_band(row, scratch, it, w);
    const int16_t* gc = reinterpret_cast<const int16_t*>(scratch + it.coef_off);
    PackSink sink{tab, BitWriter{reinterpret_cast<uint32_t*>(scratch + it.stream_off) + (pos >> 5), 0u, int(pos & 31), true}};
    code_block(w, reinterpret_cast<const int16_t*>(row), gc[size_t(w.b) * 64], w.pred >= 0 ? gc[size_t(w.pred) * 64] : 0,
               eobn[size_t(blockIdx.x) * kTileBlocks + threadIdx.x], sink);
    if (w.segment_last) { // ones up to the next byte
        const int pad = -int(apply(incl, tile_pos)) & 7;
        if (pad) sink.bw.put((1u << pad) - 1, pad);
    }
    sink.bw.finish();
}

// ------------------------------------------------------------------------------------------------
// P11
// ------------------------------------------------------------------------------------------------

__device__ inline void lane_bytes(const Item& it, const uint8_t* scratch, uint32_t part, uint32_t (&dw)[8], uint32_t& starts)
{
    const size_t lane = size_t(part) * 256 + threadIdx.x;
    const uint4* s    = reinterpret_cast<const uint4*>(scratch + it.stream_off) + lane * 2;
    const uint4 a = s[0], b = s[1];
    dw[0] = a.x, dw[1] = a.y, dw[2] = a.z, dw[3] = a.w, dw[4] = b.x, dw[5] = b.y, dw[6] = b.z, dw[7] = b.w;
    starts = reinterpret_cast<const uint32_t*>(scratch + it.starts_off)[lane];
}
__device__ inline uint32_t count_ff(const uint32_t (&dw)[8])
{
    uint32_t ff = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t v = dw[q] & (dw[q] >> 4) & 0x0F0F0F0Fu;
        const uint32_t t = v & (v >> 2);
        ff += __popc(t & (t >> 1) & 0x01010101u);
    }
    return ff;
}

__global__ __launch_bounds__(256) void prog_write_files(
    const Item* __restrict__ shadow, const ProgItem* __restrict__ pitems, int n, uint32_t chunks, const uint8_t* __restrict__ scratch,
    const Cursor* __restrict__ tile_sum, const Cursor* __restrict__ tile_before, const Count* __restrict__ counts, const Count* __restrict__ count_before,
    unsigned long long* __restrict__ d_sizes, int* __restrict__ d_status)
{
    __shared__ uint32_t lds[256];
    __shared__ uint32_t header_before[kProgScans + 1]; // bytes of the DHTs and scan headers in front of each scan's
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int i          = item_of_chunk(shadow, n, chunk);
        const Item& it       = shadow[i];
        const ProgItem& pi   = pitems[i];
        const ProgWork* work = reinterpret_cast<const ProgWork*>(scratch + pi.work_off);
        const uint32_t part  = chunk - it.chunk_start;
        const uint32_t bytes = stream_bytes(shadow, i, tile_sum, tile_before);
        const uint32_t last_chunk = shadow[i + 1].chunk_start - 1;
        const Count all           = compose(count_before[last_chunk], counts[last_chunk]);
        __syncthreads(); // (the round before has read header_before)
        if (threadIdx.x == 0) {
            uint32_t at = 0;
            for (uint32_t s = 0; s < pi.scans_n; ++s) {
                header_before[s] = at;
                for (int t = 0; t < pi.scans[s].tables; ++t) at += work->dht_len[pi.scans[s].slot + t];
                at += pi.scans[s].sos_len;
            }
            header_before[pi.scans_n] = at;
        }
        __syncthreads();
        uint32_t table_status = 0u;
        for (uint32_t t = 0; t < pi.slots_n; ++t) table_status = max(table_status, work->status[t]);
        // the size is known before a byte is written
        const uint64_t size = table_status ? 0u : uint64_t(pi.prefix_len) + header_before[pi.scans_n] + bytes + all.ff + 2u * all.starts + 2u;
        const bool fits     = size <= it.capacity;
        if (part == 0 && threadIdx.x == 0) {
            d_sizes[pi.item]  = size;
            d_status[pi.item] = table_status ? int(table_status) : fits ? 0 : 1;
        }
        if (table_status || !fits || uint64_t(part) * kChunkBytes >= bytes) continue;
        uint8_t* out = it.out;
        if (part == 0) {
            for (uint32_t k = threadIdx.x; k < pi.prefix_len; k += 256) out[k] = pi.prefix[k];
            if (threadIdx.x == 0) out[size - 2] = 0xFF, out[size - 1] = 0xD9;
        }
        uint32_t dw[8], starts;
        lane_bytes(it, scratch, part, dw, starts);
        const uint32_t mine = count_ff(dw) | uint32_t(__popc(starts)) << 16;
        lds[threadIdx.x]    = mine;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            uint32_t v = lds[threadIdx.x];
            if (int(threadIdx.x) >= off) v += lds[threadIdx.x - off];
            __syncthreads();
            lds[threadIdx.x] = v;
            __syncthreads();
        }
        const uint32_t before_lane = lds[threadIdx.x] - mine;
        __syncthreads();
        const Count before = counts[chunk].reset ? Count{1u, 0u, 0u} : count_before[chunk];
        const uint32_t p0  = part * uint32_t(kChunkBytes) + threadIdx.x * kChunkLane;
        uint32_t marker    = before.starts + (before_lane >> 16);
        uint32_t next      = 0; // the first scan that begins at or behind this lane's first byte
        while (next < pi.scans_n && work->scan_pos[next] < p0) ++next;
        uint8_t* o = out + pi.prefix_len + header_before[next] + p0 + before.ff + (before_lane & 0xFFFFu) + 2u * marker;
#pragma unroll 1
        for (int k = 0; k < kChunkLane; ++k) {
            if (p0 + k < bytes) {
                if (next < pi.scans_n && work->scan_pos[next] == p0 + k) { // the scan's DHTs and its header
                    const ProgScan& sc = pi.scans[next];
                    for (int t = 0; t < sc.tables; ++t) {
                        const uint8_t* dht = work->dht[sc.slot + t];
                        const uint32_t len = work->dht_len[sc.slot + t];
                        for (uint32_t j = 0; j < len; ++j) o[j] = dht[j];
                        o += len;
                    }
                    for (uint32_t j = 0; j < sc.sos_len; ++j) o[j] = sc.sos[j];
                    o += sc.sos_len;
                    ++next;
                }
                if (starts >> k & 1u) { // RST0 .. RST7 in turn, from RST0 in every scan (a scan's first byte is no segment start)
                    o[0] = 0xFF;
                    o[1] = uint8_t(0xD0 + ((marker - pi.scans[next - 1].marks_before) & 7u));
                    o += 2;
                    ++marker;
                }
                const uint8_t v = uint8_t(dw[k >> 2] >> (8 * (k & 3)));
                *o++            = v;
                if (v == 0xFF) *o++ = 0x00;
            }
        }
    }
}

} // namespace

hipError_t launch_prog_front(const Plan& plan, uint8_t* d_scratch, hipStream_t stream)
{
    const ProgPlan& pp     = plan.prog;
    const Item* shadow     = reinterpret_cast<const Item*>(d_scratch + pp.shadow_off);
    const ProgItem* pitems = reinterpret_cast<const ProgItem*>(d_scratch + pp.items_off);
    uint8_t* facts         = d_scratch + pp.facts_off;
    uint16_t* eobn         = reinterpret_cast<uint16_t*>(d_scratch + pp.eobn_off);
    const size_t lds       = size_t(pp.slots) * 256 * sizeof(uint32_t); // the tables of the item that has the most
    prog_facts<<<pp.tiles, kTileBlocks, 0, stream>>>(shadow, pitems, pp.n, d_scratch, facts, eobn);
    prog_runs<<<pp.tiles, kTileBlocks, 0, stream>>>(shadow, pitems, pp.n, facts, eobn);
    prog_symbols<<<pp.tiles, kTileBlocks, lds, stream>>>(shadow, pitems, pp.n, d_scratch, eobn, pp.slots);
    return hipGetLastError();
}

hipError_t launch_prog_back(const Plan& plan, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, hipStream_t stream)
{
    const ProgPlan& pp     = plan.prog;
    const Item* shadow     = reinterpret_cast<const Item*>(d_scratch + pp.shadow_off);
    const ProgItem* pitems = reinterpret_cast<const ProgItem*>(d_scratch + pp.items_off);
    const uint16_t* eobn   = reinterpret_cast<const uint16_t*>(d_scratch + pp.eobn_off);
    uint32_t* bits         = reinterpret_cast<uint32_t*>(d_scratch + pp.bits_off);
    Cursor* tile_sum       = reinterpret_cast<Cursor*>(d_scratch + pp.tile_sum_off);
    Cursor* tile_before    = reinterpret_cast<Cursor*>(d_scratch + pp.tile_before_off);
    Count* counts          = reinterpret_cast<Count*>(d_scratch + pp.count_off);
    Count* count_before    = reinterpret_cast<Count*>(d_scratch + pp.count_before_off);
    const size_t lds       = size_t(pp.slots) * 256 * sizeof(uint32_t);
    prog_count_bits<<<pp.tiles, kTileBlocks, lds, stream>>>(shadow, pitems, pp.n, d_scratch, eobn, bits, tile_sum);
    hipError_t e = launch_scan_tiles(tile_sum, tile_before, pp.tiles, stream);
    if (e == hipSuccess) e = launch_clear_streams(shadow, pp.n, pp.chunks, d_scratch, tile_sum, tile_before, stream);
    if (e != hipSuccess) return e;
    prog_pack<<<pp.tiles, kTileBlocks, lds, stream>>>(shadow, pitems, pp.n, d_scratch, eobn, bits, tile_before);
    e = launch_count_bytes(shadow, pp.n, pp.chunks, d_scratch, tile_sum, tile_before, counts, count_before, stream);
    if (e != hipSuccess) return e;
    prog_write_files<<<pp.chunks < 4096u ? pp.chunks : 4096u, 256, 0, stream>>>(shadow, pitems, pp.n, pp.chunks, d_scratch, tile_sum, tile_before, counts, count_before,
                                                                                 d_sizes, d_status);
    return hipGetLastError();
}

} // namespace enc
} // namespace jg
