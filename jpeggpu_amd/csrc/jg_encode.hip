// jg_encode.hip -- baseline JPEG encoding for gfx950: eight launches per call (ten with optimised Huffman tables), whatever the
// number of images and their sizes.
//
//   1 encode_blocks   one lane per 8 x 8 block: gather through the item's strides (edge rules of jccolor / jcsample),
//                     colour conversion, chroma downsampling, jpeg_fdct_islow, quantisation; int16 coefficients in zigzag
//                     order at the block's place in MCU stream order. A dummy block transforms the block whose DC it copies.
//   2 count_bits      one lane per block: DC difference against the previous block of its component, the block's bit count,
//                     and the tile's cursor function (jg_encode.hpp: Cursor)
//   3 scan<Cursor>    ONE workgroup: what lies before each tile
//   4 clear_streams   zeroes each item's unstuffed stream and segment-start bits up to the length now known
//   5 pack_blocks     one lane per block: its codes at its bit offset. The first and last dword of a block are shared with its
//                     neighbours and OR-ed in atomically (the result does not depend on the order), those between are stored.
//   6 count_bytes     per chunk of the unstuffed stream: 0xFF bytes and segment starts
//   7 scan<Count>     ONE workgroup: what lies before each chunk
//   8 write_files     sizes and the capacity test first; then header, stuffed bytes, restart markers and EOI at their final
//                     places in the caller's slot
//
// A call with at least one item that asks for optimised Huffman tables has two launches more, between 1 and 2:
//
//   1a count_symbols  one lane per block of such an item: its DC category and AC symbols into a histogram of the tile in LDS,
//                     whose non-zero bins are added to the item's counts (integer atomics: the order does not show)
//   1b build_tables   one wave per item and table: jpeg_gen_optimal_table (jchuff.c) on those counts, the item's own encoder
//                     tables and its DHT segments
//
// Every later stage reads an item's tables through the item (tables_of), so the two kinds of item mix in one call.
//
// A progressive item (Item::header_len == kProgressiveHeader) takes part in launch 1 only: stages 2 and 5 pass over its
// tiles, and it has no chunks among those of 4 and 6 - 8. Its scans are coded by the ELEVEN launches of jg_encode_prog.hip,
// enqueued behind 1b, among them build_prog_tables here (build_table on the counts of each scan) and, on the progressive
// items' own tiles and chunks, launches 3, 4, 6 and 7 as they are. A call without such an item enqueues none of them.
//
// A transcode call (jpeggpu_ext_transcode_batch; jg_transcode.hpp) is the same sequence with gather_blocks in place of launch 1
// -- the items' coefficients come from the decoder's entropy stage, not from pixels -- and finish_transcode behind the last
// launch, which reports the items whose source holds a coefficient the target cannot code. With an item that has an orientation
// (jpeggpu_ext_set_transcode_orientation) or a crop (jpeggpu_ext_set_transcode_crop) the call launches gather_blocks<true>,
// which maps blocks and coefficients on the way.
//
// jpeggpu_ext_write_coefficients_batch is a transcode call whose sources are the caller's tensors, every item mapped with the
// identity (jg_coefficients.cpp), so it launches gather_blocks<true> and what follows it. jpeggpu_ext_read_coefficients_batch
// is the one launch of read_blocks at the end of this file: the gather's walk of the decoder's entries, stored as tensors.
//
// jpeggpu_ext_encode_fit_batch (jg_encode_fit.hip) searches the quality that fits a byte budget: its own pixel stage keeps the
// unquantised transform, and every evaluation enqueues launches (1a, 1b,) 2 - 7 from here as they are (launch_table_stages,
// launch_size_stages), the final pass launch 8 as well (launch_write_files). What the two files share on the device -- the
// cursor algebra, the pixel stage up to the transform, the quantiser's division, a file's length -- is jg_encode_device.h.
//
// No kernel waits for another workgroup: every dependency is a launch boundary.
#include "jg_encode_device.h"
#include "jg_encode_prog.hpp"
#include "jg_huff_core.h"
#include "jg_output_device.h"
#include "jg_transcode.hpp"

#include <hip/hip_runtime.h>

namespace jg {
namespace enc {
namespace {

// ------------------------------------------------------------------------------------------------
// 1: pixels to coefficients
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kTileBlocks) void encode_blocks(const Item* __restrict__ items, int n, uint8_t* __restrict__ scratch)
{
    const Item& it = items[item_of_tile(items, n, blockIdx.x)];
    const int b    = (blockIdx.x - it.tile_start) * kTileBlocks + threadIdx.x;
    if (b >= it.blocks) return;
    int d[64], comp;
    bool dummy;
    transform_block(it, b, d, comp, dummy);

    const uint16_t* divisor = it.divisor[comp > 0];
    uint4* out              = reinterpret_cast<uint4*>(scratch + it.coef_off) + size_t(b) * 8;
    uint32_t packed[32];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        int t = quantize(d[kNatural[k]], divisor[k]);
        if (dummy && k) t = 0;
        if (k & 1) packed[k >> 1] |= uint32_t(t) << 16;
        else packed[k >> 1] = uint32_t(t) & 0xFFFFu;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) out[q] = make_uint4(packed[4 * q], packed[4 * q + 1], packed[4 * q + 2], packed[4 * q + 3]);
}

// ------------------------------------------------------------------------------------------------
// 2, 5: bits per block, and the codes themselves
// ------------------------------------------------------------------------------------------------

constexpr int kLdsRow = 33; // dwords per block in LDS: 32 of coefficients and one so that the lanes' rows fall on different banks

/// A tile's coefficients into LDS (coalesced), rows beyond the item's blocks zero.
__device__ inline void load_tile(uint32_t* lds, const uint32_t* coef, int first_block, int blocks)
{
    for (int i = threadIdx.x; i < kTileBlocks * 32; i += kTileBlocks) {
        const int blk = i >> 5, w = i & 31;
        lds[blk * kLdsRow + w] = first_block + blk < blocks ? coef[size_t(first_block + blk) * 32 + w] : 0u;
    }
}

struct BlockPlace {
    int mcu, j;
    bool segment_first, segment_last; // the block opens / closes a restart segment (or the scan)
    int table;                        // 0 luma, 1 chroma
    int pred_block;                   // the previous block of its component in the segment, -1: none
};
__device__ inline BlockPlace place_of(const Item& it, int b)
{
    BlockPlace p;
    p.mcu                = b / it.blocks_per_mcu;
    p.j                  = b - p.mcu * it.blocks_per_mcu;
    const int ri         = it.restart_interval;
    const bool first_mcu = ri ? p.mcu % ri == 0 : p.mcu == 0;
    const int luma       = it.hs * it.vs;
    p.segment_first      = first_mcu && p.j == 0;
    p.segment_last       = b == it.blocks - 1 || (ri && p.j == it.blocks_per_mcu - 1 && (p.mcu + 1) % ri == 0);
    if (it.hs == 0) { // the item's own frame (jg_encode.hpp: Frame): the block's entry of the two maps, shifted out of uniform words
        const uint32_t m = uint32_t(it.frame.map >> (6 * p.j)) & 63u;
        p.table          = it.frame.select >> (m & 3u) & 1;
        // behind the first block of its component in the MCU the block in front is the component's; the first one follows
        // the component's last block of the MCU in front
        p.pred_block = m >> 2 ? b - 1 : first_mcu ? -1 : b - it.blocks_per_mcu + (int(it.frame.last >> (4 * p.j)) & 15);
        return p;
    }
    p.table              = p.j >= luma;
    if (p.j < luma && p.j > 0) p.pred_block = b - 1;
    else if (first_mcu) p.pred_block = -1;
    else p.pred_block = p.j < luma ? b - it.blocks_per_mcu + luma - 1 : b - it.blocks_per_mcu;
    return p;
}

__device__ inline int category(int v) { return 32 - __clz(abs(v)); } // abs(v) < 2^31: __clz(0) is 32
/// The category of a DC difference, held to what the tables and the bound of a block's bits cover. Pixels never reach the
/// limit; a transcode item's source can, and then the item is uncodable and its file is never written (gather_blocks).
__device__ inline int dc_category(int diff) { return min(category(diff), 11); }

/// Inclusive scan of the workgroup's cursors in LDS (Hillis-Steele: kTileBlocks lanes, 8 steps); returns the lane's value.
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

__global__ __launch_bounds__(kTileBlocks) void count_bits(
    const Item* __restrict__ items, int n, const Tables* __restrict__ tables, uint8_t* __restrict__ scratch, uint32_t* __restrict__ bits, Cursor* __restrict__ tile_sum)
{
    __shared__ uint32_t coefs[kTileBlocks * kLdsRow];
    __shared__ uint8_t dc_len[2 * 16], ac_len[2 * 256];
    __shared__ Cursor cursors[kTileBlocks];
    const Item& it    = items[item_of_tile(items, n, blockIdx.x)];
    if (progressive(it)) { // (the tile scan reads every tile's function)
        if (threadIdx.x == 0) tile_sum[blockIdx.x] = Cursor{kConst, 0u, 0u};
        return;
    }
    const int first   = (blockIdx.x - it.tile_start) * kTileBlocks;
    const int b       = first + threadIdx.x;
    const int16_t* gc = reinterpret_cast<const int16_t*>(scratch + it.coef_off);
    load_tile(coefs, reinterpret_cast<const uint32_t*>(gc), first, it.blocks);
    const Tables* tab = tables_of(it, scratch, tables);
    for (int i = threadIdx.x; i < 2 * 256; i += kTileBlocks) ac_len[i] = tab->ac[i] & 0xFF;
    if (threadIdx.x < 2 * 16) dc_len[threadIdx.x] = tab->dc[threadIdx.x] & 0xFF;
    __syncthreads();
    Cursor mine{kAdd, 0u, 0u};
    if (b < it.blocks) {
        const BlockPlace p = place_of(it, b);
        const int16_t* c   = reinterpret_cast<const int16_t*>(coefs + threadIdx.x * kLdsRow);
        const int diff     = c[0] - (p.pred_block >= 0 ? gc[size_t(p.pred_block) * 64] : 0);
        int s              = dc_category(diff);
        uint32_t total     = dc_len[p.table * 16 + s] + s;
        int run            = 0;
        for (int k = 1; k < 64; ++k) {
            const int v = c[k];
            if (v == 0) {
                ++run;
                continue;
            }
            total += (run >> 4) * ac_len[p.table * 256 + 0xF0];
            s = category(v);
            total += ac_len[p.table * 256 + ((run & 15) << 4 | s)] + s;
            run = 0;
        }
        if (run) total += ac_len[p.table * 256];
        bits[size_t(blockIdx.x) * kTileBlocks + threadIdx.x] = total;
        mine = p.segment_first ? Cursor{kRound, 0u, total} : Cursor{kAdd, total, 0u};
    }
    const Cursor incl = scan_cursors(cursors, mine);
    if (threadIdx.x == kTileBlocks - 1)
        tile_sum[blockIdx.x] = blockIdx.x == it.tile_start ? Cursor{kConst, 0u, apply(incl, 0u)} : incl;
}

/// The writer of one block's codes: bits gather in a 64-bit window and leave as whole dwords of the stream (its bytes most
/// significant first, so a dword is byte-swapped on its way out).
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
        if (first) atomicOr(word, v); // shared with the block in front
        else *word = v;               // all 32 bits are this block's
        first = false;
        ++word;
    }
    __device__ void finish()
    {
        if (n) atomicOr(word, __builtin_bswap32(uint32_t(acc << (32 - n)))); // shared with the block behind
    }
};

__global__ __launch_bounds__(kTileBlocks) void pack_blocks(
    const Item* __restrict__ items, int n, const Tables* __restrict__ tables, uint8_t* __restrict__ scratch, const uint32_t* __restrict__ bits,
    const Cursor* __restrict__ tile_before)
{
    __shared__ uint32_t coefs[kTileBlocks * kLdsRow];
    __shared__ uint32_t dc_tab[2 * 16], ac_tab[2 * 256];
    __shared__ Cursor cursors[kTileBlocks];
    const Item& it    = items[item_of_tile(items, n, blockIdx.x)];
    if (progressive(it)) return;
    const int first   = (blockIdx.x - it.tile_start) * kTileBlocks;
    const int b       = first + threadIdx.x;
    const int16_t* gc = reinterpret_cast<const int16_t*>(scratch + it.coef_off);
    load_tile(coefs, reinterpret_cast<const uint32_t*>(gc), first, it.blocks);
    const Tables* tab = tables_of(it, scratch, tables);
    for (int i = threadIdx.x; i < 2 * 256; i += kTileBlocks) ac_tab[i] = tab->ac[i];
    if (threadIdx.x < 2 * 16) dc_tab[threadIdx.x] = tab->dc[threadIdx.x];
    const bool valid = b < it.blocks;
    BlockPlace p{};
    Cursor mine{kAdd, 0u, 0u};
    if (valid) {
        p                    = place_of(it, b);
        const uint32_t total = bits[size_t(blockIdx.x) * kTileBlocks + threadIdx.x];
        mine                 = p.segment_first ? Cursor{kRound, 0u, total} : Cursor{kAdd, total, 0u};
    }
    const Cursor incl = scan_cursors(cursors, mine); // (its first barrier also covers the loads above)
    if (!valid) return;
    const uint32_t tile_pos = blockIdx.x == it.tile_start ? 0u : apply(tile_before[blockIdx.x], 0u);
    uint32_t pos            = threadIdx.x ? apply(cursors[threadIdx.x - 1], tile_pos) : tile_pos;
    if (p.segment_first) pos = roundup8(pos);
    if (p.segment_first && b) { // a restart marker goes in front of this byte
        uint32_t* starts = reinterpret_cast<uint32_t*>(scratch + it.starts_off);
        atomicOr(starts + (pos >> 8), 1u << (pos >> 3 & 31));
    }
    BitWriter bw{reinterpret_cast<uint32_t*>(scratch + it.stream_off) + (pos >> 5), 0u, int(pos & 31), true};
    const int16_t* c = reinterpret_cast<const int16_t*>(coefs + threadIdx.x * kLdsRow);
    {
        const int diff = c[0] - (p.pred_block >= 0 ? gc[size_t(p.pred_block) * 64] : 0);
        const int s    = dc_category(diff);
        const uint32_t e = dc_tab[p.table * 16 + s];
        bw.put(e >> 8, e & 0xFF);
        if (s) bw.put(uint32_t(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s); // a negative v is sent as v - 1 in s bits
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = c[k];
        if (v == 0) {
            ++run;
            continue;
        }
        const uint32_t zrl = ac_tab[p.table * 256 + 0xF0];
        for (; run > 15; run -= 16) bw.put(zrl >> 8, zrl & 0xFF);
        const int s      = category(v);
        const uint32_t e = ac_tab[p.table * 256 + (run << 4 | s)];
        bw.put((e >> 8) << s | (uint32_t(v < 0 ? v - 1 : v) & ((1u << s) - 1)), (e & 0xFF) + s);
        run = 0;
    }
    if (run) {
        const uint32_t eob = ac_tab[p.table * 256];
        bw.put(eob >> 8, eob & 0xFF);
    }
    if (p.segment_last) { // ones up to the next byte
        const int pad = -int(apply(incl, tile_pos)) & 7;
        if (pad) bw.put((1u << pad) - 1, pad);
    }
    bw.finish();
}

// ------------------------------------------------------------------------------------------------
// 1a, 1b: optimised tables -- the symbols of an item, and jpeg_gen_optimal_table on their counts
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kTileBlocks) void count_symbols(const Item* __restrict__ items, int n, uint8_t* __restrict__ scratch)
{
    __shared__ uint32_t coefs[kTileBlocks * kLdsRow];
    __shared__ uint32_t hist[2 * kTableCounts];
    const Item& it = items[item_of_tile(items, n, blockIdx.x)];
    if (!optimized(it)) return;
    const int first   = (blockIdx.x - it.tile_start) * kTileBlocks;
    const int b       = first + threadIdx.x;
    const int16_t* gc = reinterpret_cast<const int16_t*>(scratch + it.coef_off);
    load_tile(coefs, reinterpret_cast<const uint32_t*>(gc), first, it.blocks);
    for (int i = threadIdx.x; i < 2 * kTableCounts; i += kTileBlocks) hist[i] = 0u;
    __syncthreads();
    if (b < it.blocks) { // what jchuff.c's htest_one_block counts
        const BlockPlace p = place_of(it, b);
        const int16_t* c   = reinterpret_cast<const int16_t*>(coefs + threadIdx.x * kLdsRow);
        const int diff     = c[0] - (p.pred_block >= 0 ? gc[size_t(p.pred_block) * 64] : 0);
        uint32_t* h        = hist + p.table * kTableCounts;
        atomicAdd(h + dc_category(diff), 1u);
        h += kDcSymbols;
        int run = 0;
        for (int k = 1; k < 64; ++k) {
            const int v = c[k];
            if (v == 0) {
                ++run;
                continue;
            }
            if (run > 15) atomicAdd(h + 0xF0, uint32_t(run >> 4));
            atomicAdd(h + ((run & 15) << 4 | category(v)), 1u);
            run = 0;
        }
        if (run) atomicAdd(h, 1u);
    }
    __syncthreads();
    uint32_t* counts = &opt_state(it, scratch)->counts[0][0];
    for (int i = threadIdx.x; i < 2 * kTableCounts; i += kTileBlocks)
        if (hist[i]) atomicAdd(counts + i, hist[i]); // integer sums: the order of the tiles does not show
}

/// What one wave needs in LDS to build a table.
struct TableLds {
    uint32_t all[34];  // symbols per code length 1..32, the pseudo-symbol included: libjpeg's bits[], limited in place
    uint32_t real[34]; // the same without the pseudo-symbol and before limiting, then its exclusive prefix sums
    uint32_t first_code[17], first_pos[17];
    uint32_t n_values;
};

constexpr int kTableOk = 0, kTableOverflow = 2, kTableEmpty = 3; // jpeggpu_ext_encode_status
constexpr uint32_t kFreqLimit = 1000000000u;                     // where libjpeg's search for the least count starts

/// jpeg_gen_optimal_table (jchuff.c) by ONE wave of 64 lanes on counts[0 .. n_sym), n_sym <= 256: 16 `bits` bytes, the
/// `values` in the order of the DHT segment (*n_values of them) and, for codes_out != nullptr, code << 8 | length of every
/// symbol below n_sym by Annex C from those two (0 for a symbol without a code). Returns kTableOk; kTableOverflow for a code
/// length above 32 before limiting (libjpeg's JERR_HUFF_CLEN_OVERFLOW); kTableEmpty for counts that are all zero, where
/// libjpeg's loops leave their arrays, or beyond what its search covers (a count of 2^28, a sum of 10^9). Then bits and
/// codes are zeros and there are no values.
///
/// Lane l owns the symbols l, l + 64, .. l + 256 (symbol 256 is libjpeg's pseudo-symbol of count 1, which keeps the code of
/// all ones unused). A merge takes the two least non-zero counts, of equal counts the LARGEST index as libjpeg's `<=` does:
/// both are the least keys count * 512 + (511 - index) of the wave. libjpeg then walks the chains of both trees to lengthen
/// the code of every member; here every symbol knows the root of its tree, and those of either root do that themselves.
__device__ int build_table(const uint32_t* counts, int n_sym, TableLds& lds, uint8_t* bits_out, uint8_t* values_out, uint32_t* codes_out, int* n_values)
{
    constexpr int kOwn  = 5;
    constexpr uint64_t kNone = ~uint64_t(0);
    const int lane = threadIdx.x;
    uint32_t freq[kOwn];
    int root[kOwn], size[kOwn], rank[kOwn];
    uint64_t total = 0;
    bool beyond    = false;
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
        const int e = lane + 64 * j;
        uint32_t f  = e < n_sym ? counts[e] : 0u;
        beyond |= f >= (1u << 28);
        total += f;
        freq[j] = e == 256 ? 1u : f;
        root[j] = e, size[j] = 0, rank[j] = 0;
    }
    for (int off = 32; off; off >>= 1) total += __shfl_xor(total, off, 64);
    int status = total == 0 || total >= kFreqLimit || __any(beyond) ? kTableEmpty : kTableOk;
    while (status == kTableOk) { // (uniform: at most 256 merges)
        uint64_t m1 = kNone, m2 = kNone;
#pragma unroll
        for (int j = 0; j < kOwn; ++j) {
            const uint64_t key = freq[j] ? uint64_t(freq[j]) << 9 | uint32_t(511 - (lane + 64 * j)) : kNone;
            if (key < m1) m2 = m1, m1 = key;
            else if (key < m2) m2 = key;
        }
        for (int off = 32; off; off >>= 1) { // the two least of the wave: the keys of symbols with a count are distinct
            const uint64_t o1 = __shfl_xor(m1, off, 64), o2 = __shfl_xor(m2, off, 64);
            const uint64_t lo = m1 < o1 ? m1 : o1, hi = m1 < o1 ? o1 : m1, second = m2 < o2 ? m2 : o2;
            m1 = lo, m2 = hi < second ? hi : second;
        }
        if (m2 == kNone) break; // one tree is left
        const int c1 = 511 - int(m1 & 511u), c2 = 511 - int(m2 & 511u);
#pragma unroll
        for (int j = 0; j < kOwn; ++j) {
            const int e = lane + 64 * j;
            if (root[j] == c1 || root[j] == c2) ++size[j], root[j] = c1;
            if (e == c1) freq[j] += uint32_t(m2 >> 9);
            if (e == c2) freq[j] = 0u;
        }
    }
    if (lane < 34) lds.all[lane] = lds.real[lane] = 0u;
    __syncthreads();
    bool over = false;
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
        if (size[j] > 32) over = true;
        else if (size[j]) {
            atomicAdd(&lds.all[size[j]], 1u);
            if (lane + 64 * j < 256) atomicAdd(&lds.real[size[j]], 1u);
        }
    }
    __syncthreads();
    if (status == kTableOk && __any(over)) status = kTableOverflow;
    if (status != kTableOk) {
        if (lane < 16) bits_out[lane] = 0;
        if (codes_out)
            for (int e = lane; e < n_sym; e += 64) codes_out[e] = 0u;
        *n_values = 0;
        return status;
    }
    if (lane == 0) {
        uint32_t* bits = lds.all;
        for (int i = 32; i > 16; --i) { // libjpeg's length limiting: a pair of the longest codes moves up by one, a shorter code pays
            while (bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && bits[j] == 0) --j; // (a tree of 257 leaves this deep always has a shorter code)
                bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1;
            }
        }
        int i = 16;
        while (i > 0 && bits[i] == 0) --i;
        bits[i] -= 1; // the pseudo-symbol leaves the longest length
        uint32_t code = 0, pos = 0, before = 0;
        for (int len = 1; len <= 16; ++len) {
            lds.first_code[len] = code, lds.first_pos[len] = pos;
            code = (code + bits[len]) << 1;
            pos += bits[len];
        }
        for (int len = 1; len <= 32; ++len) {
            const uint32_t here = lds.real[len];
            lds.real[len]       = before;
            before += here;
        }
        lds.n_values = before;
    }
    __syncthreads();
    // huffval lists the symbols by code length BEFORE limiting, then by value: a symbol's place is the symbols of shorter
    // lengths and those of its own length in front of it
    for (int s = 1; s <= 32; ++s) {
        uint32_t at = lds.real[s];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long same = __ballot(size[j] == s);
            if (size[j] == s) rank[j] = int(at + __popcll(same & ((1ull << lane) - 1ull)));
            at += uint32_t(__popcll(same));
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e   = lane + 64 * j;
        uint32_t code = 0u;
        if (size[j]) {
            values_out[rank[j]] = uint8_t(e);
            for (int len = 1; len <= 16; ++len) // Annex C on (bits, values): after limiting the length is not size[j]
                if (uint32_t(rank[j]) >= lds.first_pos[len] && uint32_t(rank[j]) - lds.first_pos[len] < lds.all[len])
                    code = (lds.first_code[len] + uint32_t(rank[j]) - lds.first_pos[len]) << 8 | uint32_t(len);
        }
        if (codes_out && e < n_sym) codes_out[e] = code;
    }
    if (lane < 16) bits_out[lane] = uint8_t(lds.all[lane + 1]);
    *n_values = int(lds.n_values);
    return kTableOk;
}

__global__ __launch_bounds__(64) void build_tables(const Item* __restrict__ items, int n, uint8_t* __restrict__ scratch)
{
    __shared__ TableLds lds;
    const Item& it = items[blockIdx.x >> 2];
    const int t    = blockIdx.x & 3; // DC0, AC0, DC1, AC1
    if (!optimized(it) || ((it.hs ? it.channels == 1 : it.frame.select == 0) && t >= 2)) return; // no block is coded with tables 1
    OptState* st    = opt_state(it, scratch);
    OptWork* work   = reinterpret_cast<OptWork*>(scratch + st->work_off);
    const int table = t >> 1, ac = t & 1;
    uint8_t* seg    = work->dht[t];
    int n_values    = 0;
    const int status = build_table(st->counts[table] + (ac ? kDcSymbols : 0), ac ? 256 : kDcSymbols, lds, seg + 5, seg + 21,
                                   ac ? work->tables.ac + 256 * table : work->tables.dc + 16 * table, &n_values);
    if (threadIdx.x == 0) {
        const uint32_t len = 2u + 17u + uint32_t(n_values);
        seg[0] = 0xFF, seg[1] = 0xC4, seg[2] = uint8_t(len >> 8), seg[3] = uint8_t(len), seg[4] = uint8_t(ac << 4 | table);
        st->dht_len[t]      = len + 2u;
        st->table_status[t] = uint32_t(status);
    }
}

/// One wave per progressive item and table: the table of a scan from the counts prog_symbols made, its codes and its DHT.
__global__ __launch_bounds__(64) void build_prog_tables(const ProgItem* __restrict__ pitems, uint8_t* __restrict__ scratch, int slots)
{
    __shared__ TableLds lds;
    const ProgItem& pi = pitems[blockIdx.x / slots]; // `slots`: the most tables an item of the call has (ProgPlan::slots)
    const int slot     = blockIdx.x % slots;
    if (slot >= int(pi.slots_n)) return;
    ProgWork* work   = reinterpret_cast<ProgWork*>(scratch + pi.work_off);
    const int ac     = pi.slot_class_id[slot] >> 4;
    uint8_t* seg     = work->dht[slot];
    int n_values     = 0;
    const int status = build_table(work->counts[slot], ac ? 256 : kDcSymbols, lds, seg + 5, seg + 21, work->codes[slot], &n_values);
    if (threadIdx.x == 0) {
        const uint32_t len = 2u + 17u + uint32_t(n_values);
        seg[0] = 0xFF, seg[1] = 0xC4, seg[2] = uint8_t(len >> 8), seg[3] = uint8_t(len), seg[4] = pi.slot_class_id[slot];
        work->dht_len[slot] = len + 2u;
        work->status[slot]  = uint32_t(status);
    }
}

__global__ __launch_bounds__(64) void tables_from_counts(const uint32_t* __restrict__ counts, uint8_t* __restrict__ out, int* __restrict__ status)
{
    __shared__ TableLds lds;
    uint8_t* o   = out + size_t(blockIdx.x) * (16 + 256);
    int n_values = 0;
    const int st = build_table(counts + size_t(blockIdx.x) * 256, 256, lds, o, o + 16, nullptr, &n_values);
    for (int i = n_values + threadIdx.x; i < 256; i += 64) o[16 + i] = 0;
    if (threadIdx.x == 0) status[blockIdx.x] = st;
}

// ------------------------------------------------------------------------------------------------
// 3, 7: the scans between the stages, one workgroup each
// ------------------------------------------------------------------------------------------------

/// before[i] = in[0] o .. o in[i - 1]. Each lane composes a run of consecutive elements, the lanes' results are scanned in
/// LDS, and each lane walks its run once more.
template <class T>
__global__ __launch_bounds__(kScanThreads) void scan_before(const T* __restrict__ in, T* __restrict__ before, uint32_t count)
{
    __shared__ T lds[kScanThreads];
    const uint32_t per = (count + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = min(count, threadIdx.x * per), hi = min(count, lo + per);
    T run{};
    for (uint32_t i = lo; i < hi; ++i) run = compose(run, in[i]);
    lds[threadIdx.x] = run;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        T v = lds[threadIdx.x];
        if (int(threadIdx.x) >= off) v = compose(lds[threadIdx.x - off], v);
        __syncthreads();
        lds[threadIdx.x] = v;
        __syncthreads();
    }
    run = threadIdx.x ? lds[threadIdx.x - 1] : T{};
    for (uint32_t i = lo; i < hi; ++i) {
        before[i] = run;
        run       = compose(run, in[i]);
    }
}

// ------------------------------------------------------------------------------------------------
// 4, 6, 8: the byte stages, one workgroup per chunk of an item's unstuffed stream
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void clear_streams(
    const Item* __restrict__ items, int n, uint32_t chunks, uint8_t* __restrict__ scratch, const Cursor* __restrict__ tile_sum,
    const Cursor* __restrict__ tile_before)
{
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int i         = item_of_chunk(items, n, chunk);
        const Item& it      = items[i];
        const uint32_t part = chunk - it.chunk_start;
        if (uint64_t(part) * kChunkBytes >= stream_bytes(items, i, tile_sum, tile_before)) continue;
        uint4* s = reinterpret_cast<uint4*>(scratch + it.stream_off + uint64_t(part) * kChunkBytes);
        s[threadIdx.x]       = make_uint4(0u, 0u, 0u, 0u);
        s[threadIdx.x + 256] = make_uint4(0u, 0u, 0u, 0u);
        reinterpret_cast<uint32_t*>(scratch + it.starts_off)[size_t(part) * 256 + threadIdx.x] = 0u;
    }
}

/// The lane's kChunkLane bytes of the stream (zero beyond its end: the chunk was cleared as a whole) and its segment-start bits.
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
        const uint32_t v = dw[q] & (dw[q] >> 4) & 0x0F0F0F0Fu; // a byte is 0xFF where both nibbles are 0xF
        const uint32_t t = v & (v >> 2);
        ff += __popc(t & (t >> 1) & 0x01010101u);
    }
    return ff;
}

__global__ __launch_bounds__(256) void count_bytes(
    const Item* __restrict__ items, int n, uint32_t chunks, const uint8_t* __restrict__ scratch, const Cursor* __restrict__ tile_sum,
    const Cursor* __restrict__ tile_before, Count* __restrict__ counts)
{
    __shared__ uint32_t sum[2];
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int i         = item_of_chunk(items, n, chunk);
        const Item& it      = items[i];
        const uint32_t part = chunk - it.chunk_start;
        const uint32_t reset = part == 0;
        if (uint64_t(part) * kChunkBytes >= stream_bytes(items, i, tile_sum, tile_before)) {
            if (threadIdx.x == 0) counts[chunk] = Count{reset, 0u, 0u};
            continue;
        }
        if (threadIdx.x < 2) sum[threadIdx.x] = 0u;
        __syncthreads();
        uint32_t dw[8], starts;
        lane_bytes(it, scratch, part, dw, starts);
        const uint32_t ff = count_ff(dw);
        if (ff) atomicAdd(&sum[0], ff); // integer sums: the order does not show
        if (starts) atomicAdd(&sum[1], uint32_t(__popc(starts)));
        __syncthreads();
        if (threadIdx.x == 0) counts[chunk] = Count{reset, sum[0], sum[1]};
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void write_files(
    const Item* __restrict__ items, int n, uint32_t chunks, const uint8_t* __restrict__ scratch, const uint8_t* __restrict__ blob,
    const Cursor* __restrict__ tile_sum, const Cursor* __restrict__ tile_before, const Count* __restrict__ counts, const Count* __restrict__ count_before,
    unsigned long long* __restrict__ d_sizes, int* __restrict__ d_status)
{
    __shared__ uint32_t lds[256];
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int i          = item_of_chunk(items, n, chunk);
        const Item& it       = items[i];
        const uint32_t part  = chunk - it.chunk_start;
        // the size is known before a byte is written (jg_encode_device.h: file_size)
        const FileSize fs    = file_size(items, i, blob, tile_sum, tile_before, counts, count_before);
        const uint32_t bytes = fs.bytes, header_len = fs.header_len, table_status = fs.table_status;
        const uint64_t size  = fs.size;
        const OptState* st   = optimized(it) ? opt_state(it, blob) : nullptr;
        const bool fits      = size <= it.capacity;
        if (part == 0 && threadIdx.x == 0) {
            d_sizes[i]  = size;
            d_status[i] = table_status ? int(table_status) : fits ? 0 : 1;
        }
        if (table_status || !fits || uint64_t(part) * kChunkBytes >= bytes) continue;
        uint8_t* out = it.out;
        if (part == 0) {
            if (st) {
                const OptWork* work = reinterpret_cast<const OptWork*>(scratch + st->work_off);
                uint32_t at         = st->prefix_len;
                const uint8_t* prefix = long_prefix(st->prefix_len) ? reinterpret_cast<const uint8_t*>(st + 1) : st->prefix; // (a long one: behind the state)
                for (uint32_t k = threadIdx.x; k < st->prefix_len; k += 256) out[k] = prefix[k];
                for (int t = 0; t < 4; ++t) {
                    for (uint32_t k = threadIdx.x; k < st->dht_len[t]; k += 256) out[at + k] = work->dht[t][k];
                    at += st->dht_len[t];
                }
                for (uint32_t k = threadIdx.x; k < st->suffix_len; k += 256) out[at + k] = st->suffix[k];
            } else {
                for (uint32_t k = threadIdx.x; k < header_len; k += 256) out[k] = blob[it.header_off + k];
            }
            if (threadIdx.x == 0) out[size - 2] = 0xFF, out[size - 1] = 0xD9;
        }
        uint32_t dw[8], starts;
        lane_bytes(it, scratch, part, dw, starts);
        // what the lanes in front of this one add: 0xFF bytes in the low half, segment starts in the high half (<= 8192 each)
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
        uint8_t* o         = out + header_len + p0 + before.ff + (before_lane & 0xFFFFu) + 2u * marker;
#pragma unroll
        for (int k = 0; k < kChunkLane; ++k) {
            if (p0 + k < bytes) {
                if (starts >> k & 1u) {
                    o[0] = 0xFF;
                    o[1] = uint8_t(0xD0 + (marker & 7u)); // RST0 .. RST7 in turn
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

// ------------------------------------------------------------------------------------------------
// 1 of a transcode call: coefficients from the decoder's entropy stage (jg_transcode.hpp) in place of encode_blocks
// ------------------------------------------------------------------------------------------------

/// Block b of an item's MCU stream as a block of its component's padded grid.
/// kOriented, and the item has an orientation or a crop (GatherSrc::oriented): the block of the SOURCE's grid that the
/// target's block is, and `dummy` for a luma block beyond the target's real grid -- then the block is the real one whose DC
/// the encoder gives it (encode_blocks), and only that DC is the source's. Such an item never reads the source's own dummy
/// blocks. In order: the written grid's block, plus the crop's offset in the uncropped target's grid, mirrored there,
/// exchanged.
struct SrcBlock {
    int comp, bx, by;
    bool dummy;
};
template <bool kOriented>
__device__ inline SrcBlock src_block(const Item& it, const GatherSrc& src, int b)
{
    const int mcu = b / it.blocks_per_mcu, j = b - mcu * it.blocks_per_mcu;
    const int my = mcu / it.mcus_x, mx = mcu - my * it.mcus_x;
    const int luma = it.hs * it.vs;
    SrcBlock sb{0, mx, my, false};
    if (it.hs == 0) { // the item's own frame: every component has h x v blocks in the MCU, and dummy blocks where they exceed 1
        const uint32_t m = uint32_t(it.frame.map >> (6 * j)) & 63u;
        const int xo = m >> 2 & 3u, yo = m >> 4;
        sb.comp     = m & 3u;
        const int h = it.frame.hv >> (8 * sb.comp) & 15u, v = it.frame.hv >> (8 * sb.comp + 4) & 15u;
        sb.bx = mx * h + xo, sb.by = my * v + yo;
        if (!kOriented || !src.oriented) return sb;
        // the MCU's real blocks of the component are rx x ry from its first one on; the block in front of a dummy one, and
        // of that one, in the MCU's order ends at the last real block of the row, or of the last real row
        const int rx = min(h, it.frame.grid_w[sb.comp] - mx * h), ry = min(v, it.frame.grid_h[sb.comp] - my * v);
        if (xo >= rx || yo >= ry) {
            sb.dummy = true;
            sb.bx = mx * h + rx - 1, sb.by = my * v + min(yo, ry - 1);
        }
    } else if (j >= luma) {
        sb.comp = 1 + j - luma;
    } else {
        const int yo = j / it.hs;
        sb.bx = mx * it.hs + j - yo * it.hs, sb.by = my * it.vs + yo;
    }
    if (!kOriented || !src.oriented) return sb;
    if (sb.comp == 0 && it.hs) {
        if (sb.by >= it.grid_h) {
            sb.dummy = true;
            sb.by -= 1;
            sb.bx = min(mx * it.hs + it.hs - 1, it.grid_w - 1);
        } else if (sb.bx >= it.grid_w) {
            sb.dummy = true;
            sb.bx    = it.grid_w - 1;
        }
    }
    const GatherComp& c = src.comp[sb.comp];
    sb.bx += c.off_x, sb.by += c.off_y;
    const int x = src.mirror_x ? c.dst_x - 1 - sb.bx : sb.bx, y = src.mirror_y ? c.dst_y - 1 - sb.by : sb.by;
    sb.bx = src.transpose ? y : x, sb.by = src.transpose ? x : y;
    return sb;
}

// An orientation in the coefficient domain, by the source's zigzag index: where the entry goes when the block is transposed
// (natural 8 v + u to 8 u + v), and which entries a mirror of the source's x (odd u) and of its y (odd v) negates.
__device__ const uint8_t kZigzagTransposed[64] = {0,  2,  1,  5,  4,  3,  9,  8,  7,  6,  14, 13, 12, 11, 10, 20, 19, 18, 17, 16, 15, 27,
                                                  26, 25, 24, 23, 22, 21, 35, 34, 33, 32, 31, 30, 29, 28, 42, 41, 40, 39, 38, 37, 36, 48,
                                                  47, 46, 45, 44, 43, 53, 52, 51, 50, 49, 57, 56, 55, 54, 60, 59, 58, 62, 61, 63};
constexpr uint64_t kZigzagOddU = 0xB56AAD55554AA952ull, kZigzagOddV = 0xD6AB555AA5552A94ull;

/// A progressive source's block `w` (natural order, two coefficients a dword) to the lane's row, in the target's zigzag order:
/// kTranspose exchanges u and v, neg_u / neg_v negate the source's odd horizontal / vertical frequencies. Every index of `w`
/// is a constant once the loop is unrolled, so the array stays in registers. True: a coefficient the target cannot code.
template <bool kTranspose>
__device__ inline bool oriented_row(const uint32_t (&w)[32], uint32_t* row, bool neg_u, bool neg_v)
{
    constexpr uint8_t nat[64] = JG_ORDER_NATURAL;
    bool bad                  = false;
#pragma unroll
    for (int k = 0; k < 64; k += 2) {
        const int a = kTranspose ? (nat[k] & 7) << 3 | nat[k] >> 3 : nat[k], b = kTranspose ? (nat[k + 1] & 7) << 3 | nat[k + 1] >> 3 : nat[k + 1];
        int lo = int16_t(w[a >> 1] >> (16 * (a & 1))), hi = int16_t(w[b >> 1] >> (16 * (b & 1)));
        if (k && abs(lo) >= 1024) bad = true, lo = 0;
        if (abs(hi) >= 1024) bad = true, hi = 0;
        if (((a & 1) && neg_u) != ((a & 8) && neg_v)) lo = -lo; // (k == 0: a == 0, the DC keeps its sign)
        if (((b & 1) && neg_u) != ((b & 8) && neg_v)) hi = -hi;
        row[k >> 1] = (uint32_t(lo) & 0xFFFFu) | uint32_t(hi) << 16;
    }
    return bad;
}

/// The data unit of a baseline source that holds the block, -1: no scan codes it (a dummy block of a component's own scan).
/// kOriented: counted from GatherSrc::first_unit, as the IDCT stage counts from its first_mcu (jg_idct.hip); a unit in front
/// of it was not decoded and is -1 (transcode_spec refuses an item that would read one, on either side of what was kept).
template <bool kOriented>
__device__ inline int src_unit(const GatherSrc& src, const GatherComp& c, int bx, int by)
{
    int unit;
    if (!c.interleaved) {
        unit = bx < c.vis_x && by < c.vis_y ? by * c.vis_x + bx : -1;
    } else {
        const int mx = bx / c.h, my = by / c.v;
        unit         = (my * c.mcus_x + mx) * c.du_per_mcu + c.k0 + (by - my * c.v) * c.h + (bx - mx * c.h);
    }
    if (kOriented) unit = unit >= src.first_unit ? unit - src.first_unit : -1;
    return unit;
}

/// A unit's record with its first entry held inside the buffer, as idct_scaled_kernel holds it (jg_idct.hip): a record
/// that a corrupt stream never wrote must not lead out of it.
__device__ inline uint2_t src_record(const GatherComp& c, int unit)
{
    uint2_t rec = static_cast<const uint2_t*>(c.du_tab)[unit];
    rec.x       = uint32_t(rec.x < c.sym_limit ? rec.x : c.sym_limit);
    return rec;
}

/// The AC coefficients of a baseline source's unit: put(zigzag index, value) for each entry behind the DC, an escaped value
/// joined with its escape entry as in the IDCT stage. One 2-byte load is in flight ahead of the entry in hand; a unit has
/// at most 127 entries, which src_record's clamp keeps inside the buffer.
template <class F>
__device__ __forceinline__ void walk_entries(const GatherComp& c, uint2_t rec, F&& put)
{
    const uint32_t cnt = rec.y & 0x7Fu;
    const bool esc     = (rec.y & kUnitHasEscape) != 0;
    uint32_t e         = cnt > 1u ? c.sym[sym_advance(rec.x, 1u)] : 0u;
    for (uint32_t i = 1; i < cnt; ++i) {
        const bool more     = i + 1 < cnt;
        const uint32_t next = more ? c.sym[sym_advance(rec.x, i + 1)] : 0u;
        const uint32_t zz   = sym_entry_index(e);
        if (zz) // index 0 behind the DC: the escape of the coefficient in front
            put(zz, esc && more && sym_entry_index(next) == 0 ? sym_entry_value(e, next) : sym_entry_value(e));
        e = next;
    }
}

/// The source's DC coefficient of block b, absolute.
template <bool kOriented>
__device__ inline int src_dc(const Item& it, const GatherSrc& src, int b)
{
    const SrcBlock sb   = src_block<kOriented>(it, src, b);
    const GatherComp& c = src.comp[sb.comp];
    if (c.coef) return c.coef[(int64_t(sb.by) * c.blocks_x + sb.bx) * 64];
    const int unit = src_unit<kOriented>(src, c, sb.bx, sb.by);
    return unit < 0 ? 0 : int16_t(c.sym[src_record(c, unit).x]);
}

/// One lane per block of the target's MCU stream. The lane fills its row of the tile in LDS -- rows kLdsRow dwords apart,
/// so the lanes of a wave that store the same zigzag index fall on different banks -- from the unit's entries (escapes as
/// in the IDCT stage) or from the component's coefficient array, transposed to zigzag order; then the workgroup stores the
/// tile in whole lines. What the target cannot code -- an AC coefficient of category above 10, a DC difference of category
/// above 11 -- marks the item: its capacity becomes 0, so that no later stage writes its slot, the coefficient is stored
/// as 0, so that every table index of the later stages stays in range, and finish_transcode reports it.
/// A baseline source's unit is walked entry by entry, one 2-byte load in flight ahead of the one in hand, up to 127 of them:
/// what the kernel takes follows the entries per unit. The measured 1.5 ms per 64 photographs is for
/// photographic units of a dozen entries or two; a source of dense units (every coefficient coded, every one escaped) takes
/// several times as long per block. GatherSrc::shadow_off is a 32-bit offset: the blob it points into is below 4 GB.
/// kOriented: the instantiation of a call with a mapped item: of orientation 2..8 (jpeggpu_ext_set_transcode_orientation) or
/// with a crop (jpeggpu_ext_set_transcode_crop), which is the identity orientation behind an offset. The lane
/// reads the source block that src_block names and stores each coefficient at the transposed zigzag index with its mirror's
/// sign; a dummy block of such an item takes one DC from the source and nothing else. An item of orientation 1 in such a
/// call goes the same way with an identity mapping and gets the values the other instantiation gives it.
template <bool kOriented>
__global__ __launch_bounds__(kTileBlocks) void gather_blocks(Item* items, int n, uint8_t* scratch) // (the items lie in the scratch)
{
    __shared__ uint32_t tile[kTileBlocks * kLdsRow];
    Item& it       = items[item_of_tile(items, n, blockIdx.x)];
    GatherSrc& src = *const_cast<GatherSrc*>(reinterpret_cast<const GatherSrc*>(it.src));
    const int first = (blockIdx.x - it.tile_start) * kTileBlocks;
    const int b     = first + threadIdx.x;
    uint32_t* row   = tile + threadIdx.x * kLdsRow;
    bool bad        = false;
    if (b < it.blocks) {
        const SrcBlock sb   = src_block<kOriented>(it, src, b);
        const GatherComp& c = src.comp[sb.comp];
        int dc              = 0;
        // what the orientation does to the SOURCE's frequencies: its stored x is mirrored (odd u change sign), its stored y
        const bool transpose = kOriented && src.transpose;
        const bool neg_u = kOriented && (transpose ? src.mirror_y : src.mirror_x), neg_v = kOriented && (transpose ? src.mirror_x : src.mirror_y);
        if (kOriented && sb.dummy) {
#pragma unroll
            for (int k = 0; k < 32; ++k) row[k] = 0u;
            dc     = src_dc<kOriented>(it, src, b);
            row[0] = uint32_t(dc) & 0xFFFFu;
        } else if (c.coef) {
            constexpr uint8_t nat[64] = JG_ORDER_NATURAL;
            const uint4* p            = reinterpret_cast<const uint4*>(c.coef + (int64_t(sb.by) * c.blocks_x + sb.bx) * 64);
            uint32_t w[32];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint4 v = p[q];
                w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
            }
            dc = int16_t(w[0]);
            if (kOriented) {
                bad = transpose ? oriented_row<true>(w, row, neg_u, neg_v) : oriented_row<false>(w, row, neg_u, neg_v);
            } else {
#pragma unroll
                for (int k = 0; k < 64; k += 2) {
                    int lo = int16_t(w[nat[k] >> 1] >> (16 * (nat[k] & 1))), hi = int16_t(w[nat[k + 1] >> 1] >> (16 * (nat[k + 1] & 1)));
                    if (k && abs(lo) >= 1024) bad = true, lo = 0;
                    if (abs(hi) >= 1024) bad = true, hi = 0;
                    row[k >> 1] = (uint32_t(lo) & 0xFFFFu) | uint32_t(hi) << 16;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 32; ++k) row[k] = 0u;
            const int unit = src_unit<kOriented>(src, c, sb.bx, sb.by);
            if (unit >= 0) {
                const uint2_t rec  = src_record(c, unit);
                int16_t* r16       = reinterpret_cast<int16_t*>(row);
                const uint64_t neg = kOriented ? (neg_u ? kZigzagOddU : 0ull) ^ (neg_v ? kZigzagOddV : 0ull) : 0ull;
                dc                 = int16_t(c.sym[rec.x]);
                r16[0]             = int16_t(dc);
                walk_entries(c, rec, [&](uint32_t zz, int v) {
                    if (abs(v) >= 1024) bad = true, v = 0;
                    if (kOriented) r16[transpose ? kZigzagTransposed[zz] : zz] = int16_t(neg >> zz & 1u ? -v : v);
                    else r16[zz] = int16_t(v);
                });
            }
        }
        const BlockPlace p = place_of(it, b);
        if (abs(dc - (p.pred_block >= 0 ? src_dc<kOriented>(it, src, p.pred_block) : 0)) >= 2048) bad = true;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) { // (every workgroup that finds one stores the same values)
        src.uncodable = 1u;
        it.capacity   = 0u;
        if (src.shadow_off) reinterpret_cast<Item*>(scratch + src.shadow_off)->capacity = 0u;
    }
    uint4* out     = reinterpret_cast<uint4*>(scratch + it.coef_off) + size_t(first) * 8;
    const int rows = min(kTileBlocks, it.blocks - first);
    for (int i = threadIdx.x; i < rows * 8; i += kTileBlocks) {
        const uint32_t* s = tile + (i >> 3) * kLdsRow + (i & 7) * 4;
        out[i]            = make_uint4(s[0], s[1], s[2], s[3]);
    }
}

/// The status of the items gather_blocks marked, behind every stage that wrote one.
__global__ __launch_bounds__(256) void finish_transcode(const Item* __restrict__ items, int n, unsigned long long* __restrict__ d_sizes, int* __restrict__ d_status)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !reinterpret_cast<const GatherSrc*>(items[i].src)->uncodable) return;
    d_sizes[i]  = 0u;
    d_status[i] = JPEGGPU_EXT_ENCODE_UNCODABLE;
}

// ------------------------------------------------------------------------------------------------
// jpeggpu_ext_read_coefficients_batch: the decoder's coefficients as the caller's tensors (jg_transcode.hpp: ReadItem)
// ------------------------------------------------------------------------------------------------

/// The item that owns a tile of a read call: the last whose first tile is not behind it. items[n] is a sentinel.
__device__ inline int read_item_of_tile(const ReadItem* items, int n, uint32_t tile)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].tile_start[0] <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/// One lane per block of the TARGET: a workgroup owns kReadTile consecutive blocks of one component's raster over its real
/// grid, so what it stores is one contiguous run of the component's tensor, in whole 128-byte lines. The lane fills its row
/// of the tile in LDS in NATURAL order -- rows kLdsRow dwords apart, as gather_blocks keeps them: lanes that write the same
/// index fall on different banks, and the 16-byte pieces the lanes then read back (8 lanes a row of int16, 16 a row of
/// float) are conflict-free in each half of the wave -- from the unit's entries, walked as gather_blocks walks them, or, for
/// a progressive source, from its block of the padded coefficient array. A block no scan codes stays 64 zeros.
/// T int16_t: the values. T float / _Float16: float(value) * float(factor), one binary32 multiply, then float_bits<T>.
template <class T>
__global__ __launch_bounds__(kReadTile) void read_blocks(const ReadItem* __restrict__ items, int n)
{
    __shared__ uint32_t tile[kReadTile * kLdsRow];
    const ReadItem& it = items[read_item_of_tile(items, n, blockIdx.x)];
    int comp           = 0;
    for (int c = 1; c < 4; ++c) comp += it.tile_start[c] <= blockIdx.x; // (a component the frame lacks starts at the item's end)
    const GatherComp& c = it.src.comp[comp];
    const int grid_w = it.grid_w[comp], blocks = grid_w * it.grid_h[comp];
    const int first = (blockIdx.x - it.tile_start[comp]) * kReadTile;
    const int b     = first + threadIdx.x;
    uint32_t* row   = tile + threadIdx.x * kLdsRow;
    if (b < blocks) {
        const int by = b / grid_w, bx = b - by * grid_w;
        if (c.coef) {
            const uint4* p = reinterpret_cast<const uint4*>(c.coef + (int64_t(by) * c.blocks_x + bx) * 64);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint4 v = p[q];
                row[4 * q] = v.x, row[4 * q + 1] = v.y, row[4 * q + 2] = v.z, row[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 32; ++k) row[k] = 0u;
            const int unit = c.sym ? src_unit<false>(it.src, c, bx, by) : -1;
            if (unit >= 0) {
                const uint2_t rec = src_record(c, unit);
                int16_t* r16      = reinterpret_cast<int16_t*>(row);
                r16[0]            = int16_t(c.sym[rec.x]);
                walk_entries(c, rec, [&](uint32_t zz, int v) { r16[kNatural[zz]] = int16_t(v); });
            }
        }
    }
    __syncthreads();
    const int rows = min(kReadTile, blocks - first);
    if constexpr (sizeof(T) == 2 && !std::is_same<T, _Float16>::value) {
        uint4* out = reinterpret_cast<uint4*>(it.dst[comp]) + size_t(first) * 8;
        for (int i = threadIdx.x; i < rows * 8; i += kReadTile) {
            const uint32_t* s = tile + (i >> 3) * kLdsRow + (i & 7) * 4;
            out[i]            = make_uint4(s[0], s[1], s[2], s[3]);
        }
    } else {
        constexpr int kPer = 16 / int(sizeof(T)), kParts = 64 / kPer; // elements a lane stores, lanes a block
        const uint16_t* factor = it.factor[comp];
        uint4* out             = reinterpret_cast<uint4*>(it.dst[comp]) + size_t(first) * kParts;
        for (int i = threadIdx.x; i < rows * kParts; i += kReadTile) {
            const int part    = i % kParts;
            const uint32_t* s = tile + (i / kParts) * kLdsRow + part * (kPer / 2);
            uint32_t e[kPer], d[4];
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int v = int16_t(s[k >> 1] >> (16 * (k & 1)));
                e[k]        = float_bits<T>(__fmul_rn(float(v), float(factor[part * kPer + k])));
            }
            tensor_pack<int(sizeof(T)), kPer>(e, d);
            out[i] = make_uint4(d[0], d[1], d[2], d[3]);
        }
    }
}

} // namespace

hipError_t launch_read_blocks(const ReadItem* d_items, int n, uint32_t tiles, int type, hipStream_t stream)
{
    if (type == JPEGGPU_EXT_COEF_F32) read_blocks<float><<<tiles, kReadTile, 0, stream>>>(d_items, n);
    else if (type == JPEGGPU_EXT_COEF_F16) read_blocks<_Float16><<<tiles, kReadTile, 0, stream>>>(d_items, n);
    else read_blocks<int16_t><<<tiles, kReadTile, 0, stream>>>(d_items, n);
    return hipGetLastError();
}

hipError_t launch_encode(const Plan& plan, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, hipStream_t stream, bool transcode)
{
    const Item* items = reinterpret_cast<const Item*>(d_scratch + plan.items_off);
    if (transcode && plan.oriented) gather_blocks<true><<<plan.tiles, kTileBlocks, 0, stream>>>(reinterpret_cast<Item*>(d_scratch + plan.items_off), plan.n, d_scratch);
    else if (transcode) gather_blocks<false><<<plan.tiles, kTileBlocks, 0, stream>>>(reinterpret_cast<Item*>(d_scratch + plan.items_off), plan.n, d_scratch);
    else encode_blocks<<<plan.tiles, kTileBlocks, 0, stream>>>(items, plan.n, d_scratch);
    const auto finish = [&] { // a transcode call's last launch
        if (transcode) finish_transcode<<<(uint32_t(plan.n) + 255u) / 256u, 256, 0, stream>>>(items, plan.n, d_sizes, d_status);
        return hipGetLastError();
    };
    launch_table_stages(plan, d_scratch, stream);
    if (plan.prog.n) { // the progressive items' own launches; the rest of the call follows as it always did
        hipError_t e = launch_prog_front(plan, d_scratch, stream);
        if (e == hipSuccess) e = launch_prog_tables(plan, d_scratch, stream);
        if (e == hipSuccess) e = launch_prog_back(plan, d_scratch, d_sizes, d_status, stream);
        if (e != hipSuccess) return e;
        if (plan.chunks == 0u) return finish(); // every item is progressive
    }
    launch_size_stages(plan, d_scratch, stream);
    launch_write_files(plan, d_scratch, d_sizes, d_status, stream);
    return finish();
}

int launch_table_stages(const Plan& plan, uint8_t* d_scratch, hipStream_t stream)
{
    if (!plan.optimized) return 0;
    const Item* items = reinterpret_cast<const Item*>(d_scratch + plan.items_off);
    count_symbols<<<plan.tiles, kTileBlocks, 0, stream>>>(items, plan.n, d_scratch);
    build_tables<<<uint32_t(plan.n) * 4u, 64, 0, stream>>>(items, plan.n, d_scratch);
    return 2;
}

int launch_size_stages(const Plan& plan, uint8_t* d_scratch, hipStream_t stream)
{
    const Item* items     = reinterpret_cast<const Item*>(d_scratch + plan.items_off);
    const Tables* tables  = reinterpret_cast<const Tables*>(d_scratch + plan.tables_off);
    uint32_t* bits        = reinterpret_cast<uint32_t*>(d_scratch + plan.bits_off);
    Cursor* tile_sum      = reinterpret_cast<Cursor*>(d_scratch + plan.tile_sum_off);
    Cursor* tile_before   = reinterpret_cast<Cursor*>(d_scratch + plan.tile_before_off);
    Count* counts         = reinterpret_cast<Count*>(d_scratch + plan.count_off);
    Count* count_before   = reinterpret_cast<Count*>(d_scratch + plan.count_before_off);
    const uint32_t chunk_grid = plan.chunks < 4096u ? plan.chunks : 4096u;
    count_bits<<<plan.tiles, kTileBlocks, 0, stream>>>(items, plan.n, tables, d_scratch, bits, tile_sum);
    scan_before<Cursor><<<1, kScanThreads, 0, stream>>>(tile_sum, tile_before, plan.tiles);
    clear_streams<<<chunk_grid, 256, 0, stream>>>(items, plan.n, plan.chunks, d_scratch, tile_sum, tile_before);
    pack_blocks<<<plan.tiles, kTileBlocks, 0, stream>>>(items, plan.n, tables, d_scratch, bits, tile_before);
    count_bytes<<<chunk_grid, 256, 0, stream>>>(items, plan.n, plan.chunks, d_scratch, tile_sum, tile_before, counts);
    scan_before<Count><<<1, kScanThreads, 0, stream>>>(counts, count_before, plan.chunks);
    return 6;
}

int launch_write_files(const Plan& plan, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, hipStream_t stream)
{
    const Item* items   = reinterpret_cast<const Item*>(d_scratch + plan.items_off);
    Cursor* tile_sum    = reinterpret_cast<Cursor*>(d_scratch + plan.tile_sum_off);
    Cursor* tile_before = reinterpret_cast<Cursor*>(d_scratch + plan.tile_before_off);
    Count* counts       = reinterpret_cast<Count*>(d_scratch + plan.count_off);
    Count* count_before = reinterpret_cast<Count*>(d_scratch + plan.count_before_off);
    write_files<<<plan.chunks < 4096u ? plan.chunks : 4096u, 256, 0, stream>>>(items, plan.n, plan.chunks, d_scratch, d_scratch, tile_sum, tile_before, counts, count_before,
                                                                             d_sizes, d_status);
    return 1;
}

hipError_t launch_prog_tables(const Plan& plan, uint8_t* d_scratch, hipStream_t stream)
{
    build_prog_tables<<<uint32_t(plan.prog.n) * uint32_t(plan.prog.slots), 64, 0, stream>>>(reinterpret_cast<const ProgItem*>(d_scratch + plan.prog.items_off), d_scratch,
                                                                                           plan.prog.slots);
    return hipGetLastError();
}

hipError_t launch_scan_tiles(const Cursor* tile_sum, Cursor* tile_before, uint32_t tiles, hipStream_t stream)
{
    scan_before<Cursor><<<1, kScanThreads, 0, stream>>>(tile_sum, tile_before, tiles);
    return hipGetLastError();
}

hipError_t launch_clear_streams(const Item* items, int n, uint32_t chunks, uint8_t* d_scratch, const Cursor* tile_sum, const Cursor* tile_before, hipStream_t stream)
{
    clear_streams<<<chunks < 4096u ? chunks : 4096u, 256, 0, stream>>>(items, n, chunks, d_scratch, tile_sum, tile_before);
    return hipGetLastError();
}

hipError_t launch_count_bytes(const Item* items, int n, uint32_t chunks, const uint8_t* d_scratch, const Cursor* tile_sum, const Cursor* tile_before, Count* counts,
                              Count* count_before, hipStream_t stream)
{
    count_bytes<<<chunks < 4096u ? chunks : 4096u, 256, 0, stream>>>(items, n, chunks, d_scratch, tile_sum, tile_before, counts);
    scan_before<Count><<<1, kScanThreads, 0, stream>>>(counts, count_before, chunks);
    return hipGetLastError();
}

hipError_t launch_tables_from_counts(const uint32_t* d_counts, int n_tables, uint8_t* d_bits_values, int* d_status, hipStream_t stream)
{
    tables_from_counts<<<uint32_t(n_tables), 64, 0, stream>>>(d_counts, d_bits_values, d_status);
    return hipGetLastError();
}

} // namespace enc
} // namespace jg
