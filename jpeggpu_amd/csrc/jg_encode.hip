// jg_encode.hip -- baseline JPEG encoding for gfx950: eight launches per call, whatever the number of images and their sizes.
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
// No kernel waits for another workgroup: every dependency is a launch boundary.
#include "jg_encode.hpp"

#include <hip/hip_runtime.h>

namespace jg {
namespace enc {
namespace {

__device__ const uint8_t kNatural[64] = { // natural index of zigzag position k
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ inline uint32_t roundup8(uint32_t x) { return (x + 7u) & ~7u; }

__device__ inline uint32_t apply(Cursor f, uint32_t x)
{
    return f.kind == kAdd ? x + f.a : f.kind == kRound ? roundup8(x + f.a) + f.b : f.b;
}
/// f first, then g.
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

/// The item that owns a tile (a chunk): the last whose first tile (chunk) is not behind it. items[n] is a sentinel.
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

/// Bytes of item i's unstuffed stream, padding of the last segment included: where the cursor stands behind its last tile.
__device__ inline uint32_t stream_bytes(const Item* items, int i, const Cursor* tile_sum, const Cursor* tile_before)
{
    const uint32_t last = items[i + 1].tile_start - 1;
    return (apply(compose(tile_before[last], tile_sum[last]), 0u) + 7u) >> 3;
}

// ------------------------------------------------------------------------------------------------
// 1: pixels to coefficients
// ------------------------------------------------------------------------------------------------

__device__ inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

/// One pass of jpeg_fdct_islow (jfdctint.c) over d[0], d[S], .. d[7 S]. FIRST: the row pass (results scaled by 4).
template <int S, bool FIRST>
__device__ inline void fdct_pass(int* d)
{
    constexpr int N = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0]     = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
    d[4 * S] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
    int z1   = (t12 + t13) * 4433;
    d[2 * S] = descale(z1 + t13 * 6270, N);
    d[6 * S] = descale(z1 - t12 * 15137, N);
    z1       = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * S] = descale(u4 + z1 + z3, N);
    d[5 * S] = descale(u5 + z2 + z4, N);
    d[3 * S] = descale(u6 + z2 + z3, N);
    d[S]     = descale(u7 + z1 + z4, N);
}

__global__ __launch_bounds__(kTileBlocks) void encode_blocks(const Item* __restrict__ items, int n, uint8_t* __restrict__ scratch)
{
    const Item& it = items[item_of_tile(items, n, blockIdx.x)];
    const int b    = (blockIdx.x - it.tile_start) * kTileBlocks + threadIdx.x;
    if (b >= it.blocks) return;
    const int mcu = b / it.blocks_per_mcu, j = b - mcu * it.blocks_per_mcu;
    const int my = mcu / it.mcus_x, mx = mcu - my * it.mcus_x;
    const int luma_blocks = it.hs * it.vs;
    const int w = it.width, h = it.height;
    // the block of its component's plane that this lane transforms, and the input samples per sample of that plane
    int bx, by, fx = 1, fy = 1, comp = 0;
    bool dummy = false;
    if (j < luma_blocks) {
        const int yo = j / it.hs, xo = j - yo * it.hs;
        bx = mx * it.hs + xo;
        by = my * it.vs + yo;
        // jccoefct.c: a block of the MCU beyond the component's grid is 63 zeros and the DC of the block before it in the MCU's
        // order -- at the right edge the last real block of its row, below the grid the last block of the row above
        if (by >= it.grid_h) {
            dummy = true;
            by -= 1;
            bx = min(mx * it.hs + it.hs - 1, it.grid_w - 1);
        } else if (bx >= it.grid_w) {
            dummy = true;
            bx    = it.grid_w - 1;
        }
    } else {
        comp = 1 + j - luma_blocks;
        bx = mx, by = my, fx = it.hs, fy = it.vs;
    }
    // jccolor.c's fixed point; grey input is the sample itself
    int kr = 19595, kg = 38470, kb = 7471, rnd = 32768;
    if (comp == 1) kr = -11059, kg = -21709, kb = 32768, rnd = (128 << 16) + 32767;
    if (comp == 2) kr = 32768, kg = -27439, kb = -5329, rnd = (128 << 16) + 32767;
    const bool grey    = it.channels == 1;
    const int shift    = (fx == 2) + (fy == 2);
    const int plane_h  = (h + fy - 1) / fy; // rows: the input repeats its last row to a multiple of fy only, then the LAST DOWNSAMPLED row repeats
    const uint8_t* src = it.src;
    const int64_t cs   = it.channel_stride;

    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int cy = min(by * 8 + r, plane_h - 1);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int cx = bx * 8 + c;
            int sum      = 0;
            for (int dy = 0; dy < fy; ++dy) {
                const uint8_t* row = src + int64_t(min(cy * fy + dy, h - 1)) * it.row_pitch;
                for (int dx = 0; dx < fx; ++dx) {
                    const uint8_t* p = row + int64_t(min(cx * fx + dx, w - 1)) * it.pixel_stride; // columns: the last sample repeats
                    sum += grey ? int(p[0]) : (kr * int(p[0]) + kg * int(p[cs]) + kb * int(p[2 * cs]) + rnd) >> 16;
                }
            }
            // jcsample.c: h2v1 bias 0, 1, 0, 1 .., h2v2 bias 1, 2, 1, 2 .. along the output row
            const int bias = fx == 2 ? (fy == 2 ? 1 + (cx & 1) : (cx & 1)) : 0;
            d[r * 8 + c]   = ((sum + bias) >> shift) - 128;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct_pass<1, true>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct_pass<8, false>(d + c);

    const uint16_t* divisor = it.divisor[comp > 0];
    uint4* out              = reinterpret_cast<uint4*>(scratch + it.coef_off) + size_t(b) * 8;
    uint32_t packed[32];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int c       = d[kNatural[k]];
        const uint32_t dv = divisor[k];
        int t             = int((uint32_t(abs(c)) + (dv >> 1)) / dv);
        t                 = c < 0 ? -t : t;
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
    p.table              = p.j >= luma;
    if (p.j < luma && p.j > 0) p.pred_block = b - 1;
    else if (first_mcu) p.pred_block = -1;
    else p.pred_block = p.j < luma ? b - it.blocks_per_mcu + luma - 1 : b - it.blocks_per_mcu;
    return p;
}

__device__ inline int category(int v) { return 32 - __clz(abs(v)); } // abs(v) < 2^31: __clz(0) is 32

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
    const int first   = (blockIdx.x - it.tile_start) * kTileBlocks;
    const int b       = first + threadIdx.x;
    const int16_t* gc = reinterpret_cast<const int16_t*>(scratch + it.coef_off);
    load_tile(coefs, reinterpret_cast<const uint32_t*>(gc), first, it.blocks);
    for (int i = threadIdx.x; i < 2 * 256; i += kTileBlocks) ac_len[i] = tables->ac[i] & 0xFF;
    if (threadIdx.x < 2 * 16) dc_len[threadIdx.x] = tables->dc[threadIdx.x] & 0xFF;
    __syncthreads();
    Cursor mine{kAdd, 0u, 0u};
    if (b < it.blocks) {
        const BlockPlace p = place_of(it, b);
        const int16_t* c   = reinterpret_cast<const int16_t*>(coefs + threadIdx.x * kLdsRow);
        const int diff     = c[0] - (p.pred_block >= 0 ? gc[size_t(p.pred_block) * 64] : 0);
        int s              = category(diff);
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
    const int first   = (blockIdx.x - it.tile_start) * kTileBlocks;
    const int b       = first + threadIdx.x;
    const int16_t* gc = reinterpret_cast<const int16_t*>(scratch + it.coef_off);
    load_tile(coefs, reinterpret_cast<const uint32_t*>(gc), first, it.blocks);
    for (int i = threadIdx.x; i < 2 * 256; i += kTileBlocks) ac_tab[i] = tables->ac[i];
    if (threadIdx.x < 2 * 16) dc_tab[threadIdx.x] = tables->dc[threadIdx.x];
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
        const int s    = category(diff);
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
        const uint32_t bytes = stream_bytes(items, i, tile_sum, tile_before);
        // the size is known before a byte is written: header, stream, a 0x00 per 0xFF, two bytes per marker, EOI
        const uint32_t last_chunk = items[i + 1].chunk_start - 1;
        const Count all           = compose(count_before[last_chunk], counts[last_chunk]);
        const uint64_t size       = uint64_t(it.header_len) + bytes + all.ff + 2u * all.starts + 2u;
        const bool fits           = size <= it.capacity;
        if (part == 0 && threadIdx.x == 0) {
            d_sizes[i]  = size;
            d_status[i] = fits ? 0 : 1;
        }
        if (!fits || uint64_t(part) * kChunkBytes >= bytes) continue;
        uint8_t* out = it.out;
        if (part == 0) {
            for (uint32_t k = threadIdx.x; k < it.header_len; k += 256) out[k] = blob[it.header_off + k];
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
        uint8_t* o         = out + it.header_len + p0 + before.ff + (before_lane & 0xFFFFu) + 2u * marker;
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

} // namespace

hipError_t launch_encode(const Plan& plan, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, hipStream_t stream)
{
    const Item* items     = reinterpret_cast<const Item*>(d_scratch + plan.items_off);
    const Tables* tables  = reinterpret_cast<const Tables*>(d_scratch + plan.tables_off);
    uint32_t* bits        = reinterpret_cast<uint32_t*>(d_scratch + plan.bits_off);
    Cursor* tile_sum      = reinterpret_cast<Cursor*>(d_scratch + plan.tile_sum_off);
    Cursor* tile_before   = reinterpret_cast<Cursor*>(d_scratch + plan.tile_before_off);
    Count* counts         = reinterpret_cast<Count*>(d_scratch + plan.count_off);
    Count* count_before   = reinterpret_cast<Count*>(d_scratch + plan.count_before_off);
    const uint32_t chunk_grid = plan.chunks < 4096u ? plan.chunks : 4096u;
    encode_blocks<<<plan.tiles, kTileBlocks, 0, stream>>>(items, plan.n, d_scratch);
    count_bits<<<plan.tiles, kTileBlocks, 0, stream>>>(items, plan.n, tables, d_scratch, bits, tile_sum);
    scan_before<Cursor><<<1, kScanThreads, 0, stream>>>(tile_sum, tile_before, plan.tiles);
    clear_streams<<<chunk_grid, 256, 0, stream>>>(items, plan.n, plan.chunks, d_scratch, tile_sum, tile_before);
    pack_blocks<<<plan.tiles, kTileBlocks, 0, stream>>>(items, plan.n, tables, d_scratch, bits, tile_before);
    count_bytes<<<chunk_grid, 256, 0, stream>>>(items, plan.n, plan.chunks, d_scratch, tile_sum, tile_before, counts);
    scan_before<Count><<<1, kScanThreads, 0, stream>>>(counts, count_before, plan.chunks);
    write_files<<<chunk_grid, 256, 0, stream>>>(items, plan.n, plan.chunks, d_scratch, d_scratch, tile_sum, tile_before, counts, count_before, d_sizes, d_status);
    return hipGetLastError();
}

} // namespace enc
} // namespace jg
