// jg_encode_device.h -- device code that the encoder's kernel files share: jg_encode.hip (every call) and jg_encode_fit.hip
// (the search for the quality that fits a byte budget). What a kernel of either file does to a tile, a block or a size is
// written once, here: the cursor algebra, the owner of a tile or chunk, the pixel stage up to the transform, the quantiser's
// division, and the length of a file as write_files totals it.
#ifndef JG_ENCODE_DEVICE_H_
#define JG_ENCODE_DEVICE_H_

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

/// An item with optimised tables keeps its state where the others keep their header (jg_encode.hpp: Item::header_len).
__device__ inline bool optimized(const Item& it) { return it.header_len == 0u; }
/// A progressive item's blocks are transformed here and coded by jg_encode_prog.hip.
__device__ inline bool progressive(const Item& it) { return it.header_len == kProgressiveHeader; }
__device__ inline OptState* opt_state(const Item& it, uint8_t* scratch) { return reinterpret_cast<OptState*>(scratch + it.header_off); }
__device__ inline const OptState* opt_state(const Item& it, const uint8_t* scratch) { return reinterpret_cast<const OptState*>(scratch + it.header_off); }
/// The tables an item's blocks are coded with: the call's Annex K tables, or the item's own.
__device__ inline const Tables* tables_of(const Item& it, const uint8_t* scratch, const Tables* standard)
{
    return optimized(it) ? &reinterpret_cast<const OptWork*>(scratch + opt_state(it, scratch)->work_off)->tables : standard;
}

/// Bytes of item i's unstuffed stream, padding of the last segment included: where the cursor stands behind its last tile.
__device__ inline uint32_t stream_bytes(const Item* items, int i, const Cursor* tile_sum, const Cursor* tile_before)
{
    const uint32_t last = items[i + 1].tile_start - 1;
    return (apply(compose(tile_before[last], tile_sum[last]), 0u) + 7u) >> 3;
}

/// The length of item i's file, known once the second scan has run and before a byte of it is written: header, stream, a
/// 0x00 per 0xFF, two bytes per restart marker, EOI. An item with optimised tables has its header in parts -- what the host
/// wrote around what build_tables made --, and a table libjpeg refuses leaves it without a file: `size` 0.
struct FileSize {
    uint32_t bytes;        // of the unstuffed stream
    uint32_t header_len;
    uint32_t table_status; // jpeggpu_ext_encode_status of the worst of its tables, 0: fine
    uint64_t size;
};
__device__ inline FileSize file_size(const Item* items, int i, const uint8_t* blob, const Cursor* tile_sum, const Cursor* tile_before, const Count* counts,
                                     const Count* count_before)
{
    const Item& it = items[i];
    FileSize f;
    f.bytes                   = stream_bytes(items, i, tile_sum, tile_before);
    const uint32_t last_chunk = items[i + 1].chunk_start - 1;
    const Count all           = compose(count_before[last_chunk], counts[last_chunk]);
    const OptState* st        = optimized(it) ? opt_state(it, blob) : nullptr;
    f.header_len = it.header_len, f.table_status = 0u;
    if (st) {
        f.header_len = st->prefix_len + st->suffix_len;
        for (int t = 0; t < 4; ++t) {
            f.header_len += st->dht_len[t];
            f.table_status = max(f.table_status, st->table_status[t]);
        }
    }
    f.size = f.table_status ? 0u : uint64_t(f.header_len) + f.bytes + all.ff + 2u * all.starts + 2u;
    return f;
}

// ------------------------------------------------------------------------------------------------
// pixels to the transform of a block
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

/// Block b of an item's MCU stream, from the item's pixels to jpeg_fdct_islow's output in d (natural order, 8 times the DCT):
/// gather through the item's strides (edge rules of jccolor / jcsample), colour conversion, chroma downsampling, the two
/// passes. `comp`: the block's component. `dummy`: a block of the MCU beyond the component's grid, which transforms the
/// block whose DC it copies and keeps none of its AC.
__device__ inline void transform_block(const Item& it, int b, int (&d)[64], int& comp, bool& dummy)
{
    const int mcu = b / it.blocks_per_mcu, j = b - mcu * it.blocks_per_mcu;
    const int my = mcu / it.mcus_x, mx = mcu - my * it.mcus_x;
    const int luma_blocks = it.hs * it.vs;
    const int w = it.width, h = it.height;
    // the block of its component's plane that this lane transforms, and the input samples per sample of that plane
    int bx, by, fx = 1, fy = 1;
    comp  = 0;
    dummy = false;
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
}

/// The quantiser's rounded division (jcdctmgr.c): c is 8 times the DCT coefficient, dv 8 times the quantiser.
__device__ inline int quantize(int c, uint32_t dv)
{
    const int t = int((uint32_t(abs(c)) + (dv >> 1)) / dv);
    return c < 0 ? -t : t;
}

} // namespace
} // namespace enc
} // namespace jg

#endif // JG_ENCODE_DEVICE_H_
