// jg_encode_fit.hip -- the kernels of a budget call (jg_encode_fit.hpp) for gfx950, around the size stages of jg_encode.hip:
//
//   T transform_blocks   ONCE per call, one lane per 8 x 8 block: encode_blocks' pixel stage (jg_encode_device.h:
//                        transform_block) with the UNQUANTISED transform stored, int16 in zigzag order at the block's place
//                        in MCU stream order; a dummy block keeps its DC only
//   per probe:
//   R requantize_blocks  one lane per block: eight 16-byte rows of the stored transform in, the quantiser's rounded division
//                        by the item's divisors, eight 16-byte rows out to where encode_blocks would have stored them. The
//                        first tile of an item with optimised tables zeroes the item's symbol counts for this probe.
//     (1a, 1b) 2 - 7     jg_encode.hip as it is: after them every item's size(q) is known on the device
//   D fit_decide         one workgroup per item: lane 0 totals size(q) as write_files does (file_size), compares it with the
//                        budget and moves the item's search on; then the 128 lanes derive the next quality's divisors and
//                        the 2 x 64 DQT bytes of the item's header (jg_quant.h) from the quality now in device memory
//   final pass: R, (1a, 1b), 2 - 8 at the chosen quality, and
//   F fit_finish         the chosen qualities and the status of the items over budget
//
// An item whose search has ended sits out the remaining probes: fit_decide sets its Item::blocks to 0, so every lane of its
// tiles leaves R, 1a, 2 and 5 at their test against the item's blocks, its stream is empty and its chunks leave 4 and 6 at
// their test against the stream's length. The last decision puts the count back. No kernel waits for another workgroup.
//
// The stored transform is int16, as libjpeg-turbo's DCTELEM is for 8-bit samples. The range holds: jpeg_fdct_islow
// returns 8 times the DCT F(u, v) = 1/4 C(u) C(v) sum f(x, y) cos cos with |f| <= 128; per dimension C(u) sum |cos| is at
// most 8 / sqrt(2) (u = 0 and u = 4: 5.657, every other u less), so |F| <= 1/4 x 128 x 32 = 1024 and |8 F| <= 8192, a
// quarter of int16's range; the fixed-point passes add a few units of rounding to that, not a factor.
#include "jg_encode_device.h"
#include "jg_encode_fit.hpp"
#include "jg_quant.h"

#include <hip/hip_runtime.h>

namespace jg {
namespace enc {
namespace {

__global__ __launch_bounds__(kTileBlocks) void transform_blocks(const Item* __restrict__ items, int n, const FitItem* __restrict__ fit, uint8_t* __restrict__ scratch)
{
    const int i    = item_of_tile(items, n, blockIdx.x);
    const Item& it = items[i];
    const int b    = (blockIdx.x - it.tile_start) * kTileBlocks + threadIdx.x;
    if (b >= it.blocks) return;
    int d[64], comp;
    bool dummy;
    transform_block(it, b, d, comp, dummy);
    uint4* out = reinterpret_cast<uint4*>(scratch + fit[i].raw_off) + size_t(b) * 8;
    uint32_t packed[32];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int c = dummy && k ? 0 : d[kNatural[k]]; // |c| <= 8192 and a little (above)
        if (k & 1) packed[k >> 1] |= uint32_t(c) << 16;
        else packed[k >> 1] = uint32_t(c) & 0xFFFFu;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) out[q] = make_uint4(packed[4 * q], packed[4 * q + 1], packed[4 * q + 2], packed[4 * q + 3]);
}

__global__ __launch_bounds__(kTileBlocks) void requantize_blocks(const Item* __restrict__ items, int n, const FitItem* __restrict__ fit, uint8_t* __restrict__ scratch)
{
    const int i    = item_of_tile(items, n, blockIdx.x);
    const Item& it = items[i];
    if (it.blocks == 0) return; // its search has ended
    if (blockIdx.x == it.tile_start && optimized(it)) { // count_symbols adds to them, behind this launch
        uint32_t* counts = &opt_state(it, scratch)->counts[0][0];
        for (int k = threadIdx.x; k < 2 * kTableCounts; k += kTileBlocks) counts[k] = 0u;
    }
    const int b = (blockIdx.x - it.tile_start) * kTileBlocks + threadIdx.x;
    if (b >= it.blocks) return;
    const int j             = b % it.blocks_per_mcu;
    const uint16_t* divisor = it.divisor[j >= it.hs * it.vs];
    const uint4* in         = reinterpret_cast<const uint4*>(scratch + fit[i].raw_off) + size_t(b) * 8;
    uint4* out              = reinterpret_cast<uint4*>(scratch + it.coef_off) + size_t(b) * 8;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 v        = in[q];
        const uint32_t w[4]  = {v.x, v.y, v.z, v.w};
        uint32_t r[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int k   = 8 * q + 2 * p;
            const int lo  = quantize(int16_t(w[p] & 0xFFFFu), divisor[k]);
            const int hi  = quantize(int16_t(w[p] >> 16), divisor[k + 1]);
            r[p]          = (uint32_t(lo) & 0xFFFFu) | uint32_t(hi) << 16;
        }
        out[q] = make_uint4(r[0], r[1], r[2], r[3]);
    }
}

__global__ __launch_bounds__(128) void fit_decide(Item* items, FitItem* fit, uint8_t* blob, const Cursor* __restrict__ tile_sum,
                                                  const Cursor* __restrict__ tile_before, const Count* __restrict__ counts, const Count* __restrict__ count_before,
                                                  int last)
{
    __shared__ int next_quality; // 0: the item's tables stay
    const int i = blockIdx.x;
    Item& it    = items[i];
    FitItem& f  = fit[i];
    if (threadIdx.x == 0) {
        int q = f.q;
        if (f.phase != kFitDone) {
            const bool fits = file_size(items, i, blob, tile_sum, tile_before, counts, count_before).size <= f.max_bytes;
            if (f.phase == kFitHigh) {
                if (fits) f.phase = kFitDone; // q is hi
                else if (f.lo == f.hi) f.phase = kFitDone, f.over = 1;
                else f.phase = kFitLow, q = f.lo;
            } else if (f.phase == kFitLow) {
                if (!fits) f.phase = kFitDone, f.over = 1; // q is lo
                else f.best = f.lo, f.a = f.lo + 1, f.b = f.hi - 1, f.phase = kFitBisect;
            } else {
                if (fits) f.best = q, f.a = q + 1;
                else f.b = q - 1;
            }
            if (f.phase == kFitBisect) {
                if (f.a <= f.b) q = (f.a + f.b) / 2;
                else f.phase = kFitDone, q = f.best;
            }
        }
        next_quality = q != f.q ? q : 0;
        f.q          = q;
        // a finished item sits out the remaining probes; the final pass codes every item, and an item over budget into no slot
        it.blocks = last || f.phase != kFitDone ? f.blocks : 0;
        if (f.over) it.capacity = 0u;
    }
    __syncthreads();
    const int q = next_quality;
    if (q == 0) return;
    const int t = threadIdx.x >> 6, k = threadIdx.x & 63;
    const int v = quantizer(t, q, kNatural[k]);
    it.divisor[t][k] = uint16_t(8 * v);
    if (f.dqt_off[t]) blob[f.dqt_off[t] + k] = uint8_t(v);
}

__global__ __launch_bounds__(256) void fit_finish(const FitItem* __restrict__ fit, int n, int* __restrict__ d_status, int* __restrict__ d_quality)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    d_quality[i] = fit[i].q;
    // write_files found the file of quality_min larger than the capacity of 0 it was given, and reported its size
    if (fit[i].over && d_status[i] == JPEGGPU_EXT_ENCODE_TOO_SMALL) d_status[i] = JPEGGPU_EXT_ENCODE_OVER_BUDGET;
}

} // namespace

hipError_t launch_encode_fit(const Plan& plan, int probes, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, int* d_quality, hipStream_t stream,
                             int* launched)
{
    Item* items         = reinterpret_cast<Item*>(d_scratch + plan.items_off);
    FitItem* fit        = reinterpret_cast<FitItem*>(d_scratch + plan.fit_off);
    Cursor* tile_sum    = reinterpret_cast<Cursor*>(d_scratch + plan.tile_sum_off);
    Cursor* tile_before = reinterpret_cast<Cursor*>(d_scratch + plan.tile_before_off);
    Count* counts       = reinterpret_cast<Count*>(d_scratch + plan.count_off);
    Count* count_before = reinterpret_cast<Count*>(d_scratch + plan.count_before_off);
    int count           = 0;
    transform_blocks<<<plan.tiles, kTileBlocks, 0, stream>>>(items, plan.n, fit, d_scratch);
    ++count;
    for (int p = 0; p <= probes; ++p) { // the last round is the final pass
        requantize_blocks<<<plan.tiles, kTileBlocks, 0, stream>>>(items, plan.n, fit, d_scratch);
        count += 1 + launch_table_stages(plan, d_scratch, stream) + launch_size_stages(plan, d_scratch, stream);
        if (p == probes) break;
        fit_decide<<<uint32_t(plan.n), 128, 0, stream>>>(items, fit, d_scratch, tile_sum, tile_before, counts, count_before, p == probes - 1);
        ++count;
    }
    count += launch_write_files(plan, d_scratch, d_sizes, d_status, stream);
    fit_finish<<<(uint32_t(plan.n) + 255u) / 256u, 256, 0, stream>>>(fit, plan.n, d_status, d_quality);
    *launched = count + 1;
    return hipGetLastError();
}

} // namespace enc
} // namespace jg
