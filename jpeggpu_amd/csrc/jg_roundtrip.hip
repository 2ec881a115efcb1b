// jg_roundtrip.hip -- the pixels an image has after it was saved as a baseline JPEG and opened again, without the file:
// ONE launch takes every block of every item of a call from pixels to quantised coefficients and back to samples.
//
//   roundtrip_blocks  one lane per 8 x 8 block: the encoder's first stage (encode_blocks of jg_encode.hip: gather through the
//                     item's strides with jccolor's and jcsample's rules, jpeg_fdct_islow, the quantiser) and then, on the 64
//                     quantised values still in the lane's registers, the decoder's ISLOW transform (idct_kernel of
//                     jg_idct.hip: dequantisation, jpeg_idct_islow, the range limit). No coefficient reaches memory.
//
// Entropy coding is lossless, so nothing between those two stages changes a pixel, and nothing here needs the MCU stream
// order or the encoder's dummy blocks: a dummy block is a luma block beyond the component's real grid
// (ceil(w / 8) x ceil(h / 8)), which lies wholly outside the image, and the decoder's output stage reads no luma sample out
// there (only chroma is upsampled, and every chroma block of the MCU grid is real). So the kernel walks each component's
// REAL blocks only, row by row: luma's grid, then Cb's and Cr's mcus_x x mcus_y.
//
// A grey item is finished by this launch: the lane stores its block into the item's `dst`, clipped to width x height. An
// RGB item's blocks go into pitched component planes in d_scratch (whole blocks, so no store is clipped), and the batched
// conversion of jg_output.hip (rgb_batch_kernel: fancy upsampling, YCbCr -> RGB) makes the pixels of them in a second launch.
//
// The device functions restate jg_encode.hip's and jg_idct.hip's, whose numbers they are; those files stay as they are.
#include "jg_roundtrip.hpp"

#include <hip/hip_runtime.h>

namespace jg {
namespace rt {
namespace {

/// The item that owns a tile: the last whose first tile is not behind it.
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

/// One 8-point pass of jpeg_idct_islow (jidctint.c, CONST_BITS = 13) over d[0], d[S], .. d[7 S]: the eight outputs before
/// their DESCALE, output i in place of input i (row i of a column in pass 1, column i of a row in pass 2).
template <int S>
__device__ inline void islow8(int* d)
{
    const int in0 = d[0], in1 = d[S], in2 = d[2 * S], in3 = d[3 * S], in4 = d[4 * S], in5 = d[5 * S], in6 = d[6 * S], in7 = d[7 * S];
    // even part: the rotator is sqrt(2) c(-6)
    const int z1   = (in2 + in6) * 4433;
    const int tmp2 = z1 + in6 * -15137;
    const int tmp3 = z1 + in2 * 6270;
    const int tmp0 = (in0 + in4) * (1 << 13);
    const int tmp1 = (in0 - in4) * (1 << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    // odd part
    int t0 = in7, t1 = in5, t2 = in3, t3 = in1;
    int o1 = t0 + t3, o2 = t1 + t2, o3 = t0 + t2, o4 = t1 + t3;
    const int z5 = (o3 + o4) * 9633;
    t0 = t0 * 2446;
    t1 = t1 * 16819;
    t2 = t2 * 25172;
    t3 = t3 * 12299;
    o1 = o1 * -7373;
    o2 = o2 * -20995;
    o3 = o3 * -16069 + z5;
    o4 = o4 * -3196 + z5;
    t0 += o1 + o3;
    t1 += o2 + o4;
    t2 += o2 + o3;
    t3 += o1 + o4;
    d[0] = tmp10 + t3, d[7 * S] = tmp10 - t3;
    d[S] = tmp11 + t2, d[6 * S] = tmp11 - t2;
    d[2 * S] = tmp12 + t1, d[5 * S] = tmp12 - t1;
    d[3 * S] = tmp13 + t0, d[4 * S] = tmp13 - t0;
}

/// libjpeg's post-IDCT range limit (the sample_range_limit table indexed with x & RANGE_MASK, RANGE_MASK = 1023): x wrapped
/// to a 10-bit signed value, clamped to -128..127, plus 128. Not a plain clamp: a checkerboard at a coarse quantiser
/// overshoots far enough to wrap.
__device__ inline uint32_t range_limit(int x)
{
    const int w = static_cast<int>(static_cast<uint32_t>(x) << 22) >> 22;
    return static_cast<uint32_t>(min(max(w, -128), 127) + 128);
}

} // namespace

__global__ __launch_bounds__(kTileBlocks) void roundtrip_blocks(const Item* __restrict__ items, int n, uint8_t* __restrict__ scratch)
{
    const Item& it = items[item_of_tile(items, n, blockIdx.x)];
    const int b    = (blockIdx.x - it.tile_start) * kTileBlocks + threadIdx.x;
    if (b >= it.blocks) return;
    const int w = it.width, h = it.height;
    // the block of its component's plane that this lane transforms, and the input samples per sample of that plane
    const int luma = it.grid_w * it.grid_h;
    int k = b, comp = 0, fx = 1, fy = 1, gw = it.grid_w;
    if (b >= luma) {
        const int chroma = it.mcus_x * it.mcus_y;
        k -= luma;
        comp = k >= chroma ? 2 : 1;
        k -= (comp - 1) * chroma;
        fx = it.hs, fy = it.vs, gw = it.mcus_x;
    }
    const int by = k / gw, bx = k - by * gw;
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

    // The quantiser and DEQUANTIZE in one step: t = (|c| + (8 q >> 1)) / (8 q) with the sign put back, then t q in int.
    // |t q| <= |c| / 8 + q / 2: jpeg_fdct_islow's outputs are 8 times the true DCT's, at most 8 * 8 * 128 * 1.3 in size,
    // and q <= 255, so a dequantised value stays below 1,500 -- far below the 32,767 up to which the first pass of
    // jpeg_idct_islow is exact in 32 bits (jg_idct.hip: kIslowPass1Max). No 64-bit path is needed. The tables are in natural
    // order, so every index below is a constant once unrolled and d[] stays in registers.
    const uint16_t* quant = it.quant[comp > 0];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int c       = d[i];
        const uint32_t q  = quant[i];
        const uint32_t dv = 8u * q;
        const int t       = int((uint32_t(abs(c)) + (dv >> 1)) / dv);
        d[i]              = (c < 0 ? -t : t) * int(q);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) { // columns, DESCALE(.., CONST_BITS - PASS1_BITS) into the int workspace
        islow8<8>(d + c);
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r * 8 + c] = (d[r * 8 + c] + (1 << 10)) >> 11;
    }
    uint32_t px[16]; // eight rows of eight samples, two dwords a row
#pragma unroll
    for (int r = 0; r < 8; ++r) { // rows, DESCALE(.., CONST_BITS + PASS1_BITS + 3) and the range limit
        islow8<1>(d + 8 * r);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            lo |= range_limit((d[r * 8 + c] + (1 << 17)) >> 18) << (8 * c);
            hi |= range_limit((d[r * 8 + 4 + c] + (1 << 17)) >> 18) << (8 * c);
        }
        px[2 * r] = lo, px[2 * r + 1] = hi;
    }

    if (grey) { // the output itself: no alignment is asked of dst, and the block is clipped to the image
        uint8_t* out = it.dst + int64_t(by) * 8 * it.pitch[0] + bx * 8;
        const int cols = min(8, w - bx * 8), rows = min(8, h - by * 8);
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (r < rows && c < cols) out[int64_t(r) * it.pitch[0] + c] = uint8_t(px[2 * r + (c >> 2)] >> (8 * (c & 3)));
        return;
    }
    // a plane of whole blocks: plane_off is a multiple of 256, the pitch of 16, so a row of the block is one aligned 8-byte store
    const int pitch = it.pitch[comp > 0];
    uint8_t* out    = scratch + it.plane_off[comp] + int64_t(by) * 8 * pitch + bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) *reinterpret_cast<uint2*>(out + int64_t(r) * pitch) = make_uint2(px[2 * r], px[2 * r + 1]);
}

hipError_t launch_roundtrip_blocks(const Item* d_items, int n, uint32_t tiles, uint8_t* d_scratch, hipStream_t stream)
{
    hipLaunchKernelGGL(roundtrip_blocks, dim3(tiles), dim3(kTileBlocks), 0, stream, d_items, n, d_scratch);
    return hipGetLastError();
}

} // namespace rt
} // namespace jg
