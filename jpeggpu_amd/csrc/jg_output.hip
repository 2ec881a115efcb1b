// jg_output.hip -- gfx950 (CDNA4, wave64) kernels of the RGB output stage: from decoded planes to what a caller looks at.
//
//   upsample_kernel         nearest-neighbour chroma replication, planes to planes
//   rgbi_kernel             replication + the JFIF matrix in float -> interleaved RGB (the reference's conv_to_rgbi)
//   fancy_rgbi_kernel       libjpeg's fancy chroma upsampling + integer YCbCr -> interleaved RGB (jdsample.c, jdcolor.c),
//                           of a whole image (<false>) or of a rectangle read from the planes' windows (<true>)
//   fancy_color_kernel      the same for every colour model: RGB-, CMYK- and YCCK-coded files too, as Pillow converts them
//   fancy_mirrored_kernel / the same pixels written where an EXIF orientation displays them: 2..4 mirror the row kernel's
//   fancy_transposed_kernel stores, 5..8 turn a square tile through LDS (jpeggpu_ext_planes_to_rgbi_oriented)
//   resize_h_kernel /       batched resize to one size with Pillow's BILINEAR / BICUBIC arithmetic: the horizontal taps
//   resize_v_kernel         straight from the planes' windows (fancy RGB in LDS), then the vertical taps (jpeggpu_ext_resize_to_rgb);
//                           resize_h_color_kernel: the horizontal pass of a call that holds items of the other models;
//                           resize_h_oriented_kernel / resize_t_kernel: the first pass of items whose displayed x runs
//                           against stored x, or down stored columns (jpeggpu_ext_resize_to_rgb_oriented)
//   resize_v_tensor_kernel  the vertical pass once more, for a model's input: bytes, float, half or bfloat16 elements,
//                           normalised as ToTensor + Normalize do, items flipped left to right where asked
//                           (jpeggpu_ext_resize_to_tensor)
//   rgb_batch_kernel /      the conversion of MANY images at their own sizes, any model and orientation, from a device table
//   rgb_batch_transposed_kernel  of items: one launch for orientations 1..4 and one for 5..8, interleaved (HWC) or planar
//                           (CHW) output (jpeggpu_ext_batch_to_rgb)
//   reduce_kernel           Pillow's Image.reduce of many images in one launch: integer box averages of the items' RGB into
//                           planes the resize passes read, the stage in front of a thumbnail's resize
//                           (jpeggpu_ext_thumbnail_to_rgb)
//
// Nothing here is shared with the decode path (jg_kernels.hip): the stage reads finished planes. What the grey output stage
// (jg_output_gray.hip) uses as well -- the staged tile, fancy_sample, the tensor element and its stores -- is in
// jg_output_device.h.
#include "jg_output.hpp"
#include "jg_output_device.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <type_traits>

namespace jg {

namespace {

/// The 4-pixel store of every RGB kernel: R, G, B of `np` (1..4) consecutive pixels, out[3 * i + c], to `drow`. Three
/// dwords when all four pixels are there and `drow` is aligned (a wave then writes 768 contiguous bytes), bytes otherwise.
__device__ __forceinline__ void store_rgb4(uint8_t* drow, const uint32_t (&out)[12], int np)
{
    if (np == 4 && (reinterpret_cast<uintptr_t>(drow) & 3) == 0) {
        uint32_t* d = reinterpret_cast<uint32_t*>(drow);
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = out[4 * k] | out[4 * k + 1] << 8 | out[4 * k + 2] << 16 | out[4 * k + 3] << 24;
    } else {
        for (int i = 0; i < 3 * np; ++i) drow[i] = static_cast<uint8_t>(out[i]);
    }
}

/// Chroma replication: each lane produces 4 consecutive output pixels of one row.
__global__ __launch_bounds__(256) void upsample_kernel(
    const uint8_t* __restrict__ src, int src_pitch, int src_w, int src_h,
    uint8_t* __restrict__ dst, int dst_pitch, int dst_w, int dst_h,
    int num_x, int den_x, int num_y, int den_y)
{
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int y  = blockIdx.y;
    if (x0 >= dst_w || y >= dst_h) return;
    const int sy        = min(y * num_y / den_y, src_h - 1);
    const uint8_t* srow = src + static_cast<size_t>(sy) * src_pitch;
    uint8_t* drow       = dst + static_cast<size_t>(y) * dst_pitch + x0;
    uint32_t px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) px[i] = srow[min((x0 + i) * num_x / den_x, src_w - 1)];
    if (x0 + 4 <= dst_w && (reinterpret_cast<uintptr_t>(drow) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(drow) = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
    } else {
        for (int i = 0; i < 4 && x0 + i < dst_w; ++i) drow[i] = static_cast<uint8_t>(px[i]);
    }
}

/// Chroma replication + YCbCr -> RGB, interleaved 8-bit output; the arithmetic of the reference's host
/// helper `conv_to_rgbi` (util/util.h:62-104): nearest-neighbour replication, the JFIF matrix in float,
/// roundf, clamp. Each lane produces 4 consecutive pixels (12 bytes) of one row. With one component the
/// sample is copied to R, G and B (util.h:47-58).
struct RgbiParams {
    const uint8_t* plane[3];
    int pitch[3], w[3], h[3];
    int num_x[3], num_y[3]; // sampling factors; the maxima are the denominators
    int den_x, den_y;
    int ncomp;
};

__global__ __launch_bounds__(256) void rgbi_kernel(RgbiParams p, uint8_t* __restrict__ dst, int dst_pitch, int width, int height)
{
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int y  = blockIdx.y;
    if (x0 >= width || y >= height) return;
    uint32_t out[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = min(x0 + i, width - 1);
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cc = c < p.ncomp ? c : 0;
            const int sy = min(y * p.num_y[cc] / p.den_y, p.h[cc] - 1);
            const int sx = min(x * p.num_x[cc] / p.den_x, p.w[cc] - 1);
            v[c]         = static_cast<float>(p.plane[cc][static_cast<size_t>(sy) * p.pitch[cc] + sx]);
        }
        float r = v[0], g = v[0], b = v[0];
        if (p.ncomp == 3) {
            r = v[0] + 1.402f * (v[2] - 128.f);
            g = v[0] - .344136f * (v[1] - 128.f) - .714136f * (v[2] - 128.f);
            b = v[0] + 1.772f * (v[1] - 128.f);
        }
        out[3 * i + 0] = static_cast<uint32_t>(fmaxf(0.f, fminf(roundf(r), 255.f)));
        out[3 * i + 1] = static_cast<uint32_t>(fmaxf(0.f, fminf(roundf(g), 255.f)));
        out[3 * i + 2] = static_cast<uint32_t>(fmaxf(0.f, fminf(roundf(b), 255.f)));
    }
    store_rgb4(dst + static_cast<size_t>(y) * dst_pitch + static_cast<size_t>(x0) * 3, out, min(4, width - x0));
}

// ------------------------------------------------------------------------------------------------
// libjpeg's fancy upsampling (jdsample.c, do_fancy_upsampling) + its integer YCbCr -> RGB (jdcolor.c, ycc_rgb_convert):
// what libjpeg-turbo gives a caller that asks for JCS_RGB. Per component, by the ratio of the largest sampling factors to
// its own (FancyComp::mode, chosen on the host): a copy or replication (int_upsample), h2v1_fancy_upsample,
// h2v2_fancy_upsample or h1v2_fancy_upsample. Samples outside the plane -- the column left of the first and right of the
// last, the row above the first and below the last -- are copies of the edge samples, which is what libjpeg's edge
// formulas and context rows amount to; the plane's extent is libjpeg's downsampled_width / downsampled_height
// (jpeggpu_decoder_parse_header's sizes), so no padding sample is read.
//
// Three steps, each written once: fancy_stage puts the samples under a tile of image pixels, with a one-sample halo, in
// LDS; fancy_pixel makes the RGB of one image pixel from the staged tiles; store_rgb4 writes four of them.
//
// `kAllModels`, a compile-time variant of all three and of the kernels built on them. false: grey and YCbCr sources, three
// tiles (7.8 KB of LDS) -- nearly every file there is. true: every colour model (FancyColor, jg_output.hpp), four tiles:
// the fourth component of a CMYK or YCCK file is upsampled like the others, by its own FancyMode.
// ------------------------------------------------------------------------------------------------

template <bool kAllModels>
struct Fancy {
    static constexpr int kComps = kAllModels ? 4 : 3; // tiles staged, and entries of the tile origins
    using Tiles = FancyTile[kComps];
};

/// Stage the samples under the image pixels (ix0, iy0) .. (ix0 + cw - 1, iy0 + ch - 1), cw <= kFancyTileW and ch <=
/// kFancyTileH: per component, samples floor(ix0 / hr) - 1 .. floor((ix0 + cw - 1) / hr) + 1 and the rows alike, at most
/// 256 + 2 columns and 8 + 2 rows (ratio 1). (bx, by)[k]: full-plane coordinates of tiles[k][0][0]. The loads are clamped
/// to the window: that is the edge rule. `kWindowed` false: the windows are the full planes (origin 0), a compile-time
/// fact. The caller's barrier makes the tiles visible.
template <bool kWindowed, bool kAllModels>
__device__ __forceinline__ void fancy_stage(
    const FancySource& s, typename Fancy<kAllModels>::Tiles& tiles, int ix0, int iy0, int cw, int ch,
    int (&bx)[Fancy<kAllModels>::kComps], int (&by)[Fancy<kAllModels>::kComps])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < Fancy<kAllModels>::kComps; ++k) {
        const FancyComp& c = s.comp[k];
        bx[k] = ix0 / c.hr - 1;
        by[k] = iy0 / c.vr - 1;
        if (k >= s.ncomp) continue;
        const int nx = (ix0 + cw - 1) / c.hr + 2 - bx[k], ny = (iy0 + ch - 1) / c.vr + 2 - by[k];
        const int ox = kWindowed ? c.ox : 0, oy = kWindowed ? c.oy : 0;
        for (int j = 0; j < ny; ++j) {
            const uint8_t* row = c.plane + static_cast<size_t>(min(max(by[k] + j - oy, 0), c.h - 1)) * c.pitch;
            for (int i = t; i < nx; i += 256) tiles[k][j][i] = row[min(max(bx[k] + i - ox, 0), c.w - 1)];
        }
    }
}

/// Pillow's cmyk2rgb (Convert.c) for one channel: K - MULDIV255(ink, K), ink and K in 0..255. The product is below 2^16.
__device__ __forceinline__ uint32_t cmyk_channel(int ink, int K)
{
    const int t = ink * K + 128;
    return clamp255(K - (((t >> 8) + t) >> 8));
}

/// R, G, B of image pixel (x, y) from the staged tiles: jdcolor.c's ycc_rgb_convert, or the grey sample three times;
/// with kAllModels also the samples as they are (RGB) and, of four components, the CMYK rule on top of either: the inks
/// are 255 - the samples (CMYK) or r, g, b themselves (YCCK).
template <bool kAllModels>
__device__ __forceinline__ void fancy_pixel(
    const FancySource& s, const typename Fancy<kAllModels>::Tiles& tiles, const int (&bx)[Fancy<kAllModels>::kComps],
    const int (&by)[Fancy<kAllModels>::kComps], int x, int y, uint32_t* rgb)
{
    const int Y = fancy_sample(s.comp[0], tiles[0], bx[0], by[0], x, y);
    if (kAllModels ? s.ncomp >= 3 : s.ncomp == 3) {
        const int c1 = fancy_sample(s.comp[1], tiles[1], bx[1], by[1], x, y);
        const int c2 = fancy_sample(s.comp[2], tiles[2], bx[2], by[2], x, y);
        const bool ycc = !kAllModels || s.color == kFancyYCbCr || s.color == kFancyYCCK;
        if (ycc) {
            const int cb = c1 - 128, cr = c2 - 128;
            rgb[0] = clamp255(Y + ((91881 * cr + (1 << 15)) >> 16));                // FIX(1.40200)
            rgb[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + (1 << 15)) >> 16)); // FIX(0.34414), FIX(0.71414)
            rgb[2] = clamp255(Y + ((116130 * cb + (1 << 15)) >> 16));               // FIX(1.77200)
        } else {
            rgb[0] = static_cast<uint32_t>(Y);
            rgb[1] = static_cast<uint32_t>(c1);
            rgb[2] = static_cast<uint32_t>(c2);
        }
        if constexpr (kAllModels) {
            if (s.ncomp == 4) {
                const int K = fancy_sample(s.comp[3], tiles[3], bx[3], by[3], x, y);
#pragma unroll
                for (int i = 0; i < 3; ++i) rgb[i] = cmyk_channel(ycc ? static_cast<int>(rgb[i]) : 255 - static_cast<int>(rgb[i]), K);
            }
        }
    } else {
        rgb[0] = rgb[1] = rgb[2] = static_cast<uint32_t>(Y);
    }
}

/// Interleaved 8-bit RGB of the source's rectangle: output pixel (x, y) is image pixel (x + p.x, y + p.y). One
/// workgroup: an output tile of kFancyTileW x kFancyTileH pixels; each lane converts a 2 x 4 quad -- 4 pixels of 2 rows
/// -- and stores each row's 12 bytes. `kWindowed` false is the whole image, whose window and rectangle terms are zero
/// and cost nothing. The two kernels below are its instantiations by name: fancy_rgbi_kernel for grey and YCbCr sources,
/// fancy_color_kernel for every model.
template <bool kWindowed, bool kAllModels>
__device__ __forceinline__ void fancy_rgbi_tile(const FancySource& p, uint8_t* dst, int dst_pitch, int width, int height)
{
    __shared__ typename Fancy<kAllModels>::Tiles s_t;
    const int t  = threadIdx.x;
    const int x0 = blockIdx.x * kFancyTileW, y0 = blockIdx.y * kFancyTileH;
    const int px = kWindowed ? p.x : 0, py = kWindowed ? p.y : 0;
    int bx[Fancy<kAllModels>::kComps], by[Fancy<kAllModels>::kComps];
    fancy_stage<kWindowed, kAllModels>(p, s_t, x0 + px, y0 + py, kFancyTileW, kFancyTileH, bx, by);
    __syncthreads();
    const int x = x0 + 4 * (t & 63);
    if (x >= width) return;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = y0 + 2 * (t >> 6) + dy;
        if (y >= height) break;
        uint32_t out[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) fancy_pixel<kAllModels>(p, s_t, bx, by, min(x + i, width - 1) + px, y + py, &out[3 * i]);
        store_rgb4(dst + static_cast<size_t>(y) * dst_pitch + static_cast<size_t>(x) * 3, out, min(4, width - x));
    }
}

template <bool kWindowed>
__global__ __launch_bounds__(256) void fancy_rgbi_kernel(FancySource p, uint8_t* __restrict__ dst, int dst_pitch, int width, int height)
{
    fancy_rgbi_tile<kWindowed, false>(p, dst, dst_pitch, width, height);
}

template <bool kWindowed>
__global__ __launch_bounds__(256) void fancy_color_kernel(FancySource p, uint8_t* __restrict__ dst, int dst_pitch, int width, int height)
{
    fancy_rgbi_tile<kWindowed, true>(p, dst, dst_pitch, width, height);
}

// ------------------------------------------------------------------------------------------------
// The same conversion written where an EXIF orientation displays it (jpeggpu_ext.h has the table). Upsampling and colour
// conversion stay in stored coordinates -- fancy_stage, fancy_sample and fancy_pixel as they are -- and only the place a
// pixel is written changes. `flips`: bit 0, displayed x runs against the stored axis it lies along; bit 1, displayed y.
// ------------------------------------------------------------------------------------------------

/// Orientations 2..4: fancy_rgbi_tile's tile and quads; a lane's four pixels are made in displayed order and stored at
/// the mirrored position, so a wave still writes one contiguous run per row (dwords if the mirrored start is aligned).
template <bool kWindowed, bool kAllModels>
__device__ __forceinline__ void fancy_mirrored_tile(const FancySource& p, uint8_t* dst, int dst_pitch, int width, int height, int flips)
{
    __shared__ typename Fancy<kAllModels>::Tiles s_t;
    const int t  = threadIdx.x;
    const int x0 = blockIdx.x * kFancyTileW, y0 = blockIdx.y * kFancyTileH;
    const int px = kWindowed ? p.x : 0, py = kWindowed ? p.y : 0;
    int bx[Fancy<kAllModels>::kComps], by[Fancy<kAllModels>::kComps];
    fancy_stage<kWindowed, kAllModels>(p, s_t, x0 + px, y0 + py, kFancyTileW, kFancyTileH, bx, by);
    __syncthreads();
    const int x = x0 + 4 * (t & 63);
    if (x >= width) return;
    const int np = min(4, width - x);
    const bool mx = flips & 1, my = flips & 2;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = y0 + 2 * (t >> 6) + dy;
        if (y >= height) break;
        uint32_t out[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) { // displayed pixel i of the lane's run: stored x + np - 1 - i when mirrored
            const int xs = mx ? max(x + np - 1 - i, x) : min(x + i, width - 1);
            fancy_pixel<kAllModels>(p, s_t, bx, by, xs + px, y + py, &out[3 * i]);
        }
        store_rgb4(dst + static_cast<size_t>(my ? height - 1 - y : y) * dst_pitch + static_cast<size_t>(mx ? width - x - np : x) * 3, out, np);
    }
}

template <bool kWindowed, bool kAllModels>
__global__ __launch_bounds__(256) void fancy_mirrored_kernel(FancySource p, uint8_t* __restrict__ dst, int dst_pitch, int width, int height, int flips)
{
    fancy_mirrored_tile<kWindowed, kAllModels>(p, dst, dst_pitch, width, height, flips);
}

/// Orientations 5..8: stored rows become displayed columns. The row kernel's 256 x 8 tile written transposed would store
/// 24 bytes per displayed row, so a workgroup takes kOrientTile x kOrientTile stored pixels: eight strips of 64 x 8 are
/// staged and converted as ever, and their RGB (one dword per pixel) is kept in LDS, s_rgb[stored y][stored x], rows
/// kOrientTile + 1 dwords apart -- the write-out reads it down a column, 65 dwords from lane to lane, which is one bank on
/// (64 banks of 4 bytes), so neither side conflicts. Then one wave per displayed row: the row's 3 x 64 = 192 contiguous
/// bytes as 48 dwords (49 if the row does not start on a dword: the two ends go out as bytes), each put together from
/// the two pixels it overlaps. LDS per workgroup: 16640 bytes of s_rgb + the staged tiles (7800, or 10400 for all models).
template <bool kWindowed, bool kAllModels>
__device__ __forceinline__ void fancy_transposed_tile(const FancySource& p, uint8_t* dst, int dst_pitch, int width, int height, int flips)
{
    __shared__ typename Fancy<kAllModels>::Tiles s_t;
    __shared__ uint32_t s_rgb[kOrientTile][kOrientTile + 1];
    const int t  = threadIdx.x;
    const int x0 = blockIdx.x * kOrientTile, y0 = blockIdx.y * kOrientTile;
    const int nw = min(kOrientTile, width - x0), nh = min(kOrientTile, height - y0);
    const int px = kWindowed ? p.x : 0, py = kWindowed ? p.y : 0;
    for (int s0 = 0; s0 < nh; s0 += kFancyTileH) {
        const int ch = min(kFancyTileH, nh - s0);
        int bx[Fancy<kAllModels>::kComps], by[Fancy<kAllModels>::kComps];
        fancy_stage<kWindowed, kAllModels>(p, s_t, x0 + px, y0 + s0 + py, nw, ch, bx, by);
        __syncthreads();
        for (int q = t; q < kFancyTileH * kOrientTile; q += 256) {
            const int qy = q / kOrientTile, qx = q % kOrientTile;
            if (qy >= ch || qx >= nw) continue;
            uint32_t rgb[3];
            fancy_pixel<kAllModels>(p, s_t, bx, by, x0 + qx + px, y0 + s0 + qy + py, rgb);
            s_rgb[s0 + qy][qx] = rgb[0] | rgb[1] << 8 | rgb[2] << 16;
        }
        __syncthreads(); // the next strip's staging overwrites the tiles; the last one: s_rgb is complete
    }
    const bool mx = flips & 1, my = flips & 2;
    const int ox0 = mx ? height - y0 - nh : y0; // the displayed columns of the tile's stored rows, nh of them
    const int nbytes = 3 * nh, lane = t & 63;
    for (int row = t >> 6; row < nw; row += 4) { // displayed row: stored column x0 + row
        const int oy = my ? width - 1 - (x0 + row) : x0 + row;
        uint8_t* a   = dst + static_cast<size_t>(oy) * dst_pitch + static_cast<size_t>(ox0) * 3;
        const int b0 = 4 * lane - static_cast<int>(reinterpret_cast<uintptr_t>(a) & 3); // the lane's dword: bytes b0 .. b0 + 3 of the run
        if (b0 + 4 <= 0 || b0 >= nbytes) continue;
        if (b0 >= 0 && b0 + 4 <= nbytes) { // pixels b0 / 3 and the next hold its four bytes
            const int p0 = b0 / 3, r = b0 - 3 * p0;
            const uint32_t v0 = s_rgb[mx ? nh - 1 - p0 : p0][row], v1 = s_rgb[mx ? nh - 2 - p0 : p0 + 1][row];
            *reinterpret_cast<uint32_t*>(a + b0) = static_cast<uint32_t>((v0 | static_cast<uint64_t>(v1) << 24) >> (8 * r));
        } else {
            for (int b = max(b0, 0); b < min(b0 + 4, nbytes); ++b) {
                const int pi = b / 3;
                a[b] = static_cast<uint8_t>(s_rgb[mx ? nh - 1 - pi : pi][row] >> (8 * (b - 3 * pi)));
            }
        }
    }
}

template <bool kWindowed, bool kAllModels>
__global__ __launch_bounds__(256) void fancy_transposed_kernel(FancySource p, uint8_t* __restrict__ dst, int dst_pitch, int width, int height, int flips)
{
    fancy_transposed_tile<kWindowed, kAllModels>(p, dst, dst_pitch, width, height, flips);
}

/// Taps of a horizontal-pass workgroup's columns: int32 weights[columns][taps], from LDS when they fit
/// (kResizeLdsTaps per column) or else straight from the table; RGB of a chunk: one dword (R | G << 8 | B << 16) per pixel.
/// A product of a weight (|w| < 2^23: normalised weights stay below 1.2) and a sample fits v_mul_i32_i24.
template <class W>
__device__ __forceinline__ void resize_taps_h(const W* w, const uint32_t* px, int j0, int j1, int (&acc)[3])
{
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {
        const int wj = w[j];
        const uint32_t v = px[j];
        acc[0] += __mul24(wj, static_cast<int>(v & 255u));
        acc[1] += __mul24(wj, static_cast<int>((v >> 8) & 255u));
        acc[2] += __mul24(wj, static_cast<int>((v >> 16) & 255u));
    }
}

/// Batched resize (jpeggpu_ext_resize_to_rgb), pass 1: the horizontal taps, read from the planes' windows. A workgroup
/// owns kResizeHTileW output columns of kResizeHTileH rectangle rows of one item (found by a search of the items' first
/// tiles). The input columns those columns' taps read are converted to RGB in chunks of up to kFancyTileW: the window
/// samples under a chunk are staged with their halo (fancy_stage), each pixel gets fancy_pixel into LDS, and each lane
/// accumulates its output pixel's taps that fall in the chunk. The result is clamped to uint8 (Pillow keeps its
/// intermediate image in 8 bits) and written to the item's `mid` rows; the crop's full-resolution RGB never leaves LDS.
/// `kAllModels` (resize_h_color_kernel): a call with an item that is not grey or YCbCr; its items of those two models are
/// converted as ever. resize_h_kernel is the instantiation for calls of grey and YCbCr items alone. (The pointers are
/// __restrict__ on the kernels only: the qualifier repeated here cost resize_h_kernel ten VGPRs once inlined.)
/// `kOriented` (resize_h_oriented_kernel): an item may carry kResizeMirrorStore, and its result then goes to the mirrored
/// column of `mid`.
template <bool kAllModels, bool kOriented = false>
__device__ __forceinline__ void resize_h_tile(
    const ResizeJob* jobs, const int* first_tile, int n, int out_w, typename Fancy<kAllModels>::Tiles& s_t,
    uint32_t (&s_rgb)[kResizeHTileH][kFancyTileW], int (&s_w)[kResizeHTileW * kResizeLdsTaps])
{
    const int b = blockIdx.x;
    int lo = 0, hi = n - 1; // the last item whose first tile is <= b
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (first_tile[m] <= b) lo = m;
        else hi = m - 1;
    }
    const ResizeJob& J = jobs[lo];
    const int col_tiles = (out_w + kResizeHTileW - 1) / kResizeHTileW;
    const int tile = b - first_tile[lo], ty = tile / col_tiles, tx = tile - ty * col_tiles;
    const int r0 = J.row0 + ty * kResizeHTileH;                  // the tile's first rectangle row
    const int nr = min(kResizeHTileH, J.row0 + J.rows - r0);
    const int ox0 = tx * kResizeHTileW, ox1 = min(ox0 + kResizeHTileW, out_w) - 1;
    const int* __restrict__ tab = J.tab_x;
    const int a = tab[2 * ox0], e = tab[2 * ox1] + tab[2 * ox1 + 1]; // input columns [a, e) (first and last are monotone)
    const FancySource& src = J.src;
    const int t = threadIdx.x, r = t / kResizeHTileW, col = t % kResizeHTileW, ox = ox0 + col;
    const bool mine = r < nr && ox < out_w;
    const int taps = J.taps_x;
    const bool lds_w = taps <= kResizeLdsTaps;
    const int* __restrict__ wts = tab + 2 * out_w + static_cast<size_t>(ox0) * taps; // the tile's columns are consecutive
    if (lds_w) // made visible by the chunk loop's first barrier
        for (int q = t; q < (ox1 - ox0 + 1) * taps; q += 256) s_w[q] = wts[q];
    int f = 0, cnt = 0;
    if (mine) {
        f   = tab[2 * ox];
        cnt = tab[2 * ox + 1];
    }
    int acc[3] = {0, 0, 0};
    for (int c0 = a; c0 < e; c0 += kFancyTileW) {
        const int cw  = min(kFancyTileW, e - c0);
        const int ix0 = c0 + src.x, iy0 = r0 + src.y; // the chunk's origin in the image
        int bx[Fancy<kAllModels>::kComps], by[Fancy<kAllModels>::kComps];
        fancy_stage<true, kAllModels>(src, s_t, ix0, iy0, cw, nr, bx, by);
        __syncthreads();
        for (int q = t; q < kResizeHTileH * kFancyTileW; q += 256) {
            const int qy = q / kFancyTileW, qx = q % kFancyTileW;
            if (qy >= nr || qx >= cw) continue;
            uint32_t rgb[3];
            fancy_pixel<kAllModels>(src, s_t, bx, by, ix0 + qx, iy0 + qy, rgb);
            s_rgb[qy][qx] = rgb[0] | rgb[1] << 8 | rgb[2] << 16;
        }
        __syncthreads();
        if (mine) { // taps j0 .. j1 - 1 of the column, relative to its first, lie in this chunk
            const int j0 = max(f, c0) - f, j1 = min(f + cnt, c0 + cw) - f;
            const uint32_t* px = &s_rgb[r][f - c0];
            if (lds_w) resize_taps_h(&s_w[col * taps], px, j0, j1, acc);
            else resize_taps_h(wts + static_cast<size_t>(col) * taps, px, j0, j1, acc);
        }
        __syncthreads();
    }
    if (mine) {
        int sx = ox;
        if constexpr (kOriented) sx = (J.pad_ & kResizeMirrorStore) ? out_w - 1 - ox : ox;
        uint8_t* o = J.mid + static_cast<size_t>(r0 - J.row0 + r) * J.mid_pitch + 3 * sx;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = static_cast<uint8_t>(clamp255((acc[c] + (1 << 21)) >> 22));
    }
}

__global__ __launch_bounds__(256) void resize_h_kernel(const ResizeJob* __restrict__ jobs, const int* __restrict__ first_tile, int n, int out_w)
{
    __shared__ Fancy<false>::Tiles s_t;
    __shared__ uint32_t s_rgb[kResizeHTileH][kFancyTileW];
    __shared__ int s_w[kResizeHTileW * kResizeLdsTaps];
    resize_h_tile<false>(jobs, first_tile, n, out_w, s_t, s_rgb, s_w);
}

__global__ __launch_bounds__(256) void resize_h_color_kernel(const ResizeJob* __restrict__ jobs, const int* __restrict__ first_tile, int n, int out_w)
{
    __shared__ Fancy<true>::Tiles s_t;
    __shared__ uint32_t s_rgb[kResizeHTileH][kFancyTileW];
    __shared__ int s_w[kResizeHTileW * kResizeLdsTaps];
    resize_h_tile<true>(jobs, first_tile, n, out_w, s_t, s_rgb, s_w);
}

template <bool kAllModels>
__global__ __launch_bounds__(256) void resize_h_oriented_kernel(const ResizeJob* __restrict__ jobs, const int* __restrict__ first_tile, int n, int out_w)
{
    __shared__ typename Fancy<kAllModels>::Tiles s_t;
    __shared__ uint32_t s_rgb[kResizeHTileH][kFancyTileW];
    __shared__ int s_w[kResizeHTileW * kResizeLdsTaps];
    resize_h_tile<kAllModels, true>(jobs, first_tile, n, out_w, s_t, s_rgb, s_w);
}

/// Batched resize, the first pass of an item with orientation 5..8: Pillow's first, rounded pass runs along displayed x,
/// which is stored y, so the taps (tab_x, permuted by the host for stored rows) run down stored columns, and a row of
/// `mid` -- a displayed row -- is a stored column of the rectangle (J.row0 / J.rows count those). A workgroup owns up to
/// kResizeTTileW stored columns, one per lane, and kResizeTTileK output columns: the stored rows their taps read are staged
/// in strips of kFancyTileH (fancy_stage as ever), each lane converts its column's pixel of a strip row (fancy_pixel) and
/// adds it to the output columns whose taps hold that row -- the tap ranges and weights are the same for every lane, so
/// the tests are uniform and the weights broadcast. No RGB goes through LDS or global memory. A lane then writes its 3 x
/// kResizeTTileK bytes of `mid`. What bounds it: the staging of a strip (one barrier pair per eight stored rows, for 256
/// columns) and the K uniform tests per pixel; see DESIGN.md, f-9.
template <bool kAllModels>
__device__ __forceinline__ void resize_t_tile(
    const ResizeJob* jobs, const int* first_tile, int n, int out_w, typename Fancy<kAllModels>::Tiles& s_t,
    int (&s_w)[kResizeTTileK * kResizeLdsTaps])
{
    constexpr int K = kResizeTTileK;
    const int b = blockIdx.x;
    int lo = 0, hi = n - 1; // the last item whose first tile is <= b (items of the other kind have no tiles)
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (first_tile[m] <= b) lo = m;
        else hi = m - 1;
    }
    const ResizeJob& J = jobs[lo];
    const int k_tiles = (out_w + K - 1) / K;
    const int tile = b - first_tile[lo], tc = tile / k_tiles, tk = tile - tc * k_tiles;
    const int c0 = J.row0 + tc * kResizeTTileW; // the tile's first stored column of the rectangle
    const int cw = min(kResizeTTileW, J.row0 + J.rows - c0);
    const int ox0 = tk * K, nk = min(K, out_w - ox0);
    const int* __restrict__ tab = J.tab_x;
    const FancySource& src = J.src;
    const int t = threadIdx.x, taps = J.taps_x;
    const bool lds_w = taps <= kResizeLdsTaps;
    const int* __restrict__ wts = tab + 2 * out_w + static_cast<size_t>(ox0) * taps;
    if (lds_w) // made visible by the strip loop's first barrier
        for (int q = t; q < nk * taps; q += 256) s_w[q] = wts[q];
    int f[K], cnt[K], a = 0x7fffffff, e = 0; // stored rows [a, e): what the K columns' taps read (any order of the columns)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        f[k] = cnt[k] = 0;
        if (k < nk) {
            f[k]   = tab[2 * (ox0 + k)];
            cnt[k] = tab[2 * (ox0 + k) + 1];
            a      = min(a, f[k]);
            e      = max(e, f[k] + cnt[k]);
        }
    }
    int acc[K][3];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0;
    for (int r = a; r < e; r += kFancyTileH) {
        const int ch  = min(kFancyTileH, e - r);
        const int ix0 = c0 + src.x, iy0 = r + src.y; // the strip's origin in the image
        int bx[Fancy<kAllModels>::kComps], by[Fancy<kAllModels>::kComps];
        fancy_stage<true, kAllModels>(src, s_t, ix0, iy0, cw, ch, bx, by);
        __syncthreads();
        if (t < cw) {
            for (int rr = 0; rr < ch; ++rr) {
                uint32_t rgb[3];
                fancy_pixel<kAllModels>(src, s_t, bx, by, ix0 + t, iy0 + rr, rgb);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int j = r + rr - f[k];
                    if (j < 0 || j >= cnt[k]) continue;
                    const int wj = lds_w ? s_w[k * taps + j] : wts[static_cast<size_t>(k) * taps + j];
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[k][c] += mul24(wj, static_cast<int>(rgb[c]));
                }
            }
        }
        __syncthreads();
    }
    if (t >= cw) return;
    uint32_t v[3 * K];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * k + c] = clamp255((acc[k][c] + (1 << 21)) >> 22);
    uint8_t* o = J.mid + static_cast<size_t>(c0 - J.row0 + t) * J.mid_pitch + 3 * ox0; // 8-byte aligned: 3 K = 24 bytes per tile
    if (nk == K) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int d = 0; d < 3 * K / 4; ++d) o4[d] = v[4 * d] | v[4 * d + 1] << 8 | v[4 * d + 2] << 16 | v[4 * d + 3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 3 * K; ++k)
            if (k < 3 * nk) o[k] = static_cast<uint8_t>(v[k]);
    }
}

template <bool kAllModels>
__global__ __launch_bounds__(256) void resize_t_kernel(const ResizeJob* __restrict__ jobs, const int* __restrict__ first_tile, int n, int out_w)
{
    __shared__ typename Fancy<kAllModels>::Tiles s_t;
    __shared__ int s_w[kResizeTTileK * kResizeLdsTaps];
    resize_t_tile<kAllModels>(jobs, first_tile, n, out_w, s_t, s_w);
}

/// Batched resize, pass 2: the vertical taps over the items' `mid` rows, one item per blockIdx.y. Each lane makes 4
/// consecutive output pixels of one row (3 dword loads per tap row), so a wave stores 768 contiguous bytes in NHWC, or
/// 256 per channel plane in NCHW.
__global__ __launch_bounds__(256) void resize_v_kernel(const ResizeJob* __restrict__ jobs, int out_w, int out_h, int layout, uint8_t* __restrict__ dst)
{
    const ResizeJob& J = jobs[blockIdx.y];
    const int col_tiles = (out_w + kResizeVTileW - 1) / kResizeVTileW;
    const int t = threadIdx.x;
    const int x = (blockIdx.x % col_tiles) * kResizeVTileW + 4 * (t & 63);
    const int y = (blockIdx.x / col_tiles) * kResizeVTileH + (t >> 6);
    if (x >= out_w || y >= out_h) return;
    const int* __restrict__ tab = J.tab_y;
    const int f = tab[2 * y] - J.row0, cnt = tab[2 * y + 1];
    const int* __restrict__ wts = tab + 2 * out_h + static_cast<size_t>(y) * J.taps_y;
    const int np = min(4, out_w - x); // pixels of this lane
    int acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0;
    for (int j = 0; j < cnt; ++j) {
        const int w = wts[j];
        const uint8_t* s = J.mid + static_cast<size_t>(f + j) * J.mid_pitch + 3 * x; // 4-byte aligned: mid_pitch % 16 == 0
        if (np == 4) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const uint32_t v = s4[d];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[4 * d + k] += __mul24(w, static_cast<int>((v >> (8 * k)) & 255u));
            }
        } else {
            for (int k = 0; k < 3 * np; ++k) acc[k] += __mul24(w, static_cast<int>(s[k]));
        }
    }
    uint32_t o[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = clamp255((acc[k] + (1 << 21)) >> 22);
    const size_t item = blockIdx.y;
    if (layout == 0) {
        store_rgb4(dst + ((item * out_h + y) * out_w + x) * 3, o, np);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t* d = dst + ((item * 3 + c) * out_h + y) * out_w + x;
            if (np == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
                *reinterpret_cast<uint32_t*>(d) = o[c] | o[3 + c] << 8 | o[6 + c] << 16 | o[9 + c] << 24;
            } else {
                for (int i = 0; i < np; ++i) d[i] = static_cast<uint8_t>(o[3 * i + c]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The vertical pass that writes a model's input (jpeggpu_ext_resize_to_tensor): resize_v_kernel's tile, taps and clamp,
// then -- with the lane's twelve finished bytes still in registers -- the flip, the normalisation and the cast, so the
// batch is written once, as the elements the model reads. The tile body is written again here and not shared with
// resize_v_kernel: that one is to come out of the compiler as it was (the compile check).
// ------------------------------------------------------------------------------------------------

/// Batched resize, pass 2 for a tensor: resize_v_kernel's tile (kResizeVTileW x kResizeVTileH output pixels per workgroup,
/// 4 consecutive pixels of one row per lane, one item per blockIdx.y), its taps over `mid` and its clamp. What differs:
///   * an item with kResizeFlipOutput reads `mid` mirrored: output column x is column out_w - 1 - x of the unflipped
///     result (torch.flip AFTER the resize, not a resize of the mirrored source -- mirror_taps says why those differ).
///     The lane's 12 bytes then start at 3 (out_w - 4 - x), on a dword only if out_w % 4 == 0: three dword loads then,
///     and the four pixels change places in registers; for other widths every lane of a flipped item loads bytes, as
///     the last lane of a row with fewer than four pixels always does.
///   * the twelve bytes become elements of T (tensor_bits) and go out as whole runs (tensor_store_run): NHWC the lane's 12
///     contiguous elements (12, 24 or 48 bytes), NCHW (kPlanar) four elements per channel plane (4, 8 or 16 bytes, one
///     store); per element where the lane has fewer than four pixels or the address is not on a dword. `dst` is aligned
///     to the element only and rows are unpadded, so for bytes and halves with out_w % 4 != 0 most rows go out per element.
template <class T, bool kPlanar>
__global__ __launch_bounds__(256) void resize_v_tensor_kernel(const ResizeJob* __restrict__ jobs, int out_w, int out_h, TensorNorm nm, T* __restrict__ dst)
{
    constexpr int S = sizeof(T);
    const ResizeJob& J = jobs[blockIdx.y];
    const int col_tiles = (out_w + kResizeVTileW - 1) / kResizeVTileW;
    const int t = threadIdx.x;
    const int x = (blockIdx.x % col_tiles) * kResizeVTileW + 4 * (t & 63);
    const int y = (blockIdx.x / col_tiles) * kResizeVTileH + (t >> 6);
    if (x >= out_w || y >= out_h) return;
    const int* __restrict__ tab = J.tab_y;
    const int f = tab[2 * y] - J.row0, cnt = tab[2 * y + 1];
    const int* __restrict__ wts = tab + 2 * out_h + static_cast<size_t>(y) * J.taps_y;
    const int np = min(4, out_w - x); // pixels of this lane
    const bool flip = (J.pad_ & kResizeFlipOutput) != 0;
    const bool dwords = np == 4 && (!flip || (out_w & 3) == 0);
    // dwords: the lane's four mid columns start at c0, ascending; bytes: output pixel i is mid column c0 + i or c0 - i
    const int c0 = !flip ? x : dwords ? out_w - 4 - x : out_w - 1 - x;
    const int step = flip ? -3 : 3;
    int acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0;
    for (int j = 0; j < cnt; ++j) {
        const int w = wts[j];
        const uint8_t* s = J.mid + static_cast<size_t>(f + j) * J.mid_pitch + 3 * c0; // dwords: 4-byte aligned, mid_pitch % 16 == 0
        if (dwords) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const uint32_t v = s4[d];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[4 * d + k] += mul24(w, static_cast<int>((v >> (8 * k)) & 255u));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < np) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[3 * i + c] += mul24(w, static_cast<int>(s[step * i + c]));
                }
            }
        }
    }
    if (flip && dwords) { // the dword loads took the pixels in mid's order: 0 <-> 3, 1 <-> 2 (swaps of values: a selected INDEX
                          // into acc would be a runtime index into registers)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int a0 = acc[c], a1 = acc[3 + c];
            acc[c]     = acc[9 + c];
            acc[3 + c] = acc[6 + c];
            acc[6 + c] = a1;
            acc[9 + c] = a0;
        }
    }
    uint32_t e[12];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) e[3 * i + c] = tensor_bits<T>(clamp255((acc[3 * i + c] + (1 << 21)) >> 22), nm.mean[c], nm.std[c]);
    const size_t item = blockIdx.y;
    if constexpr (!kPlanar) {
        tensor_store_run<S, 12>(reinterpret_cast<uint8_t*>(dst + ((item * out_h + y) * out_w + x) * 3), e, 3 * np);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t ec[4] = {e[c], e[3 + c], e[6 + c], e[9 + c]};
            tensor_store_run<S, 4>(reinterpret_cast<uint8_t*>(dst + ((item * 3 + c) * out_h + y) * out_w + x), ec, np);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Batched conversion at the items' own sizes (jpeggpu_ext_batch_to_rgb): the tiles of fancy_mirrored_tile and
// fancy_transposed_tile over a device table of items, the way the resize passes find theirs. The tile bodies are written
// again here, on fancy_stage / fancy_pixel / store_rgb4, and not shared with the per-image kernels above: those are to come
// out of the compiler as they were (the compile check). `kPlanar`: the output is three planes (CHW).
// ------------------------------------------------------------------------------------------------

static_assert(kRgbBatchTileW == kFancyTileW && kRgbBatchTileH == kFancyTileH, "the host counts the row kernel's tiles");

/// Orientations 1..4 of a batch: one kFancyTileW x kFancyTileH tile of one item per workgroup, each lane a 2 x 4 quad stored
/// where `flips` displays it (0: fancy_rgbi_tile's store). Only the samples under the tile's part of the rectangle are
/// staged. Planar: a lane's four pixels are four consecutive bytes of each channel plane -- one dword per channel where
/// the run is whole and aligned (a wave then writes 256 contiguous bytes per plane), bytes otherwise: store_rgb4's rule.
template <bool kAllModels, bool kPlanar>
__global__ __launch_bounds__(256) void rgb_batch_kernel(const RgbJob* __restrict__ jobs, const int* __restrict__ first_tile, int n)
{
    __shared__ typename Fancy<kAllModels>::Tiles s_t;
    const int b = blockIdx.x, item = rgb_batch_item(first_tile, n, b);
    const RgbJob& J = jobs[item];
    const FancySource& p = J.src;
    const int tile = b - first_tile[item], ty = tile / J.tiles_x, tx = tile - ty * J.tiles_x;
    const int width = J.width, height = J.height;
    const int t  = threadIdx.x;
    const int x0 = tx * kFancyTileW, y0 = ty * kFancyTileH;
    const int px = p.x, py = p.y;
    int bx[Fancy<kAllModels>::kComps], by[Fancy<kAllModels>::kComps];
    fancy_stage<true, kAllModels>(p, s_t, x0 + px, y0 + py, min(kFancyTileW, width - x0), min(kFancyTileH, height - y0), bx, by);
    __syncthreads();
    const int x = x0 + 4 * (t & 63);
    if (x >= width) return;
    const int np = min(4, width - x);
    const int flips = J.flips;
    const bool mx = flips & 1, my = flips & 2;
    uint8_t* dst = J.dst;
    const int dst_pitch = J.dst_pitch;
    const size_t xd = static_cast<size_t>(mx ? width - x - np : x);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = y0 + 2 * (t >> 6) + dy;
        if (y >= height) break;
        uint32_t out[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) { // displayed pixel i of the lane's run: stored x + np - 1 - i when mirrored
            const int xs = mx ? max(x + np - 1 - i, x) : min(x + i, width - 1);
            fancy_pixel<kAllModels>(p, s_t, bx, by, xs + px, y + py, &out[3 * i]);
        }
        uint8_t* drow = dst + static_cast<size_t>(my ? height - 1 - y : y) * dst_pitch;
        if constexpr (!kPlanar) {
            store_rgb4(drow + xd * 3, out, np);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                uint8_t* d = drow + c * J.plane_stride + xd;
                if (np == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
                    *reinterpret_cast<uint32_t*>(d) = out[c] | out[3 + c] << 8 | out[6 + c] << 16 | out[9 + c] << 24;
                } else {
                    for (int i = 0; i < np; ++i) d[i] = static_cast<uint8_t>(out[3 * i + c]);
                }
            }
        }
    }
}

/// Orientations 5..8 of a batch: fancy_transposed_tile's body over one kOrientTile x kOrientTile tile of one item. Planar:
/// a displayed row of the tile is nh <= 64 contiguous bytes in each of the three planes, and ONE wave instruction stores
/// all three runs: lane 17 c + g writes dword g of channel c's run (17, not 16: a run that does not start on a dword
/// spills into one more; its two ends go out as bytes), put together from byte c of four pixels of s_rgb. Those four LDS
/// reads go down a column: pixel q of the row is dword 65 q + row, bank (q + row) mod 32 for ds_read_b32, and a lane's
/// pixels are 4 g + k, so lanes g and g + 8 of a channel meet on a bank (the three channels read the same dwords, which
/// broadcast): 2- to 3-way on four reads a row, against a third of the store instructions of a pixel-per-lane write-out.
template <bool kAllModels, bool kPlanar>
__global__ __launch_bounds__(256) void rgb_batch_transposed_kernel(const RgbJob* __restrict__ jobs, const int* __restrict__ first_tile, int n)
{
    __shared__ typename Fancy<kAllModels>::Tiles s_t;
    __shared__ uint32_t s_rgb[kOrientTile][kOrientTile + 1];
    const int b = blockIdx.x, item = rgb_batch_item(first_tile, n, b);
    const RgbJob& J = jobs[item];
    const FancySource& p = J.src;
    const int tile = b - first_tile[item], ty = tile / J.tiles_x, tx = tile - ty * J.tiles_x;
    const int width = J.width, height = J.height;
    const int t  = threadIdx.x;
    const int x0 = tx * kOrientTile, y0 = ty * kOrientTile;
    const int nw = min(kOrientTile, width - x0), nh = min(kOrientTile, height - y0);
    const int px = p.x, py = p.y;
    for (int s0 = 0; s0 < nh; s0 += kFancyTileH) {
        const int ch = min(kFancyTileH, nh - s0);
        int bx[Fancy<kAllModels>::kComps], by[Fancy<kAllModels>::kComps];
        fancy_stage<true, kAllModels>(p, s_t, x0 + px, y0 + s0 + py, nw, ch, bx, by);
        __syncthreads();
        for (int q = t; q < kFancyTileH * kOrientTile; q += 256) {
            const int qy = q / kOrientTile, qx = q % kOrientTile;
            if (qy >= ch || qx >= nw) continue;
            uint32_t rgb[3];
            fancy_pixel<kAllModels>(p, s_t, bx, by, x0 + qx + px, y0 + s0 + qy + py, rgb);
            s_rgb[s0 + qy][qx] = rgb[0] | rgb[1] << 8 | rgb[2] << 16;
        }
        __syncthreads(); // the next strip's staging overwrites the tiles; the last one: s_rgb is complete
    }
    const int flips = J.flips;
    const bool mx = flips & 1, my = flips & 2;
    const int ox0 = mx ? height - y0 - nh : y0; // the displayed columns of the tile's stored rows, nh of them
    const int lane = t & 63;
    uint8_t* dst = J.dst;
    const int dst_pitch = J.dst_pitch;
    if constexpr (!kPlanar) {
        const int nbytes = 3 * nh;
        for (int row = t >> 6; row < nw; row += 4) { // displayed row: stored column x0 + row
            const int oy = my ? width - 1 - (x0 + row) : x0 + row;
            uint8_t* a   = dst + static_cast<size_t>(oy) * dst_pitch + static_cast<size_t>(ox0) * 3;
            const int b0 = 4 * lane - static_cast<int>(reinterpret_cast<uintptr_t>(a) & 3); // the lane's dword: bytes b0 .. b0 + 3 of the run
            if (b0 + 4 <= 0 || b0 >= nbytes) continue;
            if (b0 >= 0 && b0 + 4 <= nbytes) { // pixels b0 / 3 and the next hold its four bytes
                const int p0 = b0 / 3, r = b0 - 3 * p0;
                const uint32_t v0 = s_rgb[mx ? nh - 1 - p0 : p0][row], v1 = s_rgb[mx ? nh - 2 - p0 : p0 + 1][row];
                *reinterpret_cast<uint32_t*>(a + b0) = static_cast<uint32_t>((v0 | static_cast<uint64_t>(v1) << 24) >> (8 * r));
            } else {
                for (int k = max(b0, 0); k < min(b0 + 4, nbytes); ++k) {
                    const int pi = k / 3;
                    a[k] = static_cast<uint8_t>(s_rgb[mx ? nh - 1 - pi : pi][row] >> (8 * (k - 3 * pi)));
                }
            }
        }
    } else {
        const int c = lane / 17, g = lane - 17 * c;
        if (c >= 3) return;
        const size_t plane = c * J.plane_stride;
        for (int row = t >> 6; row < nw; row += 4) {
            const int oy = my ? width - 1 - (x0 + row) : x0 + row;
            uint8_t* a   = dst + plane + static_cast<size_t>(oy) * dst_pitch + ox0;
            const int b0 = 4 * g - static_cast<int>(reinterpret_cast<uintptr_t>(a) & 3); // the lane's dword: pixels b0 .. b0 + 3 of the run
            if (b0 + 4 <= 0 || b0 >= nh) continue;
            if (b0 >= 0 && b0 + 4 <= nh) {
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) v |= ((s_rgb[mx ? nh - 1 - (b0 + k) : b0 + k][row] >> (8 * c)) & 255u) << (8 * k);
                *reinterpret_cast<uint32_t*>(a + b0) = v;
            } else {
                for (int k = max(b0, 0); k < min(b0 + 4, nh); ++k) a[k] = static_cast<uint8_t>(s_rgb[mx ? nh - 1 - k : k][row] >> (8 * c));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Box reduction in front of a thumbnail's resize (jpeggpu_ext_thumbnail_to_rgb): Pillow's Image.reduce((fx, fy)) of every
// item that has factors, from a device table of items and a tile list like the batched conversion's. The source is read
// as everywhere else -- fancy_stage, fancy_pixel -- so an item's full RGB at its decoded size is never written: only the
// reduced planes are, which the resize passes then read as an RGB-coded (or grey) source with factors 1.
// ------------------------------------------------------------------------------------------------

/// One workgroup: kReduceTileW reduced columns of J.rows_per_tile reduced rows of one item. The source pixels under them
/// are taken in chunks of kFancyTileW columns, and a chunk in rounds of kFancyTileH rows: a lane owns one source column of
/// the chunk, converts its pixel of every staged row and keeps the column's sum in registers until a box ends (its last
/// row, or the image's), then adds it to the box's sum in LDS -- fx lanes meet there, once per box and column. The sums are
/// exact in 32 bits (the host refuses boxes of more than 2^23 pixels), and so is (sum + n / 2) * m: m <= 2^24 / n.
/// A grey source has one plane: only its first channel is summed and written.
template <bool kAllModels>
__global__ __launch_bounds__(256) void reduce_kernel(const ReduceJob* __restrict__ jobs, const int* __restrict__ first_tile, int n)
{
    __shared__ typename Fancy<kAllModels>::Tiles s_t;
    __shared__ uint32_t s_sum[kReduceTileH][kReduceTileW][3];
    const int b = blockIdx.x, item = rgb_batch_item(first_tile, n, b);
    const ReduceJob& J = jobs[item];
    const FancySource& p = J.src;
    const int tile = b - first_tile[item], ty = tile / J.tiles_x, tx = tile - ty * J.tiles_x;
    const int t = threadIdx.x;
    const int fx = J.fx, fy = J.fy;
    const int rx0 = tx * kReduceTileW, ry0 = ty * J.rows_per_tile; // the tile's first reduced column and row
    const int nrx = min(kReduceTileW, J.red_w - rx0), nry = min(J.rows_per_tile, J.red_h - ry0);
    const int sx0 = rx0 * fx, sx1 = min((rx0 + nrx) * fx, J.width);  // the source columns and rows under the tile
    const int sy0 = ry0 * fy, sy1 = min((ry0 + nry) * fy, J.height);
    const int chans = p.ncomp == 1 ? 1 : 3;
    for (int q = t; q < kReduceTileH * kReduceTileW * 3; q += 256) (&s_sum[0][0][0])[q] = 0; // before the first barrier below
    for (int c0 = sx0; c0 < sx1; c0 += kFancyTileW) {
        const int cw = min(kFancyTileW, sx1 - c0);
        const int rx = (c0 + t) / fx - rx0; // the lane's reduced column in the tile (t < cw)
        uint32_t acc[3] = {0, 0, 0};
        for (int r = sy0; r < sy1; r += kFancyTileH) {
            const int ch = min(kFancyTileH, sy1 - r);
            int bx[Fancy<kAllModels>::kComps], by[Fancy<kAllModels>::kComps];
            fancy_stage<true, kAllModels>(p, s_t, c0 + p.x, r + p.y, cw, ch, bx, by);
            __syncthreads();
            if (t < cw) {
                for (int rr = 0; rr < ch; ++rr) {
                    uint32_t rgb[3];
                    fancy_pixel<kAllModels>(p, s_t, bx, by, c0 + t + p.x, r + rr + p.y, rgb);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += rgb[c];
                    const int done = r + rr + 1; // source rows summed so far: a box ends on a multiple of fy, or with the image
                    if (done % fy == 0 || done == sy1) {
                        const int ry = (done - 1) / fy - ry0;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            if (c < chans) atomicAdd(&s_sum[ry][rx][c], acc[c]);
                            acc[c] = 0;
                        }
                    }
                }
            }
            __syncthreads(); // the next round's staging overwrites the tiles; the last one: the sums are complete
        }
    }
    for (int q = t; q < nry * nrx; q += 256) {
        const int ry = q / nrx, rx = q - ry * nrx;
        const int gx = rx0 + rx, gy = ry0 + ry;
        const int nx = min(fx, J.width - gx * fx), ny = min(fy, J.height - gy * fy); // the box's pixels: fewer at the edges
        const uint32_t half = static_cast<uint32_t>(nx * ny) >> 1, m = J.mult[(nx != fx ? 1 : 0) | (ny != fy ? 2 : 0)];
        uint8_t* o = J.dst + static_cast<size_t>(gy) * J.pitch + gx;
        for (int c = 0; c < chans; ++c) o[c * J.plane_stride] = static_cast<uint8_t>(((s_sum[ry][rx][c] + half) * m) >> 24);
    }
}

} // namespace

// ------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------

hipError_t launch_upsample(
    const uint8_t* src, int src_pitch, int src_w, int src_h,
    uint8_t* dst, int dst_pitch, int dst_w, int dst_h,
    int num_x, int den_x, int num_y, int den_y, hipStream_t stream)
{
    if (dst_w <= 0 || dst_h <= 0) return hipSuccess;
    const dim3 grid((dst_w + 1023) / 1024, dst_h);
    upsample_kernel<<<grid, 256, 0, stream>>>(
        src, src_pitch, src_w, src_h, dst, dst_pitch, dst_w, dst_h, num_x, den_x, num_y, den_y);
    return hipGetLastError();
}

hipError_t launch_rgbi(
    const uint8_t* const* planes, const int* pitch, const int* w, const int* h, const int* num_x, const int* num_y,
    int den_x, int den_y, int ncomp, uint8_t* dst, int dst_pitch, int width, int height, hipStream_t stream)
{
    if (width <= 0 || height <= 0) return hipSuccess;
    RgbiParams p{};
    for (int c = 0; c < 3; ++c) {
        const int cc = c < ncomp ? c : 0;
        p.plane[c] = planes[cc];
        p.pitch[c] = pitch[cc];
        p.w[c]     = w[cc];
        p.h[c]     = h[cc];
        p.num_x[c] = num_x[cc];
        p.num_y[c] = num_y[cc];
    }
    p.den_x = den_x;
    p.den_y = den_y;
    p.ncomp = ncomp;
    const dim3 grid((width + 1023) / 1024, height);
    rgbi_kernel<<<grid, 256, 0, stream>>>(p, dst, dst_pitch, width, height);
    return hipGetLastError();
}

hipError_t launch_rgbi_fancy(const FancySource& src, uint8_t* dst, int dst_pitch, int width, int height, hipStream_t stream)
{
    if (width <= 0 || height <= 0) return hipSuccess;
    bool windowed = src.x != 0 || src.y != 0;
    for (const FancyComp& c : src.comp) windowed = windowed || c.ox != 0 || c.oy != 0;
    const dim3 grid((width + kFancyTileW - 1) / kFancyTileW, (height + kFancyTileH - 1) / kFancyTileH);
    if (fancy_all_models(src)) {
        if (windowed) fancy_color_kernel<true><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height);
        else fancy_color_kernel<false><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height);
    } else {
        if (windowed) fancy_rgbi_kernel<true><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height);
        else fancy_rgbi_kernel<false><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height);
    }
    return hipGetLastError();
}

hipError_t launch_resize(
    const ResizeJob* d_jobs, const int* d_first_tile, int n, int h_tiles, int out_w, int out_h, int layout, bool all_models,
    uint8_t* dst, hipStream_t stream)
{
    if (n <= 0 || h_tiles <= 0 || out_w <= 0 || out_h <= 0) return hipSuccess;
    if (all_models) resize_h_color_kernel<<<h_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n, out_w);
    else resize_h_kernel<<<h_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n, out_w);
    const int v_tiles = ((out_w + kResizeVTileW - 1) / kResizeVTileW) * ((out_h + kResizeVTileH - 1) / kResizeVTileH);
    resize_v_kernel<<<dim3(v_tiles, n), 256, 0, stream>>>(d_jobs, out_w, out_h, layout, dst);
    return hipGetLastError();
}

hipError_t launch_rgbi_oriented(const FancySource& src, int orientation, uint8_t* dst, int dst_pitch, int width, int height, hipStream_t stream)
{
    if (width <= 0 || height <= 0) return hipSuccess;
    bool windowed = src.x != 0 || src.y != 0;
    for (const FancyComp& c : src.comp) windowed = windowed || c.ox != 0 || c.oy != 0;
    const bool all = fancy_all_models(src);
    const int flips = (orient_mirrors_x(orientation) ? 1 : 0) | (orient_mirrors_y(orientation) ? 2 : 0);
    if (orient_transposes(orientation)) {
        const dim3 grid((width + kOrientTile - 1) / kOrientTile, (height + kOrientTile - 1) / kOrientTile);
        if (all) {
            if (windowed) fancy_transposed_kernel<true, true><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height, flips);
            else fancy_transposed_kernel<false, true><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height, flips);
        } else {
            if (windowed) fancy_transposed_kernel<true, false><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height, flips);
            else fancy_transposed_kernel<false, false><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height, flips);
        }
    } else {
        const dim3 grid((width + kFancyTileW - 1) / kFancyTileW, (height + kFancyTileH - 1) / kFancyTileH);
        if (all) {
            if (windowed) fancy_mirrored_kernel<true, true><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height, flips);
            else fancy_mirrored_kernel<false, true><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height, flips);
        } else {
            if (windowed) fancy_mirrored_kernel<true, false><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height, flips);
            else fancy_mirrored_kernel<false, false><<<grid, 256, 0, stream>>>(src, dst, dst_pitch, width, height, flips);
        }
    }
    return hipGetLastError();
}

namespace {
/// The first pass of a call with orientations: the horizontal pass of its items of 1..4 (the instantiation that knows
/// kResizeMirrorStore only where an item carries it) and the transposing pass of its items of 5..8.
void launch_resize_first(
    const ResizeJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int h_tiles, int t_tiles, bool mirror_store, int out_w,
    bool all_models, hipStream_t stream)
{
    if (h_tiles > 0) {
        if (!mirror_store) {
            if (all_models) resize_h_color_kernel<<<h_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n, out_w);
            else resize_h_kernel<<<h_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n, out_w);
        } else if (all_models) resize_h_oriented_kernel<true><<<h_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n, out_w);
        else resize_h_oriented_kernel<false><<<h_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n, out_w);
    }
    if (t_tiles > 0) {
        if (all_models) resize_t_kernel<true><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n, out_w);
        else resize_t_kernel<false><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n, out_w);
    }
}

template <class T>
void launch_resize_v_tensor(const ResizeJob* d_jobs, int n, int out_w, int out_h, int layout, const TensorNorm& norm, void* dst, hipStream_t stream)
{
    const int v_tiles = ((out_w + kResizeVTileW - 1) / kResizeVTileW) * ((out_h + kResizeVTileH - 1) / kResizeVTileH);
    if (layout == 0) resize_v_tensor_kernel<T, false><<<dim3(v_tiles, n), 256, 0, stream>>>(d_jobs, out_w, out_h, norm, static_cast<T*>(dst));
    else resize_v_tensor_kernel<T, true><<<dim3(v_tiles, n), 256, 0, stream>>>(d_jobs, out_w, out_h, norm, static_cast<T*>(dst));
}
} // namespace

hipError_t launch_resize_oriented(
    const ResizeJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int h_tiles, int t_tiles, bool mirror_store,
    int out_w, int out_h, int layout, bool all_models, uint8_t* dst, hipStream_t stream)
{
    if (t_tiles <= 0 && !mirror_store) return launch_resize(d_jobs, d_first_tile, n, h_tiles, out_w, out_h, layout, all_models, dst, stream);
    if (n <= 0 || out_w <= 0 || out_h <= 0) return hipSuccess;
    launch_resize_first(d_jobs, d_first_tile, d_first_tile_t, n, h_tiles, t_tiles, mirror_store, out_w, all_models, stream);
    const int v_tiles = ((out_w + kResizeVTileW - 1) / kResizeVTileW) * ((out_h + kResizeVTileH - 1) / kResizeVTileH);
    resize_v_kernel<<<dim3(v_tiles, n), 256, 0, stream>>>(d_jobs, out_w, out_h, layout, dst);
    return hipGetLastError();
}

hipError_t launch_resize_tensor(
    const ResizeJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int h_tiles, int t_tiles, bool mirror_store,
    int out_w, int out_h, int layout, bool all_models, int type, const TensorNorm& norm, void* dst, hipStream_t stream)
{
    if (n <= 0 || out_w <= 0 || out_h <= 0) return hipSuccess;
    if (type != kTensorU8 && type != kTensorF32 && type != kTensorF16 && type != kTensorBF16) return hipErrorInvalidValue;
    launch_resize_first(d_jobs, d_first_tile, d_first_tile_t, n, h_tiles, t_tiles, mirror_store, out_w, all_models, stream);
    switch (type) {
    case kTensorU8: launch_resize_v_tensor<uint8_t>(d_jobs, n, out_w, out_h, layout, norm, dst, stream); break;
    case kTensorF32: launch_resize_v_tensor<float>(d_jobs, n, out_w, out_h, layout, norm, dst, stream); break;
    case kTensorF16: launch_resize_v_tensor<_Float16>(d_jobs, n, out_w, out_h, layout, norm, dst, stream); break;
    default: launch_resize_v_tensor<__hip_bfloat16>(d_jobs, n, out_w, out_h, layout, norm, dst, stream); break;
    }
    return hipGetLastError();
}

hipError_t launch_rgb_batch(
    const RgbJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int row_tiles, int t_tiles, bool planar, bool all_models,
    hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (row_tiles > 0) {
        if (all_models) {
            if (planar) rgb_batch_kernel<true, true><<<row_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n);
            else rgb_batch_kernel<true, false><<<row_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n);
        } else {
            if (planar) rgb_batch_kernel<false, true><<<row_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n);
            else rgb_batch_kernel<false, false><<<row_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n);
        }
    }
    if (t_tiles > 0) {
        if (all_models) {
            if (planar) rgb_batch_transposed_kernel<true, true><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n);
            else rgb_batch_transposed_kernel<true, false><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n);
        } else {
            if (planar) rgb_batch_transposed_kernel<false, true><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n);
            else rgb_batch_transposed_kernel<false, false><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n);
        }
    }
    return hipGetLastError();
}

hipError_t launch_reduce(const ReduceJob* d_jobs, const int* d_first_tile, int n, int tiles, bool all_models, hipStream_t stream)
{
    if (n <= 0 || tiles <= 0) return hipSuccess;
    if (all_models) reduce_kernel<true><<<tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n);
    else reduce_kernel<false><<<tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n);
    return hipGetLastError();
}

} // namespace jg
