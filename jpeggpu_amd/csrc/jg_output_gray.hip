// jg_output_gray.hip -- gfx950 (CDNA4, wave64) kernels of the GREY output stage: from decoded planes to one 8-bit channel,
// what libjpeg hands a caller of out_color_space = JCS_GRAYSCALE and Pillow one of draft("L", ..).
//
//   gray_batch_kernel /           many images to grey at their own sizes from a device table of items, one launch for
//   gray_batch_transposed_kernel  orientations 1..4 and one for 5..8 (jpeggpu_ext_batch_to_gray); an item of orientation 1
//                                 whose component 0 is at full resolution is a pitched copy of a window of plane 0, done
//                                 by the same launch in 16-byte pieces
//   gray_image_kernel /           the same tiles for ONE image whose descriptor travels as a kernel argument
//   gray_image_transposed_kernel  (jpeggpu_ext_crop_to_gray_oriented)
//   gray_resize_h_kernel /        batched resize to one size with Pillow's arithmetic on one 8-bit band: the first pass of
//   gray_resize_t_kernel          items of orientations 1..4 / 5..8, one byte per pixel into the items' `mid` rows
//   gray_resize_v_kernel          the vertical pass: bytes, float, half or bfloat16 elements, one channel
//                                 (jpeggpu_ext_resize_view_to_gray_tensor)
//
// The grey of a pixel is component 0 of a grey or YCbCr source, upsampled where its factors are below the frame's maxima
// (fancy_sample: the RGB kernels' rules), or jdcolor.c's rgb_gray_convert of the three upsampled samples of an RGB-coded
// source. `kRgb`, a compile-time variant of every kernel but the vertical pass: false stages ONE component tile in LDS
// (2.6 KB), true three, for calls that hold an RGB-coded item. What the RGB stage (jg_output.hip) does three times per
// pixel -- convert, keep in LDS or in `mid`, store -- happens once here.
//
// A translation unit of its own: the RGB kernels are to come out of the compiler as they were.
#include "jg_output.hpp"
#include "jg_output_device.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

namespace jg {

namespace {

template <bool kRgb>
struct Gray {
    static constexpr int kComps = kRgb ? 3 : 1;
    using Tiles = FancyTile[kComps];
};

/// fancy_stage of the RGB stage for the components a grey needs: the samples under the image pixels (ix0, iy0) ..
/// (ix0 + cw - 1, iy0 + ch - 1) with their one-sample halo, clamped to the window. (bx, by)[k]: full-plane coordinates of
/// tiles[k][0][0]. The caller's barrier makes the tiles visible.
template <bool kRgb>
__device__ __forceinline__ void gray_stage(
    const FancySource& s, typename Gray<kRgb>::Tiles& tiles, int ix0, int iy0, int cw, int ch, int (&bx)[Gray<kRgb>::kComps],
    int (&by)[Gray<kRgb>::kComps])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < Gray<kRgb>::kComps; ++k) {
        const FancyComp& c = s.comp[k];
        bx[k] = ix0 / c.hr - 1;
        by[k] = iy0 / c.vr - 1;
        if (k >= s.ncomp) continue;
        const int nx = (ix0 + cw - 1) / c.hr + 2 - bx[k], ny = (iy0 + ch - 1) / c.vr + 2 - by[k];
        for (int j = 0; j < ny; ++j) {
            const uint8_t* row = c.plane + static_cast<size_t>(min(max(by[k] + j - c.oy, 0), c.h - 1)) * c.pitch;
            for (int i = t; i < nx; i += 256) tiles[k][j][i] = row[min(max(bx[k] + i - c.ox, 0), c.w - 1)];
        }
    }
}

/// The grey of image pixel (x, y): component 0, or jdcolor.c's rgb_gray_convert of an RGB-coded source's three samples,
/// (19595 R + 38470 G + 7471 B + 32768) >> 16 (FIX(0.29900), FIX(0.58700), FIX(0.11400), ONE_HALF).
template <bool kRgb>
__device__ __forceinline__ uint32_t gray_pixel(
    const FancySource& s, const typename Gray<kRgb>::Tiles& tiles, const int (&bx)[Gray<kRgb>::kComps], const int (&by)[Gray<kRgb>::kComps], int x,
    int y)
{
    const int a = fancy_sample(s.comp[0], tiles[0], bx[0], by[0], x, y);
    if constexpr (kRgb) {
        if (s.ncomp == 3) {
            const int g = fancy_sample(s.comp[1], tiles[1], bx[1], by[1], x, y);
            const int b = fancy_sample(s.comp[2], tiles[2], bx[2], by[2], x, y);
            return static_cast<uint32_t>((19595 * a + 38470 * g + 7471 * b + 32768) >> 16);
        }
    }
    return static_cast<uint32_t>(a);
}

/// Four grey pixels, out[i], of which the lane has the first `np`, to `d`: a dword where all four are there and `d` is
/// aligned (a wave then writes 256 contiguous bytes), bytes otherwise.
__device__ __forceinline__ void store_gray4(uint8_t* d, const uint32_t (&out)[4], int np)
{
    if (np == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d) = out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24;
    } else {
        for (int i = 0; i < np; ++i) d[i] = static_cast<uint8_t>(out[i]);
    }
}

/// Sixteen bytes that ask for no alignment (the load of the copy below: source and destination rows are aligned
/// independently) and sixteen that lie on a 16-byte boundary (its store).
typedef uint32_t GrayBytes16 __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t GrayAligned16 __attribute__((ext_vector_type(4), aligned(16)));

/// Orientations 1..4: one kFancyTileW x kFancyTileH tile of item J, the RGB stage's rgb_batch_kernel with one channel.
///   * The grey is a copy (orientation 1, one component at full resolution): no LDS. The tile's rows are runs of up to 256
///     bytes of plane 0's window; a run goes out in the 16-byte pieces of its DESTINATION's alignment, 17 at most, one lane
///     each, 8 rows at once: an unaligned 16-byte load and an aligned 16-byte store, and bytes for the two pieces at the
///     run's ends. The source needs no clamp: the rectangle lies inside the window (the host checks it).
///   * Otherwise one component tile (three for an RGB-coded item) is staged, and each lane converts a 2 x 4 quad and
///     stores each row's four bytes where `flips` displays them.
template <bool kRgb>
__device__ __forceinline__ void gray_tile(const RgbJob& J, int tile, typename Gray<kRgb>::Tiles& s_t)
{
    const FancySource& p = J.src;
    const int ty = tile / J.tiles_x, tx = tile - ty * J.tiles_x;
    const int width = J.width, height = J.height;
    const int t  = threadIdx.x;
    const int x0 = tx * kFancyTileW, y0 = ty * kFancyTileH;
    const int px = p.x, py = p.y;
    uint8_t* dst = J.dst;
    const int dst_pitch = J.dst_pitch;
    const FancyComp& c0 = p.comp[0];
    if (J.flips == 0 && p.ncomp == 1 && c0.hr == 1 && c0.vr == 1) { // (uniform)
        const int y = y0 + (t >> 5), piece = t & 31;
        const int n = min(kFancyTileW, width - x0); // bytes of a run
        if (y >= height) return;
        uint8_t* d       = dst + static_cast<size_t>(y) * dst_pitch + x0;
        const uint8_t* s = c0.plane + static_cast<size_t>(y + py - c0.oy) * c0.pitch + (x0 + px - c0.ox);
        const int b0 = 16 * piece - static_cast<int>(reinterpret_cast<uintptr_t>(d) & 15); // the lane's piece: bytes b0 .. b0 + 15 of the run
        if (b0 >= n) return;
        if (b0 >= 0 && b0 + 16 <= n) {
            *reinterpret_cast<GrayAligned16*>(d + b0) = *reinterpret_cast<const GrayBytes16*>(s + b0);
        } else {
            for (int b = max(b0, 0); b < min(b0 + 16, n); ++b) d[b] = s[b];
        }
        return;
    }
    int bx[Gray<kRgb>::kComps], by[Gray<kRgb>::kComps];
    gray_stage<kRgb>(p, s_t, x0 + px, y0 + py, min(kFancyTileW, width - x0), min(kFancyTileH, height - y0), bx, by);
    __syncthreads();
    const int x = x0 + 4 * (t & 63);
    if (x >= width) return;
    const int np = min(4, width - x);
    const bool mx = J.flips & 1, my = J.flips & 2;
    const size_t xd = static_cast<size_t>(mx ? width - x - np : x);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = y0 + 2 * (t >> 6) + dy;
        if (y >= height) break;
        uint32_t out[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { // displayed pixel i of the lane's run: stored x + np - 1 - i when mirrored
            const int xs = mx ? max(x + np - 1 - i, x) : min(x + i, width - 1);
            out[i] = gray_pixel<kRgb>(p, s_t, bx, by, xs + px, y + py);
        }
        store_gray4(dst + static_cast<size_t>(my ? height - 1 - y : y) * dst_pitch + xd, out, np);
    }
}

/// Orientations 5..8: one kOrientTile x kOrientTile tile of stored pixels of item J. Eight strips of 64 x 8 are staged and
/// converted as ever and their grey kept in LDS, s_g[stored y][stored x], rows kOrientTile + 4 bytes apart. Then one wave
/// per displayed row -- a stored column --: its nh <= 64 contiguous bytes as 16 dwords (17 if the row does not start on a
/// dword: the two ends go out as bytes), each put together from four bytes read down the column.
template <bool kRgb>
__device__ __forceinline__ void gray_transposed_tile(
    const RgbJob& J, int tile, typename Gray<kRgb>::Tiles& s_t, uint8_t (&s_g)[kOrientTile][kOrientTile + 4])
{
    const FancySource& p = J.src;
    const int ty = tile / J.tiles_x, tx = tile - ty * J.tiles_x;
    const int width = J.width, height = J.height;
    const int t  = threadIdx.x;
    const int x0 = tx * kOrientTile, y0 = ty * kOrientTile;
    const int nw = min(kOrientTile, width - x0), nh = min(kOrientTile, height - y0);
    const int px = p.x, py = p.y;
    for (int s0 = 0; s0 < nh; s0 += kFancyTileH) {
        const int ch = min(kFancyTileH, nh - s0);
        int bx[Gray<kRgb>::kComps], by[Gray<kRgb>::kComps];
        gray_stage<kRgb>(p, s_t, x0 + px, y0 + s0 + py, nw, ch, bx, by);
        __syncthreads();
        for (int q = t; q < kFancyTileH * kOrientTile; q += 256) {
            const int qy = q / kOrientTile, qx = q % kOrientTile;
            if (qy >= ch || qx >= nw) continue;
            s_g[s0 + qy][qx] = static_cast<uint8_t>(gray_pixel<kRgb>(p, s_t, bx, by, x0 + qx + px, y0 + s0 + qy + py));
        }
        __syncthreads(); // the next strip's staging overwrites the tiles; the last one: s_g is complete
    }
    const bool mx = J.flips & 1, my = J.flips & 2;
    const int ox0 = mx ? height - y0 - nh : y0; // the displayed columns of the tile's stored rows, nh of them
    const int g = t & 63;
    if (g > 16) return;
    for (int row = t >> 6; row < nw; row += 4) { // displayed row: stored column x0 + row
        const int oy = my ? width - 1 - (x0 + row) : x0 + row;
        uint8_t* a   = J.dst + static_cast<size_t>(oy) * J.dst_pitch + ox0;
        const int b0 = 4 * g - static_cast<int>(reinterpret_cast<uintptr_t>(a) & 3); // the lane's dword: pixels b0 .. b0 + 3 of the run
        if (b0 + 4 <= 0 || b0 >= nh) continue;
        if (b0 >= 0 && b0 + 4 <= nh) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v |= static_cast<uint32_t>(s_g[mx ? nh - 1 - (b0 + k) : b0 + k][row]) << (8 * k);
            *reinterpret_cast<uint32_t*>(a + b0) = v;
        } else {
            for (int k = max(b0, 0); k < min(b0 + 4, nh); ++k) a[k] = s_g[mx ? nh - 1 - k : k][row];
        }
    }
}

template <bool kRgb>
__global__ __launch_bounds__(256) void gray_batch_kernel(const RgbJob* __restrict__ jobs, const int* __restrict__ first_tile, int n)
{
    __shared__ typename Gray<kRgb>::Tiles s_t;
    const int b = blockIdx.x, item = rgb_batch_item(first_tile, n, b);
    gray_tile<kRgb>(jobs[item], b - first_tile[item], s_t);
}

template <bool kRgb>
__global__ __launch_bounds__(256) void gray_batch_transposed_kernel(const RgbJob* __restrict__ jobs, const int* __restrict__ first_tile, int n)
{
    __shared__ typename Gray<kRgb>::Tiles s_t;
    __shared__ uint8_t s_g[kOrientTile][kOrientTile + 4];
    const int b = blockIdx.x, item = rgb_batch_item(first_tile, n, b);
    gray_transposed_tile<kRgb>(jobs[item], b - first_tile[item], s_t, s_g);
}

template <bool kRgb>
__global__ __launch_bounds__(256) void gray_image_kernel(RgbJob job)
{
    __shared__ typename Gray<kRgb>::Tiles s_t;
    gray_tile<kRgb>(job, blockIdx.x, s_t);
}

template <bool kRgb>
__global__ __launch_bounds__(256) void gray_image_transposed_kernel(RgbJob job)
{
    __shared__ typename Gray<kRgb>::Tiles s_t;
    __shared__ uint8_t s_g[kOrientTile][kOrientTile + 4];
    gray_transposed_tile<kRgb>(job, blockIdx.x, s_t, s_g);
}

// ------------------------------------------------------------------------------------------------
// The batched resize on one band: the RGB stage's passes (resize_h_tile, resize_t_tile, resize_v_tensor_kernel) with one
// byte per pixel in LDS, in `mid` (rows of out_w bytes padded to 16) and in the accumulators. Tables, rounding and the
// clamp to 8 bits after the first pass are the same: Pillow's ImagingResample treats every band alike.
// ------------------------------------------------------------------------------------------------

/// First pass of items of orientations 1..4: a workgroup owns kResizeHTileW output columns of kResizeHTileH rectangle rows
/// of one item. The input columns their taps read are made grey in chunks of up to kFancyTileW (gray_stage, gray_pixel
/// into s_g), and each lane accumulates its output pixel's taps that fall in the chunk. An item with kResizeMirrorStore
/// writes its result to the mirrored column of `mid`.
template <bool kRgb>
__global__ __launch_bounds__(256) void gray_resize_h_kernel(const ResizeJob* __restrict__ jobs, const int* __restrict__ first_tile, int n, int out_w)
{
    __shared__ typename Gray<kRgb>::Tiles s_t;
    __shared__ uint8_t s_g[kResizeHTileH][kFancyTileW];
    __shared__ int s_w[kResizeHTileW * kResizeLdsTaps];
    const int b = blockIdx.x, item = rgb_batch_item(first_tile, n, b);
    const ResizeJob& J = jobs[item];
    const int col_tiles = (out_w + kResizeHTileW - 1) / kResizeHTileW;
    const int tile = b - first_tile[item], ty = tile / col_tiles, tx = tile - ty * col_tiles;
    const int r0 = J.row0 + ty * kResizeHTileH; // the tile's first rectangle row
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
    int acc = 0;
    for (int c0 = a; c0 < e; c0 += kFancyTileW) {
        const int cw  = min(kFancyTileW, e - c0);
        const int ix0 = c0 + src.x, iy0 = r0 + src.y; // the chunk's origin in the image
        int bx[Gray<kRgb>::kComps], by[Gray<kRgb>::kComps];
        gray_stage<kRgb>(src, s_t, ix0, iy0, cw, nr, bx, by);
        __syncthreads();
        for (int q = t; q < kResizeHTileH * kFancyTileW; q += 256) {
            const int qy = q / kFancyTileW, qx = q % kFancyTileW;
            if (qy >= nr || qx >= cw) continue;
            s_g[qy][qx] = static_cast<uint8_t>(gray_pixel<kRgb>(src, s_t, bx, by, ix0 + qx, iy0 + qy));
        }
        __syncthreads();
        if (mine) { // taps j0 .. j1 - 1 of the column, relative to its first, lie in this chunk
            const int j0 = max(f, c0) - f, j1 = min(f + cnt, c0 + cw) - f;
            const uint8_t* px = &s_g[r][0] + (f - c0);
            const int* w = lds_w ? &s_w[col * taps] : wts + static_cast<size_t>(col) * taps;
            for (int j = j0; j < j1; ++j) acc += mul24(w[j], static_cast<int>(px[j]));
        }
        __syncthreads();
    }
    if (mine) {
        const int sx = (J.pad_ & kResizeMirrorStore) ? out_w - 1 - ox : ox;
        J.mid[static_cast<size_t>(r0 - J.row0 + r) * J.mid_pitch + sx] = static_cast<uint8_t>(clamp255((acc + (1 << 21)) >> 22));
    }
}

/// First pass of items of orientations 5..8 (the RGB stage's resize_t_tile): the taps run down stored columns, a row of
/// `mid` is a stored column of the rectangle. A workgroup owns up to kResizeTTileW stored columns, one per lane, and
/// kResizeTTileK output columns; a lane then writes its kResizeTTileK bytes of `mid` (8-byte aligned: two dwords).
template <bool kRgb>
__global__ __launch_bounds__(256) void gray_resize_t_kernel(const ResizeJob* __restrict__ jobs, const int* __restrict__ first_tile, int n, int out_w)
{
    constexpr int K = kResizeTTileK;
    __shared__ typename Gray<kRgb>::Tiles s_t;
    __shared__ int s_w[K * kResizeLdsTaps];
    const int b = blockIdx.x, item = rgb_batch_item(first_tile, n, b);
    const ResizeJob& J = jobs[item];
    const int k_tiles = (out_w + K - 1) / K;
    const int tile = b - first_tile[item], tc = tile / k_tiles, tk = tile - tc * k_tiles;
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
    int acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0;
    for (int r = a; r < e; r += kFancyTileH) {
        const int ch  = min(kFancyTileH, e - r);
        const int ix0 = c0 + src.x, iy0 = r + src.y; // the strip's origin in the image
        int bx[Gray<kRgb>::kComps], by[Gray<kRgb>::kComps];
        gray_stage<kRgb>(src, s_t, ix0, iy0, cw, ch, bx, by);
        __syncthreads();
        if (t < cw) {
            for (int rr = 0; rr < ch; ++rr) {
                const int v = static_cast<int>(gray_pixel<kRgb>(src, s_t, bx, by, ix0 + t, iy0 + rr));
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int j = r + rr - f[k];
                    if (j < 0 || j >= cnt[k]) continue;
                    const int wj = lds_w ? s_w[k * taps + j] : wts[static_cast<size_t>(k) * taps + j];
                    acc[k] += mul24(wj, v);
                }
            }
        }
        __syncthreads();
    }
    if (t >= cw) return;
    uint32_t v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = clamp255((acc[k] + (1 << 21)) >> 22);
    uint8_t* o = J.mid + static_cast<size_t>(c0 - J.row0 + t) * J.mid_pitch + ox0; // 8-byte aligned: mid_pitch % 16 == 0, K = 8
    static_assert(K == 8, "two dwords per lane");
    if (nk == K) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
        o4[1] = v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (k < nk) o[k] = static_cast<uint8_t>(v[k]);
    }
}

/// The vertical pass: kResizeVTileW x kResizeVTileH output pixels per workgroup, 4 consecutive pixels of one row per lane
/// (one dword of `mid` per tap row), one item per blockIdx.y. An item with kResizeFlipOutput reads `mid` mirrored, as in
/// the RGB stage's tensor pass: a dword where out_w % 4 == 0, whose pixels then change places in registers, bytes
/// otherwise. The four bytes become elements of T (tensor_bits with the one mean and std) and go out as one run. With one
/// channel n x out_h x out_w x 1 and n x 1 x out_h x out_w are the same bytes: the pass knows no layout.
template <class T>
__global__ __launch_bounds__(256) void gray_resize_v_kernel(const ResizeJob* __restrict__ jobs, int out_w, int out_h, float mean, float std, T* __restrict__ dst)
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
    const bool dword = np == 4 && (!flip || (out_w & 3) == 0);
    // dword: the lane's four mid columns start at c0, ascending; bytes: output pixel i is mid column c0 + i or c0 - i
    const int c0 = !flip ? x : dword ? out_w - 4 - x : out_w - 1 - x;
    const int step = flip ? -1 : 1;
    int acc[4] = {0, 0, 0, 0};
    for (int j = 0; j < cnt; ++j) {
        const int w = wts[j];
        const uint8_t* s = J.mid + static_cast<size_t>(f + j) * J.mid_pitch + c0; // dword: 4-byte aligned, mid_pitch % 16 == 0
        if (dword) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(s);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += mul24(w, static_cast<int>((v >> (8 * k)) & 255u));
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < np) acc[i] += mul24(w, static_cast<int>(s[step * i]));
        }
    }
    if (flip && dword) { // the dword load took the pixels in mid's order: 0 <-> 3, 1 <-> 2
        const int a0 = acc[0], a1 = acc[1];
        acc[0] = acc[3], acc[1] = acc[2], acc[2] = a1, acc[3] = a0;
    }
    uint32_t e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = tensor_bits<T>(clamp255((acc[i] + (1 << 21)) >> 22), mean, std);
    const size_t item = blockIdx.y;
    tensor_store_run<S, 4>(reinterpret_cast<uint8_t*>(dst + (item * out_h + y) * out_w + x), e, np);
}

template <class T>
void launch_gray_v(const ResizeJob* d_jobs, int n, int out_w, int out_h, float mean, float std, void* dst, hipStream_t stream)
{
    const int v_tiles = ((out_w + kResizeVTileW - 1) / kResizeVTileW) * ((out_h + kResizeVTileH - 1) / kResizeVTileH);
    gray_resize_v_kernel<T><<<dim3(v_tiles, n), 256, 0, stream>>>(d_jobs, out_w, out_h, mean, std, static_cast<T*>(dst));
}

} // namespace

hipError_t launch_gray_image(const RgbJob& job, bool transposes, hipStream_t stream)
{
    if (job.width <= 0 || job.height <= 0) return hipSuccess;
    const int tiles = static_cast<int>(rgb_batch_tiles(job.width, job.height, transposes));
    const bool rgb = job.src.ncomp == 3;
    if (transposes) {
        if (rgb) gray_image_transposed_kernel<true><<<tiles, 256, 0, stream>>>(job);
        else gray_image_transposed_kernel<false><<<tiles, 256, 0, stream>>>(job);
    } else {
        if (rgb) gray_image_kernel<true><<<tiles, 256, 0, stream>>>(job);
        else gray_image_kernel<false><<<tiles, 256, 0, stream>>>(job);
    }
    return hipGetLastError();
}

hipError_t launch_gray_batch(
    const RgbJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int row_tiles, int t_tiles, bool rgb, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (row_tiles > 0) {
        if (rgb) gray_batch_kernel<true><<<row_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n);
        else gray_batch_kernel<false><<<row_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n);
    }
    if (t_tiles > 0) {
        if (rgb) gray_batch_transposed_kernel<true><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n);
        else gray_batch_transposed_kernel<false><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n);
    }
    return hipGetLastError();
}

hipError_t launch_gray_resize(
    const ResizeJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int h_tiles, int t_tiles, int out_w, int out_h, bool rgb,
    int type, float mean, float std, void* dst, hipStream_t stream)
{
    if (n <= 0 || out_w <= 0 || out_h <= 0) return hipSuccess;
    if (type != kTensorU8 && type != kTensorF32 && type != kTensorF16 && type != kTensorBF16) return hipErrorInvalidValue;
    if (h_tiles > 0) {
        if (rgb) gray_resize_h_kernel<true><<<h_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n, out_w);
        else gray_resize_h_kernel<false><<<h_tiles, 256, 0, stream>>>(d_jobs, d_first_tile, n, out_w);
    }
    if (t_tiles > 0) {
        if (rgb) gray_resize_t_kernel<true><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n, out_w);
        else gray_resize_t_kernel<false><<<t_tiles, 256, 0, stream>>>(d_jobs, d_first_tile_t, n, out_w);
    }
    switch (type) {
    case kTensorU8: launch_gray_v<uint8_t>(d_jobs, n, out_w, out_h, mean, std, dst, stream); break;
    case kTensorF32: launch_gray_v<float>(d_jobs, n, out_w, out_h, mean, std, dst, stream); break;
    case kTensorF16: launch_gray_v<_Float16>(d_jobs, n, out_w, out_h, mean, std, dst, stream); break;
    default: launch_gray_v<__hip_bfloat16>(d_jobs, n, out_w, out_h, mean, std, dst, stream); break;
    }
    return hipGetLastError();
}

} // namespace jg
