// jg_output_jobs.h -- the records of the RGB output stage: what the host plan (jg_output_plan.cpp) builds and the kernels
// (jg_output.hip) read, with the tile arithmetic both sides count by. Free of HIP: a plain C++ compiler reads it.
#ifndef JG_OUTPUT_JOBS_H_
#define JG_OUTPUT_JOBS_H_

#include <cstddef>
#include <cstdint>

namespace jg {

/// How libjpeg upsamples a component (jdsample.c, jinit_upsampler), by the ratios hr = h_max / h_c, vr = v_max / v_c and
/// the width of its FULL plane: 2h1v and 2h2v take the fancy path only on planes wider than 2 samples.
enum FancyMode : int { kFancyReplicate = 0, kFancyH2V1 = 1, kFancyH2V2 = 2, kFancyH1V2 = 3 };
inline int fancy_mode(int hr, int vr, int full_w)
{
    if (hr == 2 && vr == 1 && full_w > 2) return kFancyH2V1;
    if (hr == 2 && vr == 2 && full_w > 2) return kFancyH2V2;
    if (hr == 1 && vr == 2) return kFancyH1V2;
    return kFancyReplicate;
}

/// What the libjpeg-exact conversions read: a rectangle of an image whose top-left pixel is (x, y), given as each
/// component's decoded WINDOW (jpeggpu_ext_set_crop) -- its plane, its size and its origin in the component's full plane.
/// Loads are clamped to the window: for every sample a pixel of the rectangle reads that is libjpeg's clamp to the plane,
/// because the window holds the rectangle's samples and their one-sample halo, clipped to the plane (the host checks
/// it). A whole image is the case origin 0, window = full plane, rectangle at (0, 0). Built by the host
/// (jg_output_plan.cpp, fancy_source), read by the kernels.
struct FancyComp {
    const uint8_t* plane;
    int pitch, w, h; // the window
    int ox, oy;      // its origin in the full plane
    int hr, vr;      // output pixels per sample: h_max / h_c, v_max / v_c
    int mode;        // FancyMode
};
/// The colour model of a source: what the upsampled samples of a pixel mean (the values of enum jpeggpu_ext_color_space).
///   grey      the sample three times
///   YCbCr     jdcolor.c's ycc_rgb_convert
///   RGB       the three samples as they are
///   CMYK      Pillow's cmyk2rgb of Adobe's inverted samples s_0..s_3: the inks c_i = 255 - s_i, K = s_3,
///             out_i = K - MULDIV255(c_i, K), with MULDIV255(a, b) = ((t >> 8) + t) >> 8, t = a b + 128 (exact in 32-bit
///             integers, no division)
///   YCCK      ycc_rgb_convert of components 0..2, then the CMYK rule with the inks c_i = r, g, b (libjpeg hands out
///             255 - r, ... in place of the samples, and Pillow inverts those like any CMYK file's)
enum FancyColor : int { kFancyGray = 1, kFancyYCbCr = 2, kFancyRGB = 3, kFancyCMYK = 4, kFancyYCCK = 5 };
struct FancySource {
    FancyComp comp[4]; // entries from ncomp on are component 0
    int x, y;
    int ncomp;         // 1, 3 or 4
    int color;         // FancyColor; one that fits ncomp (the host checks it)
};
/// Grey and YCbCr sources take the kernels' three-tile instantiations; RGB, CMYK and YCCK ones the instantiations that
/// stage a fourth tile and know every model.
inline bool fancy_all_models(const FancySource& s) { return s.color != kFancyGray && s.color != kFancyYCbCr; }

/// EXIF orientation of an output (jpeggpu_ext.h has the table): what the eight values do to the stored image. Values 5..8
/// turn rows into columns; `x` / `y`: the DISPLAYED x / y axis runs against the stored axis it lies along.
inline bool orient_valid(int o) { return o >= 1 && o <= 8; }
inline bool orient_transposes(int o) { return o >= 5; }
inline bool orient_mirrors_x(int o) { return o == 2 || o == 3 || o == 6 || o == 7; }
inline bool orient_mirrors_y(int o) { return o == 3 || o == 4 || o == 7 || o == 8; }

/// The transposing conversions' tile (launch_rgbi_oriented, launch_rgb_batch): kOrientTile x kOrientTile stored pixels
/// per workgroup.
constexpr int kOrientTile = 64;

/// One item of a batched resize (launch_resize), in device memory: a source rectangle resampled to out_w x out_h RGB by
/// two separable passes whose weight tables the host computed (jpeggpu_ext_resize_weights). A table of n output
/// coordinates with `taps` taps each is int32 {first, count}[n] followed by int32 weights[n][taps] (22 fraction bits).
struct ResizeJob {
    FancySource src;
    int row0, rows;            // rectangle rows row0 .. row0 + rows - 1: the rows the vertical taps read
    int taps_x, taps_y;
    const int* tab_x;          // out_w columns
    const int* tab_y;          // out_h rows
    uint8_t* mid;              // rows x out_w RGB of the horizontal pass, rows mid_pitch bytes apart
    int mid_pitch;             // a multiple of 16
    int pad_;                  // flags: kResizeMirrorStore (oriented calls), kResizeFlipOutput (tensor calls)
};
/// ResizeJob::pad_ of an item of launch_resize_oriented whose displayed x runs against stored x (orientations 2 and 3):
/// tab_x is in stored order -- column out_w - 1 - ox of the displayed table, its taps reversed -- and the horizontal pass
/// writes table column ox' to mid column out_w - 1 - ox'.
constexpr int kResizeMirrorStore = 1;
/// ResizeJob::pad_ of an item of launch_resize_tensor whose RESULT is flipped left to right: output column x is column
/// out_w - 1 - x of the unflipped result. Only the tensor pass reads it (mirrored columns of `mid`); the first passes
/// test kResizeMirrorStore alone, so tables, `mid` and orientations are what they are without the flag.
constexpr int kResizeFlipOutput = 2;
constexpr int kResizeHTileW = 32, kResizeHTileH = 8; // horizontal pass: output columns x rows per workgroup
constexpr int kResizeVTileW = 256, kResizeVTileH = 4; // vertical pass: output pixels x rows per workgroup
/// Horizontal-pass workgroups of one item.
inline int resize_h_tiles(int rows, int out_w)
{
    return ((rows + kResizeHTileH - 1) / kResizeHTileH) * ((out_w + kResizeHTileW - 1) / kResizeHTileW);
}
/// The transposing first pass of items with orientations 5..8: displayed x lies along stored y, so the rounded pass runs
/// down stored columns. A workgroup owns kResizeTTileW stored columns (rows of `mid`) and kResizeTTileK output columns.
constexpr int kResizeTTileW = 256, kResizeTTileK = 8;
inline int resize_t_tiles(int rows, int out_w)
{
    return ((rows + kResizeTTileW - 1) / kResizeTTileW) * ((out_w + kResizeTTileK - 1) / kResizeTTileK);
}

/// The element of launch_resize_tensor's output (the values of enum jpeggpu_ext_tensor_type) and its size in bytes.
enum TensorType : int { kTensorU8 = 0, kTensorF32 = 1, kTensorF16 = 2, kTensorBF16 = 3 };
inline int tensor_elem_size(int type) { return type == kTensorU8 ? 1 : type == kTensorF32 ? 4 : 2; }
/// What the tensor pass does to byte u of channel c for the float types: ((float(u) / 255) - mean[c]) / std[c], each
/// operation a binary32 one rounded to nearest even on its own (jpeggpu_ext.h has the contract). Passed by value.
struct TensorNorm {
    float mean[3], std[3];
};

/// One item of a batched conversion (launch_rgb_batch), in device memory: a source rectangle written at its own size
/// where `flips` and the kernel that takes it display it. Interleaved (HWC): R, G, B of displayed pixel (x, y) at
/// dst + y * dst_pitch + 3 * x; planar (CHW): channel c at dst + c * plane_stride + y * dst_pitch + x.
struct RgbJob {
    FancySource src;     // as fancy_source builds it (windows, rectangle origin, modes, colour)
    uint8_t* dst;
    int dst_pitch;
    size_t plane_stride; // CHW only
    int width, height;   // the STORED rectangle
    int flips;           // bit 0: displayed x runs against the stored axis it lies along; bit 1: displayed y
    int tiles_x;         // tiles per tile row of this item
};
/// Workgroups of one item: kRgbBatchTileW x kRgbBatchTileH tiles (orientations 1..4: the row kernels' tile) or kOrientTile
/// squares (5..8) of the stored rectangle. rgb_batch_tiles_x: RgbJob::tiles_x.
constexpr int kRgbBatchTileW = 256, kRgbBatchTileH = 8;
inline int rgb_batch_tiles_x(int width, bool transposes)
{
    return transposes ? (width + kOrientTile - 1) / kOrientTile : (width + kRgbBatchTileW - 1) / kRgbBatchTileW;
}
inline int64_t rgb_batch_tiles(int width, int height, bool transposes)
{
    const int rows = transposes ? (height + kOrientTile - 1) / kOrientTile : (height + kRgbBatchTileH - 1) / kRgbBatchTileH;
    return static_cast<int64_t>(rgb_batch_tiles_x(width, transposes)) * rows;
}

/// One item of a batched box reduction (launch_reduce), in device memory: the source's width x height RGB (grey: its one
/// channel) averaged over boxes of fx x fy pixels -- fewer in the last column and row when the size is no multiple --
/// into red_w x red_h planes, ceil(width / fx) x ceil(height / fy): Pillow's Image.reduce((fx, fy)) of the whole image.
/// A result is ((sum + n / 2) * m) >> 24 in 32-bit unsigned arithmetic, n the pixels of its box; m =
/// uint32(float(1 << 24) / float(n)), a binary32 division that the HOST makes (reduce_multiplier), for the four boxes an
/// item can have: mult[0] whole, [1] last column, [2] last row, [3] both.
struct ReduceJob {
    FancySource src;
    int width, height;   // the source rectangle
    int fx, fy;
    int red_w, red_h;
    uint8_t* dst;        // plane c at dst + c * plane_stride, rows `pitch` apart; one plane for a grey source, else three
    int pitch;
    size_t plane_stride;
    uint32_t mult[4];
    int rows_per_tile;   // reduced rows a workgroup owns (reduce_rows_per_tile)
    int tiles_x;         // tiles per tile row of this item
};
inline uint32_t reduce_multiplier(int n) { return static_cast<uint32_t>(static_cast<float>(1 << 24) / static_cast<float>(n)); }
/// A workgroup owns kReduceTileW reduced columns and as many reduced rows, kReduceTileH at most, as fit the eight source
/// rows that are staged at once (one row where fy exceeds four: its source rows then take several rounds).
constexpr int kReduceTileW = 64, kReduceTileH = 8;
inline int reduce_rows_per_tile(int fy) { return fy >= kReduceTileH ? 1 : kReduceTileH / fy; }
inline int reduce_tiles_x(int red_w) { return (red_w + kReduceTileW - 1) / kReduceTileW; }
inline int64_t reduce_tiles(int red_w, int red_h, int fy)
{
    const int rows = reduce_rows_per_tile(fy);
    return static_cast<int64_t>(reduce_tiles_x(red_w)) * ((red_h + rows - 1) / rows);
}

// The three job records cross from the host compiler's object to the device's: one layout for both (LP64).
static_assert(sizeof(FancySource) == 176 && offsetof(FancySource, x) == 160, "struct FancySource");
static_assert(sizeof(ResizeJob) == 224 && offsetof(ResizeJob, row0) == 176 && offsetof(ResizeJob, tab_x) == 192 && offsetof(ResizeJob, mid) == 208 &&
                  offsetof(ResizeJob, pad_) == 220,
              "struct ResizeJob");
static_assert(sizeof(RgbJob) == 216 && offsetof(RgbJob, dst) == 176 && offsetof(RgbJob, plane_stride) == 192 && offsetof(RgbJob, tiles_x) == 212,
              "struct RgbJob");
static_assert(sizeof(ReduceJob) == 248 && offsetof(ReduceJob, dst) == 200 && offsetof(ReduceJob, plane_stride) == 216 && offsetof(ReduceJob, mult) == 224 &&
                  offsetof(ReduceJob, tiles_x) == 244,
              "struct ReduceJob");

} // namespace jg

#endif // JG_OUTPUT_JOBS_H_
