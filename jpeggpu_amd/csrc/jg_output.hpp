// jg_output.hpp -- launch interface of the RGB output stage (jg_output.hip; all launches are asynchronous on `stream`).
// The records the launches take are jg_output_jobs.h's.
#ifndef JG_OUTPUT_HPP_
#define JG_OUTPUT_HPP_

#include "jg_output_jobs.h"

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace jg {

/// Nearest-neighbour replication of one plane: dst[y][x] = src[y * num_y / den_y][x * num_x / den_x]
/// (integer part of the reference's host helper util/util.h:62-91).
hipError_t launch_upsample(
    const uint8_t* src, int src_pitch, int src_w, int src_h,
    uint8_t* dst, int dst_pitch, int dst_w, int dst_h,
    int num_x, int den_x, int num_y, int den_y, hipStream_t stream);

/// Nearest-neighbour replication + YCbCr -> interleaved RGB8 (reference host helper util/util.h:62-104);
/// `ncomp` 1 (grey copied to R, G, B) or 3.
hipError_t launch_rgbi(
    const uint8_t* const* planes, const int* pitch, const int* w, const int* h, const int* num_x, const int* num_y,
    int den_x, int den_y, int ncomp, uint8_t* dst, int dst_pitch, int width, int height, hipStream_t stream);

/// libjpeg's fancy upsampling + the source's colour conversion -> interleaved RGB8 (jdsample.c, jdcolor.c, Pillow's
/// Convert.c) of the width x height pixels at the source's rectangle origin.
hipError_t launch_rgbi_fancy(const FancySource& src, uint8_t* dst, int dst_pitch, int width, int height, hipStream_t stream);

/// launch_rgbi_fancy with the pixels written where `orientation` (2..8) displays them: `width` x `height` is the stored
/// rectangle, `dst` holds the displayed one. 2..4 keep the row kernel's tile and mirror each lane's store; 5..8 take the
/// transposing kernel: kOrientTile x kOrientTile stored pixels per workgroup, whose RGB goes through LDS so that a wave
/// stores 3 x kOrientTile contiguous bytes of one displayed row.
hipError_t launch_rgbi_oriented(
    const FancySource& src, int orientation, uint8_t* dst, int dst_pitch, int width, int height, hipStream_t stream);

/// The two passes for `n` items: `d_jobs` ResizeJob[n] and `d_first_tile` int[n] (each item's first horizontal-pass
/// workgroup; `h_tiles` of them in all) in device memory. `layout` 0: dst is n x out_h x out_w x 3 (NHWC), 1: n x 3 x out_h
/// x out_w (NCHW). `all_models`: some item is not grey or YCbCr (fancy_all_models); the horizontal pass then runs as the
/// instantiation that knows every model, for all items of the call.
hipError_t launch_resize(
    const ResizeJob* d_jobs, const int* d_first_tile, int n, int h_tiles, int out_w, int out_h, int layout, bool all_models,
    uint8_t* dst, hipStream_t stream);

/// launch_resize for a call with orientations: items of 1..4 take the horizontal pass (`d_first_tile`, `h_tiles`; one of
/// them with kResizeMirrorStore: `mirror_store`, the instantiation that knows the flag), items of 5..8 the transposing
/// pass (`d_first_tile_t`, `t_tiles`; for them ResizeJob::row0 / rows count stored columns and tab_x runs over stored
/// rows); an item has no tiles in the list of the other kind. The vertical pass is launch_resize's. Without mirrored and
/// transposed items this launches exactly what launch_resize does.
hipError_t launch_resize_oriented(
    const ResizeJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int h_tiles, int t_tiles, bool mirror_store,
    int out_w, int out_h, int layout, bool all_models, uint8_t* dst, hipStream_t stream);

/// launch_resize_oriented with another vertical pass: the first-pass launches are exactly that call's, then
/// resize_v_tensor_kernel writes elements of `type` (a TensorType) to `dst` (aligned to the element), normalised by `norm`
/// unless they are bytes, items with kResizeFlipOutput flipped left to right. At most three launches, two without items of 5..8.
hipError_t launch_resize_tensor(
    const ResizeJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int h_tiles, int t_tiles, bool mirror_store,
    int out_w, int out_h, int layout, bool all_models, int type, const TensorNorm& norm, void* dst, hipStream_t stream);

/// The conversion of `n` items: `d_jobs` RgbJob[n], `d_first_tile` int[n] (each item's first workgroup of the row
/// kernel; `row_tiles` in all) and `d_first_tile_t` int[n] (the same for the transposing kernel, `t_tiles`) in device
/// memory. Items of orientations 1..4 have their tiles in the first list, items of 5..8 in the second, none in the other.
/// At most two launches: none for a list without tiles. `planar`: CHW. `all_models`: some item is not grey or YCbCr
/// (fancy_all_models); both kernels then run as the instantiation that knows every model, for all items of the call.
hipError_t launch_rgb_batch(
    const RgbJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int row_tiles, int t_tiles, bool planar, bool all_models,
    hipStream_t stream);

/// The reduction of `n` items in one launch: `d_jobs` ReduceJob[n] and `d_first_tile` int[n] (each item's first workgroup;
/// `tiles` in all) in device memory. `all_models`: some item is not grey or YCbCr (fancy_all_models).
hipError_t launch_reduce(const ReduceJob* d_jobs, const int* d_first_tile, int n, int tiles, bool all_models, hipStream_t stream);

// The grey output stage (jg_output_gray.hip). Its sources are fancy_source's with `gray` set: one component (grey and
// YCbCr files: component 0) or three (RGB-coded files: jdcolor.c's rgb_gray_convert); `rgb`: some item of the call is of
// the second kind, and every kernel of the call then runs as the instantiation that stages three tiles.

/// One image to grey where job.flips and `transposes` display it: the tiles of launch_gray_batch for a descriptor that
/// travels as a kernel argument. One launch.
hipError_t launch_gray_image(const RgbJob& job, bool transposes, hipStream_t stream);

/// launch_rgb_batch for one 8-bit channel: displayed pixel (x, y) of an item at dst + y * dst_pitch + x. At most two
/// launches. An item of orientation 1 whose component 0 is at full resolution is copied, in the row kernel's launch.
hipError_t launch_gray_batch(
    const RgbJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int row_tiles, int t_tiles, bool rgb, hipStream_t stream);

/// launch_resize_tensor for one channel: ResizeJob::mid holds one byte per pixel, `dst` is n x out_h x out_w elements of
/// `type`, normalised by the one `mean` and `std` unless they are bytes. Two launches, three with items of 5..8 beside
/// others.
hipError_t launch_gray_resize(
    const ResizeJob* d_jobs, const int* d_first_tile, const int* d_first_tile_t, int n, int h_tiles, int t_tiles, int out_w, int out_h, bool rgb,
    int type, float mean, float std, void* dst, hipStream_t stream);

} // namespace jg

#endif // JG_OUTPUT_HPP_
