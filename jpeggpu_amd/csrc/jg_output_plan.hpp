// jg_output_plan.hpp -- the host plan of the RGB output stage (jg_output_plan.cpp): every check of a call's arguments, the
// weight tables, the scratch layouts, and the fill of the bytes a call stages and copies. Free of HIP: jg_output.cpp runs
// the plans on the device, tests/emu/output_plan_check_main.cpp runs them under sanitizers without one.
#ifndef JG_OUTPUT_PLAN_HPP_
#define JG_OUTPUT_PLAN_HPP_

#include "jg_output_jobs.h"

#include <jpeggpu/jpeggpu.h>
#include <jpeggpu/jpeggpu_ext.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace jg {

/// The colour model the entry points without one assume: grey for one component, YCbCr for three, none for any other count.
int color_by_count(const jpeggpu_img_info* info);

/// Every check of a libjpeg-exact conversion's source, and its description for the kernels: the planes `src` of `info`,
/// which are the windows of a cropped decode if `crop` is given and the whole planes otherwise, read as the colour model
/// `color` (enum jpeggpu_ext_color_space; one that does not fit the component count, or UNKNOWN: JPEGGPU_NOT_SUPPORTED). `replicate`: every
/// component is replicated (libjpeg at 1/8 scale: jdsample.c turns fancy upsampling off when min_DCT_scaled_size is 1);
/// the colour conversion stays jdcolor.c's. `rect_w` x `rect_h`, if asked for: the rectangle -- the crop's, or else the
/// image's extent by its planes (callers that convert a whole image bring their own size, and the kernel's clamp is
/// their edge rule).
/// `gray`: the source of a GREY output (jg_output_gray.hip): CMYK and YCCK are JPEGGPU_NOT_SUPPORTED; of a grey or YCbCr
/// image only component 0 is described (ncomp 1, colour GRAY, its ratios still those to the frame's largest factors) and
/// only its plane and window are looked at -- the other planes may be NULL --; an RGB-coded image keeps its three.
/// The statuses and their order are API. One order differs between the callers: jpeggpu_ext_crop_to_rgbi_* refuse a
/// window outside its plane before non-integral ratios (`window_first`), jpeggpu_ext_resize_to_rgb after them.
jpeggpu_status fancy_source(
    const jpeggpu_img_info* info, int color, const jpeggpu_ext_crop_info* crop, const jpeggpu_img* src, bool replicate, bool window_first,
    FancySource& s, int* rect_w = nullptr, int* rect_h = nullptr, bool gray = false);

/// Pillow's ksize: the most taps an output coordinate of a resize of `extent` input samples to `out` can get. `extent` is
/// the input size of every resize but a thumbnail's, whose box may end inside a sample (jpeggpu_ext_resize_box_weights).
int resize_max_taps(double extent, int out, int filter);

/// One direction of one item, in DISPLAYED pixels: the item's whole image of `full` samples is resized to `resized`, the
/// output is coordinates x0 .. x0 + out - 1 of that, and the item's rectangle holds samples origin .. origin + extent - 1.
/// A call without views resizes the rectangle itself: full = extent, resized = out, x0 = origin = 0. `box`: how much of
/// `full` the resize covers, which is `full` itself for every call but a thumbnail's (Pillow's box: it may end inside a
/// sample, and the scale is box / resized).
struct ResizeAxis {
    int full, resized, x0, origin, extent;
    double box;
};

/// Where everything of one call sits in d_scratch: the descriptors, each item's first tile, the tables (together the
/// part the host stages and copies, `head` bytes), then each item's horizontal-pass rows.
struct ResizePlan {
    int out_w = 0, out_h = 0, filter = 0; // of the call
    std::vector<ResizeJob> jobs;          // without the table and scratch pointers: fill_resize binds them
    std::vector<int> first_tile, in_w, in_h;
    std::vector<ResizeAxis> ax, ay; // the two directions of each item, displayed
    std::vector<size_t> off_tab_x, off_tab_y, off_mid;
    size_t off_first = 0, head = 0, total = 0;
    int h_tiles      = 0;
    bool all_models  = false; // an item that is not grey or YCbCr (fancy_all_models)
    // a call with orientations (jpeggpu_ext_resize_to_rgb_oriented): in_w x in_h is the DISPLAYED rectangle; items of 5..8
    // have their tiles in first_tile_t (the transposing first pass) and none in first_tile, the others the other way round
    std::vector<int> orient, first_tile_t;
    size_t off_first_t = 0;
    int t_tiles        = 0;
    bool mirror_store  = false; // an item with kResizeMirrorStore
};

/// Every check of a call's items, and its plan. `colors`: each item's colour model, or null: by its component count
/// (color_by_count). `orients`: each item's EXIF
/// orientation, or null: 1 for all -- the plan, the scratch layout and the launches are then what they were without it.
/// `views`: each item's window of the resize of its whole image (jpeggpu_ext_resize_view_to_tensor), or null: every item's
/// rectangle is resized to out_w x out_h -- which is the view {out_w, out_h, 0, 0} of an item that is a whole image.
/// `boxes` (with views only; jpeggpu_ext_thumbnail_to_rgb): item i's resize covers boxes[2 i] x boxes[2 i + 1] of its whole
/// image, or null: all of it, as in every other call. `gray`: a call of the grey stage -- the items' sources are grey ones
/// (fancy_source), a row of `mid` holds one byte per pixel, and `all_models` says that an item is RGB-coded.
jpeggpu_status plan_resize(
    const jpeggpu_ext_resize_item* items, const jpeggpu_ext_color_space* colors, const int* orients, const jpeggpu_ext_resize_view* views, int n,
    int out_w, int out_h, int filter, ResizePlan& p, const float* boxes = nullptr, bool gray = false);

/// The staged part of a planned call, written to the `p.head` bytes at `h`: the descriptors, bound to the 256-aligned
/// device address `base` of the scratch, the first-tile lists, and each item's two tables -- those of the DISPLAYED axes,
/// permuted for the stored order where an axis is mirrored. `flips` (host, one per item, or null): the items that get
/// kResizeFlipOutput; the vertical tensor pass alone reads it, so tables and `mid` stay as they are.
jpeggpu_status fill_resize(const ResizePlan& p, const unsigned char* flips, uint8_t* base, uint8_t* h);

/// Where everything of one jpeggpu_ext_batch_to_rgb call sits in d_scratch: the descriptors, then each item's first tile
/// in the row kernel's list and in the transposing kernel's. All of it is staged and copied (`total`, without the room
/// to align the pointer).
struct RgbBatchLayout {
    size_t off_first = 0, off_first_t = 0, total = 0;
};
RgbBatchLayout rgb_batch_layout(int n);

struct RgbBatchPlan {
    RgbBatchLayout at;
    std::vector<RgbJob> jobs;
    std::vector<int> first_tile, first_tile_t;
    int row_tiles = 0, t_tiles = 0;
    bool all_models = false; // an item that is not grey or YCbCr (fancy_all_models)
};

/// Every check of a call's items, and their descriptors. `gray`: a call of the grey stage (jpeggpu_ext_batch_to_gray) --
/// grey sources, one byte per pixel (dst_pitch >= the displayed width; `layout` and plane_stride are not read), and
/// `all_models` says that an item is RGB-coded.
jpeggpu_status plan_rgb_batch(const jpeggpu_ext_rgb_item* items, int n, int layout, RgbBatchPlan& p, bool gray = false);
/// The plan's staged bytes, written to the `p.at.total` bytes at `h`.
void fill_rgb_batch(const RgbBatchPlan& p, uint8_t* h);

/// Where everything of one thumbnail call sits in d_scratch, and what the resize passes are told: the reduction's
/// descriptors and tile list (`head` bytes, staged and copied), the reduced planes of the items that reduce, then the whole
/// layout of a resize call with views (ResizePlan) at `off_resize`. An item that reduces enters the resize as a made-up
/// whole image of its reduced planes -- one grey component or three RGB-coded ones, factors 1 --; any other item as itself.
struct ThumbnailPlan {
    ResizePlan resize;
    std::vector<ReduceJob> jobs; // of the items that reduce, in their order
    std::vector<int> first_tile;
    std::vector<jpeggpu_img_info> infos;
    std::vector<jpeggpu_img> imgs;
    std::vector<jpeggpu_ext_resize_item> items;
    std::vector<jpeggpu_ext_color_space> colors;
    std::vector<jpeggpu_ext_resize_view> views;
    std::vector<float> boxes;
    size_t off_first = 0, head = 0, off_resize = 0, total = 0;
    int tiles        = 0;
    bool all_models  = false; // an item that reduces and is RGB-coded
};

/// Every check of a call's items, and its plan. `base`: the 256-aligned start of the scratch (the reduced planes' addresses
/// go into the descriptors; the size call passes an address that nothing dereferences).
jpeggpu_status plan_thumbnails(
    const jpeggpu_ext_resize_item* items, const jpeggpu_ext_color_space* colors, const jpeggpu_ext_thumbnail* plans, int n, int canvas_w,
    int canvas_h, int filter, uint8_t* base, ThumbnailPlan& t);
/// The reduction's staged bytes, written to the `t.head` bytes at `h` (the resize's are fill_resize's of t.resize).
void fill_thumbnails(const ThumbnailPlan& t, uint8_t* h);

/// What Pillow's Image.thumbnail does to a width x height file: jpeggpu_ext_thumbnail_plan.
jpeggpu_status thumbnail_steps(int width, int height, int req_w, int req_h, int filter, double reducing_gap, jpeggpu_ext_thumbnail* plan);

/// The tensor calls' own checks, made first; `s`: the spec handed to the kernels.
jpeggpu_status tensor_spec(const jpeggpu_ext_tensor_spec* spec, jpeggpu_ext_tensor_spec& s);

} // namespace jg

#endif // JG_OUTPUT_PLAN_HPP_
