// jg_output.cpp -- the RGB output stage's entry points of the exported C ABI (include/jpeggpu/jpeggpu_ext.h) that touch
// the device: they have jg_output_plan.cpp check and plan a call, stage and copy what the plan fills, and launch the
// kernels of jg_output.hip. The stage reads finished planes and knows nothing of the decoder. The JPEG round trip
// (jg_roundtrip.hip) is launched from here too: its second half is this stage, and it shares the staging ring.
#include "jg_output.hpp"
#include "jg_output_plan.hpp"
#include "jg_roundtrip.hpp"
#include "jg_staging.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>

namespace {

jpeggpu_status launched(hipError_t err) { return err == hipSuccess ? JPEGGPU_SUCCESS : JPEGGPU_INTERNAL_ERROR; }

/// The 256-aligned start of a caller's scratch: what the plans' offsets count from.
uint8_t* scratch_base(void* d_scratch) { return reinterpret_cast<uint8_t*>(jg::align_up(reinterpret_cast<uintptr_t>(d_scratch), 256)); }

/// The output stage's staging ring (the encoder keeps its own: a resize call does not wait for an encode call's lock).
jg::StagingRing& staging()
{
    static jg::StagingRing* s = new jg::StagingRing;
    return *s;
}

enum jpeggpu_status planes_to_rgbi_libjpeg(
    const struct jpeggpu_img_info* info, int color, const struct jpeggpu_img* src, uint8_t* dst, int dst_pitch, int width, int height,
    jpeggpu_stream_t stream, bool replicate)
{
    if (!info || !src || !dst || width <= 0 || height <= 0 || dst_pitch < 3 * width) return JPEGGPU_INVALID_ARGUMENT;
    jg::FancySource s;
    const jpeggpu_status st = jg::fancy_source(info, color, nullptr, src, replicate, false, s);
    if (st != JPEGGPU_SUCCESS) return st;
    return launched(jg::launch_rgbi_fancy(s, dst, dst_pitch, width, height, stream));
}

enum jpeggpu_status crop_to_rgbi_libjpeg(
    const struct jpeggpu_img_info* info, int color, const struct jpeggpu_ext_crop_info* crop, const struct jpeggpu_img* src, uint8_t* dst,
    int dst_pitch, jpeggpu_stream_t stream, bool replicate)
{
    if (!info || !crop || !src || !dst || crop->width <= 0 || crop->height <= 0 || crop->x < 0 || crop->y < 0 || dst_pitch < 3 * crop->width)
        return JPEGGPU_INVALID_ARGUMENT;
    jg::FancySource s;
    const jpeggpu_status st = jg::fancy_source(info, color, crop, src, replicate, true, s);
    if (st != JPEGGPU_SUCCESS) return st;
    return launched(jg::launch_rgbi_fancy(s, dst, dst_pitch, crop->width, crop->height, stream));
}

/// A finished plan on the device: its staged part filled, copied to the scratch and the passes launched. `spec` null:
/// uint8 through resize_v_kernel; else, checked by the caller, the tensor pass. Every check of the call has been made.
enum jpeggpu_status run_resize(
    const jg::ResizePlan& p, enum jpeggpu_ext_output_layout layout, const struct jpeggpu_ext_tensor_spec* spec, void* dst, void* d_scratch,
    jpeggpu_stream_t stream)
{
    uint8_t* base = scratch_base(d_scratch);
    const int n   = static_cast<int>(p.jobs.size());
    std::lock_guard<std::mutex> lock(staging().mu);
    const jpeggpu_status staged =
        staging().stage_and_copy(p.head, [&](uint8_t* h) { return jg::fill_resize(p, spec ? spec->flips : nullptr, base, h); }, base, stream);
    if (staged != JPEGGPU_SUCCESS) return staged;
    const jg::ResizeJob* d_jobs = reinterpret_cast<const jg::ResizeJob*>(base);
    const int* d_first = reinterpret_cast<const int*>(base + p.off_first);
    const int* d_first_t = reinterpret_cast<const int*>(base + p.off_first_t);
    if (!spec)
        return launched(jg::launch_resize_oriented(d_jobs, d_first, d_first_t, n, p.h_tiles, p.t_tiles, p.mirror_store, p.out_w, p.out_h, layout,
                                                   p.all_models, static_cast<uint8_t*>(dst), stream));
    jg::TensorNorm norm;
    for (int c = 0; c < 3; ++c) {
        norm.mean[c] = spec->mean[c];
        norm.std[c]  = spec->std[c];
    }
    return launched(jg::launch_resize_tensor(d_jobs, d_first, d_first_t, n, p.h_tiles, p.t_tiles, p.mirror_store, p.out_w, p.out_h, layout,
                                             p.all_models, spec->type, norm, dst, stream));
}

/// The plan and the checks of every resize call but the thumbnails', then run_resize. `colors` null: each item's model by
/// its component count. `orients` null: orientation 1 for all. `spec`: as run_resize's. `views` null: every item's
/// rectangle resized to the output; else each item's window (jpeggpu_ext_resize_view_to_tensor).
enum jpeggpu_status resize_to_rgb(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const int* orients, int n, int out_w, int out_h,
    enum jpeggpu_ext_filter filter, enum jpeggpu_ext_output_layout layout, void* dst, void* d_scratch, size_t scratch_size,
    jpeggpu_stream_t stream, const struct jpeggpu_ext_tensor_spec* spec = nullptr, const struct jpeggpu_ext_resize_view* views = nullptr)
{
    jg::ResizePlan p;
    const jpeggpu_status st = jg::plan_resize(items, colors, orients, views, n, out_w, out_h, filter, p);
    if (st != JPEGGPU_SUCCESS) return st;
    if (!dst || !d_scratch || (layout != JPEGGPU_EXT_NHWC && layout != JPEGGPU_EXT_NCHW) || scratch_size < p.total)
        return JPEGGPU_INVALID_ARGUMENT;
    if (spec && reinterpret_cast<uintptr_t>(dst) % jg::tensor_elem_size(spec->type) != 0) return JPEGGPU_INVALID_ARGUMENT;
    return run_resize(p, layout, spec, dst, d_scratch, stream);
}

} // namespace

extern "C" {

enum jpeggpu_status jpeggpu_ext_upsample_planes(
    const struct jpeggpu_img_info* info,
    const struct jpeggpu_img* src,
    struct jpeggpu_img* dst,
    int width,
    int height,
    jpeggpu_stream_t stream)
{
    if (!info || !src || !dst || width <= 0 || height <= 0) return JPEGGPU_INVALID_ARGUMENT;
    const int nc = info->num_components;
    if (nc < 1 || nc > JPEGGPU_MAX_COMP) return JPEGGPU_INVALID_ARGUMENT;
    int sx_max = 0, sy_max = 0;
    for (int c = 0; c < nc; ++c) {
        if (info->subsampling.x[c] < 1 || info->subsampling.y[c] < 1) return JPEGGPU_INVALID_ARGUMENT;
        sx_max = info->subsampling.x[c] > sx_max ? info->subsampling.x[c] : sx_max;
        sy_max = info->subsampling.y[c] > sy_max ? info->subsampling.y[c] : sy_max;
    }
    for (int c = 0; c < nc; ++c) {
        if (!src->image[c] || !dst->image[c] || dst->pitch[c] < width || src->pitch[c] < info->sizes_x[c])
            return JPEGGPU_INVALID_ARGUMENT;
        const hipError_t err = jg::launch_upsample(
            src->image[c], src->pitch[c], info->sizes_x[c], info->sizes_y[c],
            dst->image[c], dst->pitch[c], width, height,
            info->subsampling.x[c], sx_max, info->subsampling.y[c], sy_max, stream);
        if (err != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    }
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_planes_to_rgbi(
    const struct jpeggpu_img_info* info,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    int width,
    int height,
    jpeggpu_stream_t stream)
{
    if (!info || !src || !dst || width <= 0 || height <= 0 || dst_pitch < 3 * width) return JPEGGPU_INVALID_ARGUMENT;
    const int nc = info->num_components;
    if (nc != 1 && nc != 3) return JPEGGPU_NOT_SUPPORTED; // as the reference's helper (util/util.h:42-45)
    int sx_max = 0, sy_max = 0;
    for (int c = 0; c < nc; ++c) {
        if (info->subsampling.x[c] < 1 || info->subsampling.y[c] < 1) return JPEGGPU_INVALID_ARGUMENT;
        if (!src->image[c] || src->pitch[c] < info->sizes_x[c]) return JPEGGPU_INVALID_ARGUMENT;
        sx_max = info->subsampling.x[c] > sx_max ? info->subsampling.x[c] : sx_max;
        sy_max = info->subsampling.y[c] > sy_max ? info->subsampling.y[c] : sy_max;
    }
    return launched(jg::launch_rgbi(
        src->image, src->pitch, info->sizes_x, info->sizes_y, info->subsampling.x, info->subsampling.y,
        sx_max, sy_max, nc, dst, dst_pitch, width, height, stream));
}

enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_fancy_cs(
    const struct jpeggpu_img_info* info, enum jpeggpu_ext_color_space color, const struct jpeggpu_img* src, uint8_t* dst, int dst_pitch,
    int width, int height, jpeggpu_stream_t stream)
{
    return planes_to_rgbi_libjpeg(info, color, src, dst, dst_pitch, width, height, stream, false);
}

enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_replicate_cs(
    const struct jpeggpu_img_info* info, enum jpeggpu_ext_color_space color, const struct jpeggpu_img* src, uint8_t* dst, int dst_pitch,
    int width, int height, jpeggpu_stream_t stream)
{
    return planes_to_rgbi_libjpeg(info, color, src, dst, dst_pitch, width, height, stream, true);
}

enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_fancy_cs(
    const struct jpeggpu_img_info* info, enum jpeggpu_ext_color_space color, const struct jpeggpu_ext_crop_info* crop,
    const struct jpeggpu_img* src, uint8_t* dst, int dst_pitch, jpeggpu_stream_t stream)
{
    return crop_to_rgbi_libjpeg(info, color, crop, src, dst, dst_pitch, stream, false);
}

enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_replicate_cs(
    const struct jpeggpu_img_info* info, enum jpeggpu_ext_color_space color, const struct jpeggpu_ext_crop_info* crop,
    const struct jpeggpu_img* src, uint8_t* dst, int dst_pitch, jpeggpu_stream_t stream)
{
    return crop_to_rgbi_libjpeg(info, color, crop, src, dst, dst_pitch, stream, true);
}

// The entry points without a colour model: grey or YCbCr by the component count.
enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_fancy(
    const struct jpeggpu_img_info* info, const struct jpeggpu_img* src, uint8_t* dst, int dst_pitch, int width, int height,
    jpeggpu_stream_t stream)
{
    return planes_to_rgbi_libjpeg(info, jg::color_by_count(info), src, dst, dst_pitch, width, height, stream, false);
}

enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_replicate(
    const struct jpeggpu_img_info* info, const struct jpeggpu_img* src, uint8_t* dst, int dst_pitch, int width, int height,
    jpeggpu_stream_t stream)
{
    return planes_to_rgbi_libjpeg(info, jg::color_by_count(info), src, dst, dst_pitch, width, height, stream, true);
}

enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_fancy(
    const struct jpeggpu_img_info* info, const struct jpeggpu_ext_crop_info* crop, const struct jpeggpu_img* src, uint8_t* dst,
    int dst_pitch, jpeggpu_stream_t stream)
{
    return crop_to_rgbi_libjpeg(info, jg::color_by_count(info), crop, src, dst, dst_pitch, stream, false);
}

enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_replicate(
    const struct jpeggpu_img_info* info, const struct jpeggpu_ext_crop_info* crop, const struct jpeggpu_img* src, uint8_t* dst,
    int dst_pitch, jpeggpu_stream_t stream)
{
    return crop_to_rgbi_libjpeg(info, jg::color_by_count(info), crop, src, dst, dst_pitch, stream, true);
}

// EXIF orientation: the displayed image of the same conversions.
enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_oriented(
    const struct jpeggpu_img_info* info, enum jpeggpu_ext_color_space color, int orientation, int replicate, const struct jpeggpu_img* src,
    uint8_t* dst, int dst_pitch, int width, int height, jpeggpu_stream_t stream)
{
    if (!jg::orient_valid(orientation)) return JPEGGPU_INVALID_ARGUMENT;
    if (orientation == 1) return planes_to_rgbi_libjpeg(info, color, src, dst, dst_pitch, width, height, stream, replicate != 0);
    if (!info || !src || !dst || width <= 0 || height <= 0 || dst_pitch < 3 * (jg::orient_transposes(orientation) ? height : width))
        return JPEGGPU_INVALID_ARGUMENT;
    jg::FancySource s;
    const jpeggpu_status st = jg::fancy_source(info, color, nullptr, src, replicate != 0, false, s);
    if (st != JPEGGPU_SUCCESS) return st;
    return launched(jg::launch_rgbi_oriented(s, orientation, dst, dst_pitch, width, height, stream));
}

enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_oriented(
    const struct jpeggpu_img_info* info, enum jpeggpu_ext_color_space color, int orientation, int replicate,
    const struct jpeggpu_ext_crop_info* crop, const struct jpeggpu_img* src, uint8_t* dst, int dst_pitch, jpeggpu_stream_t stream)
{
    if (!jg::orient_valid(orientation)) return JPEGGPU_INVALID_ARGUMENT;
    if (orientation == 1) return crop_to_rgbi_libjpeg(info, color, crop, src, dst, dst_pitch, stream, replicate != 0);
    if (!info || !crop || !src || !dst || crop->width <= 0 || crop->height <= 0 || crop->x < 0 || crop->y < 0 ||
        dst_pitch < 3 * (jg::orient_transposes(orientation) ? crop->height : crop->width))
        return JPEGGPU_INVALID_ARGUMENT;
    jg::FancySource s;
    const jpeggpu_status st = jg::fancy_source(info, color, crop, src, replicate != 0, true, s);
    if (st != JPEGGPU_SUCCESS) return st;
    return launched(jg::launch_rgbi_oriented(s, orientation, dst, dst_pitch, crop->width, crop->height, stream));
}

// The batched resize: plain, with colour models, with orientations, as a model's input (flip, ToTensor, Normalize and the
// cast in the vertical pass), and as Resize + CenterCrop (a window of the resize of each item's whole image).
enum jpeggpu_status jpeggpu_ext_resize_to_rgb(
    const struct jpeggpu_ext_resize_item* items, int n, int out_w, int out_h, enum jpeggpu_ext_filter filter,
    enum jpeggpu_ext_output_layout layout, uint8_t* dst, void* d_scratch, size_t scratch_size, jpeggpu_stream_t stream)
{
    return resize_to_rgb(items, nullptr, nullptr, n, out_w, out_h, filter, layout, dst, d_scratch, scratch_size, stream);
}

enum jpeggpu_status jpeggpu_ext_resize_to_rgb_cs(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, int n, int out_w, int out_h,
    enum jpeggpu_ext_filter filter, enum jpeggpu_ext_output_layout layout, uint8_t* dst, void* d_scratch, size_t scratch_size,
    jpeggpu_stream_t stream)
{
    if (!colors) return JPEGGPU_INVALID_ARGUMENT;
    return resize_to_rgb(items, colors, nullptr, n, out_w, out_h, filter, layout, dst, d_scratch, scratch_size, stream);
}

enum jpeggpu_status jpeggpu_ext_resize_to_rgb_oriented(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const int* orientations, int n, int out_w,
    int out_h, enum jpeggpu_ext_filter filter, enum jpeggpu_ext_output_layout layout, uint8_t* dst, void* d_scratch, size_t scratch_size,
    jpeggpu_stream_t stream)
{
    if (!colors || !orientations) return JPEGGPU_INVALID_ARGUMENT;
    return resize_to_rgb(items, colors, orientations, n, out_w, out_h, filter, layout, dst, d_scratch, scratch_size, stream);
}

enum jpeggpu_status jpeggpu_ext_resize_to_tensor(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const int* orientations, int n, int out_w,
    int out_h, enum jpeggpu_ext_filter filter, enum jpeggpu_ext_output_layout layout, const struct jpeggpu_ext_tensor_spec* spec, void* dst,
    void* d_scratch, size_t scratch_size, jpeggpu_stream_t stream)
{
    jpeggpu_ext_tensor_spec s;
    const jpeggpu_status st = jg::tensor_spec(spec, s);
    if (st != JPEGGPU_SUCCESS) return st;
    return resize_to_rgb(items, colors, orientations, n, out_w, out_h, filter, layout, dst, d_scratch, scratch_size, stream, &s);
}

enum jpeggpu_status jpeggpu_ext_resize_view_to_tensor(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const int* orientations,
    const struct jpeggpu_ext_resize_view* views, int n, int out_w, int out_h, enum jpeggpu_ext_filter filter,
    enum jpeggpu_ext_output_layout layout, const struct jpeggpu_ext_tensor_spec* spec, void* dst, void* d_scratch, size_t scratch_size,
    jpeggpu_stream_t stream)
{
    jpeggpu_ext_tensor_spec s;
    const jpeggpu_status st = jg::tensor_spec(spec, s);
    if (st != JPEGGPU_SUCCESS) return st;
    if (!views) return JPEGGPU_INVALID_ARGUMENT;
    return resize_to_rgb(items, colors, orientations, n, out_w, out_h, filter, layout, dst, d_scratch, scratch_size, stream, &s, views);
}

// Batched conversion: many images to RGB at their own sizes.
enum jpeggpu_status jpeggpu_ext_batch_to_rgb(
    const struct jpeggpu_ext_rgb_item* items, int n, enum jpeggpu_ext_image_layout layout, void* d_scratch, size_t scratch_size,
    jpeggpu_stream_t stream)
{
    jg::RgbBatchPlan p;
    const jpeggpu_status st = jg::plan_rgb_batch(items, n, layout, p);
    if (st != JPEGGPU_SUCCESS) return st;
    if (!d_scratch || scratch_size < jpeggpu_ext_batch_rgb_scratch_size(n)) return JPEGGPU_INVALID_ARGUMENT;
    uint8_t* base = scratch_base(d_scratch);
    std::lock_guard<std::mutex> lock(staging().mu);
    const jpeggpu_status staged = staging().stage_and_copy(
        p.at.total,
        [&](uint8_t* h) {
            jg::fill_rgb_batch(p, h);
            return JPEGGPU_SUCCESS;
        },
        base, stream);
    if (staged != JPEGGPU_SUCCESS) return staged;
    return launched(jg::launch_rgb_batch(
        reinterpret_cast<const jg::RgbJob*>(base), reinterpret_cast<const int*>(base + p.at.off_first),
        reinterpret_cast<const int*>(base + p.at.off_first_t), n, p.row_tiles, p.t_tiles, layout == JPEGGPU_EXT_CHW, p.all_models, stream));
}

// Grey output (jg_output_gray.hip): one image, a batch at the items' own sizes, a batch resized to one 1-channel tensor.
enum jpeggpu_status jpeggpu_ext_crop_to_gray_oriented(
    const struct jpeggpu_img_info* info, enum jpeggpu_ext_color_space color, int orientation, int replicate,
    const struct jpeggpu_ext_crop_info* crop, const struct jpeggpu_img* src, uint8_t* dst, int dst_pitch, jpeggpu_stream_t stream)
{
    if (!jg::orient_valid(orientation)) return JPEGGPU_INVALID_ARGUMENT;
    if (!info || !src || !dst || (crop && (crop->width <= 0 || crop->height <= 0 || crop->x < 0 || crop->y < 0))) return JPEGGPU_INVALID_ARGUMENT;
    jg::RgbJob j{};
    const jpeggpu_status st = jg::fancy_source(info, color, crop, src, replicate != 0, true, j.src, &j.width, &j.height, true);
    if (st != JPEGGPU_SUCCESS) return st;
    const bool tr = jg::orient_transposes(orientation);
    if (j.width <= 0 || j.height <= 0 || dst_pitch < (tr ? j.height : j.width)) return JPEGGPU_INVALID_ARGUMENT;
    j.dst       = dst;
    j.dst_pitch = dst_pitch;
    j.flips     = (jg::orient_mirrors_x(orientation) ? 1 : 0) | (jg::orient_mirrors_y(orientation) ? 2 : 0);
    j.tiles_x   = jg::rgb_batch_tiles_x(j.width, tr);
    return launched(jg::launch_gray_image(j, tr, stream));
}

enum jpeggpu_status jpeggpu_ext_batch_to_gray(
    const struct jpeggpu_ext_rgb_item* items, int n, void* d_scratch, size_t scratch_size, jpeggpu_stream_t stream)
{
    jg::RgbBatchPlan p;
    const jpeggpu_status st = jg::plan_rgb_batch(items, n, JPEGGPU_EXT_HWC, p, true);
    if (st != JPEGGPU_SUCCESS) return st;
    if (!d_scratch || scratch_size < jpeggpu_ext_batch_gray_scratch_size(n)) return JPEGGPU_INVALID_ARGUMENT;
    uint8_t* base = scratch_base(d_scratch);
    std::lock_guard<std::mutex> lock(staging().mu);
    const jpeggpu_status staged = staging().stage_and_copy(
        p.at.total,
        [&](uint8_t* h) {
            jg::fill_rgb_batch(p, h);
            return JPEGGPU_SUCCESS;
        },
        base, stream);
    if (staged != JPEGGPU_SUCCESS) return staged;
    return launched(jg::launch_gray_batch(
        reinterpret_cast<const jg::RgbJob*>(base), reinterpret_cast<const int*>(base + p.at.off_first),
        reinterpret_cast<const int*>(base + p.at.off_first_t), n, p.row_tiles, p.t_tiles, p.all_models, stream));
}

enum jpeggpu_status jpeggpu_ext_resize_view_to_gray_tensor(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const int* orientations,
    const struct jpeggpu_ext_resize_view* views, int n, int out_w, int out_h, enum jpeggpu_ext_filter filter,
    enum jpeggpu_ext_output_layout layout, const struct jpeggpu_ext_tensor_spec* spec, void* dst, void* d_scratch, size_t scratch_size,
    jpeggpu_stream_t stream)
{
    jpeggpu_ext_tensor_spec s;
    if (spec) { // one mean and one std: the tensor calls' checks on three copies of them
        s = *spec;
        s.mean[1] = s.mean[2] = s.mean[0];
        s.std[1] = s.std[2] = s.std[0];
    }
    jpeggpu_status st = jg::tensor_spec(spec ? &s : nullptr, s);
    if (st != JPEGGPU_SUCCESS) return st;
    jg::ResizePlan p;
    st = jg::plan_resize(items, colors, orientations, views, n, out_w, out_h, filter, p, nullptr, true);
    if (st != JPEGGPU_SUCCESS) return st;
    if (!dst || !d_scratch || (layout != JPEGGPU_EXT_NHWC && layout != JPEGGPU_EXT_NCHW) || scratch_size < p.total) return JPEGGPU_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(dst) % jg::tensor_elem_size(s.type) != 0) return JPEGGPU_INVALID_ARGUMENT;
    uint8_t* base = scratch_base(d_scratch);
    std::lock_guard<std::mutex> lock(staging().mu);
    const jpeggpu_status staged = staging().stage_and_copy(p.head, [&](uint8_t* h) { return jg::fill_resize(p, s.flips, base, h); }, base, stream);
    if (staged != JPEGGPU_SUCCESS) return staged;
    return launched(jg::launch_gray_resize(
        reinterpret_cast<const jg::ResizeJob*>(base), reinterpret_cast<const int*>(base + p.off_first), reinterpret_cast<const int*>(base + p.off_first_t), n,
        p.h_tiles, p.t_tiles, p.out_w, p.out_h, p.all_models, s.type, s.mean[0], s.std[0], dst, stream));
}

// JPEG round trip (jg_roundtrip.hip): the encoder's first stage and the ISLOW transform in one launch, then the batched
// conversion above on the planes of the RGB items.
enum jpeggpu_status jpeggpu_ext_roundtrip_batch(
    const struct jpeggpu_ext_roundtrip_item* items, int n, enum jpeggpu_ext_image_layout layout, void* d_scratch, size_t scratch_size,
    jpeggpu_stream_t stream)
{
    jg::rt::Plan p;
    uint8_t* base = scratch_base(d_scratch ? d_scratch : reinterpret_cast<void*>(uintptr_t{256}));
    const jpeggpu_status st = jg::rt::plan_roundtrip(items, n, layout, base, p);
    if (st != JPEGGPU_SUCCESS) return st;
    if (!d_scratch || scratch_size < p.total + 256) return JPEGGPU_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(staging().mu);
    const jpeggpu_status staged = staging().stage_and_copy(
        p.head,
        [&](uint8_t* h) {
            jg::rt::fill_roundtrip(p, h);
            return JPEGGPU_SUCCESS;
        },
        base, stream);
    if (staged != JPEGGPU_SUCCESS) return staged;
    const hipError_t err = jg::rt::launch_roundtrip_blocks(reinterpret_cast<const jg::rt::Item*>(base + p.off_items), n, p.tiles, base, stream);
    if (err != hipSuccess || p.n_rgb == 0) return launched(err);
    return launched(jg::launch_rgb_batch(
        reinterpret_cast<const jg::RgbJob*>(base), reinterpret_cast<const int*>(base + p.rgb.at.off_first),
        reinterpret_cast<const int*>(base + p.rgb.at.off_first_t), p.n_rgb, p.rgb.row_tiles, p.rgb.t_tiles, layout == JPEGGPU_EXT_CHW, p.rgb.all_models,
        stream));
}

// Thumbnails: Pillow's Image.thumbnail of a batch -- draft, reduce, resize.
enum jpeggpu_status jpeggpu_ext_thumbnail_to_rgb(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const struct jpeggpu_ext_thumbnail* plans, int n,
    int canvas_w, int canvas_h, enum jpeggpu_ext_filter filter, uint8_t* dst, void* d_scratch, size_t scratch_size, jpeggpu_stream_t stream)
{
    jg::ThumbnailPlan t;
    uint8_t* base = scratch_base(d_scratch ? d_scratch : reinterpret_cast<void*>(uintptr_t{256}));
    const jpeggpu_status st = jg::plan_thumbnails(items, colors, plans, n, canvas_w, canvas_h, filter, base, t);
    if (st != JPEGGPU_SUCCESS) return st;
    if (!dst || !d_scratch || scratch_size < t.total) return JPEGGPU_INVALID_ARGUMENT;
    if (t.tiles > 0) { // the reduction of the items that have factors: one launch
        std::lock_guard<std::mutex> lock(staging().mu);
        const jpeggpu_status staged = staging().stage_and_copy(
            t.head,
            [&](uint8_t* h) {
                jg::fill_thumbnails(t, h);
                return JPEGGPU_SUCCESS;
            },
            base, stream);
        if (staged != JPEGGPU_SUCCESS) return staged;
        const hipError_t err = jg::launch_reduce(reinterpret_cast<const jg::ReduceJob*>(base), reinterpret_cast<const int*>(base + t.off_first),
                                                 static_cast<int>(t.jobs.size()), t.tiles, t.all_models, stream);
        if (err != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    }
    // the two resize passes over the canvas: a view larger than the resized image leaves zeros around it
    return run_resize(t.resize, JPEGGPU_EXT_NHWC, nullptr, dst, base + t.off_resize, stream);
}

} // extern "C"
