// jg_output_plan.cpp -- the host plan of the RGB output stage (jg_output_plan.hpp): argument checks, Pillow's weight
// tables, the scratch layouts of the batched calls and the fill of their staged bytes, and the exported functions of
// include/jpeggpu/jpeggpu_ext.h that launch nothing. Nothing here touches the device: no HIP header, a plain C++ compiler
// builds it, and tests/test_output_plan_host.py runs it under ASan and UBSan in a stand-alone program.
//
// The double arithmetic of the tables and of the thumbnail sizes is Pillow's term by term: no contraction into fused
// multiply-adds (the pragma below for hipcc's clang; other compilers get -ffp-contract=off).
#include "jg_output_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace jg {

static_assert(kFancyGray == int{JPEGGPU_EXT_COLOR_GRAY} && kFancyYCbCr == int{JPEGGPU_EXT_COLOR_YCBCR} && kFancyRGB == int{JPEGGPU_EXT_COLOR_RGB} &&
                  kFancyCMYK == int{JPEGGPU_EXT_COLOR_CMYK} && kFancyYCCK == int{JPEGGPU_EXT_COLOR_YCCK},
              "FancyColor is enum jpeggpu_ext_color_space");
static_assert(kTensorU8 == int{JPEGGPU_EXT_TENSOR_U8} && kTensorF32 == int{JPEGGPU_EXT_TENSOR_F32} && kTensorF16 == int{JPEGGPU_EXT_TENSOR_F16} &&
                  kTensorBF16 == int{JPEGGPU_EXT_TENSOR_BF16},
              "TensorType is enum jpeggpu_ext_tensor_type");
// the layout the ctypes mirror (jpeggpu_amd/api.py, TensorSpec) is written for
static_assert(offsetof(jpeggpu_ext_tensor_spec, type) == 0 && offsetof(jpeggpu_ext_tensor_spec, mean) == 4 && offsetof(jpeggpu_ext_tensor_spec, std) == 16 &&
                  offsetof(jpeggpu_ext_tensor_spec, flips) == 32 && sizeof(jpeggpu_ext_tensor_spec) == 40,
              "struct jpeggpu_ext_tensor_spec");

namespace {
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
bool filter_known(int filter) { return filter == JPEGGPU_EXT_FILTER_BILINEAR || filter == JPEGGPU_EXT_FILTER_BICUBIC; }
} // namespace

int color_by_count(const jpeggpu_img_info* info)
{
    return !info ? JPEGGPU_EXT_COLOR_UNKNOWN : info->num_components == 1 ? JPEGGPU_EXT_COLOR_GRAY : info->num_components == 3 ? JPEGGPU_EXT_COLOR_YCBCR : JPEGGPU_EXT_COLOR_UNKNOWN;
}

jpeggpu_status fancy_source(
    const jpeggpu_img_info* info, int color, const jpeggpu_ext_crop_info* crop, const jpeggpu_img* src, bool replicate, bool window_first,
    FancySource& s, int* rect_w, int* rect_h, bool gray)
{
    if (!info || !src) return JPEGGPU_INVALID_ARGUMENT;
    const int nc = info->num_components;
    const int fits = color == JPEGGPU_EXT_COLOR_GRAY ? 1 : color == JPEGGPU_EXT_COLOR_YCBCR || color == JPEGGPU_EXT_COLOR_RGB ? 3
                     : color == JPEGGPU_EXT_COLOR_CMYK || color == JPEGGPU_EXT_COLOR_YCCK ? 4 : 0;
    if (fits == 0 || nc != fits) return JPEGGPU_NOT_SUPPORTED; // without a model: 2 or 4 components, as jpeggpu_ext_planes_to_rgbi
    if (gray && fits == 4) return JPEGGPU_NOT_SUPPORTED;       // libjpeg has no grey of CMYK and YCCK
    // the components the output reads: all of them, or for a grey of a YCbCr source component 0 alone (the others' planes
    // are not looked at: a luma-only decode has none); the sampling maxima are the frame's either way
    const int used = gray && color != JPEGGPU_EXT_COLOR_RGB ? 1 : nc;
    int sx_max = 0, sy_max = 0;
    bool outside = false; // a window that does not lie inside its plane
    for (int c = 0; c < nc; ++c) {
        if (info->subsampling.x[c] < 1 || info->subsampling.y[c] < 1) return JPEGGPU_INVALID_ARGUMENT;
        sx_max = std::max(sx_max, info->subsampling.x[c]);
        sy_max = std::max(sy_max, info->subsampling.y[c]);
        if (c >= used) continue;
        if (!src->image[c] || src->pitch[c] < info->sizes_x[c] || info->sizes_x[c] < 1 || info->sizes_y[c] < 1)
            return JPEGGPU_INVALID_ARGUMENT;
        if (crop)
            outside = outside || crop->origin_x[c] < 0 || crop->origin_y[c] < 0 || crop->origin_x[c] + info->sizes_x[c] > crop->full_x[c] ||
                      crop->origin_y[c] + info->sizes_y[c] > crop->full_y[c];
    }
    if (outside && window_first) return JPEGGPU_INVALID_ARGUMENT;
    for (int c = 0; c < nc; ++c) // libjpeg upsamples by integral ratios only (jdsample.c)
        if (sx_max % info->subsampling.x[c] != 0 || sy_max % info->subsampling.y[c] != 0) return JPEGGPU_NOT_SUPPORTED;
    if (crop) {
        if (crop->width <= 0 || crop->height <= 0 || crop->x < 0 || crop->y < 0 || outside) return JPEGGPU_INVALID_ARGUMENT;
        for (int c = 0; c < used; ++c) { // every sample the rectangle reads, and its halo, clipped to the plane, is in the window
            const int hr = sx_max / info->subsampling.x[c], vr = sy_max / info->subsampling.y[c];
            const int lo_x = std::max(crop->x / hr - 1, 0), hi_x = std::min((crop->x + crop->width - 1) / hr + 1, crop->full_x[c] - 1);
            const int lo_y = std::max(crop->y / vr - 1, 0), hi_y = std::min((crop->y + crop->height - 1) / vr + 1, crop->full_y[c] - 1);
            if (lo_x < crop->origin_x[c] || hi_x >= crop->origin_x[c] + info->sizes_x[c] || lo_y < crop->origin_y[c] ||
                hi_y >= crop->origin_y[c] + info->sizes_y[c])
                return JPEGGPU_INVALID_ARGUMENT;
        }
    }
    s = FancySource{};
    for (int k = 0; k < 4; ++k) {
        const int cc = k < used ? k : 0;
        FancyComp& f = s.comp[k];
        f.plane      = src->image[cc];
        f.pitch      = src->pitch[cc];
        f.w          = info->sizes_x[cc];
        f.h          = info->sizes_y[cc];
        f.ox         = crop ? crop->origin_x[cc] : 0;
        f.oy         = crop ? crop->origin_y[cc] : 0;
        f.hr         = sx_max / info->subsampling.x[cc];
        f.vr         = sy_max / info->subsampling.y[cc];
        f.mode       = replicate ? kFancyReplicate : fancy_mode(f.hr, f.vr, crop ? crop->full_x[cc] : f.w); // on the FULL plane's width
    }
    s.x     = crop ? crop->x : 0;
    s.y     = crop ? crop->y : 0;
    s.ncomp = used;
    s.color = used == nc ? color : JPEGGPU_EXT_COLOR_GRAY;
    if (rect_w && rect_h) {
        if (crop) {
            *rect_w = crop->width;
            *rect_h = crop->height;
        } else { // a plane of the largest factors has the image's extent
            for (int c = 0; c < nc; ++c) {
                if (info->subsampling.x[c] == sx_max) *rect_w = info->sizes_x[c];
                if (info->subsampling.y[c] == sy_max) *rect_h = info->sizes_y[c];
            }
        }
    }
    return JPEGGPU_SUCCESS;
}

// ------------------------------------------------------------------------------------------------
// batched resize (jpeggpu_ext_resize_to_rgb): Pillow's weight tables, the items' descriptors, the scratch layout
// ------------------------------------------------------------------------------------------------

namespace {
constexpr int kResizePrecision = 22; // fraction bits of a weight (Pillow's PRECISION_BITS for 8-bit images)

double resize_support(int filter) { return filter == JPEGGPU_EXT_FILTER_BILINEAR ? 1.0 : 2.0; }
} // namespace

int resize_max_taps(double extent, int out, int filter)
{
#pragma clang fp contract(off)
    const double scale = extent / out;
    const double fs    = scale < 1.0 ? 1.0 : scale;
    return static_cast<int>(std::ceil(resize_support(filter) * fs)) * 2 + 1;
}

namespace {

/// Pillow's bilinear (triangle) and bicubic (a = -0.5) filters, term by term.
double resize_filter(int filter, double x)
{
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (filter == JPEGGPU_EXT_FILTER_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

/// Taps first .. first + count - 1 of output coordinate x: `in` samples, of which the resize covers `extent`.
void resize_bounds(int in, double extent, int out, int filter, int x, int* first, int* count)
{
#pragma clang fp contract(off)
    const double scale   = extent / out;
    const double fs      = scale < 1.0 ? 1.0 : scale;
    const double support = resize_support(filter) * fs;
    const double center  = (x + 0.5) * scale;
    const int lo         = std::max(static_cast<int>(center - support + 0.5), 0);
    const int hi         = std::min(static_cast<int>(center + support + 0.5), in);
    *first               = lo;
    *count               = hi - lo;
}

/// The table of in -> out (in != out, or an extent that is not `in`) for output coordinates x0 .. x0 + n_out - 1 into
/// first / count / w[n_out][stride], stride >= resize_max_taps; Pillow's precompute_coeffs + normalize_coeffs_8bpc. A
/// coordinate outside [0, out) gets no taps (resize_carry_empty gives its `first` a value). The whole table is x0 = 0,
/// n_out = out.
void resize_table(int in, double extent, int out, int filter, int x0, int n_out, int* first, int* count, int* w, int stride)
{
#pragma clang fp contract(off)
    const double scale = extent / out;
    const double fs    = scale < 1.0 ? 1.0 : scale;
    const double ss    = 1.0 / fs;
    const double one   = static_cast<double>(1 << kResizePrecision);
    std::vector<double> k(static_cast<size_t>(stride));
    for (int e = 0; e < n_out; ++e) {
        const int64_t x = static_cast<int64_t>(x0) + e;
        int lo = 0, n = 0;
        if (x >= 0 && x < out) resize_bounds(in, extent, out, filter, static_cast<int>(x), &lo, &n);
        const double center = (x + 0.5) * scale;
        double sum          = 0.0;
        for (int j = 0; j < n; ++j) {
            k[j] = resize_filter(filter, ((j + lo) - center + 0.5) * ss);
            sum += k[j];
        }
        if (sum != 0.0)
            for (int j = 0; j < n; ++j) k[j] /= sum;
        first[e] = lo;
        count[e] = n;
        int* row = w + static_cast<size_t>(e) * stride;
        for (int j = 0; j < stride; ++j)
            row[j] = j >= n ? 0 : k[j] < 0 ? static_cast<int>(-0.5 + k[j] * one) : static_cast<int>(0.5 + k[j] * one);
    }
}

/// A direction whose size does not change: one tap of weight 1 (Pillow skips the pass; the result is the same).
/// Coordinates x0 .. x0 + n_out - 1 of `size`, those outside [0, size) without a tap.
void resize_identity(int size, int x0, int n_out, int* first, int* count, int* w, int stride)
{
    for (int e = 0; e < n_out; ++e) {
        const int64_t x = static_cast<int64_t>(x0) + e;
        const bool in = x >= 0 && x < size;
        first[e] = in ? static_cast<int>(x) : 0;
        count[e] = in ? 1 : 0;
        for (int j = 0; j < stride; ++j) w[static_cast<size_t>(e) * stride + j] = in && j == 0 ? 1 << kResizePrecision : 0;
    }
}

/// Entries without taps (a window's coordinates outside the resized image: padding) keep the kernels' reading of the
/// table true: resize_h_tile takes a tile's input range from its first entry's `first` and its last entry's
/// first + count, so an empty entry in front of the image carries the `first` of the first entry with taps, and one
/// behind it first + count of the last. `first` is then rebased by `origin`. A table without empty entries only has
/// `origin` subtracted.
void resize_carry_empty(int* first, const int* count, int n_out, int origin)
{
    int a = 0, b = n_out - 1;
    while (a < n_out && count[a] == 0) ++a;
    while (b >= 0 && count[b] == 0) --b;
    for (int e = 0; e < n_out; ++e) {
        if (a > b) first[e] = 0; // no entry has taps
        else if (e < a) first[e] = first[a] - origin;
        else if (e > b) first[e] = first[b] + count[b] - origin;
    }
    for (int e = a; e <= b; ++e) first[e] -= origin;
}

/// One item's axis is skipped (resize_identity) when nothing changes along it: the size stays and the extent is the size.
bool resize_axis_same(int in, double extent, int out) { return in == out && extent == static_cast<double>(in); }

int resize_taps(int in, double extent, int out, int filter) { return resize_axis_same(in, extent, out) ? 1 : resize_max_taps(extent, out, filter); }

/// Table bytes of one direction: {first, count}[out] + weights[out][taps]
size_t resize_table_bytes(int out, int taps) { return sizeof(int) * static_cast<size_t>(out) * (2 + static_cast<size_t>(taps)); }

/// Samples [*lo, *hi) of the whole image that the taps of the window's coordinates read; false if no coordinate of the
/// window lies in the resized image. (first and first + count do not decrease with the coordinate.)
bool resize_axis_range(const ResizeAxis& a, int out, int filter, int* lo, int* hi)
{
    const int64_t c0 = std::max<int64_t>(a.x0, 0), c1 = std::min<int64_t>(static_cast<int64_t>(a.x0) + out, a.resized) - 1;
    if (c0 > c1) return false;
    if (resize_axis_same(a.full, a.box, a.resized)) {
        *lo = static_cast<int>(c0);
        *hi = static_cast<int>(c1) + 1;
        return true;
    }
    int f0 = 0, n0 = 0, f1 = 0, n1 = 0;
    resize_bounds(a.full, a.box, a.resized, filter, static_cast<int>(c0), &f0, &n0);
    resize_bounds(a.full, a.box, a.resized, filter, static_cast<int>(c1), &f1, &n1);
    *lo = f0;
    *hi = f1 + n1;
    return true;
}

/// The table the kernels get for one direction, before any mirroring: {first, count}[out], weights[out][taps] at `t`,
/// `first` relative to the rectangle.
void resize_axis_table(const ResizeAxis& a, int out, int taps, int filter, int* t)
{
    std::vector<int> first(static_cast<size_t>(out)), cnt(static_cast<size_t>(out));
    if (resize_axis_same(a.full, a.box, a.resized)) resize_identity(a.resized, a.x0, out, first.data(), cnt.data(), t + 2 * out, taps);
    else resize_table(a.full, a.box, a.resized, filter, a.x0, out, first.data(), cnt.data(), t + 2 * out, taps);
    resize_carry_empty(first.data(), cnt.data(), out, a.origin);
    for (int x = 0; x < out; ++x) {
        t[2 * x]     = first[x];
        t[2 * x + 1] = cnt[x];
    }
}

/// The item's WHOLE stored image at its scale: the full plane of a component with the largest factors (a cropped decode),
/// or the rectangle itself, which then is the image. After fancy_source has accepted the item.
void resize_item_full(const jpeggpu_ext_resize_item& it, int in_w, int in_h, int* full_w, int* full_h)
{
    *full_w = in_w;
    *full_h = in_h;
    if (!it.crop) return;
    int sx_max = 0, sy_max = 0;
    for (int c = 0; c < it.info->num_components; ++c) {
        sx_max = std::max(sx_max, it.info->subsampling.x[c]);
        sy_max = std::max(sy_max, it.info->subsampling.y[c]);
    }
    for (int c = 0; c < it.info->num_components; ++c) {
        if (it.info->subsampling.x[c] == sx_max) *full_w = it.crop->full_x[c];
        if (it.info->subsampling.y[c] == sy_max) *full_h = it.crop->full_y[c];
    }
}

/// A weight table of `out` coordinates over an axis of `in` samples, turned to run against the axis: coordinate x keeps
/// its place, its taps are sample in - 1 - s for every s they were, so first becomes in - first - count and the weights
/// are reversed. The weights themselves are never computed again for the mirrored axis: Pillow's float centres are not
/// symmetric to the last of the 22 fraction bits. `t`: {first, count}[out], weights[out][taps].
void mirror_taps(int* t, int in, int out, int taps)
{
    for (int x = 0; x < out; ++x) {
        const int cnt = t[2 * x + 1];
        t[2 * x]      = in - t[2 * x] - cnt;
        int* w        = t + 2 * out + static_cast<size_t>(x) * taps;
        std::reverse(w, w + cnt);
    }
}

/// The table's coordinates in reverse order: entry x becomes entry out - 1 - x (mirror_taps + this: the table of a
/// mirrored axis in stored order, first ascending again).
void reverse_columns(int* t, int out, int taps)
{
    for (int x = 0, y = out - 1; x < y; ++x, --y) {
        std::swap(t[2 * x], t[2 * y]);
        std::swap(t[2 * x + 1], t[2 * y + 1]);
        std::swap_ranges(t + 2 * out + static_cast<size_t>(x) * taps, t + 2 * out + static_cast<size_t>(x + 1) * taps, t + 2 * out + static_cast<size_t>(y) * taps);
    }
}

} // namespace

jpeggpu_status plan_resize(
    const jpeggpu_ext_resize_item* items, const jpeggpu_ext_color_space* colors, const int* orients, const jpeggpu_ext_resize_view* views, int n,
    int out_w, int out_h, int filter, ResizePlan& p, const float* boxes, bool gray)
{
    if (!items || n <= 0 || n > 65535 || out_w <= 0 || out_h <= 0) return JPEGGPU_INVALID_ARGUMENT;
    if (!filter_known(filter)) return JPEGGPU_NOT_SUPPORTED;
    bool transposing = false;
    for (int i = 0; orients && i < n; ++i) {
        if (!orient_valid(orients[i])) return JPEGGPU_INVALID_ARGUMENT;
        transposing = transposing || orient_transposes(orients[i]);
    }
    try {
        p.orient.assign(n, 1);
        if (orients) p.orient.assign(orients, orients + n);
        if (transposing) p.first_tile_t.resize(n);
        p.jobs.resize(n);
        p.first_tile.resize(n);
        p.in_w.resize(n);
        p.in_h.resize(n);
        p.ax.resize(n);
        p.ay.resize(n);
        p.off_tab_x.resize(n);
        p.off_tab_y.resize(n);
        p.off_mid.resize(n);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    p.out_w        = out_w;
    p.out_h        = out_h;
    p.filter       = filter;
    size_t off     = align_up(sizeof(ResizeJob) * n, 256);
    p.off_first    = off;
    off            = align_up(off + sizeof(int) * n, 256);
    if (transposing) {
        p.off_first_t = off;
        off           = align_up(off + sizeof(int) * n, 256);
    }
    int64_t tiles  = 0, tiles_t = 0;
    const int pitch = static_cast<int>(align_up((gray ? 1 : 3) * static_cast<size_t>(out_w), 16)); // a grey call keeps one byte per pixel
    for (int i = 0; i < n; ++i) {
        // the item's checks and its descriptor, without the table and scratch pointers; in_w x in_h is the rectangle
        p.jobs[i] = ResizeJob{};
        const jpeggpu_status st = fancy_source(items[i].info, colors ? static_cast<int>(colors[i]) : color_by_count(items[i].info), items[i].crop,
                                               items[i].src, views && views[i].replicate != 0, false, p.jobs[i].src, &p.in_w[i], &p.in_h[i], gray);
        if (st != JPEGGPU_SUCCESS) return st;
        p.all_models = p.all_models || fancy_all_models(p.jobs[i].src);
        const int o = p.orient[i];
        ResizeAxis& ax = p.ax[i];
        ResizeAxis& ay = p.ay[i];
        if (views) { // the window of the resize of the whole displayed image; the rectangle lies somewhere in that image
            const jpeggpu_ext_resize_view& v = views[i];
            if (v.resized_w <= 0 || v.resized_h <= 0) return JPEGGPU_INVALID_ARGUMENT;
            int fw = 0, fh = 0, rx = items[i].crop ? items[i].crop->x : 0, ry = items[i].crop ? items[i].crop->y : 0;
            resize_item_full(items[i], p.in_w[i], p.in_h[i], &fw, &fh);
            if (static_cast<int64_t>(rx) + p.in_w[i] > fw || static_cast<int64_t>(ry) + p.in_h[i] > fh) return JPEGGPU_INVALID_ARGUMENT;
            // the stored rectangle in displayed coordinates: jpeggpu_ext_orient_rect's map, the other way
            const int sx = orient_transposes(o) ? ry : rx, sw = orient_transposes(o) ? p.in_h[i] : p.in_w[i], fx = orient_transposes(o) ? fh : fw;
            const int sy = orient_transposes(o) ? rx : ry, sh = orient_transposes(o) ? p.in_w[i] : p.in_h[i], fy = orient_transposes(o) ? fw : fh;
            ax = ResizeAxis{fx, v.resized_w, v.x, orient_mirrors_x(o) ? fx - sx - sw : sx, sw, boxes ? static_cast<double>(boxes[2 * i]) : fx};
            ay = ResizeAxis{fy, v.resized_h, v.y, orient_mirrors_y(o) ? fy - sy - sh : sy, sh, boxes ? static_cast<double>(boxes[2 * i + 1]) : fy};
        }
        if (orient_transposes(o)) std::swap(p.in_w[i], p.in_h[i]); // the displayed rectangle from here on
        if (!views) {
            ax = ResizeAxis{p.in_w[i], out_w, 0, 0, p.in_w[i], static_cast<double>(p.in_w[i])};
            ay = ResizeAxis{p.in_h[i], out_h, 0, 0, p.in_h[i], static_cast<double>(p.in_h[i])};
        }
        // the samples the taps read: columns and rows of the displayed image, all of them inside the rectangle
        int lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0;
        if (!resize_axis_range(ax, out_w, filter, &lo_x, &hi_x) || !resize_axis_range(ay, out_h, filter, &lo_y, &hi_y))
            return JPEGGPU_INVALID_ARGUMENT; // a window beside the resized image
        if (lo_x < ax.origin || hi_x > ax.origin + ax.extent || lo_y < ay.origin || hi_y > ay.origin + ay.extent) return JPEGGPU_INVALID_ARGUMENT;
        ResizeJob& j = p.jobs[i];
        j.taps_x     = resize_taps(ax.full, ax.box, ax.resized, filter);
        j.taps_y     = resize_taps(ay.full, ay.box, ay.resized, filter);
        j.mid_pitch  = pitch;
        p.off_tab_x[i] = off;
        off += align_up(resize_table_bytes(out_w, j.taps_x), 16);
        p.off_tab_y[i] = off;
        off += align_up(resize_table_bytes(out_h, j.taps_y), 16);
        // the rectangle rows the vertical taps read (all of them when the height does not change)
        j.row0 = orient_mirrors_y(o) ? ay.origin + ay.extent - hi_y : lo_y - ay.origin; // rows of `mid` are in stored order (mirror_taps)
        j.rows = hi_y - lo_y;
        if (!orient_transposes(o) && orient_mirrors_x(o)) {
            j.pad_         = kResizeMirrorStore;
            p.mirror_store = true;
        }
        p.first_tile[i] = static_cast<int>(tiles);
        if (transposing) p.first_tile_t[i] = static_cast<int>(tiles_t);
        if (orient_transposes(o)) tiles_t += resize_t_tiles(j.rows, out_w);
        else tiles += resize_h_tiles(j.rows, out_w);
        if (tiles > INT32_MAX || tiles_t > INT32_MAX) return JPEGGPU_INVALID_ARGUMENT;
    }
    p.head  = off;
    p.h_tiles = static_cast<int>(tiles);
    p.t_tiles = static_cast<int>(tiles_t);
    for (int i = 0; i < n; ++i) {
        p.off_mid[i] = off;
        off          = align_up(off + static_cast<size_t>(p.jobs[i].rows) * pitch, 256);
    }
    p.total = off + 256; // room to align the caller's pointer
    return JPEGGPU_SUCCESS;
}

jpeggpu_status fill_resize(const ResizePlan& p, const unsigned char* flips, uint8_t* base, uint8_t* h)
{
    const size_t n = p.jobs.size();
    try {
        for (size_t i = 0; i < n; ++i) {
            ResizeJob j = p.jobs[i];
            j.tab_x     = reinterpret_cast<const int*>(base + p.off_tab_x[i]);
            j.tab_y     = reinterpret_cast<const int*>(base + p.off_tab_y[i]);
            j.mid       = base + p.off_mid[i];
            const ResizeAxis* axes[2] = {&p.ax[i], &p.ay[i]};
            const int dims[2][2] = {{p.out_w, j.taps_x}, {p.out_h, j.taps_y}};
            const size_t offs[2] = {p.off_tab_x[i], p.off_tab_y[i]};
            for (int d = 0; d < 2; ++d) {
                const int in = axes[d]->extent, out = dims[d][0], taps = dims[d][1]; // `first` counts from the rectangle's edge
                int* t = reinterpret_cast<int*>(h + offs[d]);
                resize_axis_table(*axes[d], out, taps, p.filter, t);
                // the tables are those of the DISPLAYED axes; a mirrored axis gets them permuted for the stored order
                const int o = p.orient[i];
                if (d == 0 ? orient_mirrors_x(o) : orient_mirrors_y(o)) mirror_taps(t, in, out, taps);
                if (d == 0 && (j.pad_ & kResizeMirrorStore)) reverse_columns(t, out, taps);
            }
            if (flips && flips[i]) j.pad_ |= kResizeFlipOutput;
            std::memcpy(h + sizeof(ResizeJob) * i, &j, sizeof(ResizeJob));
        }
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    std::memcpy(h + p.off_first, p.first_tile.data(), sizeof(int) * n);
    if (!p.first_tile_t.empty()) std::memcpy(h + p.off_first_t, p.first_tile_t.data(), sizeof(int) * n);
    return JPEGGPU_SUCCESS;
}

// ------------------------------------------------------------------------------------------------
// batched conversion (jpeggpu_ext_batch_to_rgb): the items' descriptors and the scratch layout
// ------------------------------------------------------------------------------------------------

RgbBatchLayout rgb_batch_layout(int n)
{
    RgbBatchLayout l;
    l.off_first   = align_up(sizeof(RgbJob) * static_cast<size_t>(n), 256);
    l.off_first_t = align_up(l.off_first + sizeof(int) * static_cast<size_t>(n), 256);
    l.total       = align_up(l.off_first_t + sizeof(int) * static_cast<size_t>(n), 256);
    return l;
}

jpeggpu_status plan_rgb_batch(const jpeggpu_ext_rgb_item* items, int n, int layout, RgbBatchPlan& p, bool gray)
{
    if (!items || n <= 0 || n > 65535 || (layout != JPEGGPU_EXT_HWC && layout != JPEGGPU_EXT_CHW)) return JPEGGPU_INVALID_ARGUMENT;
    try {
        p.jobs.resize(n);
        p.first_tile.resize(n);
        p.first_tile_t.resize(n);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    p.at = rgb_batch_layout(n);
    int64_t tiles = 0, tiles_t = 0;
    for (int i = 0; i < n; ++i) {
        const jpeggpu_ext_rgb_item& it = items[i];
        if (!it.dst || !orient_valid(it.orientation)) return JPEGGPU_INVALID_ARGUMENT;
        RgbJob& j = p.jobs[i];
        j         = RgbJob{};
        const jpeggpu_status st = fancy_source(it.info, it.color, it.crop, it.src, it.replicate != 0, true, j.src, &j.width, &j.height, gray);
        if (st != JPEGGPU_SUCCESS) return st;
        const bool tr = orient_transposes(it.orientation);
        const int64_t ow = tr ? j.height : j.width, oh = tr ? j.width : j.height; // the displayed rectangle
        if (gray ? it.dst_pitch < ow
                 : layout == JPEGGPU_EXT_HWC ? it.dst_pitch < 3 * ow : it.dst_pitch < ow || it.plane_stride < static_cast<size_t>(it.dst_pitch) * oh)
            return JPEGGPU_INVALID_ARGUMENT;
        p.all_models   = p.all_models || fancy_all_models(j.src);
        j.dst          = it.dst;
        j.dst_pitch    = it.dst_pitch;
        j.plane_stride = it.plane_stride;
        j.flips        = (orient_mirrors_x(it.orientation) ? 1 : 0) | (orient_mirrors_y(it.orientation) ? 2 : 0);
        j.tiles_x      = rgb_batch_tiles_x(j.width, tr);
        p.first_tile[i]   = static_cast<int>(tiles);
        p.first_tile_t[i] = static_cast<int>(tiles_t);
        (tr ? tiles_t : tiles) += rgb_batch_tiles(j.width, j.height, tr);
        if (tiles > INT32_MAX || tiles_t > INT32_MAX) return JPEGGPU_INVALID_ARGUMENT;
    }
    p.row_tiles = static_cast<int>(tiles);
    p.t_tiles   = static_cast<int>(tiles_t);
    return JPEGGPU_SUCCESS;
}

void fill_rgb_batch(const RgbBatchPlan& p, uint8_t* h)
{
    const size_t n = p.jobs.size();
    std::memcpy(h, p.jobs.data(), sizeof(RgbJob) * n);
    std::memcpy(h + p.at.off_first, p.first_tile.data(), sizeof(int) * n);
    std::memcpy(h + p.at.off_first_t, p.first_tile_t.data(), sizeof(int) * n);
}

// ------------------------------------------------------------------------------------------------
// thumbnails (jpeggpu_ext_thumbnail_plan, jpeggpu_ext_thumbnail_to_rgb): Pillow's size rule, and the call's layout
// ------------------------------------------------------------------------------------------------

namespace {
/// Image.thumbnail's round_aspect: of floor(number) and ceil(number) the one whose aspect ratio is nearer the image's, the
/// floor on a tie, and 1 at least. `along_x`: the result is a width beside the height `other`, else a height beside the
/// width `other` (a height of 0 counts as a perfect fit, and then becomes 1).
int round_aspect(double number, double aspect, int other, bool along_x)
{
#pragma clang fp contract(off)
    const double lo = std::floor(number), hi = std::ceil(number);
    const auto key = [&](double v) { return along_x ? std::fabs(aspect - v / other) : v == 0.0 ? 0.0 : std::fabs(aspect - other / v); };
    const double pick = key(hi) < key(lo) ? hi : lo;
    return std::max(static_cast<int>(pick), 1);
}
} // namespace

jpeggpu_status thumbnail_steps(int width, int height, int req_w, int req_h, int filter, double reducing_gap, jpeggpu_ext_thumbnail* plan)
{
#pragma clang fp contract(off)
    if (!plan || width < 1 || height < 1 || width > 65535 || height > 65535 || req_w < 1 || req_h < 1 || reducing_gap != reducing_gap ||
        (reducing_gap > 0.0 && reducing_gap < 1.0) || reducing_gap > 65536.0)
        return JPEGGPU_INVALID_ARGUMENT;
    if (!filter_known(filter)) return JPEGGPU_NOT_SUPPORTED;
    const bool gap = reducing_gap > 0.0;
    jpeggpu_ext_thumbnail p{};
    p.scale = p.fx = p.fy = 1;
    p.dec_w = p.red_w = p.out_w = width;
    p.dec_h = p.red_h = p.out_h = height;
    p.box_w = static_cast<float>(width);
    p.box_h = static_cast<float>(height);
    p.identity = 1;
    if (req_w >= width && req_h >= height) { // nothing happens: the full-scale decode
        *plan = p;
        return JPEGGPU_SUCCESS;
    }
    // 1. the final size (preserve_aspect_ratio)
    int x = req_w, y = req_h;
    const double aspect = static_cast<double>(width) / height;
    if (static_cast<double>(x) / y >= aspect) x = round_aspect(y * aspect, aspect, y, true);
    else y = round_aspect(x / aspect, aspect, x, false);
    p.out_w = x;
    p.out_h = y;
    // 2. draft() for the request times the gap
    if (gap) {
        const double dw = req_w * reducing_gap, dh = req_h * reducing_gap;
        const int rw = dw >= 2147483647.0 ? INT32_MAX : static_cast<int>(dw), rh = dh >= 2147483647.0 ? INT32_MAX : static_cast<int>(dh);
        const int s = std::min(width / rw, height / rh);
        p.scale = s >= 8 ? 8 : s >= 4 ? 4 : s >= 2 ? 2 : 1;
    }
    p.dec_w = p.red_w = (width + p.scale - 1) / p.scale;
    p.dec_h = p.red_h = (height + p.scale - 1) / p.scale;
    double bx = static_cast<double>(width) / p.scale, by = static_cast<double>(height) / p.scale;
    // 3. the draft already hit the size
    if (p.dec_w == x && p.dec_h == y) {
        p.box_w = static_cast<float>(p.dec_w);
        p.box_h = static_cast<float>(p.dec_h);
        *plan = p;
        return JPEGGPU_SUCCESS;
    }
    p.identity = 0;
    // 4. reduce
    if (gap) {
        p.fx = std::max(static_cast<int>(bx / x / reducing_gap), 1);
        p.fy = std::max(static_cast<int>(by / y / reducing_gap), 1);
        if (p.fx > 1 || p.fy > 1) {
            p.red_w = (p.dec_w + p.fx - 1) / p.fx;
            p.red_h = (p.dec_h + p.fy - 1) / p.fy;
            bx /= p.fx;
            by /= p.fy;
        }
    }
    // 5. the box passes through C as binary32
    p.box_w = static_cast<float>(bx);
    p.box_h = static_cast<float>(by);
    // 6. Pillow resizes such an image vertically first
    if (p.red_h > static_cast<int64_t>(p.red_w) * 100 && y < p.red_h) return JPEGGPU_NOT_SUPPORTED;
    *plan = p;
    return JPEGGPU_SUCCESS;
}

jpeggpu_status plan_thumbnails(
    const jpeggpu_ext_resize_item* items, const jpeggpu_ext_color_space* colors, const jpeggpu_ext_thumbnail* plans, int n, int canvas_w,
    int canvas_h, int filter, uint8_t* base, ThumbnailPlan& t)
{
    if (!items || !plans || n <= 0 || n > 65535 || canvas_w <= 0 || canvas_h <= 0) return JPEGGPU_INVALID_ARGUMENT;
    if (!filter_known(filter)) return JPEGGPU_NOT_SUPPORTED;
    int nr = 0;
    for (int i = 0; i < n; ++i) nr += plans[i].fx > 1 || plans[i].fy > 1 ? 1 : 0;
    try {
        t.jobs.resize(nr);
        t.first_tile.resize(nr);
        t.infos.resize(n);
        t.imgs.resize(n);
        t.items.resize(n);
        t.colors.resize(n);
        t.views.resize(n);
        t.boxes.resize(2 * static_cast<size_t>(n));
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    size_t off  = align_up(sizeof(ReduceJob) * nr, 256);
    t.off_first = off;
    off         = align_up(off + sizeof(int) * nr, 256);
    t.head      = off;
    int64_t tiles = 0;
    for (int i = 0, r = 0; i < n; ++i) {
        const jpeggpu_ext_thumbnail& pl = plans[i];
        const int color = colors ? static_cast<int>(colors[i]) : color_by_count(items[i].info);
        if (items[i].crop) return JPEGGPU_INVALID_ARGUMENT; // a thumbnail is of a whole image
        FancySource src;
        int w = 0, h = 0;
        const jpeggpu_status st = fancy_source(items[i].info, color, nullptr, items[i].src, pl.replicate != 0, false, src, &w, &h);
        if (st != JPEGGPU_SUCCESS) return st;
        if (color == JPEGGPU_EXT_COLOR_CMYK || color == JPEGGPU_EXT_COLOR_YCCK) return JPEGGPU_NOT_SUPPORTED; // Pillow's thumbnail of those is CMYK
        if (pl.dec_w != w || pl.dec_h != h || pl.fx < 1 || pl.fy < 1 || pl.red_w != (w + pl.fx - 1) / pl.fx || pl.red_h != (h + pl.fy - 1) / pl.fy ||
            pl.out_w < 1 || pl.out_h < 1 || pl.out_w > canvas_w || pl.out_h > canvas_h || !(pl.box_w > 0.0f) || !(pl.box_h > 0.0f) ||
            !std::isfinite(pl.box_w) || !std::isfinite(pl.box_h))
            return JPEGGPU_INVALID_ARGUMENT;
        const bool reduces = pl.fx > 1 || pl.fy > 1;
        if (pl.identity && (reduces || pl.out_w != w || pl.out_h != h)) return JPEGGPU_INVALID_ARGUMENT;
        if (static_cast<int64_t>(pl.fx) * pl.fy > (1 << 23)) return JPEGGPU_NOT_SUPPORTED; // a box's sum must fit 32 bits
        if (!pl.identity && pl.red_h > static_cast<int64_t>(pl.red_w) * 100 && pl.out_h < pl.red_h) return JPEGGPU_NOT_SUPPORTED; // Pillow: vertical pass first
        t.items[i]  = items[i];
        t.colors[i] = static_cast<jpeggpu_ext_color_space>(color);
        t.views[i]  = jpeggpu_ext_resize_view{pl.out_w, pl.out_h, 0, 0, reduces ? 0 : pl.replicate};
        t.boxes[2 * i]     = pl.identity ? static_cast<float>(w) : pl.box_w;
        t.boxes[2 * i + 1] = pl.identity ? static_cast<float>(h) : pl.box_h;
        if (!reduces) continue;
        const int nc       = src.ncomp == 1 ? 1 : 3;
        const int pitch    = static_cast<int>(align_up(static_cast<size_t>(pl.red_w), 16));
        const size_t plane = static_cast<size_t>(pitch) * pl.red_h;
        ReduceJob& j   = t.jobs[r];
        j              = ReduceJob{};
        j.src          = src;
        j.width        = w;
        j.height       = h;
        j.fx           = pl.fx;
        j.fy           = pl.fy;
        j.red_w        = pl.red_w;
        j.red_h        = pl.red_h;
        j.dst          = base + off;
        j.pitch        = pitch;
        j.plane_stride = plane;
        const int last_x = w - (pl.red_w - 1) * pl.fx, last_y = h - (pl.red_h - 1) * pl.fy; // pixels of the last column's and row's boxes
        j.mult[0]      = reduce_multiplier(pl.fx * pl.fy);
        j.mult[1]      = reduce_multiplier(last_x * pl.fy);
        j.mult[2]      = reduce_multiplier(pl.fx * last_y);
        j.mult[3]      = reduce_multiplier(last_x * last_y);
        j.rows_per_tile = reduce_rows_per_tile(pl.fy);
        j.tiles_x      = reduce_tiles_x(pl.red_w);
        t.all_models   = t.all_models || fancy_all_models(src);
        t.first_tile[r] = static_cast<int>(tiles);
        tiles += reduce_tiles(pl.red_w, pl.red_h, pl.fy);
        if (tiles > INT32_MAX) return JPEGGPU_INVALID_ARGUMENT;
        jpeggpu_img_info& info = t.infos[i];
        jpeggpu_img& img       = t.imgs[i];
        info                   = jpeggpu_img_info{};
        img                    = jpeggpu_img{};
        info.num_components    = nc;
        for (int c = 0; c < nc; ++c) {
            info.sizes_x[c]       = pl.red_w;
            info.sizes_y[c]       = pl.red_h;
            info.subsampling.x[c] = 1;
            info.subsampling.y[c] = 1;
            img.image[c]          = j.dst + c * plane;
            img.pitch[c]          = pitch;
        }
        t.items[i]  = jpeggpu_ext_resize_item{&info, nullptr, &img};
        t.colors[i] = nc == 1 ? JPEGGPU_EXT_COLOR_GRAY : JPEGGPU_EXT_COLOR_RGB;
        off         = align_up(off + nc * plane, 256);
        ++r;
    }
    t.tiles      = static_cast<int>(tiles);
    t.off_resize = off;
    const jpeggpu_status st = plan_resize(t.items.data(), t.colors.data(), nullptr, t.views.data(), n, canvas_w, canvas_h, filter, t.resize, t.boxes.data());
    if (st != JPEGGPU_SUCCESS) return st;
    t.total = t.off_resize + t.resize.total + 256; // room to align the caller's pointer
    return JPEGGPU_SUCCESS;
}

void fill_thumbnails(const ThumbnailPlan& t, uint8_t* h)
{
    std::memcpy(h, t.jobs.data(), sizeof(ReduceJob) * t.jobs.size());
    std::memcpy(h + t.off_first, t.first_tile.data(), sizeof(int) * t.first_tile.size());
}

jpeggpu_status tensor_spec(const jpeggpu_ext_tensor_spec* spec, jpeggpu_ext_tensor_spec& s)
{
    if (!spec) return JPEGGPU_INVALID_ARGUMENT;
    const int type = spec->type;
    if (type != JPEGGPU_EXT_TENSOR_U8 && type != JPEGGPU_EXT_TENSOR_F32 && type != JPEGGPU_EXT_TENSOR_F16 && type != JPEGGPU_EXT_TENSOR_BF16)
        return JPEGGPU_INVALID_ARGUMENT;
    s = *spec;
    for (int c = 0; c < 3; ++c) {
        if (type == JPEGGPU_EXT_TENSOR_U8) { // ignored: the kernel is handed values that mean nothing
            s.mean[c] = 0.0f;
            s.std[c]  = 1.0f;
        } else if (!std::isfinite(s.mean[c]) || !std::isfinite(s.std[c]) || s.std[c] == 0.0f) {
            return JPEGGPU_INVALID_ARGUMENT;
        }
    }
    return JPEGGPU_SUCCESS;
}

} // namespace jg

// ------------------------------------------------------------------------------------------------
// the exported functions that launch nothing (jpeggpu_ext.h)
// ------------------------------------------------------------------------------------------------

namespace {

size_t resize_scratch_size(
    const jpeggpu_ext_resize_item* items, const jpeggpu_ext_color_space* colors, const int* orients, int n, int out_w, int out_h, int filter,
    const jpeggpu_ext_resize_view* views = nullptr, bool gray = false)
{
    jg::ResizePlan p;
    return jg::plan_resize(items, colors, orients, views, n, out_w, out_h, filter, p, nullptr, gray) == JPEGGPU_SUCCESS ? p.total : 0;
}

/// The whole table of `in` samples, of which the resize covers `extent`, to `out`, or its coordinates x0 .. x0 + n_out - 1
/// (the checks that all three exported table functions share come first).
jpeggpu_status weight_table(int in, double extent, int out, int x0, int n_out, int filter, int* first, int* count, int* w, int max_taps)
{
    if (!jg::filter_known(filter)) return JPEGGPU_NOT_SUPPORTED;
    if (!first || !count || !w || in <= 0 || out <= 0 || n_out <= 0 || !(extent > 0.0) || !std::isfinite(extent) ||
        max_taps < jg::resize_max_taps(extent, out, filter))
        return JPEGGPU_INVALID_ARGUMENT;
    try {
        if (jg::resize_axis_same(in, extent, out)) jg::resize_identity(out, x0, n_out, first, count, w, max_taps);
        else jg::resize_table(in, extent, out, filter, x0, n_out, first, count, w, max_taps);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    return JPEGGPU_SUCCESS;
}

} // namespace

extern "C" {

size_t jpeggpu_ext_resize_scratch_size_cs(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, int n, int out_w, int out_h,
    enum jpeggpu_ext_filter filter)
{
    return colors ? resize_scratch_size(items, colors, nullptr, n, out_w, out_h, filter) : 0;
}

size_t jpeggpu_ext_resize_scratch_size(
    const struct jpeggpu_ext_resize_item* items, int n, int out_w, int out_h, enum jpeggpu_ext_filter filter)
{
    return resize_scratch_size(items, nullptr, nullptr, n, out_w, out_h, filter);
}

size_t jpeggpu_ext_resize_scratch_size_oriented(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const int* orientations, int n, int out_w,
    int out_h, enum jpeggpu_ext_filter filter)
{
    return colors && orientations ? resize_scratch_size(items, colors, orientations, n, out_w, out_h, filter) : 0;
}

size_t jpeggpu_ext_resize_view_scratch_size(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const int* orientations,
    const struct jpeggpu_ext_resize_view* views, int n, int out_w, int out_h, enum jpeggpu_ext_filter filter)
{
    return views ? resize_scratch_size(items, colors, orientations, n, out_w, out_h, filter, views) : 0;
}

size_t jpeggpu_ext_resize_view_to_gray_scratch_size(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const int* orientations,
    const struct jpeggpu_ext_resize_view* views, int n, int out_w, int out_h, enum jpeggpu_ext_filter filter)
{
    return resize_scratch_size(items, colors, orientations, n, out_w, out_h, filter, views, true);
}

size_t jpeggpu_ext_batch_gray_scratch_size(int n) { return jpeggpu_ext_batch_rgb_scratch_size(n); }

size_t jpeggpu_ext_batch_rgb_scratch_size(int n)
{
    return n <= 0 || n > 65535 ? 0 : jg::rgb_batch_layout(n).total + 256; // room to align the caller's pointer
}

size_t jpeggpu_ext_thumbnail_scratch_size(
    const struct jpeggpu_ext_resize_item* items, const enum jpeggpu_ext_color_space* colors, const struct jpeggpu_ext_thumbnail* plans, int n,
    int canvas_w, int canvas_h, enum jpeggpu_ext_filter filter)
{
    jg::ThumbnailPlan t;
    uint8_t* const nowhere = reinterpret_cast<uint8_t*>(uintptr_t{256}); // the planes' addresses are computed, never read
    return jg::plan_thumbnails(items, colors, plans, n, canvas_w, canvas_h, filter, nowhere, t) == JPEGGPU_SUCCESS ? t.total : 0;
}

enum jpeggpu_status jpeggpu_ext_resize_weights(
    int in, int out, enum jpeggpu_ext_filter filter, int* first, int* count, int* weights, int max_taps)
{
    return weight_table(in, in, out, 0, out, filter, first, count, weights, max_taps);
}

enum jpeggpu_status jpeggpu_ext_resize_box_weights(
    int in, float extent, int out, enum jpeggpu_ext_filter filter, int* first, int* count, int* weights, int max_taps)
{
    return weight_table(in, extent, out, 0, out, filter, first, count, weights, max_taps);
}

enum jpeggpu_status jpeggpu_ext_resize_view_weights(
    int in, int resized, int x0, int count_out, int origin, enum jpeggpu_ext_filter filter, int* first, int* count, int* weights, int max_taps)
{
    const jpeggpu_status st = weight_table(in, in, resized, x0, count_out, filter, first, count, weights, max_taps);
    if (st == JPEGGPU_SUCCESS) jg::resize_carry_empty(first, count, count_out, origin);
    return st;
}

enum jpeggpu_status jpeggpu_ext_orient_size(int orientation, int w, int h, int* out_w, int* out_h)
{
    if (!jg::orient_valid(orientation) || w < 1 || h < 1 || !out_w || !out_h) return JPEGGPU_INVALID_ARGUMENT;
    *out_w = jg::orient_transposes(orientation) ? h : w;
    *out_h = jg::orient_transposes(orientation) ? w : h;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_orient_rect(int orientation, int w, int h, int* x, int* y, int* rw, int* rh)
{
    if (!jg::orient_valid(orientation) || w < 1 || h < 1 || !x || !y || !rw || !rh) return JPEGGPU_INVALID_ARGUMENT;
    const bool tr = jg::orient_transposes(orientation);
    const int ow = tr ? h : w, oh = tr ? w : h;
    const int dx = *x, dy = *y, dw = *rw, dh = *rh;
    if (dx < 0 || dy < 0 || dw < 1 || dh < 1 || dw > ow - dx || dh > oh - dy) return JPEGGPU_INVALID_ARGUMENT;
    // the displayed x range lies along stored y if the orientation transposes, along stored x otherwise; mirrored or not
    const int ax = jg::orient_mirrors_x(orientation) ? ow - dx - dw : dx;
    const int ay = jg::orient_mirrors_y(orientation) ? oh - dy - dh : dy;
    *x  = tr ? ay : ax;
    *y  = tr ? ax : ay;
    *rw = tr ? dh : dw;
    *rh = tr ? dw : dh;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_resize_view_rect(
    int full_w, int full_h, int orientation, const struct jpeggpu_ext_resize_view* view, int out_w, int out_h, enum jpeggpu_ext_filter filter,
    int* x, int* y, int* w, int* h)
{
    if (!jg::filter_known(filter)) return JPEGGPU_NOT_SUPPORTED;
    if (!jg::orient_valid(orientation) || full_w < 1 || full_h < 1 || !view || view->resized_w <= 0 || view->resized_h <= 0 || out_w <= 0 ||
        out_h <= 0 || !x || !y || !w || !h)
        return JPEGGPU_INVALID_ARGUMENT;
    const bool tr = jg::orient_transposes(orientation);
    const jg::ResizeAxis ax{tr ? full_h : full_w, view->resized_w, view->x, 0, 0, static_cast<double>(tr ? full_h : full_w)};
    const jg::ResizeAxis ay{tr ? full_w : full_h, view->resized_h, view->y, 0, 0, static_cast<double>(tr ? full_w : full_h)};
    int lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0;
    if (!jg::resize_axis_range(ax, out_w, filter, &lo_x, &hi_x) || !jg::resize_axis_range(ay, out_h, filter, &lo_y, &hi_y))
        return JPEGGPU_INVALID_ARGUMENT;
    *x = lo_x;
    *y = lo_y;
    *w = hi_x - lo_x;
    *h = hi_y - lo_y;
    return jpeggpu_ext_orient_rect(orientation, full_w, full_h, x, y, w, h);
}

enum jpeggpu_status jpeggpu_ext_thumbnail_plan(
    int width, int height, int req_w, int req_h, enum jpeggpu_ext_filter filter, double reducing_gap, struct jpeggpu_ext_thumbnail* plan)
{
    return jg::thumbnail_steps(width, height, req_w, req_h, filter, reducing_gap, plan);
}

} // extern "C"
