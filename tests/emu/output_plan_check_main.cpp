// output_plan_check_main.cpp -- the host plan of the RGB output stage (jg_output_plan.cpp) under AddressSanitizer + UBSan,
// without a device: where caller-supplied sizes, rectangles, views, boxes and thumbnail plans become table lengths,
// scratch offsets, tile counts and memcpy sizes. Built by tests/test_output_plan_host.py from this file and
// jg_output_plan.cpp alone.
//
//   output_plan_check_main                      the sweep below
//   output_plan_check_main cases.txt out.bin    the plans and tables of the cases in cases.txt, written to out.bin
//
// The sweep. Every case carries the status it must return; a case that succeeds is planned, its staged part is filled
// into a heap buffer of exactly the planned size (an overrun is a sanitizer report), and then
//   * table rows: a coordinate inside the resized image has count >= 1, one outside it (a view's padding) count == 0;
//     count <= taps, first >= 0 and first + count inside the item's rectangle (a thumbnail's: inside its box, rounded up);
//     the weights behind `count` are zero; the rows of `mid` that a vertical tap reads are rows the first pass writes;
//   * scratch layout: the regions start aligned as promised (256; tables and the first pass's rows 16), ascend without overlap, the staged ones end
//     at or in front of `head`, all of them in front of `total`; the descriptors point at them;
//   * tiles: the call's tile counts are the sums of the items' tiles, an item's first tile the sum of those before it;
//   * determinism: planning and filling twice gives the same bytes.
// Prints the cases per kind; the exit status is the number of the check that failed (see fail()).
//
// With two arguments: a line `W in out filter` writes status, taps, first[out], count[out], weights[out][taps] of
// jpeggpu_ext_resize_weights as int32; a line `T width height req_w req_h filter gap` writes the status as int32 and the
// struct jpeggpu_ext_thumbnail of jpeggpu_ext_thumbnail_plan. The test compares them with the shipped library's.
#include "jg_output_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

namespace {

char g_case[256] = "";

[[noreturn]] void fail(int code, const char* what)
{
    std::fprintf(stderr, "output plan check: %s: %s\n", g_case, what);
    std::exit(code);
}

uint8_t* const kBase   = reinterpret_cast<uint8_t*>(uintptr_t{0x7000} << 24); // never dereferenced
uint8_t* const kPlanes = reinterpret_cast<uint8_t*>(uintptr_t{0x3000} << 24);
uint8_t* const kDst    = reinterpret_cast<uint8_t*>(uintptr_t{0x5000} << 24);

const int kLen[] = {1, 2, 3, 7, 8, 9, 255, 256, 257, 65535};
const int kOut[] = {1, 2, 3, 224, 65535};
constexpr int kNumLen = 10, kNumOut = 5;
struct Pair {
    int in, out;
};
std::vector<Pair> pairs() // every length to every output size (1 -> 1 .. 65535 -> 65535: identity; 65535 -> 1), and 1 -> 64
{
    std::vector<Pair> p;
    for (int in : kLen)
        for (int out : kOut) p.push_back({in, out});
    p.push_back({1, 64});
    return p;
}

// ---- cases and their counts ----------------------------------------------------------------------

enum Kind { kTables, kResizePlans, kRgbPlans, kThumbSizes, kThumbPlans, kBadArgs, kKinds };
const char* const kKindName[kKinds] = {"tables", "resize plans", "rgb batch plans", "thumbnail sizes", "thumbnail plans", "bad arguments"};
int g_enumerated = 0, g_done[kKinds] = {}, g_refused[kKinds] = {};

/// A case begins: `what` names it in a failure's message.
void begin(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void begin(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
    ++g_enumerated;
}
/// A case ends: it returned `got`, it had to return `want`. True if it succeeded and its result is to be checked.
bool ended(Kind kind, int got, int want)
{
    if (got != want) {
        std::fprintf(stderr, "output plan check: %s: status %d, expected %d\n", g_case, got, want);
        std::exit(2);
    }
    ++g_done[kind];
    if (want != JPEGGPU_SUCCESS) ++g_refused[kind];
    return want == JPEGGPU_SUCCESS;
}

// ---- made-up decoded images ------------------------------------------------------------------------

struct Model {
    const char* name;
    int nc, h[4], v[4];
    jpeggpu_ext_color_space color;
};
const Model kModels[] = {
    {"grey", 1, {1}, {1}, JPEGGPU_EXT_COLOR_GRAY},
    {"444", 3, {1, 1, 1}, {1, 1, 1}, JPEGGPU_EXT_COLOR_YCBCR},
    {"422", 3, {2, 1, 1}, {1, 1, 1}, JPEGGPU_EXT_COLOR_YCBCR},
    {"440", 3, {1, 1, 1}, {2, 1, 1}, JPEGGPU_EXT_COLOR_YCBCR},
    {"420", 3, {2, 1, 1}, {2, 1, 1}, JPEGGPU_EXT_COLOR_YCBCR},
    {"411", 3, {4, 1, 1}, {1, 1, 1}, JPEGGPU_EXT_COLOR_YCBCR},
    {"cmyk", 4, {1, 1, 1, 1}, {1, 1, 1, 1}, JPEGGPU_EXT_COLOR_CMYK},
    {"ycck", 4, {2, 1, 1, 2}, {2, 1, 1, 2}, JPEGGPU_EXT_COLOR_YCCK},
};
constexpr int kNumModels = 8, kNumThumbModels = 6; // a thumbnail of a four-component file is refused

/// A decoded image of w x h pixels, or, with `rect` {x, y, w, h}, the windows of a cropped decode that just hold the
/// rectangle's samples and their halo. The plane addresses are never dereferenced.
struct Source {
    jpeggpu_img_info info{};
    jpeggpu_img img{};
    jpeggpu_ext_crop_info crop{};
    bool cropped = false;
    jpeggpu_ext_resize_item item() const { return jpeggpu_ext_resize_item{&info, cropped ? &crop : nullptr, &img}; }
};
Source make_source(const Model& m, int w, int h, const int* rect = nullptr)
{
    Source s;
    const int hmax = *std::max_element(m.h, m.h + m.nc), vmax = *std::max_element(m.v, m.v + m.nc);
    s.info.num_components = m.nc;
    s.cropped             = rect != nullptr;
    if (rect) {
        s.crop.x      = rect[0];
        s.crop.y      = rect[1];
        s.crop.width  = rect[2];
        s.crop.height = rect[3];
    }
    for (int c = 0; c < m.nc; ++c) {
        const int hr = hmax / m.h[c], vr = vmax / m.v[c];
        const int full_x = static_cast<int>((static_cast<int64_t>(w) * m.h[c] + hmax - 1) / hmax);
        const int full_y = static_cast<int>((static_cast<int64_t>(h) * m.v[c] + vmax - 1) / vmax);
        s.info.subsampling.x[c] = m.h[c];
        s.info.subsampling.y[c] = m.v[c];
        s.info.sizes_x[c]       = full_x;
        s.info.sizes_y[c]       = full_y;
        if (rect) {
            const int lo_x = std::max(rect[0] / hr - 1, 0), hi_x = std::min((rect[0] + rect[2] - 1) / hr + 1, full_x - 1);
            const int lo_y = std::max(rect[1] / vr - 1, 0), hi_y = std::min((rect[1] + rect[3] - 1) / vr + 1, full_y - 1);
            s.crop.origin_x[c] = lo_x;
            s.crop.origin_y[c] = lo_y;
            s.crop.full_x[c]   = full_x;
            s.crop.full_y[c]   = full_y;
            s.info.sizes_x[c]  = hi_x - lo_x + 1;
            s.info.sizes_y[c]  = hi_y - lo_y + 1;
        }
        s.img.image[c] = kPlanes + (static_cast<size_t>(c) << 34);
        s.img.pitch[c] = s.info.sizes_x[c];
    }
    return s;
}

/// The rectangles of an axis of `len` samples that a crop can go wrong at: all of it, an odd origin to the far edge, one
/// sample at either edge, an odd origin inside.
void axis_rect(int len, int kind, int* origin, int* extent)
{
    const int mid = (len / 2) | 1;
    switch (len < 2 ? 0 : kind) {
    case 1: *origin = 1, *extent = len - 1; break;
    case 2: *origin = 0, *extent = 1; break;
    case 3: *origin = len - 1, *extent = 1; break;
    case 4: *origin = std::min(mid, len - 1), *extent = std::min(3, len - *origin); break;
    default: *origin = 0, *extent = len;
    }
}

// ---- the checks ------------------------------------------------------------------------------------

struct Region {
    size_t offset, bytes, align;
};
/// Regions in the order the plan lays them out: aligned, ascending, none overlapping the next, all in front of `end`.
void check_regions(const std::vector<Region>& r, size_t end)
{
    for (size_t i = 0; i < r.size(); ++i) {
        if (r[i].offset % r[i].align) fail(10, "a region does not start aligned");
        if (r[i].offset > end || r[i].bytes > end - r[i].offset) fail(11, "a region does not end in front of its limit");
        if (i + 1 < r.size() && r[i].offset + r[i].bytes > r[i + 1].offset) fail(12, "two regions overlap or do not ascend");
    }
}

std::unique_ptr<uint8_t[]> exact(size_t bytes) // a heap buffer of exactly `bytes`, so that ASan sees an overrun
{
    std::unique_ptr<uint8_t[]> p(new uint8_t[bytes]);
    std::memset(p.get(), 0xA5, bytes);
    return p;
}

/// One direction's table at `t`. `reversed`: the coordinates are in stored order (kResizeMirrorStore). `lo` .. `hi`: the
/// samples a tap may read, relative to the rectangle.
void check_table(const int* t, const jg::ResizeAxis& a, int out, int taps, bool reversed, int lo, int hi)
{
    for (int e = 0; e < out; ++e) {
        const int64_t c = static_cast<int64_t>(a.x0) + (reversed ? out - 1 - e : e); // the coordinate in the resized image
        const int first = t[2 * e], count = t[2 * e + 1];
        const bool inside = c >= 0 && c < a.resized;
        if (inside ? count < 1 : count != 0) fail(30, "a coordinate inside the resized image has no tap, or one outside it has");
        if (count > taps) fail(31, "a row has more taps than its stride");
        if (first < 0 || first > a.extent || count > a.extent - first) fail(32, "a row's taps leave the rectangle");
        if (count > 0 && (first < lo || first + count > hi)) fail(33, "a row's taps leave the samples it may read");
        const int* w = t + 2 * static_cast<size_t>(out) + static_cast<size_t>(e) * taps;
        for (int k = count; k < taps; ++k)
            if (w[k] != 0) fail(34, "a weight behind a row's count is not zero");
    }
}

/// A planned resize call: layout, fill, descriptors, tables, tiles, determinism. `again`: the plan of the same arguments
/// made a second time. `boxes`: a thumbnail call's.
void check_resize(const jg::ResizePlan& p, const jg::ResizePlan& again, const unsigned char* flips, uint8_t* base, const float* boxes)
{
    const size_t n = p.jobs.size();
    std::vector<Region> staged = {{0, sizeof(jg::ResizeJob) * n, 256}, {p.off_first, sizeof(int) * n, 256}};
    if (!p.first_tile_t.empty()) staged.push_back({p.off_first_t, sizeof(int) * n, 256});
    std::vector<Region> rows;
    for (size_t i = 0; i < n; ++i) {
        staged.push_back({p.off_tab_x[i], sizeof(int) * p.out_w * (2 + static_cast<size_t>(p.jobs[i].taps_x)), 16});
        staged.push_back({p.off_tab_y[i], sizeof(int) * p.out_h * (2 + static_cast<size_t>(p.jobs[i].taps_y)), 16});
        rows.push_back({p.off_mid[i], static_cast<size_t>(p.jobs[i].rows) * p.jobs[i].mid_pitch, 16}); // the first follows the tables
    }
    check_regions(staged, p.head);
    if (p.head > p.total || rows.front().offset < p.head) fail(13, "the staged part does not end in front of the rest");
    check_regions(rows, p.total - 256); // the last 256 bytes are the room to align the caller's pointer

    const auto h = exact(p.head), h2 = exact(p.head);
    if (jg::fill_resize(p, flips, base, h.get()) != JPEGGPU_SUCCESS || jg::fill_resize(again, flips, base, h2.get()) != JPEGGPU_SUCCESS)
        fail(14, "the fill failed");
    if (std::memcmp(h.get(), h2.get(), p.head) != 0) fail(15, "planning and filling twice gives other bytes");

    int64_t tiles = 0, tiles_t = 0;
    for (size_t i = 0; i < n; ++i) {
        jg::ResizeJob j;
        std::memcpy(&j, h.get() + sizeof j * i, sizeof j);
        if (reinterpret_cast<const uint8_t*>(j.tab_x) != base + p.off_tab_x[i] || reinterpret_cast<const uint8_t*>(j.tab_y) != base + p.off_tab_y[i] ||
            j.mid != base + p.off_mid[i])
            fail(20, "a descriptor does not point at its regions");
        const int o = p.orient[i];
        const bool store = !jg::orient_transposes(o) && jg::orient_mirrors_x(o);
        if (j.pad_ != ((store ? jg::kResizeMirrorStore : 0) | (flips && flips[i] ? jg::kResizeFlipOutput : 0))) fail(21, "a descriptor's flags");
        if (j.mid_pitch % 16 || j.mid_pitch < 3 * p.out_w) fail(22, "the pitch of the first pass's rows");
        const jg::ResizeAxis &ax = p.ax[i], &ay = p.ay[i];
        if (j.rows < 1 || j.row0 < 0 || j.rows > ay.extent - j.row0) fail(23, "the rows of the first pass leave the rectangle");
        const int box_x = boxes ? static_cast<int>(std::ceil(boxes[2 * i])) : ax.extent, box_y = boxes ? static_cast<int>(std::ceil(boxes[2 * i + 1])) : ay.extent;
        if (box_x > ax.extent || box_y > ay.extent) fail(24, "a box is larger than its image");
        check_table(reinterpret_cast<const int*>(h.get() + p.off_tab_x[i]), ax, p.out_w, j.taps_x, store, 0, box_x);
        check_table(reinterpret_cast<const int*>(h.get() + p.off_tab_y[i]), ay, p.out_h, j.taps_y, false, j.row0, std::min(j.row0 + j.rows, box_y));
        int first = 0, first_t = 0;
        std::memcpy(&first, h.get() + p.off_first + sizeof(int) * i, sizeof first);
        if (!p.first_tile_t.empty()) std::memcpy(&first_t, h.get() + p.off_first_t + sizeof(int) * i, sizeof first_t);
        if (first != tiles || (!p.first_tile_t.empty() && first_t != tiles_t)) fail(40, "an item's first tile is not the sum of those before it");
        (jg::orient_transposes(o) ? tiles_t : tiles) += jg::orient_transposes(o) ? jg::resize_t_tiles(j.rows, p.out_w) : jg::resize_h_tiles(j.rows, p.out_w);
    }
    if (p.h_tiles != tiles || p.t_tiles != tiles_t) fail(41, "the tile counts are not the sums of the items' tiles");
}

// ---- the sweep: tables through the exported functions ------------------------------------------------

void table_case(int in, double extent, int resized, int x0, int n_out, int filter, int kind)
{
    begin("table %d (%.2f) -> %d, x0 %d, %d coordinates, filter %d, function %d", in, extent, resized, x0, n_out, filter, kind);
    const int taps = jg::resize_max_taps(extent, resized, filter);
    std::unique_ptr<int[]> t(new int[static_cast<size_t>(n_out) * (2 + static_cast<size_t>(taps))]); // {first, count} interleaved, as check_table reads
    std::unique_ptr<int[]> first(new int[n_out]), count(new int[n_out]);
    int* w = t.get() + 2 * static_cast<size_t>(n_out);
    const auto f = static_cast<jpeggpu_ext_filter>(filter);
    const int st = kind == 0   ? jpeggpu_ext_resize_weights(in, resized, f, first.get(), count.get(), w, taps)
                   : kind == 1 ? jpeggpu_ext_resize_box_weights(in, static_cast<float>(extent), resized, f, first.get(), count.get(), w, taps)
                               : jpeggpu_ext_resize_view_weights(in, resized, x0, n_out, 0, f, first.get(), count.get(), w, taps);
    if (!ended(kTables, st, JPEGGPU_SUCCESS)) return;
    for (int e = 0; e < n_out; ++e) {
        t[2 * e]     = first[e];
        t[2 * e + 1] = count[e];
    }
    const jg::ResizeAxis a{in, resized, x0, 0, in, extent};
    check_table(t.get(), a, n_out, taps, false, 0, static_cast<int>(std::ceil(extent)));
}

void sweep_tables()
{
    for (const Pair& p : pairs())
        for (int filter = 0; filter < 2; ++filter) {
            table_case(p.in, p.in, p.out, 0, p.out, filter, 0);
            table_case(p.in, p.in, p.out, 0, p.out, filter, 1);
            if (p.in >= 2) table_case(p.in, p.in - 0.5, p.out, 0, p.out, filter, 1); // a box that ends inside a sample
            table_case(p.in, p.in, p.out, -1, std::min(p.out, 64) + 2, filter, 2);       // padding on both sides
            table_case(p.in, p.in, p.out, p.out / 2, 1, filter, 2);
        }
}

// ---- the sweep: resize plans --------------------------------------------------------------------------

struct ResizeCall {
    std::deque<Source> sources;
    std::vector<jpeggpu_ext_resize_item> items;
    std::vector<jpeggpu_ext_color_space> colors;
    std::vector<int> orients;
    std::vector<jpeggpu_ext_resize_view> views;
    std::vector<unsigned char> flips;
    void add(const Source& s, const Model& m, int orientation)
    {
        sources.push_back(s);
        colors.push_back(m.color);
        orients.push_back(orientation);
    }
    /// Plans the call (twice), expects `want`, and checks the plan.
    void run(int out_w, int out_h, int filter, bool with_flips, int want)
    {
        const int n = static_cast<int>(sources.size());
        items.clear();
        for (const Source& s : sources) items.push_back(s.item());
        flips.assign(n, 0);
        for (int i = 0; i < n; ++i) flips[i] = (i + out_w) & 1;
        jg::ResizePlan p, again;
        const jpeggpu_ext_resize_view* v = views.empty() ? nullptr : views.data();
        const int st = jg::plan_resize(items.data(), colors.data(), orients.data(), v, n, out_w, out_h, filter, p);
        if (!ended(kResizePlans, st, want)) return;
        if (jg::plan_resize(items.data(), colors.data(), orients.data(), v, n, out_w, out_h, filter, again) != JPEGGPU_SUCCESS) fail(16, "the second plan failed");
        if (p.head != again.head || p.total != again.total) fail(15, "planning twice gives another layout");
        size_t size = 0; // what the exported size function says is the plan's total
        if (v) size = jpeggpu_ext_resize_view_scratch_size(items.data(), colors.data(), orients.data(), v, n, out_w, out_h, static_cast<jpeggpu_ext_filter>(filter));
        else size = jpeggpu_ext_resize_scratch_size_oriented(items.data(), colors.data(), orients.data(), n, out_w, out_h, static_cast<jpeggpu_ext_filter>(filter));
        if (size != p.total) fail(17, "the scratch size is not the plan's total");
        check_resize(p, again, with_flips ? flips.data() : nullptr, kBase, nullptr);
    }
};

/// The stored size of an image that `orientation` displays as w x h.
void stored(int orientation, int w, int h, int* sw, int* sh)
{
    *sw = jg::orient_transposes(orientation) ? h : w;
    *sh = jg::orient_transposes(orientation) ? w : h;
}

void sweep_resize()
{
    const std::vector<Pair> P = pairs();
    const int np = static_cast<int>(P.size());
    int k = 0;
    // every pair along x, with every filter and orientation; the pair along y, the model and n in turn
    for (int pi = 0; pi < np; ++pi)
        for (int filter = 0; filter < 2; ++filter)
            for (int o = 1; o <= 8; ++o, ++k) {
                const Pair px = P[pi], py = P[(pi * 7 + k) % np];
                const int n = k % 3 == 0 ? 1 : k % 3 == 1 || px.out > 224 || py.out > 224 ? 2 : 65;
                begin("resize %d x %d -> %d x %d, filter %d, orientation %d, n %d", px.in, py.in, px.out, py.out, filter, o, n);
                ResizeCall call;
                for (int j = 0; j < n; ++j) { // the other items: small sizes, the orientations and models in turn
                    const int oj = (o - 1 + j) % 8 + 1, w = j ? kLen[(pi + j) % 9] : px.in, h = j ? kLen[(k + j) % 9] : py.in;
                    int sw = 0, sh = 0;
                    stored(oj, w, h, &sw, &sh);
                    const Model& m = kModels[(k + j) % kNumModels];
                    call.add(make_source(m, sw, sh), m, oj);
                }
                call.run(px.out, py.out, filter, k & 1, JPEGGPU_SUCCESS);
            }
    // crop rectangles: every length, every kind of rectangle, every orientation
    for (int li = 0; li < kNumLen; ++li)
        for (int kind = 0; kind < 5; ++kind)
            for (int o = 1; o <= 8; ++o, ++k) {
                const int w = kLen[li], h = kLen[(li + kind + 3) % kNumLen], n = 1 + k % 2;
                const int out_w = kOut[k % 4], out_h = kOut[(k / 4) % 4], filter = k % 2;
                begin("resize of a rectangle of kind %d of %d x %d stored -> %d x %d, filter %d, orientation %d, n %d", kind, w, h, out_w, out_h, filter, o, n);
                ResizeCall call;
                for (int j = 0; j < n; ++j) {
                    int rect[4];
                    axis_rect(w, (kind + j) % 5, &rect[0], &rect[2]);
                    axis_rect(h, (kind + j) % 5, &rect[1], &rect[3]);
                    const Model& m = kModels[(k + j) % kNumModels];
                    call.add(make_source(m, w, h, rect), m, (o - 1 + j) % 8 + 1);
                }
                call.run(out_w, out_h, filter, k & 1, JPEGGPU_SUCCESS);
            }
    // views: a window inside the resized image, one larger than it (padding on each side), a 1 x 1 window; of a whole
    // image, and of the rectangle that jpeggpu_ext_resize_view_rect says the window reads
    for (int li = 0; li < kNumLen; ++li)
        for (int kind = 0; kind < 3; ++kind)
            for (int o = 1; o <= 8; ++o)
                for (int filter = 0; filter < 2; ++filter, ++k) {
                    const int w = kLen[li], h = kLen[(li + 3 + o) % kNumLen]; // displayed
                    const int rw = kOut[k % kNumOut], rh = kOut[(k / 2 + kind) % kNumOut], n = k % 3 == 2 && rw <= 224 && rh <= 224 ? 65 : 1 + k % 2;
                    const jpeggpu_ext_resize_view view = kind == 0   ? jpeggpu_ext_resize_view{rw, rh, rw > 2, rh > 2, k & 1}
                                                         : kind == 1 ? jpeggpu_ext_resize_view{rw, rh, -1, -1, k & 1}
                                                                     : jpeggpu_ext_resize_view{rw, rh, rw / 2, rh / 2, k & 1};
                    const int out_w = kind == 0 ? std::max(rw - 2, 1) : kind == 1 ? rw + 2 : 1;
                    const int out_h = kind == 0 ? std::max(rh - 2, 1) : kind == 1 ? rh + 2 : 1;
                    const bool cropped = (k / 3) & 1;
                    begin("view %d of %d x %d displayed resized to %d x %d, window %d x %d, filter %d, orientation %d, n %d, cropped %d", kind, w, h, rw, rh,
                          out_w, out_h, filter, o, n, cropped);
                    ResizeCall call;
                    for (int j = 0; j < n; ++j) {
                        const int oj = (o - 1 + j) % 8 + 1, wj = j ? kLen[(li + j) % 9] : w, hj = j ? kLen[(k + j) % 9] : h;
                        int sw = 0, sh = 0, rect[4];
                        stored(oj, wj, hj, &sw, &sh);
                        if (cropped && jpeggpu_ext_resize_view_rect(sw, sh, oj, &view, out_w, out_h, static_cast<jpeggpu_ext_filter>(filter), &rect[0], &rect[1], &rect[2],
                                                                    &rect[3]) != JPEGGPU_SUCCESS)
                            fail(18, "jpeggpu_ext_resize_view_rect refused a window that overlaps the resized image");
                        const Model& m = kModels[(k + j) % kNumModels];
                        call.add(make_source(m, sw, sh, cropped ? rect : nullptr), m, oj);
                        call.views.push_back(view);
                    }
                    call.run(out_w, out_h, filter, k & 1, JPEGGPU_SUCCESS);
                }
    // refusals
    const auto refuse = [&](const char* what, int want, const Model& m, int w, int h, int o, int out_w, int out_h, int filter, const jpeggpu_ext_resize_view* view,
                            int damage) {
        begin("resize refusal: %s", what);
        ResizeCall call;
        call.add(make_source(kModels[4], 64, 48), kModels[4], 1);
        call.add(make_source(m, w, h), m, o);
        if (damage == 1) call.sources[1].img.image[m.nc - 1] = nullptr;
        if (damage == 2) call.sources[1].info.sizes_x[0] = 0;
        if (damage == 3) call.sources[1].info.subsampling.x[1] = 3; // 4 : 3 is no integral ratio
        if (damage == 4) call.colors[1] = JPEGGPU_EXT_COLOR_YCBCR;     // for four components
        if (view) call.views.assign(2, *view);
        call.run(out_w, out_h, filter, false, want);
    };
    const jpeggpu_ext_resize_view beside{32, 24, 32, 0, 0}, empty{0, 24, 0, 0, 0};
    refuse("an output width of 0", JPEGGPU_INVALID_ARGUMENT, kModels[1], 8, 8, 1, 0, 8, 0, nullptr, 0);
    refuse("an output height below 0", JPEGGPU_INVALID_ARGUMENT, kModels[1], 8, 8, 1, 8, -1, 0, nullptr, 0);
    refuse("a filter that is not offered", JPEGGPU_NOT_SUPPORTED, kModels[1], 8, 8, 1, 8, 8, 2, nullptr, 0);
    refuse("orientation 0", JPEGGPU_INVALID_ARGUMENT, kModels[1], 8, 8, 0, 8, 8, 0, nullptr, 0);
    refuse("orientation 9", JPEGGPU_INVALID_ARGUMENT, kModels[1], 8, 8, 9, 8, 8, 0, nullptr, 0);
    refuse("a plane without an address", JPEGGPU_INVALID_ARGUMENT, kModels[4], 8, 8, 1, 8, 8, 0, nullptr, 1);
    refuse("a plane without samples", JPEGGPU_INVALID_ARGUMENT, kModels[4], 8, 8, 1, 8, 8, 0, nullptr, 2);
    refuse("factors without an integral ratio", JPEGGPU_NOT_SUPPORTED, kModels[5], 8, 8, 1, 8, 8, 0, nullptr, 3);
    refuse("a colour model of another component count", JPEGGPU_NOT_SUPPORTED, kModels[6], 8, 8, 1, 8, 8, 0, nullptr, 4);
    refuse("a window beside the resized image", JPEGGPU_INVALID_ARGUMENT, kModels[1], 8, 8, 1, 8, 8, 0, &beside, 0);
    refuse("a view resized to nothing", JPEGGPU_INVALID_ARGUMENT, kModels[1], 8, 8, 1, 8, 8, 0, &empty, 0);
    {
        const Source s = make_source(kModels[1], 8, 8);
        std::vector<jpeggpu_ext_resize_item> items(65536, s.item());
        jg::ResizePlan p;
        begin("resize refusal: no items");
        ended(kResizePlans, jg::plan_resize(nullptr, nullptr, nullptr, nullptr, 1, 8, 8, 0, p), JPEGGPU_INVALID_ARGUMENT);
        begin("resize refusal: n 0");
        ended(kResizePlans, jg::plan_resize(items.data(), nullptr, nullptr, nullptr, 0, 8, 8, 0, p), JPEGGPU_INVALID_ARGUMENT);
        begin("resize refusal: n 65536");
        ended(kResizePlans, jg::plan_resize(items.data(), nullptr, nullptr, nullptr, 65536, 8, 8, 0, p), JPEGGPU_INVALID_ARGUMENT);
        const Source four = make_source(kModels[6], 8, 8); // four components and no model to read them by
        items[1] = four.item();
        begin("resize refusal: four components by their count");
        ended(kResizePlans, jg::plan_resize(items.data(), nullptr, nullptr, nullptr, 2, 8, 8, 0, p), JPEGGPU_NOT_SUPPORTED);
    }
}

// ---- the sweep: RGB batch plans --------------------------------------------------------------------------

void rgb_case(int n, int layout, int w, int h, int o, int kind, int k, int damage, int want)
{
    std::deque<Source> sources;
    std::vector<jpeggpu_ext_rgb_item> items(static_cast<size_t>(std::max(n, 1)));
    for (int j = 0; j < std::min(n, 16); ++j) { // more items than that share their sources
        int rect[4];
        axis_rect(w, (kind + j) % 5, &rect[0], &rect[2]);
        axis_rect(h, (kind + j) % 5, &rect[1], &rect[3]);
        sources.push_back(make_source(kModels[(k + j) % kNumModels], w, h, (kind + j) % 5 ? rect : nullptr));
    }
    for (int j = 0; j < n && j < static_cast<int>(items.size()); ++j) {
        const Source& s = sources[j % 16];
        const int oj = (o - 1 + j) % 8 + 1;
        const int rw = s.cropped ? s.crop.width : w, rh = s.cropped ? s.crop.height : h;
        const int ow = jg::orient_transposes(oj) ? rh : rw, oh = jg::orient_transposes(oj) ? rw : rh;
        jpeggpu_ext_rgb_item& it = items[j];
        it              = jpeggpu_ext_rgb_item{&s.info, s.cropped ? &s.crop : nullptr, &s.img, kModels[(k + j % 16) % kNumModels].color, oj, j & 1, kDst + (static_cast<size_t>(j) << 36),
                                  layout == JPEGGPU_EXT_HWC ? 3 * ow : ow, static_cast<size_t>(ow) * oh};
    }
    if (damage == 1) items[n - 1].dst = nullptr;
    if (damage == 2) items[n - 1].orientation = 9;
    if (damage == 3) items[n - 1].dst_pitch -= 1;
    if (damage == 4) items[n - 1].plane_stride -= 1;
    if (damage == 5) items[n - 1].color = JPEGGPU_EXT_COLOR_UNKNOWN;
    jg::RgbBatchPlan p, again;
    const int st = jg::plan_rgb_batch(damage == 6 ? nullptr : items.data(), n, layout, p);
    if (!ended(kRgbPlans, st, want)) return;
    if (jg::plan_rgb_batch(items.data(), n, layout, again) != JPEGGPU_SUCCESS) fail(16, "the second plan failed");
    const size_t un = static_cast<size_t>(n);
    check_regions({{0, sizeof(jg::RgbJob) * un, 256}, {p.at.off_first, sizeof(int) * un, 256}, {p.at.off_first_t, sizeof(int) * un, 256}}, p.at.total);
    if (jpeggpu_ext_batch_rgb_scratch_size(n) != p.at.total + 256) fail(17, "the scratch size is not the layout's total and the room to align");
    const auto b = exact(p.at.total), b2 = exact(p.at.total);
    jg::fill_rgb_batch(p, b.get());
    jg::fill_rgb_batch(again, b2.get());
    int64_t tiles = 0, tiles_t = 0;
    for (size_t i = 0; i < un; ++i) {
        jg::RgbJob j, j2;
        std::memcpy(&j, b.get() + sizeof j * i, sizeof j);
        std::memcpy(&j2, b2.get() + sizeof j * i, sizeof j);
        // (field by field: the record has padding that nothing writes)
        if (std::memcmp(&j.src, &j2.src, sizeof j.src) != 0 || j.dst != j2.dst || j.dst_pitch != j2.dst_pitch || j.plane_stride != j2.plane_stride ||
            j.width != j2.width || j.height != j2.height || j.flips != j2.flips || j.tiles_x != j2.tiles_x)
            fail(15, "planning and filling twice gives another descriptor");
        if (j.dst != items[i].dst || j.width < 1 || j.height < 1) fail(20, "a descriptor's destination or size");
        const bool tr = jg::orient_transposes(items[i].orientation);
        int first = 0, first_t = 0;
        std::memcpy(&first, b.get() + p.at.off_first + sizeof(int) * i, sizeof first);
        std::memcpy(&first_t, b.get() + p.at.off_first_t + sizeof(int) * i, sizeof first_t);
        if (first != tiles || first_t != tiles_t || j.tiles_x != jg::rgb_batch_tiles_x(j.width, tr)) fail(40, "an item's first tile is not the sum of those before it");
        (tr ? tiles_t : tiles) += jg::rgb_batch_tiles(j.width, j.height, tr);
    }
    if (std::memcmp(b.get() + p.at.off_first, b2.get() + p.at.off_first, sizeof(int) * un) != 0 ||
        std::memcmp(b.get() + p.at.off_first_t, b2.get() + p.at.off_first_t, sizeof(int) * un) != 0)
        fail(15, "planning and filling twice gives other tile lists");
    if (p.row_tiles != tiles || p.t_tiles != tiles_t) fail(41, "the tile counts are not the sums of the items' tiles");
}

void sweep_rgb()
{
    int k = 0;
    for (int li = 0; li < kNumLen; ++li)
        for (int o = 1; o <= 8; ++o)
            for (int layout = 0; layout < 2; ++layout, ++k) {
                const int n = k % 3 == 0 ? 1 : k % 3 == 1 ? 2 : 65, w = kLen[li], h = kLen[(li + o) % kNumLen];
                begin("rgb batch of %d x %d stored, layout %d, orientation %d, n %d", w, h, layout, o, n);
                rgb_case(n, layout, w, h, o, k % 5, k, 0, JPEGGPU_SUCCESS);
            }
    for (int layout = 0; layout < 2; ++layout) {
        begin("rgb batch at the limit, n 65535, layout %d", layout);
        rgb_case(65535, layout, 257, 9, 1, 0, layout, 0, JPEGGPU_SUCCESS);
        begin("rgb batch refusal: n 65536, layout %d", layout);
        rgb_case(65536, layout, 257, 9, 1, 0, layout, 0, JPEGGPU_INVALID_ARGUMENT);
    }
    const struct {
        const char* what;
        int n, layout, damage, want;
    } bad[] = {{"n 0", 0, 0, 0, JPEGGPU_INVALID_ARGUMENT},          {"a layout that is not offered", 2, 2, 0, JPEGGPU_INVALID_ARGUMENT},
               {"no destination", 2, 0, 1, JPEGGPU_INVALID_ARGUMENT}, {"orientation 9", 2, 0, 2, JPEGGPU_INVALID_ARGUMENT},
               {"a pitch one short, HWC", 2, 0, 3, JPEGGPU_INVALID_ARGUMENT}, {"a pitch one short, CHW", 2, 1, 3, JPEGGPU_INVALID_ARGUMENT},
               {"a plane stride one short", 2, 1, 4, JPEGGPU_INVALID_ARGUMENT}, {"no colour model", 2, 0, 5, JPEGGPU_NOT_SUPPORTED},
               {"no items", 2, 0, 6, JPEGGPU_INVALID_ARGUMENT}};
    for (const auto& b : bad) {
        begin("rgb batch refusal: %s", b.what);
        rgb_case(b.n, b.layout, 9, 7, 5, 0, 1, b.damage, b.want);
    }
}

// ---- the sweep: thumbnails ----------------------------------------------------------------------------------

/// A planned thumbnail call: the reduction's layout, fill, descriptors and tiles, then the resize's.
void check_thumbnails(const jg::ThumbnailPlan& t, const jg::ThumbnailPlan& again)
{
    const size_t nr = t.jobs.size();
    check_regions({{0, sizeof(jg::ReduceJob) * nr, 256}, {t.off_first, sizeof(int) * nr, 256}}, t.head);
    if (t.head > t.off_resize || t.off_resize % 256 || t.total != t.off_resize + t.resize.total + 256) fail(13, "the resize's part of the scratch");
    const auto h = exact(t.head), h2 = exact(t.head);
    if ((t.tiles > 0) != (nr > 0)) fail(41, "items reduce and have no tiles, or the other way round");
    if (t.tiles > 0) { // as jpeggpu_ext_thumbnail_to_rgb: without a reduction there is nothing to stage
        jg::fill_thumbnails(t, h.get());
        jg::fill_thumbnails(again, h2.get());
    }
    std::vector<Region> planes;
    int64_t tiles = 0;
    for (size_t r = 0; r < nr; ++r) {
        jg::ReduceJob j, j2;
        std::memcpy(&j, h.get() + sizeof j * r, sizeof j);
        std::memcpy(&j2, h2.get() + sizeof j * r, sizeof j);
        if (std::memcmp(&j.src, &j2.src, sizeof j.src) != 0 || j.dst != j2.dst || j.pitch != j2.pitch || j.plane_stride != j2.plane_stride ||
            std::memcmp(j.mult, j2.mult, sizeof j.mult) != 0 || j.rows_per_tile != j2.rows_per_tile || j.tiles_x != j2.tiles_x)
            fail(15, "planning and filling twice gives another descriptor");
        if (j.red_w != (j.width + j.fx - 1) / j.fx || j.red_h != (j.height + j.fy - 1) / j.fy || j.pitch < j.red_w || j.plane_stride < static_cast<size_t>(j.pitch) * j.red_h)
            fail(25, "a reduced plane does not hold its image");
        planes.push_back({static_cast<size_t>(j.dst - kBase), (j.src.ncomp == 1 ? 1 : 3) * j.plane_stride, 256});
        int first = 0;
        std::memcpy(&first, h.get() + t.off_first + sizeof(int) * r, sizeof first);
        if (first != tiles || j.tiles_x != jg::reduce_tiles_x(j.red_w) || j.rows_per_tile != jg::reduce_rows_per_tile(j.fy))
            fail(40, "an item's first tile is not the sum of those before it");
        tiles += jg::reduce_tiles(j.red_w, j.red_h, j.fy);
    }
    if (!planes.empty() && planes.front().offset < t.head) fail(13, "a reduced plane lies in the staged part");
    check_regions(planes, t.off_resize);
    if (t.tiles != tiles) fail(41, "the tile count is not the sum of the items' tiles");
    check_resize(t.resize, again.resize, nullptr, kBase + t.off_resize, t.boxes.data());
}

const double kGaps[] = {0.0, 1.0, 2.0, 65536.0}; // 0: no reducing_gap

void sweep_thumbnails()
{
    int k = 0;
    for (int wi = 0; wi < kNumLen; ++wi)
        for (int hi = 0; hi < kNumLen; ++hi)
            for (int rq = 0; rq < 5; ++rq, ++k) {
                const int w = kLen[wi], h = kLen[hi], filter = k % 2;
                const int req[5][2] = {{1, 1}, {w, h}, {w + 1, h + 1}, {std::max(w / 2, 1), std::max(h / 3, 1)}, {224, 224}};
                const int rw = req[rq][0], rh = req[rq][1];
                const bool noop = rw >= w && rh >= h, tall = h > 100 && h > w;
                std::vector<jpeggpu_ext_thumbnail> plans;
                for (double gap : kGaps) {
                    // What the call must return, from its contract alone. A request that holds the image, an image of at most 100
                    // rows (the reduced one then has no more, and a column at least) and one that is not taller than wide are never
                    // "resized vertically first". For a taller one, every request here is at least as wide for its height as the
                    // image, so the thumbnail's height is the request's, and without a gap nothing is reduced: the image itself is
                    // what is resized, refused if it is more than 100 times taller than wide and the thumbnail less tall. With a
                    // gap the reduced size of a tall image takes Pillow's whole arithmetic to tell: not enumerated.
                    if (tall && !noop && gap != 0.0) continue;
                    const int want = tall && !noop && h > 100 * static_cast<int64_t>(w) && rh < h ? JPEGGPU_NOT_SUPPORTED : JPEGGPU_SUCCESS;
                    begin("thumbnail of %d x %d for %d x %d, filter %d, gap %g", w, h, rw, rh, filter, gap);
                    jpeggpu_ext_thumbnail pl{};
                    if (!ended(kThumbSizes, jpeggpu_ext_thumbnail_plan(w, h, rw, rh, static_cast<jpeggpu_ext_filter>(filter), gap, &pl), want)) continue;
                    const bool reduces = pl.fx > 1 || pl.fy > 1;
                    if ((pl.scale != 1 && pl.scale != 2 && pl.scale != 4 && pl.scale != 8) || pl.dec_w != (w + pl.scale - 1) / pl.scale || pl.dec_h != (h + pl.scale - 1) / pl.scale ||
                        pl.fx < 1 || pl.fy < 1 || pl.red_w != (reduces ? (pl.dec_w + pl.fx - 1) / pl.fx : pl.dec_w) ||
                        pl.red_h != (reduces ? (pl.dec_h + pl.fy - 1) / pl.fy : pl.dec_h) || pl.out_w < 1 || pl.out_h < 1 || pl.out_w > std::max(rw, w) ||
                        pl.out_h > std::max(rh, h) || !(pl.box_w > 0.0f) || !(pl.box_h > 0.0f) || pl.box_w > pl.red_w || pl.box_h > pl.red_h ||
                        (noop && !pl.identity) || (pl.identity && (pl.out_w != pl.dec_w || pl.out_h != pl.dec_h || reduces)))
                        fail(50, "the steps of a thumbnail do not fit each other");
                    pl.replicate = k & 1;
                    plans.push_back(pl);
                }
                if (plans.empty()) continue;
                // the call of these plans' items: n = 1, 2 or 65 (the plans in turn), the models in turn
                const int n = k % 3 == 0 ? 1 : k % 3 == 1 || w > 257 || h > 257 ? 2 : 65;
                std::deque<Source> sources;
                std::vector<jpeggpu_ext_resize_item> items;
                std::vector<jpeggpu_ext_color_space> colors;
                std::vector<jpeggpu_ext_thumbnail> call;
                int canvas_w = 1, canvas_h = 1, want = JPEGGPU_SUCCESS;
                for (int j = 0; j < n; ++j) {
                    const jpeggpu_ext_thumbnail& pl = plans[j % plans.size()];
                    const Model& m = kModels[(k + j) % kNumThumbModels];
                    sources.push_back(make_source(m, pl.dec_w, pl.dec_h));
                    colors.push_back(m.color);
                    call.push_back(pl);
                    canvas_w = std::max(canvas_w, pl.out_w);
                    canvas_h = std::max(canvas_h, pl.out_h);
                    if (static_cast<int64_t>(pl.fx) * pl.fy > (1 << 23)) want = JPEGGPU_NOT_SUPPORTED; // a box's sum must fit 32 bits (jpeggpu_ext.h)
                }
                for (const Source& s : sources) items.push_back(s.item());
                begin("thumbnails of %d x %d for %d x %d, filter %d, n %d", w, h, rw, rh, filter, n);
                jg::ThumbnailPlan t, again;
                if (!ended(kThumbPlans, jg::plan_thumbnails(items.data(), colors.data(), call.data(), n, canvas_w, canvas_h, filter, kBase, t), want)) continue;
                if (jg::plan_thumbnails(items.data(), colors.data(), call.data(), n, canvas_w, canvas_h, filter, kBase, again) != JPEGGPU_SUCCESS) fail(16, "the second plan failed");
                if (jpeggpu_ext_thumbnail_scratch_size(items.data(), colors.data(), call.data(), n, canvas_w, canvas_h, static_cast<jpeggpu_ext_filter>(filter)) != t.total)
                    fail(17, "the scratch size is not the plan's total");
                check_thumbnails(t, again);
            }
    // refusals of the size rule
    jpeggpu_ext_thumbnail pl{};
    const struct {
        const char* what;
        int w, h, rw, rh, filter;
        double gap;
        bool no_plan;
        int want;
    } bad[] = {{"1 x 65535, resized vertically first", 1, 65535, 1, 1, 1, 0.0, false, JPEGGPU_NOT_SUPPORTED},
               {"a gap that is no number", 64, 48, 8, 8, 1, std::nan(""), false, JPEGGPU_INVALID_ARGUMENT},
               {"a gap of 0.5", 64, 48, 8, 8, 1, 0.5, false, JPEGGPU_INVALID_ARGUMENT},
               {"a gap above 65536", 64, 48, 8, 8, 1, 65537.0, false, JPEGGPU_INVALID_ARGUMENT},
               {"a width of 65536", 65536, 48, 8, 8, 1, 2.0, false, JPEGGPU_INVALID_ARGUMENT},
               {"a height of 65536", 64, 65536, 8, 8, 1, 2.0, false, JPEGGPU_INVALID_ARGUMENT},
               {"a width of 0", 0, 48, 8, 8, 1, 2.0, false, JPEGGPU_INVALID_ARGUMENT},
               {"a height below 0", 64, -1, 8, 8, 1, 2.0, false, JPEGGPU_INVALID_ARGUMENT},
               {"a request 0 wide", 64, 48, 0, 8, 1, 2.0, false, JPEGGPU_INVALID_ARGUMENT},
               {"a request 0 high", 64, 48, 8, 0, 1, 2.0, false, JPEGGPU_INVALID_ARGUMENT},
               {"a filter that is not offered", 64, 48, 8, 8, 2, 2.0, false, JPEGGPU_NOT_SUPPORTED},
               {"no plan to write", 64, 48, 8, 8, 1, 2.0, true, JPEGGPU_INVALID_ARGUMENT}};
    for (const auto& b : bad) {
        begin("thumbnail refusal: %s", b.what);
        ended(kBadArgs, jpeggpu_ext_thumbnail_plan(b.w, b.h, b.rw, b.rh, static_cast<jpeggpu_ext_filter>(b.filter), b.gap, b.no_plan ? nullptr : &pl), b.want);
    }
    // refusals of the call: a plan that is not the item's, a crop, a four-component file, a canvas too small
    if (jpeggpu_ext_thumbnail_plan(80, 60, 10, 10, JPEGGPU_EXT_FILTER_BICUBIC, 2.0, &pl) != JPEGGPU_SUCCESS || pl.fx < 2) fail(51, "80 x 60 for 10 x 10 does not reduce");
    const Source s = make_source(kModels[4], pl.dec_w, pl.dec_h), four = make_source(kModels[6], pl.dec_w, pl.dec_h);
    const int rect[4] = {1, 1, 8, 8};
    const Source cropped = make_source(kModels[4], pl.dec_w, pl.dec_h, rect);
    const struct {
        const char* what;
        const Source* src;
        jpeggpu_ext_color_space color;
        int canvas_w, d_dec, d_red, n;
        int want;
    } calls[] = {{"a plan of another size", &s, JPEGGPU_EXT_COLOR_YCBCR, 10, 1, 0, 1, JPEGGPU_INVALID_ARGUMENT},
                 {"a reduced size that is not the factors'", &s, JPEGGPU_EXT_COLOR_YCBCR, 10, 0, 1, 1, JPEGGPU_INVALID_ARGUMENT},
                 {"a canvas narrower than the thumbnail", &s, JPEGGPU_EXT_COLOR_YCBCR, 9, 0, 0, 1, JPEGGPU_INVALID_ARGUMENT},
                 {"a cropped item", &cropped, JPEGGPU_EXT_COLOR_YCBCR, 10, 0, 0, 1, JPEGGPU_INVALID_ARGUMENT},
                 {"a CMYK file", &four, JPEGGPU_EXT_COLOR_CMYK, 10, 0, 0, 1, JPEGGPU_NOT_SUPPORTED},
                 {"n 0", &s, JPEGGPU_EXT_COLOR_YCBCR, 10, 0, 0, 0, JPEGGPU_INVALID_ARGUMENT},
                 {"n 65536", &s, JPEGGPU_EXT_COLOR_YCBCR, 10, 0, 0, 65536, JPEGGPU_INVALID_ARGUMENT}};
    for (const auto& c : calls) {
        begin("thumbnails refusal: %s", c.what);
        jpeggpu_ext_thumbnail p2 = pl;
        p2.dec_w += c.d_dec;
        p2.red_w += c.d_red;
        const jpeggpu_ext_resize_item item = c.src->item();
        jg::ThumbnailPlan t;
        ended(kThumbPlans, jg::plan_thumbnails(&item, &c.color, &p2, c.n, c.canvas_w, 10, JPEGGPU_EXT_FILTER_BICUBIC, kBase, t), c.want);
        if (jpeggpu_ext_thumbnail_scratch_size(&item, &c.color, &p2, c.n, c.canvas_w, 10, JPEGGPU_EXT_FILTER_BICUBIC) != 0) fail(17, "a refused call has a scratch size");
    }
    begin("thumbnails refusal: boxes of 8191 x 8191 pixels, whose sums do not fit 32 bits");
    if (jpeggpu_ext_thumbnail_plan(65535, 65535, 1, 1, JPEGGPU_EXT_FILTER_BICUBIC, 1.0, &pl) != JPEGGPU_SUCCESS || pl.fx != 8191 || pl.fy != 8191)
        fail(51, "65535 x 65535 for 1 x 1 at gap 1 is not 1/8 and factors of 8191");
    const Source big = make_source(kModels[0], pl.dec_w, pl.dec_h);
    const jpeggpu_ext_resize_item item = big.item();
    jg::ThumbnailPlan t;
    ended(kThumbPlans, jg::plan_thumbnails(&item, nullptr, &pl, 1, 1, 1, JPEGGPU_EXT_FILTER_BICUBIC, kBase, t), JPEGGPU_NOT_SUPPORTED);
}

// ---- the sweep: null pointers and non-positive sizes for the exported functions that launch nothing ----------

void sweep_bad_arguments()
{
    int a[4] = {0, 0, 4, 4}, first[8], count[8], w[8 * 9];
    const jpeggpu_ext_resize_view view{8, 8, 0, 0, 0};
    const auto F = JPEGGPU_EXT_FILTER_BICUBIC;
    const auto bad = [&](const char* what, int got, int want = JPEGGPU_INVALID_ARGUMENT) {
        begin("bad argument: %s", what);
        ended(kBadArgs, got, want);
    };
    bad("resize_weights, in 0", jpeggpu_ext_resize_weights(0, 4, F, first, count, w, 9));
    bad("resize_weights, out 0", jpeggpu_ext_resize_weights(8, 0, F, first, count, w, 9));
    bad("resize_weights, in below 0", jpeggpu_ext_resize_weights(-8, 4, F, first, count, w, 9));
    bad("resize_weights, no first", jpeggpu_ext_resize_weights(8, 4, F, nullptr, count, w, 9));
    bad("resize_weights, no count", jpeggpu_ext_resize_weights(8, 4, F, first, nullptr, w, 9));
    bad("resize_weights, no weights", jpeggpu_ext_resize_weights(8, 4, F, first, count, nullptr, 9));
    bad("resize_weights, a tap short", jpeggpu_ext_resize_weights(8, 4, F, first, count, w, 8));
    bad("resize_weights, filter", jpeggpu_ext_resize_weights(8, 4, static_cast<jpeggpu_ext_filter>(2), first, count, w, 9), JPEGGPU_NOT_SUPPORTED);
    bad("resize_box_weights, in 0", jpeggpu_ext_resize_box_weights(0, 7.5f, 4, F, first, count, w, 9));
    bad("resize_box_weights, out 0", jpeggpu_ext_resize_box_weights(8, 7.5f, 0, F, first, count, w, 9));
    bad("resize_box_weights, extent 0", jpeggpu_ext_resize_box_weights(8, 0.0f, 4, F, first, count, w, 9));
    bad("resize_box_weights, extent no number", jpeggpu_ext_resize_box_weights(8, std::nanf(""), 4, F, first, count, w, 9));
    bad("resize_box_weights, extent infinite", jpeggpu_ext_resize_box_weights(8, HUGE_VALF, 4, F, first, count, w, 9));
    bad("resize_box_weights, no first", jpeggpu_ext_resize_box_weights(8, 7.5f, 4, F, nullptr, count, w, 9));
    bad("resize_box_weights, no count", jpeggpu_ext_resize_box_weights(8, 7.5f, 4, F, first, nullptr, w, 9));
    bad("resize_box_weights, no weights", jpeggpu_ext_resize_box_weights(8, 7.5f, 4, F, first, count, nullptr, 9));
    bad("resize_box_weights, filter", jpeggpu_ext_resize_box_weights(8, 7.5f, 4, static_cast<jpeggpu_ext_filter>(-1), first, count, w, 9), JPEGGPU_NOT_SUPPORTED);
    bad("resize_view_weights, in 0", jpeggpu_ext_resize_view_weights(0, 4, 0, 4, 0, F, first, count, w, 9));
    bad("resize_view_weights, resized 0", jpeggpu_ext_resize_view_weights(8, 0, 0, 4, 0, F, first, count, w, 9));
    bad("resize_view_weights, no coordinates", jpeggpu_ext_resize_view_weights(8, 4, 0, 0, 0, F, first, count, w, 9));
    bad("resize_view_weights, no first", jpeggpu_ext_resize_view_weights(8, 4, 0, 4, 0, F, nullptr, count, w, 9));
    bad("resize_view_weights, no count", jpeggpu_ext_resize_view_weights(8, 4, 0, 4, 0, F, first, nullptr, w, 9));
    bad("resize_view_weights, no weights", jpeggpu_ext_resize_view_weights(8, 4, 0, 4, 0, F, first, count, nullptr, 9));
    bad("resize_view_weights, filter", jpeggpu_ext_resize_view_weights(8, 4, 0, 4, 0, static_cast<jpeggpu_ext_filter>(2), first, count, w, 9), JPEGGPU_NOT_SUPPORTED);
    bad("resize_view_rect, width 0", jpeggpu_ext_resize_view_rect(0, 8, 1, &view, 8, 8, F, &a[0], &a[1], &a[2], &a[3]));
    bad("resize_view_rect, height 0", jpeggpu_ext_resize_view_rect(8, 0, 1, &view, 8, 8, F, &a[0], &a[1], &a[2], &a[3]));
    bad("resize_view_rect, orientation 0", jpeggpu_ext_resize_view_rect(8, 8, 0, &view, 8, 8, F, &a[0], &a[1], &a[2], &a[3]));
    bad("resize_view_rect, no view", jpeggpu_ext_resize_view_rect(8, 8, 1, nullptr, 8, 8, F, &a[0], &a[1], &a[2], &a[3]));
    bad("resize_view_rect, out_w 0", jpeggpu_ext_resize_view_rect(8, 8, 1, &view, 0, 8, F, &a[0], &a[1], &a[2], &a[3]));
    bad("resize_view_rect, out_h 0", jpeggpu_ext_resize_view_rect(8, 8, 1, &view, 8, 0, F, &a[0], &a[1], &a[2], &a[3]));
    bad("resize_view_rect, no x", jpeggpu_ext_resize_view_rect(8, 8, 1, &view, 8, 8, F, nullptr, &a[1], &a[2], &a[3]));
    bad("resize_view_rect, no y", jpeggpu_ext_resize_view_rect(8, 8, 1, &view, 8, 8, F, &a[0], nullptr, &a[2], &a[3]));
    bad("resize_view_rect, no w", jpeggpu_ext_resize_view_rect(8, 8, 1, &view, 8, 8, F, &a[0], &a[1], nullptr, &a[3]));
    bad("resize_view_rect, no h", jpeggpu_ext_resize_view_rect(8, 8, 1, &view, 8, 8, F, &a[0], &a[1], &a[2], nullptr));
    bad("resize_view_rect, filter", jpeggpu_ext_resize_view_rect(8, 8, 1, &view, 8, 8, static_cast<jpeggpu_ext_filter>(2), &a[0], &a[1], &a[2], &a[3]), JPEGGPU_NOT_SUPPORTED);
    bad("orient_size, orientation 9", jpeggpu_ext_orient_size(9, 8, 8, &a[0], &a[1]));
    bad("orient_size, width 0", jpeggpu_ext_orient_size(1, 0, 8, &a[0], &a[1]));
    bad("orient_size, height 0", jpeggpu_ext_orient_size(1, 8, 0, &a[0], &a[1]));
    bad("orient_size, no out_w", jpeggpu_ext_orient_size(1, 8, 8, nullptr, &a[1]));
    bad("orient_size, no out_h", jpeggpu_ext_orient_size(1, 8, 8, &a[0], nullptr));
    int r[4] = {0, 0, 4, 4};
    bad("orient_rect, orientation 0", jpeggpu_ext_orient_rect(0, 8, 8, &r[0], &r[1], &r[2], &r[3]));
    bad("orient_rect, width 0", jpeggpu_ext_orient_rect(1, 0, 8, &r[0], &r[1], &r[2], &r[3]));
    bad("orient_rect, height 0", jpeggpu_ext_orient_rect(1, 8, 0, &r[0], &r[1], &r[2], &r[3]));
    bad("orient_rect, no x", jpeggpu_ext_orient_rect(1, 8, 8, nullptr, &r[1], &r[2], &r[3]));
    bad("orient_rect, no y", jpeggpu_ext_orient_rect(1, 8, 8, &r[0], nullptr, &r[2], &r[3]));
    bad("orient_rect, no rw", jpeggpu_ext_orient_rect(1, 8, 8, &r[0], &r[1], nullptr, &r[3]));
    bad("orient_rect, no rh", jpeggpu_ext_orient_rect(1, 8, 8, &r[0], &r[1], &r[2], nullptr));
    int wide[4] = {5, 0, 4, 4}, none[4] = {0, 0, 0, 4};
    bad("orient_rect, a rectangle past the edge", jpeggpu_ext_orient_rect(6, 8, 8, &wide[0], &wide[1], &wide[2], &wide[3]));
    bad("orient_rect, a rectangle 0 wide", jpeggpu_ext_orient_rect(1, 8, 8, &none[0], &none[1], &none[2], &none[3]));
    // the size functions say 0 for what their calls refuse
    const Source s = make_source(kModels[4], 64, 48);
    const jpeggpu_ext_resize_item item = s.item();
    const jpeggpu_ext_color_space color = JPEGGPU_EXT_COLOR_YCBCR;
    const int one = 1;
    const auto zero = [&](const char* what, size_t got) { bad(what, got == 0 ? JPEGGPU_INVALID_ARGUMENT : JPEGGPU_SUCCESS); };
    zero("resize_scratch_size, no items", jpeggpu_ext_resize_scratch_size(nullptr, 1, 8, 8, F));
    zero("resize_scratch_size, n 0", jpeggpu_ext_resize_scratch_size(&item, 0, 8, 8, F));
    zero("resize_scratch_size, out_w 0", jpeggpu_ext_resize_scratch_size(&item, 1, 0, 8, F));
    zero("resize_scratch_size, out_h 0", jpeggpu_ext_resize_scratch_size(&item, 1, 8, 0, F));
    zero("resize_scratch_size_cs, no colours", jpeggpu_ext_resize_scratch_size_cs(&item, nullptr, 1, 8, 8, F));
    zero("resize_scratch_size_cs, no items", jpeggpu_ext_resize_scratch_size_cs(nullptr, &color, 1, 8, 8, F));
    zero("resize_scratch_size_oriented, no orientations", jpeggpu_ext_resize_scratch_size_oriented(&item, &color, nullptr, 1, 8, 8, F));
    zero("resize_scratch_size_oriented, no colours", jpeggpu_ext_resize_scratch_size_oriented(&item, nullptr, &one, 1, 8, 8, F));
    zero("resize_scratch_size_oriented, n below 0", jpeggpu_ext_resize_scratch_size_oriented(&item, &color, &one, -1, 8, 8, F));
    zero("resize_view_scratch_size, no views", jpeggpu_ext_resize_view_scratch_size(&item, &color, &one, nullptr, 1, 8, 8, F));
    zero("resize_view_scratch_size, no items", jpeggpu_ext_resize_view_scratch_size(nullptr, &color, &one, &view, 1, 8, 8, F));
    zero("resize_view_scratch_size, out_w 0", jpeggpu_ext_resize_view_scratch_size(&item, &color, &one, &view, 1, 0, 8, F));
    zero("batch_rgb_scratch_size, n 0", jpeggpu_ext_batch_rgb_scratch_size(0));
    zero("batch_rgb_scratch_size, n below 0", jpeggpu_ext_batch_rgb_scratch_size(-1));
    zero("batch_rgb_scratch_size, n 65536", jpeggpu_ext_batch_rgb_scratch_size(65536));
    jpeggpu_ext_thumbnail pl{};
    if (jpeggpu_ext_thumbnail_plan(64, 48, 8, 8, F, 2.0, &pl) != JPEGGPU_SUCCESS) fail(51, "64 x 48 for 8 x 8 has no plan");
    zero("thumbnail_scratch_size, no items", jpeggpu_ext_thumbnail_scratch_size(nullptr, &color, &pl, 1, 8, 8, F));
    zero("thumbnail_scratch_size, no plans", jpeggpu_ext_thumbnail_scratch_size(&item, &color, nullptr, 1, 8, 8, F));
    zero("thumbnail_scratch_size, canvas_w 0", jpeggpu_ext_thumbnail_scratch_size(&item, &color, &pl, 1, 0, 8, F));
    zero("thumbnail_scratch_size, canvas_h 0", jpeggpu_ext_thumbnail_scratch_size(&item, &color, &pl, 1, 8, 0, F));
    // the tensor spec
    jpeggpu_ext_tensor_spec spec{JPEGGPU_EXT_TENSOR_F32, {0.5f, 0.5f, 0.5f}, {0.25f, 0.25f, 0.25f}, nullptr}, out{};
    bad("tensor_spec, a good one", jg::tensor_spec(&spec, out), JPEGGPU_SUCCESS);
    bad("tensor_spec, none", jg::tensor_spec(nullptr, out));
    spec.std[1] = 0.0f;
    bad("tensor_spec, a deviation of 0", jg::tensor_spec(&spec, out));
    spec.type = JPEGGPU_EXT_TENSOR_U8;
    bad("tensor_spec, bytes ignore it", jg::tensor_spec(&spec, out), JPEGGPU_SUCCESS);
    // (a type that is not offered is a C caller's to pass: in C++ the load of such an enum is itself what UBSan reports)
}

// ---- the cases of a file: plans and tables for the comparison with the shipped library -------------------------

int compare(const char* cases, const char* result)
{
    std::FILE* in = std::fopen(cases, "r");
    std::FILE* out = std::fopen(result, "wb");
    if (!in || !out) return 3;
    char line[256];
    while (std::fgets(line, sizeof line, in)) {
        int a = 0, b = 0, c = 0, d = 0, f = 0;
        char gap[64];
        if (std::sscanf(line, "W %d %d %d", &a, &b, &f) == 3) {
            const int taps = jg::resize_max_taps(a, b, f);
            std::vector<int32_t> r(2 + static_cast<size_t>(b) * (2 + static_cast<size_t>(taps)));
            r[1] = taps;
            r[0] = jpeggpu_ext_resize_weights(a, b, static_cast<jpeggpu_ext_filter>(f), r.data() + 2, r.data() + 2 + b, r.data() + 2 + 2 * static_cast<size_t>(b), taps);
            std::fwrite(r.data(), sizeof(int32_t), r.size(), out);
        } else if (std::sscanf(line, "T %d %d %d %d %d %63s", &a, &b, &c, &d, &f, gap) == 6) {
            jpeggpu_ext_thumbnail pl{};
            const int32_t st = jpeggpu_ext_thumbnail_plan(a, b, c, d, static_cast<jpeggpu_ext_filter>(f), std::strtod(gap, nullptr), &pl);
            std::fwrite(&st, sizeof st, 1, out);
            std::fwrite(&pl, sizeof pl, 1, out);
        } else {
            std::fprintf(stderr, "output plan check: a line that is no case: %s", line);
            return 4;
        }
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 3;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc == 3) return compare(argv[1], argv[2]);
    if (argc != 1) return 3;
    sweep_tables();
    sweep_resize();
    sweep_rgb();
    sweep_thumbnails();
    sweep_bad_arguments();
    int done = 0;
    std::printf("output plan check: %d cases enumerated;", g_enumerated);
    for (int k = 0; k < kKinds; ++k) {
        std::printf(" %d %s (%d refused)%s", g_done[k], kKindName[k], g_refused[k], k + 1 < kKinds ? "," : "\n");
        done += g_done[k];
    }
    if (done != g_enumerated) fail(1, "a case was enumerated and not finished");
    return 0;
}
