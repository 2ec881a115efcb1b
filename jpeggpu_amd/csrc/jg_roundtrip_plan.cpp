// jg_roundtrip_plan.cpp -- the host plan of a JPEG round trip (jg_roundtrip_plan.hpp) and jpeggpu_ext_roundtrip_scratch_size,
// which launches nothing. Nothing here touches the device: no HIP header, a plain C++ compiler builds it, and
// tests/test_roundtrip_plan_host.py runs it under ASan and UBSan in a stand-alone program.
#include "jg_roundtrip_plan.hpp"

#include <cstring>
#include <new>

namespace jg {
namespace rt {
namespace {

// the layout the ctypes mirror (jpeggpu_amd/api.py, RoundtripItem) is written for
static_assert(sizeof(jpeggpu_ext_roundtrip_item) == 80 && offsetof(jpeggpu_ext_roundtrip_item, row_pitch) == 24 &&
                  offsetof(jpeggpu_ext_roundtrip_item, quality) == 48 && offsetof(jpeggpu_ext_roundtrip_item, dst) == 56 &&
                  offsetof(jpeggpu_ext_roundtrip_item, dst_pitch) == 64 && offsetof(jpeggpu_ext_roundtrip_item, plane_stride) == 72,
              "struct jpeggpu_ext_roundtrip_item");
static_assert(sizeof(Item) % 8 == 0, "Item[n] in the staged bytes");

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Annex K.1, K.2 (natural order): the numbers of jg_quant.h
const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                               14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

/// jpeg_set_quality's table (force_baseline), natural order.
void quant_table(const uint8_t* base, int quality, uint16_t* q)
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int v = (base[i] * s + 50) / 100;
        q[i]        = uint16_t(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

bool valid(const jpeggpu_ext_roundtrip_item& s)
{
    return s.width >= 1 && s.width <= 65535 && s.height >= 1 && s.height <= 65535 && (s.channels == 1 || s.channels == 3) && s.quality >= 1 &&
           s.quality <= 100 && (s.channels == 1 || (s.subsampling >= JPEGGPU_EXT_SUBSAMPLING_444 && s.subsampling <= JPEGGPU_EXT_SUBSAMPLING_420));
}

} // namespace

void item_geometry(const jpeggpu_ext_roundtrip_item& s, Item& it)
{
    const bool grey = s.channels == 1;
    it              = Item{};
    it.width        = s.width;
    it.height       = s.height;
    it.channels     = s.channels;
    it.hs           = !grey && s.subsampling != JPEGGPU_EXT_SUBSAMPLING_444 ? 2 : 1;
    it.vs           = !grey && s.subsampling == JPEGGPU_EXT_SUBSAMPLING_420 ? 2 : 1;
    it.grid_w       = (s.width + 7) / 8;
    it.grid_h       = (s.height + 7) / 8;
    it.mcus_x       = (s.width + 8 * it.hs - 1) / (8 * it.hs);
    it.mcus_y       = (s.height + 8 * it.vs - 1) / (8 * it.vs);
    it.blocks       = it.grid_w * it.grid_h + (grey ? 0 : 2 * it.mcus_x * it.mcus_y); // at most 8192^2 * 3 < 2^31
    quant_table(kBaseLuma, s.quality, it.quant[0]);
    quant_table(kBaseChroma, s.quality, it.quant[1]);
}

jpeggpu_status plan_roundtrip(const jpeggpu_ext_roundtrip_item* items, int n, int layout, uint8_t* base, Plan& p, bool sizes_only)
{
    if (!items || n <= 0 || n > 65535) return JPEGGPU_INVALID_ARGUMENT;
    if (!sizes_only && layout != JPEGGPU_EXT_HWC && layout != JPEGGPU_EXT_CHW) return JPEGGPU_INVALID_ARGUMENT;
    int n_rgb = 0;
    for (int i = 0; i < n; ++i) {
        const jpeggpu_ext_roundtrip_item& s = items[i];
        if (!valid(s)) return JPEGGPU_INVALID_ARGUMENT;
        n_rgb += s.channels == 3;
        if (sizes_only) continue;
        if (!s.data || !s.dst) return JPEGGPU_INVALID_ARGUMENT;
        const int64_t w = s.width, h = s.height;
        if (s.channels == 1 ? s.dst_pitch < w
                            : layout == JPEGGPU_EXT_HWC ? s.dst_pitch < 3 * w : s.dst_pitch < w || s.plane_stride < static_cast<size_t>(s.dst_pitch) * h)
            return JPEGGPU_INVALID_ARGUMENT;
    }
    try {
        p.items.resize(n);
        p.infos.resize(n_rgb);
        p.imgs.resize(n_rgb);
        p.rgb_items.resize(n_rgb);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    p.n_rgb     = n_rgb;
    p.off_items = n_rgb ? rgb_batch_layout(n_rgb).total : 0;
    p.head      = align_up(p.off_items + sizeof(Item) * static_cast<size_t>(n), 256);
    uint64_t tiles = 0;
    size_t off     = p.head;
    for (int i = 0, k = 0; i < n; ++i) {
        const jpeggpu_ext_roundtrip_item& s = items[i];
        Item& it = p.items[i];
        item_geometry(s, it);
        it.src            = s.data;
        it.row_pitch      = s.row_pitch;
        it.pixel_stride   = s.pixel_stride;
        it.channel_stride = s.channel_stride;
        it.tile_start     = static_cast<uint32_t>(tiles);
        tiles += (static_cast<uint64_t>(it.blocks) + kTileBlocks - 1) / kTileBlocks;
        if (tiles * kTileBlocks >= (uint64_t{1} << 31)) return JPEGGPU_NOT_SUPPORTED;
        if (s.channels == 1) {
            it.dst      = s.dst;
            it.pitch[0] = s.dst_pitch;
            continue;
        }
        // the planes: whole blocks, rows of a multiple of 16 bytes, each plane on a 256-byte boundary
        it.pitch[0] = static_cast<int>(align_up(static_cast<size_t>(it.grid_w) * 8, 16));
        it.pitch[1] = static_cast<int>(align_up(static_cast<size_t>(it.mcus_x) * 8, 16));
        jpeggpu_img_info& info = p.infos[k];
        jpeggpu_img& img       = p.imgs[k];
        info                   = jpeggpu_img_info{};
        img                    = jpeggpu_img{};
        info.num_components    = 3;
        for (int c = 0; c < 3; ++c) {
            const int rows    = (c ? it.mcus_y : it.grid_h) * 8;
            it.plane_off[c]   = off;
            off += align_up(static_cast<size_t>(it.pitch[c > 0]) * rows, 256);
            info.sizes_x[c]       = c ? (s.width + it.hs - 1) / it.hs : s.width; // libjpeg's downsampled sizes
            info.sizes_y[c]       = c ? (s.height + it.vs - 1) / it.vs : s.height;
            info.subsampling.x[c] = c ? 1 : it.hs;
            info.subsampling.y[c] = c ? 1 : it.vs;
            img.image[c]          = base + it.plane_off[c];
            img.pitch[c]          = it.pitch[c > 0];
        }
        p.rgb_items[k] = jpeggpu_ext_rgb_item{&info, nullptr, &img, JPEGGPU_EXT_COLOR_YCBCR, 1, 0, s.dst, s.dst_pitch, s.plane_stride};
        ++k;
    }
    p.tiles = static_cast<uint32_t>(tiles);
    p.total = off;
    if (sizes_only || n_rgb == 0) return JPEGGPU_SUCCESS;
    return plan_rgb_batch(p.rgb_items.data(), n_rgb, layout, p.rgb);
}

void fill_roundtrip(const Plan& p, uint8_t* h)
{
    std::memset(h, 0, p.head);
    if (p.n_rgb) fill_rgb_batch(p.rgb, h);
    std::memcpy(h + p.off_items, p.items.data(), sizeof(Item) * p.items.size());
}

} // namespace rt
} // namespace jg

extern "C" size_t jpeggpu_ext_roundtrip_scratch_size(const struct jpeggpu_ext_roundtrip_item* items, int n)
{
    jg::rt::Plan p;
    if (jg::rt::plan_roundtrip(items, n, JPEGGPU_EXT_HWC, reinterpret_cast<uint8_t*>(uintptr_t{256}), p, true) != JPEGGPU_SUCCESS) return 0;
    return p.total + 256; // room to align the caller's pointer
}
