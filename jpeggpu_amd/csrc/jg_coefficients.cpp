// jg_coefficients.cpp -- DCT-domain access (jpeggpu_ext.h: jpeggpu_ext_read_coefficients_batch and the
// jpeggpu_ext_write_coefficients_ calls), the side that knows the decoder and the frame: what a parsed image says of its
// coefficients, the items of a read call for the kernel of jg_encode.hip, and the TranscodeSpec of a write item, whose
// source is the caller's tensors (jg_transcode.hpp). Host only; staging and launches are jg_encode.cpp's.
#include "jg_transcode.hpp"

#include "jg_decoder.hpp"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

namespace jg {
namespace enc {
namespace {

static_assert(sizeof(jpeggpu_ext_coefficient_info) == 612 && offsetof(jpeggpu_ext_coefficient_info, qtable) == 100, "struct jpeggpu_ext_coefficient_info");
static_assert(sizeof(jpeggpu_ext_coefficient_spec) == 8 && sizeof(jpeggpu_ext_coefficient_read_item) == 48, "the read call's structs");
static_assert(sizeof(jpeggpu_ext_coefficient_item) == 624 && offsetof(jpeggpu_ext_coefficient_item, coef) == 560 &&
                  offsetof(jpeggpu_ext_coefficient_item, out) == 608,
              "struct jpeggpu_ext_coefficient_item");

/// A component's real blocks along one axis: libjpeg's width_in_blocks / height_in_blocks.
int real_blocks(int pixels, int f, int fmax) { return ((pixels * f + fmax - 1) / fmax + 7) / 8; }

/// A parsed frame whose coefficients the reader hands out: no scale, no share of the restart segments, no decode window.
jpeggpu_status readable(const Decoder& d)
{
    if (!d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    if (d.crop.on || d.scale_log2 != 0 || d.shard_world != 1) return JPEGGPU_NOT_SUPPORTED;
    return JPEGGPU_SUCCESS;
}

void grids_of(const Stream& s, int* gw, int* gh)
{
    for (int c = 0; c < s.num_comp; ++c) {
        // (Component::hs is 1 x 1 for a single component, whatever its frame header says)
        gw[c] = real_blocks(s.size_x, s.comp[c].hs, s.num_comp > 1 ? s.hs_max : 1);
        gh[c] = real_blocks(s.size_y, s.comp[c].vs, s.num_comp > 1 ? s.vs_max : 1);
    }
}

} // namespace

jpeggpu_status coefficient_spec(const jpeggpu_ext_coefficient_item& it, bool need_device, TranscodeSpec& spec)
{
    spec = TranscodeSpec{};
    const int n = it.components;
    if (it.width < 1 || it.width > 65535 || it.height < 1 || it.height > 65535 || n < 1 || n > 4) return JPEGGPU_INVALID_ARGUMENT;
    if (it.restart_interval < 0 || it.restart_interval > 65535 || (it.optimize != 0 && it.optimize != 1) || (it.progressive != 0 && it.progressive != 1) ||
        (!it.out && it.capacity))
        return JPEGGPU_INVALID_ARGUMENT;
    const int cs = it.color_space;
    const int fits[6] = {n, 1, 3, 3, 4, 4}; // the component count of each colour model (UNKNOWN: any)
    if (cs < JPEGGPU_EXT_COLOR_UNKNOWN || cs > JPEGGPU_EXT_COLOR_YCCK || fits[cs] != n) return JPEGGPU_INVALID_ARGUMENT;
    int hs = 1, vs = 1, per_mcu = 0;
    for (int c = 0; c < n; ++c) {
        if (it.h[c] < 1 || it.h[c] > 4 || it.v[c] < 1 || it.v[c] > 4) return JPEGGPU_INVALID_ARGUMENT;
        if (need_device && (!it.coef[c] || (reinterpret_cast<uintptr_t>(it.coef[c]) & 15))) return JPEGGPU_INVALID_ARGUMENT;
        for (int k = 0; k < 64; ++k)
            if (it.qtable[c][k] == 0) return JPEGGPU_INVALID_ARGUMENT;
        hs = it.h[c] > hs ? it.h[c] : hs, vs = it.v[c] > vs ? it.v[c] : vs;
        per_mcu += n > 1 ? it.h[c] * it.v[c] : 1;
    }
    if (per_mcu > kMaxMcuBlocks) return JPEGGPU_INVALID_ARGUMENT;
    // a single component's MCU is one block: its factors are written back and change nothing else
    int ch[4] = {1, 1, 1, 1}, cv[4] = {1, 1, 1, 1};
    if (n > 1)
        for (int c = 0; c < n; ++c) ch[c] = it.h[c], cv[c] = it.v[c];
    else
        hs = vs = 1;

    // the encoder's own layouts (transcode_spec): they get the encoder's header and geometry
    constexpr uint8_t nat[64] = JG_ORDER_NATURAL;
    bool encoders   = n == 1;
    int subsampling = JPEGGPU_EXT_SUBSAMPLING_444;
    if (n == 3 && cs == JPEGGPU_EXT_COLOR_YCBCR && ch[1] == 1 && cv[1] == 1 && ch[2] == 1 && cv[2] == 1 &&
        std::memcmp(it.qtable[1], it.qtable[2], sizeof it.qtable[1]) == 0) {
        encoders = true;
        if (ch[0] == 1 && cv[0] == 1) subsampling = JPEGGPU_EXT_SUBSAMPLING_444;
        else if (ch[0] == 2 && cv[0] == 1) subsampling = JPEGGPU_EXT_SUBSAMPLING_422;
        else if (ch[0] == 2 && cv[0] == 2) subsampling = JPEGGPU_EXT_SUBSAMPLING_420;
        else encoders = false;
    }
    for (int t = 0; encoders && t < (n == 1 ? 1 : 2); ++t)
        for (int k = 0; encoders && k < 64; ++k) {
            if (it.qtable[t][nat[k]] > 255) encoders = false;
            spec.qtable[t][k] = static_cast<uint8_t>(it.qtable[t][nat[k]]);
        }
    spec.sampling0 = uint8_t(it.h[0] << 4 | it.v[0]);
    spec.general   = !encoders;
    spec.src.oriented = 1; // the identity, mapped: the dummy blocks are gather_blocks<true>'s

    if (spec.general) { // as transcode_spec makes the frame of a source it keeps
        spec.color_space = cs;
        static const char rgb[] = "RGB", cmyk[] = "CMYK";
        Frame& f = spec.frame;
        f.ncomp  = uint8_t(n);
        int j    = 0;
        for (int c = 0; c < n; ++c) {
            TranscodeSpec::Comp& tc = spec.comp[c];
            tc.id = cs == JPEGGPU_EXT_COLOR_GRAY || cs == JPEGGPU_EXT_COLOR_YCBCR || cs == JPEGGPU_EXT_COLOR_YCCK ? uint8_t(c + 1)
                    : cs == JPEGGPU_EXT_COLOR_RGB                                                               ? uint8_t(rgb[c])
                    : cs == JPEGGPU_EXT_COLOR_CMYK                                                              ? uint8_t(cmyk[c])
                                                                                                                : uint8_t(c);
            tc.h = uint8_t(it.h[c]), tc.v = uint8_t(it.v[c]);
            tc.select = (cs == JPEGGPU_EXT_COLOR_YCBCR || cs == JPEGGPU_EXT_COLOR_YCCK) && (c == 1 || c == 2);
            // tables are numbered by first appearance: components with equal tables share one
            int t = 0;
            while (t < spec.tables_n && std::memcmp(it.qtable[c], it.qtable[spec.table_id[t]], sizeof it.qtable[c]) != 0) ++t;
            if (t == spec.tables_n) {
                spec.table_id[t] = uint8_t(c); // (for now the component that brought it: what the loop above compares with)
                for (int k = 0; k < 64; ++k) {
                    spec.table[t][k] = it.qtable[c][nat[k]];
                    if (spec.table[t][k] > 255) spec.table16[t] = true;
                }
                ++spec.tables_n;
            }
            tc.tq = uint8_t(t);
            for (int yo = 0; yo < cv[c]; ++yo)
                for (int xo = 0; xo < ch[c]; ++xo, ++j) {
                    f.map |= uint64_t(c | xo << 2 | yo << 4) << (6 * j);
                    f.last |= uint64_t(ch[c] * cv[c] - 1) << (4 * j);
                }
            f.hv |= uint32_t(ch[c] | cv[c] << 4) << (8 * c);
            f.select |= uint8_t(tc.select << c);
            f.grid_w[c] = real_blocks(it.width, ch[c], hs), f.grid_h[c] = real_blocks(it.height, cv[c], vs);
        }
        for (int t = 0; t < spec.tables_n; ++t) spec.table_id[t] = uint8_t(t);
    }

    jpeggpu_ext_encode_item& e = spec.item;
    e.width = it.width, e.height = it.height, e.channels = n;
    e.progressive = it.progressive, e.optimize = it.optimize;
    e.quality          = 75; // (unused: the header holds the item's tables)
    e.subsampling      = spec.general ? JPEGGPU_EXT_SUBSAMPLING_444 : subsampling;
    e.restart_interval = it.restart_interval;
    e.out = it.out, e.capacity = it.capacity;

    for (int c = 0; c < n; ++c) {
        GatherComp& g = spec.src.comp[c];
        g.coef        = need_device ? it.coef[c] : nullptr;
        g.blocks_x    = real_blocks(it.width, ch[c], hs);
        g.vis_x = g.dst_x = g.blocks_x;
        g.vis_y = g.dst_y = real_blocks(it.height, cv[c], vs);
    }
    return JPEGGPU_SUCCESS;
}

} // namespace enc
} // namespace jg

using namespace jg::enc;

extern "C" {

enum jpeggpu_status jpeggpu_ext_get_coefficient_info(jpeggpu_decoder_t decoder, struct jpeggpu_ext_coefficient_info* info)
{
    if (!decoder || !info || !decoder->d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    const jg::Stream& s = decoder->d.reader.s;
    std::memset(info, 0, sizeof(*info));
    info->width = s.size_x, info->height = s.size_y, info->num_components = s.num_comp;
    info->color_space = s.color_space;
    info->progressive = s.progressive ? 1 : 0;
    grids_of(s, info->blocks_x, info->blocks_y);
    for (int c = 0; c < s.num_comp; ++c) {
        info->h[c] = s.comp[c].sampling >> 4, info->v[c] = s.comp[c].sampling & 15;
        for (int k = 0; k < 64; ++k) {
            info->qtable[c][k] = s.qtable[s.comp[c].qidx][k];
            if (info->qtable[c][k] > 255) info->table16[c] = 1;
        }
    }
    return JPEGGPU_SUCCESS;
}

size_t jpeggpu_ext_read_coefficients_scratch_size(int n)
{
    if (n <= 0 || n > 65535) return 0;
    return sizeof(ReadItem) * (size_t(n) + 1) + 256; // the items, a sentinel, and room to align the caller's pointer
}

enum jpeggpu_status jpeggpu_ext_read_coefficients_batch(
    const struct jpeggpu_ext_coefficient_read_item* items, int n, const struct jpeggpu_ext_coefficient_spec* spec, void* d_scratch, size_t scratch_size,
    jpeggpu_stream_t stream)
{
    if (!items || !spec || !d_scratch || n <= 0 || n > 65535) return JPEGGPU_INVALID_ARGUMENT;
    const int type = static_cast<int>(spec->type);
    if (type != JPEGGPU_EXT_COEF_I16 && type != JPEGGPU_EXT_COEF_F32 && type != JPEGGPU_EXT_COEF_F16) return JPEGGPU_INVALID_ARGUMENT;
    if ((spec->dequantize != 0 && spec->dequantize != 1) || (spec->dequantize && type == JPEGGPU_EXT_COEF_I16)) return JPEGGPU_INVALID_ARGUMENT;
    try {
        std::vector<ReadItem> dev(size_t(n) + 1);
        uint64_t tiles = 0;
        for (int i = 0; i < n; ++i) {
            const jpeggpu_ext_coefficient_read_item& it = items[i];
            if (!it.decoder || !it.d_tmp || (reinterpret_cast<uintptr_t>(it.d_tmp) & 255)) return JPEGGPU_INVALID_ARGUMENT;
            const jg::Decoder& d    = it.decoder->d;
            const jpeggpu_status st = readable(d);
            if (st != JPEGGPU_SUCCESS) return st;
            const jg::Stream& s = d.reader.s;
            ReadItem& r         = dev[size_t(i)];
            r                   = ReadItem{};
            grids_of(s, r.grid_w, r.grid_h);
            for (int c = 0; c < s.num_comp; ++c) {
                if (!it.dst[c] || (reinterpret_cast<uintptr_t>(it.dst[c]) & 15)) return JPEGGPU_INVALID_ARGUMENT;
                r.dst[c]              = it.dst[c];
                GatherComp& g         = r.src.comp[c];
                const jg::Scan* scan  = nullptr;
                g.vis_x = r.grid_w[c], g.vis_y = r.grid_h[c];
                if (!source_comp(d, static_cast<uint8_t*>(it.d_tmp), c, g, &scan)) g = GatherComp{}; // no scan codes it: zeros
                r.tile_start[c] = uint32_t(tiles);
                tiles += (uint64_t(r.grid_w[c]) * r.grid_h[c] + kReadTile - 1) / kReadTile;
                for (int k = 0; k < 64; ++k) r.factor[c][k] = spec->dequantize ? s.qtable[s.comp[c].qidx][k] : uint16_t(1);
            }
            for (int c = s.num_comp; c < 5; ++c) r.tile_start[c] = uint32_t(tiles);
            if (tiles * kReadTile >= (uint64_t(1) << 31)) return JPEGGPU_NOT_SUPPORTED;
        }
        dev[size_t(n)] = ReadItem{};
        for (int c = 0; c < 5; ++c) dev[size_t(n)].tile_start[c] = uint32_t(tiles);
        return read_coefficients(dev.data(), n, type, d_scratch, scratch_size, stream);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
}

} // extern "C"
