// jg_transcode.cpp -- the decoder's side of the lossless transcode (jpeggpu_ext.h): what a parsed and decoded image is to
// the encoder -- its geometry as an encoder item, its quantisation tables, and where its coefficients lie in d_tmp for the
// gather kernel (jg_transcode.hpp). Host only; the calls themselves are jg_encode.cpp's.
#include "jg_transcode.hpp"

#include "jg_decoder.hpp"

namespace jg {
namespace enc {

jpeggpu_status transcode_spec(const jpeggpu_ext_transcode_item& it, bool need_device, TranscodeSpec& spec)
{
    spec = TranscodeSpec{};
    if (!it.decoder || !it.decoder->d.parsed) return JPEGGPU_INVALID_ARGUMENT;
    if (it.restart_interval < -1 || it.restart_interval > 65535 || (it.optimize != 0 && it.optimize != 1) || (it.progressive != 0 && it.progressive != 1) ||
        (!it.out && it.capacity))
        return JPEGGPU_INVALID_ARGUMENT;
    if (need_device && (!it.d_tmp || (reinterpret_cast<uintptr_t>(it.d_tmp) & 255))) return JPEGGPU_INVALID_ARGUMENT;
    const Decoder& d = it.decoder->d;
    const Stream& s  = d.reader.s;
    // the coefficients of the frame at its own size: no scale, no share of the restart segments; a decode window only under a
    // transcode crop that stays inside it (below)
    const int* tc      = d.transcode_crop;
    const bool cropped = tc[2] > 0;
    if ((d.crop.on && !cropped) || d.scale_log2 != 0 || d.shard_world != 1) return JPEGGPU_NOT_SUPPORTED;

    // what the encoder writes: grey, or YCbCr with chroma 1 x 1 and luma 1 x 1, 2 x 1 or 2 x 2 and one chroma table
    int subsampling = JPEGGPU_EXT_SUBSAMPLING_444;
    if (s.num_comp == 3) {
        const Component& y = s.comp[0];
        if (s.color_space != kColorYCbCr || s.comp[1].hs != 1 || s.comp[1].vs != 1 || s.comp[2].hs != 1 || s.comp[2].vs != 1 || s.comp[1].qidx != s.comp[2].qidx)
            return JPEGGPU_NOT_SUPPORTED;
        if (y.hs == 1 && y.vs == 1) subsampling = JPEGGPU_EXT_SUBSAMPLING_444;
        else if (y.hs == 2 && y.vs == 1) subsampling = JPEGGPU_EXT_SUBSAMPLING_422;
        else if (y.hs == 2 && y.vs == 2) subsampling = JPEGGPU_EXT_SUBSAMPLING_420;
        else return JPEGGPU_NOT_SUPPORTED;
    } else if (s.num_comp != 1) {
        return JPEGGPU_NOT_SUPPORTED;
    }
    constexpr uint8_t nat[64] = JG_ORDER_NATURAL;
    for (int t = 0; t < (s.num_comp == 1 ? 1 : 2); ++t) {
        const int id = s.comp[t].qidx;
        if (s.qtable16[id]) return JPEGGPU_NOT_SUPPORTED; // Pq = 1
        for (int k = 0; k < 64; ++k) {
            if (s.qtable[id][nat[k]] > 255) return JPEGGPU_NOT_SUPPORTED;
            spec.qtable[t][k] = static_cast<uint8_t>(s.qtable[id][nat[k]]);
        }
    }
    spec.sampling0 = s.comp[0].sampling;

    // jpeggpu_ext_set_transcode_orientation: the stored image the new file holds is the displayed image of the source's.
    // A mirror is exact over whole iMCUs of the source only, so the mirrored STORED axes are such multiples or are cut to one
    const int o          = d.transcode_orientation;
    const bool transpose = o >= 5, mirror_x = o == 2 || o == 3 || o == 6 || o == 7, mirror_y = o == 3 || o == 4 || o == 7 || o == 8;
    const bool stored_x = transpose ? mirror_y : mirror_x, stored_y = transpose ? mirror_x : mirror_y;
    const int hs = s.num_comp == 1 ? 1 : s.comp[0].hs, vs = s.num_comp == 1 ? 1 : s.comp[0].vs;
    int w = s.size_x, h = s.size_y; // the source, trimmed
    if (stored_x && w % (8 * hs)) {
        if (!d.transcode_trim || w < 8 * hs) return JPEGGPU_NOT_SUPPORTED;
        w -= w % (8 * hs);
    }
    if (stored_y && h % (8 * vs)) {
        if (!d.transcode_trim || h < 8 * vs) return JPEGGPU_NOT_SUPPORTED;
        h -= h % (8 * vs);
    }
    if (transpose) {
        if (subsampling == JPEGGPU_EXT_SUBSAMPLING_422) return JPEGGPU_NOT_SUPPORTED; // it would be 4:4:0
        for (int t = 0; t < 2; ++t) { // entry (v, u) is the source's (u, v)
            uint8_t q[64];
            for (int k = 0; k < 64; ++k) q[(nat[k] & 7) << 3 | nat[k] >> 3] = spec.qtable[t][k];
            for (int k = 0; k < 64; ++k) spec.qtable[t][k] = q[nat[k]];
        }
        spec.sampling0 = uint8_t(spec.sampling0 << 4 | spec.sampling0 >> 4); // (a grey file's byte too: jpegtran's transpose_critical_parameters)
    }
    spec.src.oriented = o != 1 || cropped, spec.src.transpose = transpose, spec.src.mirror_x = mirror_x, spec.src.mirror_y = mirror_y;

    // jpeggpu_ext_set_transcode_crop: a rectangle of that image, from an iMCU boundary of the target on
    const int ths = transpose ? vs : hs, tvs = transpose ? hs : vs; // the target's luma factors
    int out_w = transpose ? h : w, out_h = transpose ? w : h;
    if (cropped) {
        if (tc[0] > out_w - tc[2] || tc[1] > out_h - tc[3]) return JPEGGPU_INVALID_ARGUMENT;
        if (tc[0] % (8 * ths) || tc[1] % (8 * tvs)) return JPEGGPU_NOT_SUPPORTED;
        out_w = tc[2], out_h = tc[3];
    }

    jpeggpu_ext_encode_item& e = spec.item;
    e.width = out_w, e.height = out_h, e.channels = s.num_comp;
    e.progressive = it.progressive, e.optimize = it.optimize;
    e.quality          = 75; // (unused: the header holds the source's tables)
    e.subsampling      = subsampling;
    e.restart_interval = it.restart_interval < 0 ? s.first_restart_interval : it.restart_interval;
    e.out = it.out, e.capacity = it.capacity;

    uint8_t* tmp = static_cast<uint8_t*>(it.d_tmp);
    for (int c = 0; c < s.num_comp; ++c) {
        GatherComp& g = spec.src.comp[c];
        g.vis_x = (s.comp[c].size_x + 7) / 8, g.vis_y = (s.comp[c].size_y + 7) / 8;
        const int cut_x = ((c ? (w + hs - 1) / hs : w) + 7) / 8, cut_y = ((c ? (h + vs - 1) / vs : h) + 7) / 8; // of the trimmed source
        g.dst_x = transpose ? cut_y : cut_x, g.dst_y = transpose ? cut_x : cut_y;
        // the source's blocks a cropped item reads, [sx0, sx1) x [sy0, sy1): its real blocks (the DC of a dummy block is one
        // of them) from the offset on, mirrored over the uncropped target's grid, exchanged
        int sx0 = 0, sy0 = 0, sx1 = 0, sy1 = 0;
        if (cropped) {
            g.off_x = int16_t(tc[0] / (c ? 8 * ths : 8)), g.off_y = int16_t(tc[1] / (c ? 8 * tvs : 8));
            const int nx = ((c ? (out_w + ths - 1) / ths : out_w) + 7) / 8, ny = ((c ? (out_h + tvs - 1) / tvs : out_h) + 7) / 8;
            const int x0 = mirror_x ? g.dst_x - g.off_x - nx : g.off_x, y0 = mirror_y ? g.dst_y - g.off_y - ny : g.off_y;
            sx0 = transpose ? y0 : x0, sy0 = transpose ? x0 : y0;
            sx1 = sx0 + (transpose ? ny : nx), sy1 = sy0 + (transpose ? nx : ny);
        }
        // a decode window (jpeggpu_ext_set_crop): its frame MCUs hold every block that is read. It narrows the entropy stage of
        // a single scan with restart markers only (Decoder::plan_image; below); a multi-scan file's scans and a progressive
        // file's coefficient arrays are whole, and the rule is the same for one contract.
        if (d.crop.on && (sx0 < d.crop.mx0 * s.comp[c].hs || sx1 > d.crop.mx1 * s.comp[c].hs || sy0 < d.crop.my0 * s.comp[c].vs ||
                          sy1 > d.crop.my1 * s.comp[c].vs))
            return JPEGGPU_NOT_SUPPORTED;
        if (s.progressive) {
            g.coef     = reinterpret_cast<const int16_t*>(tmp + d.plan.prog.coef[c]);
            g.blocks_x = s.prog_blocks_x[c];
            continue;
        }
        bool found = false;
        for (int i = 0; i < s.num_scans && !found; ++i) {
            const Scan& sc = s.scans[i];
            int k0         = 0;
            for (int a = 0; a < sc.num_comp && !found; ++a) {
                if (sc.comp[a].comp_idx == c) {
                    found         = true;
                    g.sym         = reinterpret_cast<const uint16_t*>(tmp + d.plan.scan[i].sym);
                    g.du_tab      = tmp + d.plan.scan[i].du_tab;
                    g.sym_limit   = sym_buffer_entries(d.sym_regions(i), d.sym_region()) - 10 * kSymSectorStride;
                    g.interleaved = sc.num_comp > 1;
                    g.du_per_mcu = sc.du_per_mcu, g.k0 = k0, g.h = sc.comp[a].h, g.v = sc.comp[a].v, g.mcus_x = sc.mcus_x;
                    if (!g.interleaved) g.vis_x = sc.mcus_x, g.vis_y = sc.mcus_y; // the scan's own grid: the component's real blocks
                    if (cropped && sc.shard_mcus) {
                        // the scan was cut to the restart segments that hold the window (Reader::cut_segments): its units count
                        // from MCU first_mcu on, and every MCU of the scan that is read must lie in the kept run
                        const int bh = g.interleaved ? g.h : 1, bv = g.interleaved ? g.v : 1;
                        const int first = (sy0 / bv) * sc.mcus_x + sx0 / bh, last = ((sy1 - 1) / bv) * sc.mcus_x + (sx1 - 1) / bh;
                        if (first < sc.first_mcu || last >= sc.first_mcu + sc.shard_mcus) return JPEGGPU_NOT_SUPPORTED;
                        spec.src.first_unit = sc.first_mcu * sc.du_per_mcu;
                    }
                }
                k0 += sc.comp[a].h * sc.comp[a].v;
            }
        }
        if (!found) return JPEGGPU_NOT_SUPPORTED;
    }
    return JPEGGPU_SUCCESS;
}

} // namespace enc
} // namespace jg
