// jg_transcode.cpp -- the decoder's side of the lossless transcode (jpeggpu_ext.h): what a parsed and decoded image is to
// the encoder -- its geometry as an encoder item, its quantisation tables, and where its coefficients lie in d_tmp for the
// gather kernel (jg_transcode.hpp). Host only; the calls themselves are jg_encode.cpp's.
#include "jg_transcode.hpp"

#include "jg_decoder.hpp"

namespace jg {
namespace enc {

/// Where component c of a parsed image lies in `tmp`, its d_tmp (jg_transcode.hpp: GatherComp; the fields that depend on an
/// item's target stay the caller's). *scan: the scan that codes a baseline source's component, nullptr for a progressive
/// source. False: no scan codes the component.
bool source_comp(const Decoder& d, uint8_t* tmp, int c, GatherComp& g, const Scan** scan)
{
    const Stream& s = d.reader.s;
    *scan           = nullptr;
    if (s.progressive) {
        g.coef     = reinterpret_cast<const int16_t*>(tmp + d.plan.prog.coef[c]);
        g.blocks_x = s.prog_blocks_x[c];
        return true;
    }
    for (int i = 0; i < s.num_scans; ++i) {
        const Scan& sc = s.scans[i];
        int k0         = 0;
        for (int a = 0; a < sc.num_comp; ++a) {
            if (sc.comp[a].comp_idx == c) {
                g.sym         = reinterpret_cast<const uint16_t*>(tmp + d.plan.scan[i].sym);
                g.du_tab      = tmp + d.plan.scan[i].du_tab;
                g.sym_limit   = sym_buffer_entries(d.sym_regions(i), d.sym_region()) - 10 * kSymSectorStride;
                g.interleaved = sc.num_comp > 1;
                g.du_per_mcu = sc.du_per_mcu, g.k0 = k0, g.h = sc.comp[a].h, g.v = sc.comp[a].v, g.mcus_x = sc.mcus_x;
                if (!g.interleaved) g.vis_x = sc.mcus_x, g.vis_y = sc.mcus_y; // the scan's own grid: the component's real blocks
                *scan = &sc;
                return true;
            }
            k0 += sc.comp[a].h * sc.comp[a].v;
        }
    }
    return false;
}

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

    // what the encoder writes: grey, or YCbCr with chroma 1 x 1 and luma 1 x 1, 2 x 1 or 2 x 2 and one chroma table, 8-bit
    // tables. In SOURCE mode (jpeggpu_ext_set_transcode_frame) such a file goes the same way to the same bytes (its tables
    // numbered 0 and 1, whatever the source calls them); every other file keeps its own frame (`general`)
    const bool keep = d.transcode_frame == JPEGGPU_EXT_TRANSCODE_FRAME_SOURCE;
    int subsampling = JPEGGPU_EXT_SUBSAMPLING_444;
    bool encoders   = true;
    if (s.num_comp == 3) {
        const Component& y = s.comp[0];
        if (s.color_space != kColorYCbCr || s.comp[1].hs != 1 || s.comp[1].vs != 1 || s.comp[2].hs != 1 || s.comp[2].vs != 1 || s.comp[1].qidx != s.comp[2].qidx)
            encoders = false;
        else if (y.hs == 1 && y.vs == 1) subsampling = JPEGGPU_EXT_SUBSAMPLING_444;
        else if (y.hs == 2 && y.vs == 1) subsampling = JPEGGPU_EXT_SUBSAMPLING_422;
        else if (y.hs == 2 && y.vs == 2) subsampling = JPEGGPU_EXT_SUBSAMPLING_420;
        else encoders = false;
    } else if (s.num_comp != 1) {
        encoders = false;
    }
    constexpr uint8_t nat[64] = JG_ORDER_NATURAL;
    for (int t = 0; encoders && t < (s.num_comp == 1 ? 1 : 2); ++t) {
        const int id = s.comp[t].qidx;
        if (s.qtable16[id]) encoders = false; // Pq = 1
        for (int k = 0; encoders && k < 64; ++k) {
            if (s.qtable[id][nat[k]] > 255) encoders = false;
            spec.qtable[t][k] = static_cast<uint8_t>(s.qtable[id][nat[k]]);
        }
    }
    if (!encoders && !keep) return JPEGGPU_NOT_SUPPORTED;
    if (s.num_comp < 1 || s.num_comp > 4) return JPEGGPU_NOT_SUPPORTED;
    spec.sampling0 = s.comp[0].sampling;

    // jpeggpu_ext_set_transcode_orientation: the stored image the new file holds is the displayed image of the source's.
    // A mirror is exact over whole iMCUs of the source only, so the mirrored STORED axes are such multiples or are cut to one
    const int o          = d.transcode_orientation;
    const bool transpose = o >= 5, mirror_x = o == 2 || o == 3 || o == 6 || o == 7, mirror_y = o == 3 || o == 4 || o == 7 || o == 8;
    const bool stored_x = transpose ? mirror_y : mirror_x, stored_y = transpose ? mirror_x : mirror_y;
    // the source's factors per component (1 x 1 for a single component) and the iMCU's
    int ch[4] = {1, 1, 1, 1}, cv[4] = {1, 1, 1, 1}, hs = 1, vs = 1, per_mcu = 0;
    for (int c = 0; c < s.num_comp; ++c) {
        if (s.num_comp > 1) ch[c] = s.comp[c].hs, cv[c] = s.comp[c].vs;
        hs = ch[c] > hs ? ch[c] : hs, vs = cv[c] > vs ? cv[c] : vs;
        per_mcu += ch[c] * cv[c];
    }
    if (per_mcu > kMaxMcuBlocks) return JPEGGPU_NOT_SUPPORTED;
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
        if (subsampling == JPEGGPU_EXT_SUBSAMPLING_422) {
            if (!keep) return JPEGGPU_NOT_SUPPORTED; // it would be 4:4:0
            encoders = false;
        }
        for (int t = 0; t < 2; ++t) { // entry (v, u) is the source's (u, v)
            uint8_t q[64];
            for (int k = 0; k < 64; ++k) q[(nat[k] & 7) << 3 | nat[k] >> 3] = spec.qtable[t][k];
            for (int k = 0; k < 64; ++k) spec.qtable[t][k] = q[nat[k]];
        }
        spec.sampling0 = uint8_t(spec.sampling0 << 4 | spec.sampling0 >> 4); // (a grey file's byte too: jpegtran's transpose_critical_parameters)
    }
    spec.src.oriented = o != 1 || cropped, spec.src.transpose = transpose, spec.src.mirror_x = mirror_x, spec.src.mirror_y = mirror_y;
    spec.general      = !encoders;

    // jpeggpu_ext_set_transcode_crop: a rectangle of that image, from an iMCU boundary of the target on
    const int ths = transpose ? vs : hs, tvs = transpose ? hs : vs; // the target's iMCU
    int out_w = transpose ? h : w, out_h = transpose ? w : h;
    if (cropped) {
        if (tc[0] > out_w - tc[2] || tc[1] > out_h - tc[3]) return JPEGGPU_INVALID_ARGUMENT;
        if (tc[0] % (8 * ths) || tc[1] % (8 * tvs)) return JPEGGPU_NOT_SUPPORTED;
        out_w = tc[2], out_h = tc[3];
    }
    const auto blocks_of = [](int pixels, int f, int fmax) { return ((pixels * f + fmax - 1) / fmax + 7) / 8; }; // of a component

    if (spec.general) { // the header of libjpeg after jpeg_copy_critical_parameters and jpeg_set_colorspace
        const int cs     = s.color_space;
        spec.color_space = cs;
        static const char rgb[] = "RGB", cmyk[] = "CMYK";
        Frame& f = spec.frame;
        f        = Frame{};
        f.ncomp  = uint8_t(s.num_comp);
        int j    = 0;
        for (int c = 0; c < s.num_comp; ++c) {
            TranscodeSpec::Comp& tcmp = spec.comp[c];
            tcmp.id     = cs == kColorGray || cs == kColorYCbCr || cs == kColorYCCK ? uint8_t(c + 1) : cs == kColorRGB ? uint8_t(rgb[c]) : cs == kColorCMYK ? uint8_t(cmyk[c]) : uint8_t(c);
            tcmp.h      = uint8_t(transpose ? cv[c] : ch[c]);
            tcmp.v      = uint8_t(transpose ? ch[c] : cv[c]);
            if (s.num_comp == 1) tcmp.h = spec.sampling0 >> 4, tcmp.v = spec.sampling0 & 15; // written back as it came
            tcmp.tq     = s.comp[c].qidx;
            tcmp.select = (cs == kColorYCbCr || cs == kColorYCCK) && (c == 1 || c == 2);
            int t       = 0;
            while (t < spec.tables_n && spec.table_id[t] != tcmp.tq) ++t;
            if (t == spec.tables_n) {
                spec.table_id[t] = tcmp.tq;
                uint16_t q[64];
                for (int k = 0; k < 64; ++k) {
                    const uint16_t v = s.qtable[tcmp.tq][nat[k]];
                    if (v > 255) spec.table16[t] = true;
                    spec.table[t][k] = v;
                    q[transpose ? (nat[k] & 7) << 3 | nat[k] >> 3 : nat[k]] = v;
                }
                if (transpose)
                    for (int k = 0; k < 64; ++k) spec.table[t][k] = q[nat[k]];
                ++spec.tables_n;
            }
            const int th = transpose ? cv[c] : ch[c], tv = transpose ? ch[c] : cv[c]; // the blocks of an MCU
            for (int yo = 0; yo < tv; ++yo)
                for (int xo = 0; xo < th; ++xo, ++j) {
                    f.map |= uint64_t(c | xo << 2 | yo << 4) << (6 * j);
                    f.last |= uint64_t(th * tv - 1) << (4 * j);
                }
            f.hv |= uint32_t(th | tv << 4) << (8 * c);
            f.select |= uint8_t(tcmp.select << c);
            f.grid_w[c] = blocks_of(out_w, th, ths), f.grid_h[c] = blocks_of(out_h, tv, tvs);
        }
    }

    jpeggpu_ext_encode_item& e = spec.item;
    e.width = out_w, e.height = out_h, e.channels = s.num_comp;
    e.progressive = it.progressive, e.optimize = it.optimize;
    e.quality          = 75; // (unused: the header holds the source's tables)
    e.subsampling      = spec.general ? JPEGGPU_EXT_SUBSAMPLING_444 : subsampling;
    e.restart_interval = it.restart_interval < 0 ? s.first_restart_interval : it.restart_interval;
    e.out = it.out, e.capacity = it.capacity;

    uint8_t* tmp = static_cast<uint8_t*>(it.d_tmp);
    for (int c = 0; c < s.num_comp; ++c) {
        GatherComp& g = spec.src.comp[c];
        g.vis_x = (s.comp[c].size_x + 7) / 8, g.vis_y = (s.comp[c].size_y + 7) / 8;
        const int cut_x = blocks_of(w, ch[c], hs), cut_y = blocks_of(h, cv[c], vs); // of the trimmed source
        const int th = transpose ? cv[c] : ch[c], tv = transpose ? ch[c] : cv[c];    // the component's factors in the target
        g.dst_x = transpose ? cut_y : cut_x, g.dst_y = transpose ? cut_x : cut_y;
        // the source's blocks a cropped item reads, [sx0, sx1) x [sy0, sy1): its real blocks (the DC of a dummy block is one
        // of them) from the offset on, mirrored over the uncropped target's grid, exchanged
        int sx0 = 0, sy0 = 0, sx1 = 0, sy1 = 0;
        if (cropped) {
            g.off_x = int16_t(tc[0] / (8 * ths) * th), g.off_y = int16_t(tc[1] / (8 * tvs) * tv);
            const int nx = blocks_of(out_w, th, ths), ny = blocks_of(out_h, tv, tvs);
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
        const Scan* sc = nullptr;
        if (!source_comp(d, tmp, c, g, &sc)) return JPEGGPU_NOT_SUPPORTED;
        if (sc && cropped && sc->shard_mcus) {
            // the scan was cut to the restart segments that hold the window (Reader::cut_segments): its units count
            // from MCU first_mcu on, and every MCU of the scan that is read must lie in the kept run
            const int bh = g.interleaved ? g.h : 1, bv = g.interleaved ? g.v : 1;
            const int first = (sy0 / bv) * sc->mcus_x + sx0 / bh, last = ((sy1 - 1) / bv) * sc->mcus_x + (sx1 - 1) / bh;
            if (first < sc->first_mcu || last >= sc->first_mcu + sc->shard_mcus) return JPEGGPU_NOT_SUPPORTED;
            spec.src.first_unit = sc->first_mcu * sc->du_per_mcu;
        }
    }
    return JPEGGPU_SUCCESS;
}

} // namespace enc
} // namespace jg
