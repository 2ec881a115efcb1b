// jg_encode_plan.cpp -- the encoder's host side that launches nothing: the Annex K tables, one description of the file an
// item becomes (FileFrame), the header writers and progression scripts that read it, the plan of a call, the fill of its
// staged blob, and the entry points of the exported C ABI (include/jpeggpu/jpeggpu_ext.h) that need no device. Free of HIP.
#include "jg_encode_plan.hpp"
#include "jg_quant.h"

#include <cstdlib>
#include <cstring>
#include <new>

namespace jg {
namespace enc {
namespace {

static_assert(sizeof(size_t) == sizeof(unsigned long long), "d_sizes is written as 64-bit words");
static_assert(sizeof(jpeggpu_ext_encode_item) == 80 && offsetof(jpeggpu_ext_encode_item, out) == 64,
              "`optimize` took the place of padding: callers built against the struct without it pass a zero there");
static_assert(offsetof(jpeggpu_ext_encode_item, channels) == 16 && offsetof(jpeggpu_ext_encode_item, progressive) == 20 &&
                  offsetof(jpeggpu_ext_encode_item, row_pitch) == 24 && offsetof(jpeggpu_ext_encode_item, channel_stride) == 40 &&
                  offsetof(jpeggpu_ext_encode_item, quality) == 48 && offsetof(jpeggpu_ext_encode_item, optimize) == 60 &&
                  offsetof(jpeggpu_ext_encode_item, capacity) == 72,
              "`progressive` took the place of the padding behind `channels`: no other member moved");

uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// The zigzag order, and Annex K.3 - K.6 (K.1 and K.2: jg_quant.h)
const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffSpec {
    uint8_t bits[16];
    int count;
    uint8_t values[162];
};
const HuffSpec kDcLuma   = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
const HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
const HuffSpec kAcLuma   = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
    162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
     0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
     0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
     0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
     0xFA}};
const HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
     0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
     0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
     0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
     0xFA}};

/// Annex C: code << 8 | length per symbol, and the longest code of the table.
int derive(const HuffSpec& spec, uint32_t* out)
{
    uint32_t code = 0;
    int k = 0, longest = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < spec.bits[len - 1]; ++i) {
            out[spec.values[k++]] = code << 8 | uint32_t(len);
            ++code;
            longest = len;
        }
        code <<= 1;
    }
    return longest;
}

/// The tables once per process, and the check that kMaxBlockBits is what they say.
const Tables& tables()
{
    static const Tables* t = [] {
        Tables* x = new Tables();
        int dc    = derive(kDcLuma, x->dc);
        int d2    = derive(kDcChroma, x->dc + 16);
        int ac    = derive(kAcLuma, x->ac);
        int a2    = derive(kAcChroma, x->ac + 256);
        if ((dc > d2 ? dc : d2) != kMaxDcCode || (ac > a2 ? ac : a2) != kMaxAcCode) std::abort();
        return x;
    }();
    return *t;
}

/// jpeg_set_quality's table (force_baseline), natural order.
/// `table` 0: luma, 1: chroma. The arithmetic is jg_quant.h's, which the device shares.
void quant_table(int table, int quality, uint8_t* q)
{
    for (int i = 0; i < 64; ++i) q[i] = uint8_t(quantizer(table, quality, i));
}

/// The ranges of an item's fields but `channels`, which depends on the frame (file_frame).
bool valid(const jpeggpu_ext_encode_item* it)
{
    return it && it->width >= 1 && it->width <= 65535 && it->height >= 1 && it->height <= 65535 && it->quality >= 1 && it->quality <= 100 &&
           it->subsampling >= JPEGGPU_EXT_SUBSAMPLING_444 && it->subsampling <= JPEGGPU_EXT_SUBSAMPLING_420 && it->restart_interval >= 0 &&
           it->restart_interval <= 65535 && (it->optimize == 0 || it->optimize == 1) && (it->progressive == 0 || it->progressive == 1);
}

/// The file an item becomes, as far as its header, its geometry and its scans go: the one description that the writers,
/// geometry() and prog_script() read. Made by file_frame() from a pixel item, from a transcode item in one of the encoder's
/// layouts (its source's tables and first sampling byte), or from a transcode item that keeps its source's frame.
struct FileFrame {
    int app;                 // the APPn segment: 0xE0 JFIF, 0xEE Adobe, 0 none
    uint8_t adobe_transform; // APP14's last byte
    bool ycc;                // three components mean YCbCr: jpeg_simple_progression gives them its ten scans
    int ncomp, dqt_n;
    struct {
        uint8_t id;
        bool wide; // Pq = 1: 16-bit entries, and the frame is SOF1
        uint16_t q[64];
    } dqt[4];                // the DQT segments as written, zigzag order
    struct {
        uint8_t id, h, v, tq, select; // SOFn's and SOS's; `select`: the component's Huffman tables, 0 or 1
    } comp[4];
    // what is coded: the factors that make the MCU (a grey pixel file writes the factors it was asked for and codes one block
    // per MCU) and each component's real blocks
    int ch[4], cv[4], grid_w[4], grid_h[4];
    // what ProgScan tells the device about a scan of component c (h, v, k0: zero for an item in the encoder's layouts,
    // whose kernels know them) and the blocks_x of an interleaved scan
    int scan_h[4], scan_v[4], scan_k0[4], interleaved_x;
};

/// false: `channels` is not a count the frame can have. `spec`: a transcode item's.
bool file_frame(const jpeggpu_ext_encode_item& it, const TranscodeSpec* spec, FileFrame& f)
{
    f       = FileFrame{};
    f.ncomp = it.channels;
    if (spec && spec->general) {
        if (f.ncomp < 1 || f.ncomp > 4) return false;
        const int cs = spec->color_space;
        f.ycc        = cs == JPEGGPU_EXT_COLOR_YCBCR;
        if (cs == JPEGGPU_EXT_COLOR_GRAY || cs == JPEGGPU_EXT_COLOR_YCBCR) f.app = 0xE0;
        if (cs == JPEGGPU_EXT_COLOR_RGB || cs == JPEGGPU_EXT_COLOR_CMYK || cs == JPEGGPU_EXT_COLOR_YCCK) f.app = 0xEE;
        f.adobe_transform = cs == JPEGGPU_EXT_COLOR_YCCK ? 2 : 0;
        f.dqt_n           = spec->tables_n;
        for (int t = 0; t < f.dqt_n; ++t) {
            f.dqt[t].id = spec->table_id[t], f.dqt[t].wide = spec->table16[t];
            std::memcpy(f.dqt[t].q, spec->table[t], sizeof f.dqt[t].q);
        }
        for (int c = 0, at = 0; c < f.ncomp; ++c) {
            f.comp[c].id = spec->comp[c].id, f.comp[c].h = spec->comp[c].h, f.comp[c].v = spec->comp[c].v;
            f.comp[c].tq = spec->comp[c].tq, f.comp[c].select = spec->comp[c].select;
            f.ch[c] = f.scan_h[c] = spec->frame.hv >> (8 * c) & 15, f.cv[c] = f.scan_v[c] = spec->frame.hv >> (8 * c + 4) & 15;
            f.grid_w[c] = spec->frame.grid_w[c], f.grid_h[c] = spec->frame.grid_h[c];
            f.scan_k0[c] = at;
            at += f.ch[c] * f.cv[c];
        }
        f.interleaved_x = f.grid_w[0];
        return true;
    }
    if (f.ncomp != 1 && f.ncomp != 3) return false;
    const int hs = it.subsampling != JPEGGPU_EXT_SUBSAMPLING_444 ? 2 : 1, vs = it.subsampling == JPEGGPU_EXT_SUBSAMPLING_420 ? 2 : 1;
    const int mh = f.ncomp == 1 ? 1 : hs, mv = f.ncomp == 1 ? 1 : vs; // the MCU in blocks of component 0
    f.app = 0xE0, f.ycc = true;
    f.dqt_n = f.ncomp == 1 ? 1 : 2;
    for (int t = 0; t < f.dqt_n; ++t) {
        uint8_t q[64];
        quant_table(t, it.quality, q);
        f.dqt[t].id = uint8_t(t);
        for (int k = 0; k < 64; ++k) f.dqt[t].q[k] = spec ? spec->qtable[t][k] : q[kNatural[k]];
    }
    for (int c = 0; c < f.ncomp; ++c) {
        // the factors that were asked for go into the frame header of a grey file too (Pillow sets them whatever the mode)
        f.comp[c].id = uint8_t(c + 1), f.comp[c].h = uint8_t(c ? 1 : spec ? spec->sampling0 >> 4 : hs), f.comp[c].v = uint8_t(c ? 1 : spec ? spec->sampling0 & 15 : vs);
        f.comp[c].tq = f.comp[c].select = uint8_t(c > 0);
        f.ch[c] = c ? 1 : mh, f.cv[c] = c ? 1 : mv;
        f.grid_w[c] = (it.width + 8 * mh / f.ch[c] - 1) / (8 * mh / f.ch[c]), f.grid_h[c] = (it.height + 8 * mv / f.cv[c] - 1) / (8 * mv / f.cv[c]);
    }
    f.interleaved_x = (it.width + 8 * mh - 1) / (8 * mh);
    return true;
}

/// jpeg_simple_progression's script (jcparam.c) as Pillow gets it: component (-1: all, interleaved), Ss, Se, Ah, Al.
const int kScriptRgb[10][5]  = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2},  {2, 1, 63, 0, 1}, {1, 1, 63, 0, 1}, {0, 6, 63, 0, 2},
                                {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {2, 1, 63, 1, 0}, {1, 1, 63, 1, 0}, {0, 1, 63, 1, 0}};
const int kScriptGrey[6][5] = {{0, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {0, 6, 63, 0, 2}, {0, 1, 63, 2, 1}, {0, 0, 0, 1, 0}, {0, 1, 63, 1, 0}};

/// The scans of a progressive item, the tables they bring and their headers, and what they add to its Geometry: the bound of
/// its unstuffed stream -- per scan its blocks at their most bits and less than a byte of padding ones per restart
/// segment --, its scan blocks, markers and slots. Three-component YCbCr gets the ten scans, a single component the six,
/// everything else jpeg_simple_progression's all-purpose script -- DC of all components interleaved (Al 1); per component
/// AC 1-5 (Al 2), AC 6-63 (Al 2), AC 1-63 (Ah 2, Al 1); the DC refinement; per component AC 1-63 (Ah 1, Al 0). A
/// component's scan runs over its real grid, its tables follow its selector.
void prog_script(const jpeggpu_ext_encode_item& it, const FileFrame& f, Geometry& g, ProgItem& pi)
{
    int script[kProgScans][5], n_scans = 0;
    const auto add = [&](int comp, int ss, int se, int ah, int al) {
        const int row[5] = {comp, ss, se, ah, al};
        std::memcpy(script[n_scans++], row, sizeof row);
    };
    if (f.ncomp == 1) {
        std::memcpy(script, kScriptGrey, sizeof kScriptGrey), n_scans = 6;
    } else if (f.ncomp == 3 && f.ycc) {
        std::memcpy(script, kScriptRgb, sizeof kScriptRgb), n_scans = 10;
    } else {
        add(-1, 0, 0, 0, 1);
        for (int c = 0; c < f.ncomp; ++c) add(c, 1, 5, 0, 2);
        for (int c = 0; c < f.ncomp; ++c) add(c, 6, 63, 0, 2);
        for (int c = 0; c < f.ncomp; ++c) add(c, 1, 63, 2, 1);
        add(-1, 0, 0, 1, 0);
        for (int c = 0; c < f.ncomp; ++c) add(c, 1, 63, 1, 0);
    }
    bool two = false; // the DC scan brings the tables its components select
    for (int c = 0; c < f.ncomp; ++c) two |= f.comp[c].select != 0;
    const uint64_t mcus = uint64_t(g.mcus_x) * g.mcus_y;
    pi         = ProgItem{};
    pi.scans_n = uint32_t(n_scans);
    uint64_t first = 0, marks = 0, bound = 0;
    int slot = 0;
    g.marker_bytes = 0;
    for (int s = 0; s < n_scans; ++s) {
        const int* row = script[s];
        ProgScan& sc   = pi.scans[s];
        sc.comp = row[0], sc.ss = row[1], sc.se = row[2], sc.ah = row[3], sc.al = row[4];
        const int c           = sc.comp < 0 ? 0 : sc.comp;
        const uint64_t blocks = sc.comp < 0 ? g.blocks : uint64_t(f.grid_w[c]) * f.grid_h[c];
        const uint64_t units  = sc.comp < 0 ? mcus : blocks; // what the restart interval counts in this scan
        const uint64_t segs   = it.restart_interval ? (units + it.restart_interval - 1) / it.restart_interval : 1;
        sc.blocks = int(blocks), sc.blocks_x = sc.comp < 0 ? f.interleaved_x : f.grid_w[c];
        sc.h = f.scan_h[c], sc.v = f.scan_v[c], sc.k0 = f.scan_k0[c];
        sc.first = uint32_t(first), sc.marks_before = uint32_t(marks);
        sc.tables = sc.ss == 0 ? (sc.ah ? 0 : sc.comp < 0 && two ? 2 : 1) : 1;
        sc.slot   = sc.tables ? slot : -1;
        for (int t = 0; t < sc.tables; ++t) pi.slot_class_id[slot++] = uint8_t(sc.ss == 0 ? t : 0x10 | f.comp[c].select);
        const int band = sc.se - sc.ss + 1;
        const int bits = sc.ss == 0 ? (sc.ah ? kProgDcRefineBits : kProgDcFirstBits) : sc.ah ? prog_ac_refine_bits(band) : prog_ac_first_bits(band);
        bound += (blocks * uint64_t(bits) + 7) / 8 + segs;
        first += blocks;
        marks += segs - 1;
        // DRI in front of the first SOS; then marker, length, Ns, (Cs, Td Ta) per component, Ss, Se, Ah Al
        uint32_t n = 0;
        if (s == 0 && it.restart_interval) {
            const uint8_t dri[6] = {0xFF, 0xDD, 0, 4, uint8_t(it.restart_interval >> 8), uint8_t(it.restart_interval)};
            std::memcpy(sc.sos, dri, 6);
            n = 6;
        }
        const int ns = sc.comp < 0 ? f.ncomp : 1;
        sc.sos[n++] = 0xFF, sc.sos[n++] = 0xDA, sc.sos[n++] = 0, sc.sos[n++] = uint8_t(6 + 2 * ns), sc.sos[n++] = uint8_t(ns);
        for (int a = 0; a < ns; ++a) {
            const int comp = sc.comp < 0 ? a : sc.comp;
            const int sel  = f.comp[comp].select;
            sc.sos[n++]    = f.comp[comp].id;
            sc.sos[n++]    = uint8_t(sc.ss == 0 ? (sc.ah == 0 ? sel << 4 : 0x00) : sel);
        }
        sc.sos[n++] = uint8_t(sc.ss), sc.sos[n++] = uint8_t(sc.se), sc.sos[n++] = uint8_t(sc.ah << 4 | sc.al);
        sc.sos_len  = n;
        g.marker_bytes += uint64_t(sc.tables) * 277 + n; // a DHT of 256 values: marker, length, class and id, 16 counts
    }
    pi.slots_n     = uint32_t(slot);
    g.slots        = slot;
    g.scan_blocks  = first;
    g.markers      = marks;
    g.stream_bound = bound;
}

/// `pi`: where a progressive item's script goes.
Geometry geometry(const jpeggpu_ext_encode_item& it, const FileFrame& f, ProgItem& pi)
{
    Geometry g{};
    int hmax = 1, vmax = 1; // the iMCU of the largest factors
    for (int c = 0; c < f.ncomp; ++c) {
        hmax = f.ch[c] > hmax ? f.ch[c] : hmax, vmax = f.cv[c] > vmax ? f.cv[c] : vmax;
        g.blocks_per_mcu += f.ch[c] * f.cv[c];
    }
    g.hs = f.ch[0], g.vs = f.cv[0];
    g.mcus_x = (it.width + 8 * hmax - 1) / (8 * hmax);
    g.mcus_y = (it.height + 8 * vmax - 1) / (8 * vmax);
    const uint64_t mcus = uint64_t(g.mcus_x) * g.mcus_y;
    g.blocks        = mcus * g.blocks_per_mcu;
    g.segments      = it.restart_interval ? (mcus + it.restart_interval - 1) / it.restart_interval : 1;
    // every block at kMaxBlockBits (optimised tables: a DC code of 16 bits), and less than a byte of padding ones per segment
    g.stream_bound = (g.blocks * (it.optimize ? kMaxBlockBitsOptimized : kMaxBlockBits) + 7) / 8 + g.segments;
    if (it.progressive) prog_script(it, f, g, pi);
    return g;
}

void put_segment(std::vector<uint8_t>& out, int marker, const uint8_t* payload, size_t len)
{
    out.push_back(0xFF);
    out.push_back(uint8_t(marker));
    out.push_back(uint8_t((len + 2) >> 8));
    out.push_back(uint8_t(len + 2));
    out.insert(out.end(), payload, payload + len);
}

/// The header as libjpeg writes it for Pillow, in the three parts an item with optimised tables needs: SOI .. SOFn (the
/// prefix), the DHTs, which for such an item the device writes, and DRI if any and SOS (the suffix). Each appends to `out`.
void write_prefix(const jpeggpu_ext_encode_item& it, const FileFrame& f, std::vector<uint8_t>& out)
{
    out.push_back(0xFF);
    out.push_back(0xD8);
    if (f.app == 0xE0) {
        static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
        put_segment(out, 0xE0, jfif, sizeof jfif);
    } else if (f.app == 0xEE) {
        const uint8_t adobe[12] = {'A', 'd', 'o', 'b', 'e', 0, 100, 0, 0, 0, 0, f.adobe_transform};
        put_segment(out, 0xEE, adobe, sizeof adobe);
    }
    bool sof1 = false;
    for (int t = 0; t < f.dqt_n; ++t) {
        uint8_t seg[1 + 128];
        size_t n = 0;
        seg[n++] = uint8_t((f.dqt[t].wide ? 0x10 : 0) | f.dqt[t].id);
        for (int k = 0; k < 64; ++k) {
            if (f.dqt[t].wide) seg[n++] = uint8_t(f.dqt[t].q[k] >> 8);
            seg[n++] = uint8_t(f.dqt[t].q[k]);
        }
        put_segment(out, 0xDB, seg, n);
        sof1 |= f.dqt[t].wide;
    }
    uint8_t sof[6 + 12] = {8, uint8_t(it.height >> 8), uint8_t(it.height), uint8_t(it.width >> 8), uint8_t(it.width), uint8_t(f.ncomp)};
    for (int c = 0; c < f.ncomp; ++c) {
        sof[6 + 3 * c] = f.comp[c].id;
        sof[7 + 3 * c] = uint8_t(f.comp[c].h << 4 | f.comp[c].v);
        sof[8 + 3 * c] = f.comp[c].tq;
    }
    put_segment(out, it.progressive ? 0xC2 : sof1 ? 0xC1 : 0xC0, sof, size_t(6 + 3 * f.ncomp));
}

void write_standard_dhts(const FileFrame& f, std::vector<uint8_t>& out)
{
    const HuffSpec* specs[4] = {&kDcLuma, &kAcLuma, &kDcChroma, &kAcChroma};
    const uint8_t ids[4]     = {0x00, 0x10, 0x01, 0x11};
    bool one                 = true; // no component selects tables 1
    for (int c = 0; c < f.ncomp; ++c) one &= f.comp[c].select == 0;
    for (int t = 0; t < (one ? 2 : 4); ++t) {
        uint8_t seg[1 + 16 + 162];
        seg[0] = ids[t];
        std::memcpy(seg + 1, specs[t]->bits, 16);
        std::memcpy(seg + 17, specs[t]->values, size_t(specs[t]->count));
        put_segment(out, 0xC4, seg, size_t(17 + specs[t]->count));
    }
}

void write_suffix(const jpeggpu_ext_encode_item& it, const FileFrame& f, std::vector<uint8_t>& out)
{
    if (it.restart_interval) {
        const uint8_t dri[2] = {uint8_t(it.restart_interval >> 8), uint8_t(it.restart_interval)};
        put_segment(out, 0xDD, dri, 2);
    }
    uint8_t sos[1 + 8 + 3] = {uint8_t(f.ncomp)};
    for (int c = 0; c < f.ncomp; ++c) sos[1 + 2 * c] = f.comp[c].id, sos[2 + 2 * c] = uint8_t(f.comp[c].select ? 0x11 : 0x00);
    sos[1 + 2 * f.ncomp] = 0x00, sos[2 + 2 * f.ncomp] = 0x3F, sos[3 + 2 * f.ncomp] = 0x00;
    put_segment(out, 0xDA, sos, size_t(4 + 2 * f.ncomp));
}

/// SOI .. the end of SOS with the Annex K tables: the header of an item without optimised tables, and the longest an
/// optimised one can get (its DHTs list at most the symbols these list: 12 categories, 162 AC symbols).
void write_header(const jpeggpu_ext_encode_item& it, const FileFrame& f, std::vector<uint8_t>& out)
{
    write_prefix(it, f, out);
    write_standard_dhts(f, out);
    write_suffix(it, f, out);
}

/// Where the 64 bytes of an item's DQT payloads lie in SOI .. SOF0 as write_prefix made it, 0: no such table.
void dqt_payloads(const uint8_t* prefix, size_t len, uint32_t at[2])
{
    at[0] = at[1] = 0u;
    for (size_t p = 2; p + 4 <= len && prefix[p] == 0xFF;) { // marker, length, and for a DQT the precision / id byte
        if (prefix[p + 1] == 0xDB && prefix[p + 4] < 2) at[prefix[p + 4]] = uint32_t(p + 5);
        p += 2 + (size_t(prefix[p + 2]) << 8 | prefix[p + 3]);
    }
}

} // namespace

jpeggpu_status make_plan(const jpeggpu_ext_encode_item* items, const TranscodeSpec* specs, int n, bool fit, bool sizes_only, CallPlan& out)
{
    if (!items || n <= 0 || n > 65535) return JPEGGPU_INVALID_ARGUMENT;
    Plan& plan = out.plan;
    plan       = Plan{};
    out.geo.resize(size_t(n));
    uint64_t tiles = 0, chunks = 0, header_bytes = 0, prog_tiles = 0, prog_chunks = 0;
    bool beyond = false; // an item the kernels cannot index: reported once every item has been found valid
    std::vector<uint8_t> part;
    ProgItem unkept;
    // what each item is: its frame, its geometry and, but for a query, its header and script -- each made once
    for (int i = 0; i < n; ++i) {
        const jpeggpu_ext_encode_item& it = items[i];
        const TranscodeSpec* spec         = specs ? specs + i : nullptr;
        FileFrame f;
        if (!valid(&it) || !file_frame(it, spec, f)) return JPEGGPU_INVALID_ARGUMENT;
        if (spec && spec->src.oriented) ++plan.oriented;
        const bool keep = it.progressive && !sizes_only;
        if (keep) out.prog.emplace_back();
        Geometry& g = out.geo[size_t(i)] = geometry(it, f, keep ? out.prog.back() : unkept);
        beyond |= g.stream_bound * 8 >= (uint64_t(1) << 32);
        tiles += (g.blocks + kTileBlocks - 1) / kTileBlocks;
        if (it.progressive) { // no header and no chunks among the call's: its stream lies in the progressive spaces
            ++plan.prog.n;
            plan.prog.slots = g.slots > plan.prog.slots ? g.slots : plan.prog.slots;
            prog_tiles += (g.scan_blocks + kTileBlocks - 1) / kTileBlocks;
            prog_chunks += (g.stream_bound + kChunkBytes - 1) / kChunkBytes;
            if (keep) {
                ProgItem& pi = out.prog.back();
                part.clear();
                write_prefix(it, f, part);
                if (part.size() > sizeof pi.prefix) return JPEGGPU_INTERNAL_ERROR;
                pi.prefix_len = uint32_t(part.size());
                std::memcpy(pi.prefix, part.data(), part.size());
            }
            continue;
        }
        chunks += (g.stream_bound + kChunkBytes - 1) / kChunkBytes;
        out.headers.resize(size_t(align_up(out.headers.size(), 16)));
        if (it.optimize) { // its OptState with the two parts of the header that the host knows
            ++plan.optimized;
            const size_t room = spec && spec->general ? size_t(kLongPrefixBytes) : 0; // (a long prefix is planned at its longest)
            g.header_bytes    = uint32_t(sizeof(OptState) + room);
            if (!sizes_only) {
                OptState st{}; // (counts, lengths and statuses zero: the device adds to them)
                part.clear();
                write_prefix(it, f, part);
                st.prefix_len = uint32_t(part.size());
                if (long_prefix(st.prefix_len) && part.size() > room) return JPEGGPU_INTERNAL_ERROR;
                const size_t at = out.headers.size();
                out.headers.resize(at + g.header_bytes);
                std::memcpy(long_prefix(st.prefix_len) ? out.headers.data() + at + sizeof st : st.prefix, part.data(), part.size()); // behind the state
                part.clear();
                write_suffix(it, f, part);
                if (part.size() > sizeof st.suffix) return JPEGGPU_INTERNAL_ERROR;
                st.suffix_len = uint32_t(part.size());
                std::memcpy(st.suffix, part.data(), part.size());
                std::memcpy(out.headers.data() + at, &st, sizeof st);
            }
        } else { // (a query writes it too, for its length)
            std::vector<uint8_t>& to = sizes_only ? part : out.headers;
            if (sizes_only) part.clear();
            const size_t at = to.size();
            write_header(it, f, to);
            g.header_bytes = uint32_t(to.size() - at);
        }
        header_bytes += align_up(g.header_bytes, 16);
    }
    if (beyond) return JPEGGPU_NOT_SUPPORTED;
    if (tiles * kTileBlocks >= (uint64_t(1) << 31) || chunks >= (uint64_t(1) << 31)) return JPEGGPU_NOT_SUPPORTED;
    if (prog_tiles * kTileBlocks >= (uint64_t(1) << 31) || prog_chunks >= (uint64_t(1) << 31)) return JPEGGPU_NOT_SUPPORTED;
    if (header_bytes + sizeof(Tables) + sizeof(Item) * (size_t(n) + 1) + 1024 >= (uint64_t(1) << 32)) return JPEGGPU_NOT_SUPPORTED; // header_off is 32 bits
    plan.n      = n;
    plan.tiles  = uint32_t(tiles);
    plan.chunks = uint32_t(chunks);
    uint64_t off = 0;
    auto take    = [&off](uint64_t bytes) {
        const uint64_t at = off;
        off               = align_up(off + bytes, 256);
        return at;
    };
    plan.tables_off       = take(sizeof(Tables));
    plan.items_off        = take(sizeof(Item) * (size_t(n) + 1)); // and a sentinel
    out.headers_off       = take(header_bytes);
    const uint64_t np     = uint64_t(plan.prog.n); // (a take of nothing leaves the offsets of a call without such items as they were)
    plan.prog.tiles       = uint32_t(prog_tiles);
    plan.prog.chunks      = uint32_t(prog_chunks);
    plan.prog.shadow_off  = take(np ? sizeof(Item) * (np + 1) : 0);
    plan.prog.items_off   = take(sizeof(ProgItem) * np);
    plan.gather_off       = take(specs ? sizeof(GatherSrc) * size_t(n) : 0);
    plan.fit_off          = take(fit ? sizeof(FitItem) * size_t(n) : 0);
    plan.blob_bytes       = off;
    plan.bits_off         = take(tiles * kTileBlocks * sizeof(uint32_t));
    plan.tile_sum_off     = take(tiles * sizeof(Cursor));
    plan.tile_before_off  = take(tiles * sizeof(Cursor));
    plan.count_off        = take(chunks * sizeof(Count));
    plan.count_before_off = take(chunks * sizeof(Count));
    plan.prog.bits_off         = take(prog_tiles * kTileBlocks * sizeof(uint32_t));
    plan.prog.facts_off        = take(prog_tiles * kTileBlocks);
    plan.prog.eobn_off         = take(prog_tiles * kTileBlocks * sizeof(uint16_t));
    plan.prog.tile_sum_off     = take(prog_tiles * sizeof(Cursor));
    plan.prog.tile_before_off  = take(prog_tiles * sizeof(Cursor));
    plan.prog.count_off        = take(prog_chunks * sizeof(Count));
    plan.prog.count_before_off = take(prog_chunks * sizeof(Count));
    // where each item's arrays lie, and with that its descriptors
    uint32_t tile = 0, chunk = 0, prog_tile = 0, prog_chunk = 0;
    uint64_t header_off = out.headers_off;
    if (!sizes_only) out.items.assign(size_t(n) + 1, Item{});
    if (!sizes_only && fit) out.fits.assign(size_t(n), FitItem{});
    for (int i = 0; i < n; ++i) {
        const Geometry& g       = out.geo[size_t(i)];
        const uint64_t chunks_i = (g.stream_bound + kChunkBytes - 1) / kChunkBytes;
        const uint64_t coef     = take(g.blocks * 128);
        const uint64_t stream   = take(chunks_i * kChunkBytes);
        const uint64_t starts   = take(chunks_i * (kChunkBytes / 8));
        const bool progressive  = items[i].progressive != 0;
        const uint64_t work     = progressive ? take(sizeof(ProgWork)) : items[i].optimize ? take(sizeof(OptWork)) : 0;
        const uint64_t raw      = take(fit ? g.blocks * 128 : 0);
        if (!sizes_only) {
            const jpeggpu_ext_encode_item& s = items[i];
            Item& d                          = out.items[size_t(i)];
            if (fit) out.fits[size_t(i)].raw_off = raw, out.fits[size_t(i)].blocks = int32_t(g.blocks);
            d.src = s.data, d.out = s.out, d.capacity = s.capacity;
            d.row_pitch = s.row_pitch, d.pixel_stride = s.pixel_stride, d.channel_stride = s.channel_stride;
            d.coef_off = coef, d.stream_off = stream, d.starts_off = starts;
            d.width = s.width, d.height = s.height, d.channels = s.channels;
            d.hs = g.hs, d.vs = g.vs, d.mcus_x = g.mcus_x, d.mcus_y = g.mcus_y;
            d.blocks_per_mcu = g.blocks_per_mcu, d.blocks = int(g.blocks);
            d.grid_w = (s.width + 7) / 8, d.grid_h = (s.height + 7) / 8;
            d.restart_interval = s.restart_interval;
            d.tile_start = tile, d.chunk_start = chunk;
            d.header_off = uint32_t(header_off), d.header_len = progressive ? kProgressiveHeader : s.optimize ? 0u : g.header_bytes;
            if (s.optimize && !progressive) std::memcpy(out.headers.data() + (header_off - out.headers_off) + offsetof(OptState, work_off), &work, sizeof work);
            if (specs && specs[i].general) { // nothing is quantised: hs 0 marks the item, and the frame lies in the divisors' place
                d.hs = d.vs = 0;
                d.frame     = specs[i].frame;
                d.grid_w = d.frame.grid_w[0], d.grid_h = d.frame.grid_h[0];
            } else {
                uint8_t q[64];
                for (int t = 0; t < 2; ++t) {
                    quant_table(t, s.quality, q);
                    for (int k = 0; k < 64; ++k) d.divisor[t][k] = uint16_t(8 * q[kNatural[k]]);
                }
            }
            if (progressive) {
                ProgItem& pi = out.prog[out.shadow.size()];
                pi.work_off  = work;
                pi.item      = uint32_t(i);
                out.shadow.push_back(d);
                out.shadow.back().tile_start  = prog_tile;
                out.shadow.back().chunk_start = prog_chunk;
            }
        }
        header_off += align_up(g.header_bytes, 16);
        tile += uint32_t((g.blocks + kTileBlocks - 1) / kTileBlocks);
        if (progressive) {
            prog_tile += uint32_t((g.scan_blocks + kTileBlocks - 1) / kTileBlocks);
            prog_chunk += uint32_t(chunks_i);
            continue;
        }
        chunk += uint32_t(chunks_i);
    }
    if (!sizes_only) {
        Item& s       = out.items[size_t(n)];
        s.tile_start  = tile;
        s.chunk_start = chunk;
        if (plan.prog.n) {
            out.shadow.push_back(Item{});
            out.shadow.back().tile_start  = prog_tile;
            out.shadow.back().chunk_start = prog_chunk;
        }
    }
    plan.total = off;
    return JPEGGPU_SUCCESS;
}

void fill_blob(const CallPlan& call, const jpeggpu_ext_encode_item* items, const TranscodeSpec* specs, const jpeggpu_ext_encode_fit_item* budgets,
               const uint8_t* base, uint8_t* h)
{
    const Plan& plan = call.plan;
    const int n      = plan.n;
    std::memset(h, 0, plan.blob_bytes);
    std::memcpy(h + plan.tables_off, &tables(), sizeof(Tables));
    Item* dev = reinterpret_cast<Item*>(h + plan.items_off);
    std::memcpy(dev, call.items.data(), sizeof(Item) * call.items.size());
    if (specs) { // each item's source behind the items, and where its capacity is kept a second time
        GatherSrc* srcs = reinterpret_cast<GatherSrc*>(h + plan.gather_off);
        for (int i = 0, k = 0; i < n; ++i) {
            srcs[i]            = specs[i].src;
            srcs[i].uncodable  = 0u;
            srcs[i].shadow_off = items[i].progressive ? uint32_t(plan.prog.shadow_off + sizeof(Item) * size_t(k++)) : 0u;
            dev[i].src         = base + plan.gather_off + sizeof(GatherSrc) * size_t(i);
        }
    }
    if (!call.headers.empty()) std::memcpy(h + call.headers_off, call.headers.data(), call.headers.size());
    if (plan.prog.n) {
        std::memcpy(h + plan.prog.shadow_off, call.shadow.data(), sizeof(Item) * call.shadow.size());
        std::memcpy(h + plan.prog.items_off, call.prog.data(), sizeof(ProgItem) * call.prog.size());
    }
    if (budgets) { // every search starts at quality_max, whose tables the items and headers above hold
        FitItem* fits = reinterpret_cast<FitItem*>(h + plan.fit_off);
        std::memcpy(fits, call.fits.data(), sizeof(FitItem) * call.fits.size());
        for (int i = 0; i < n; ++i) {
            FitItem& f  = fits[i];
            f.max_bytes = budgets[i].max_bytes;
            f.lo = budgets[i].quality_min, f.hi = f.q = budgets[i].quality_max;
            f.phase = kFitHigh;
            // the header a standard item has in the blob begins with the prefix; an optimised one keeps it in its state
            const uint32_t header_off = call.items[size_t(i)].header_off;
            const size_t prefix_at    = items[i].optimize ? offsetof(OptState, prefix) : 0;
            const size_t prefix_n     = items[i].optimize ? size_t(kPrefixBytes) : call.geo[size_t(i)].header_bytes;
            dqt_payloads(call.headers.data() + (header_off - call.headers_off) + prefix_at, prefix_n, f.dqt_off);
            for (int t = 0; t < 2; ++t)
                if (f.dqt_off[t]) f.dqt_off[t] += header_off + uint32_t(prefix_at);
        }
    }
}

size_t scratch_size_of(const jpeggpu_ext_encode_item* items, const TranscodeSpec* specs, int n, bool fit)
{
    try {
        CallPlan call;
        if (make_plan(items, specs, n, fit, true, call) != JPEGGPU_SUCCESS) return 0;
        return size_t(call.plan.total) + 256; // room to align the caller's pointer
    } catch (const std::bad_alloc&) {
        return 0;
    }
}

namespace {

/// The header calls behind their checks. `g`: the item's geometry, if the caller has it.
jpeggpu_status header_of(const jpeggpu_ext_encode_item& it, const FileFrame& f, const Geometry* g, uint8_t* host_buf, size_t* size)
{
    std::vector<uint8_t> header;
    try {
        if (it.progressive) { // every scan brings its tables: SOI .. SOF2 and what the scans' marker segments can take at most
            ProgItem pi;
            write_prefix(it, f, header);
            *size = header.size() + size_t(g ? g->marker_bytes : geometry(it, f, pi).marker_bytes);
            return JPEGGPU_NOT_SUPPORTED;
        }
        write_header(it, f, header);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    const size_t room = *size;
    *size             = header.size();
    if (it.optimize) return JPEGGPU_NOT_SUPPORTED; // its DHTs depend on the pixels; no header is longer than this one
    if (!host_buf) return JPEGGPU_SUCCESS;
    if (room < header.size()) return JPEGGPU_INVALID_ARGUMENT;
    std::memcpy(host_buf, header.data(), header.size());
    return JPEGGPU_SUCCESS;
}
jpeggpu_status header_of(const jpeggpu_ext_encode_item* item, const TranscodeSpec* spec, uint8_t* host_buf, size_t* size)
{
    FileFrame f;
    if (!valid(item) || !file_frame(*item, spec, f) || !size) return JPEGGPU_INVALID_ARGUMENT;
    return header_of(*item, f, nullptr, host_buf, size);
}

size_t bound_of(const jpeggpu_ext_encode_item* item, const TranscodeSpec* spec)
{
    FileFrame f;
    ProgItem pi;
    if (!valid(item) || !file_frame(*item, spec, f)) return 0;
    (void)tables(); // checks kMaxBlockBits against the tables
    const Geometry g = geometry(*item, f, pi);
    size_t header    = 0;
    const jpeggpu_status st = header_of(*item, f, &g, nullptr, &header);
    if (st != JPEGGPU_SUCCESS && !((item->optimize || item->progressive) && st == JPEGGPU_NOT_SUPPORTED)) return 0;
    // the header; the stream with every byte 0xFF and stuffed; a marker between segments (of every scan); EOI
    return header + 2 * size_t(g.stream_bound) + 2 * size_t(item->progressive ? g.markers : g.segments - 1) + 2;
}

/// The header, bound and scratch size of calls whose items become TranscodeSpecs through `make`.
template <class SrcItem>
jpeggpu_status spec_header(const SrcItem* item, jpeggpu_status (*make)(const SrcItem&, bool, TranscodeSpec&), uint8_t* host_buf, size_t* size)
{
    if (!item || !size) return JPEGGPU_INVALID_ARGUMENT;
    TranscodeSpec spec;
    const jpeggpu_status st = make(*item, false, spec);
    return st != JPEGGPU_SUCCESS ? st : header_of(&spec.item, &spec, host_buf, size);
}
template <class SrcItem>
size_t spec_bound(const SrcItem* item, jpeggpu_status (*make)(const SrcItem&, bool, TranscodeSpec&))
{
    TranscodeSpec spec;
    if (!item || make(*item, false, spec) != JPEGGPU_SUCCESS) return 0;
    return bound_of(&spec.item, &spec); // (an encoder layout's header is as long whatever its tables hold)
}
template <class SrcItem>
size_t spec_scratch_size(const SrcItem* items, int n, jpeggpu_status (*make)(const SrcItem&, bool, TranscodeSpec&))
{
    try {
        std::vector<TranscodeSpec> specs;
        std::vector<jpeggpu_ext_encode_item> enc;
        if (specs_of(items, n, false, make, specs, enc) != JPEGGPU_SUCCESS) return 0;
        return scratch_size_of(enc.data(), specs.data(), n, false);
    } catch (const std::bad_alloc&) {
        return 0;
    }
}

} // namespace
} // namespace enc
} // namespace jg

using namespace jg::enc;

extern "C" {

enum jpeggpu_status jpeggpu_ext_encode_header(const struct jpeggpu_ext_encode_item* item, uint8_t* host_buf, size_t* size)
{
    return header_of(item, nullptr, host_buf, size);
}
size_t jpeggpu_ext_encode_bound(const struct jpeggpu_ext_encode_item* item) { return bound_of(item, nullptr); }
size_t jpeggpu_ext_encode_scratch_size(const struct jpeggpu_ext_encode_item* items, int n) { return scratch_size_of(items, nullptr, n, false); }

enum jpeggpu_status jpeggpu_ext_transcode_header(const struct jpeggpu_ext_transcode_item* item, uint8_t* host_buf, size_t* size)
{
    return spec_header(item, transcode_spec, host_buf, size);
}
size_t jpeggpu_ext_transcode_bound(const struct jpeggpu_ext_transcode_item* item) { return spec_bound(item, transcode_spec); }
size_t jpeggpu_ext_transcode_scratch_size(const struct jpeggpu_ext_transcode_item* items, int n) { return spec_scratch_size(items, n, transcode_spec); }

enum jpeggpu_status jpeggpu_ext_write_coefficients_header(const struct jpeggpu_ext_coefficient_item* item, uint8_t* host_buf, size_t* size)
{
    return spec_header(item, coefficient_spec, host_buf, size);
}
size_t jpeggpu_ext_write_coefficients_bound(const struct jpeggpu_ext_coefficient_item* item) { return spec_bound(item, coefficient_spec); }
size_t jpeggpu_ext_write_coefficients_scratch_size(const struct jpeggpu_ext_coefficient_item* items, int n)
{
    return spec_scratch_size(items, n, coefficient_spec);
}

} // extern "C"
