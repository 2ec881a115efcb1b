// jg_encode.cpp -- the encoder's part of the exported C ABI (include/jpeggpu/jpeggpu_ext.h): argument checks, the file
// header, the size bound and the plan of a call for the kernels of jg_encode.hip. It knows nothing of the decoder: of a
// transcode item it sees the TranscodeSpec that jg_transcode.cpp made of it (jg_transcode.hpp).
#include "jg_encode_fit.hpp"
#include "jg_encode_prog.hpp"
#include "jg_quant.h"
#include "jg_staging.hpp"
#include "jg_transcode.hpp"

#include <jpeggpu/jpeggpu.h>
#include <jpeggpu/jpeggpu_ext.h>

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

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
static_assert(sizeof(Item) == 392, "the scratch size of a call without optimised items is part of the interface");

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

/// `spec`: a transcode item's, which may keep a frame of its own (TranscodeSpec::general) of up to four components.
bool valid(const jpeggpu_ext_encode_item* it, const TranscodeSpec* spec = nullptr)
{
    const bool general = spec && spec->general;
    return it && it->width >= 1 && it->width <= 65535 && it->height >= 1 && it->height <= 65535 &&
           (general ? it->channels >= 1 && it->channels <= 4 : it->channels == 1 || it->channels == 3) &&
           it->quality >= 1 && it->quality <= 100 && it->subsampling >= JPEGGPU_EXT_SUBSAMPLING_444 && it->subsampling <= JPEGGPU_EXT_SUBSAMPLING_420 &&
           it->restart_interval >= 0 && it->restart_interval <= 65535 && (it->optimize == 0 || it->optimize == 1) &&
           (it->progressive == 0 || it->progressive == 1);
}

struct Geometry {
    int hs, vs, mcus_x, mcus_y, blocks_per_mcu;
    uint64_t blocks, segments, stream_bound;
    int slots;                                   // a progressive item's Huffman tables
    uint64_t scan_blocks, markers, marker_bytes; // a progressive item's: the blocks and restart markers of all its scans, DHTs + DRI + SOS at their longest
};

/// jpeg_simple_progression's script (jcparam.c) as Pillow gets it: component (-1: all, interleaved), Ss, Se, Ah, Al.
const int kScriptRgb[10][5]  = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2},  {2, 1, 63, 0, 1}, {1, 1, 63, 0, 1}, {0, 6, 63, 0, 2},
                                {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {2, 1, 63, 1, 0}, {1, 1, 63, 1, 0}, {0, 1, 63, 1, 0}};
const int kScriptGrey[6][5] = {{0, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {0, 6, 63, 0, 2}, {0, 1, 63, 2, 1}, {0, 0, 0, 1, 0}, {0, 1, 63, 1, 0}};

/// prog_script for a transcode item that keeps its source's frame: three-component YCbCr keeps the ten scans, a single
/// component the six, everything else gets jpeg_simple_progression's all-purpose script -- DC of all components interleaved
/// (Al 1); per component AC 1-5 (Al 2), AC 6-63 (Al 2), AC 1-63 (Ah 2, Al 1); the DC refinement; per component AC 1-63
/// (Ah 1, Al 0). A component's scan runs over its real grid, its tables follow its selector.
uint64_t general_prog_script(const jpeggpu_ext_encode_item& it, const Geometry& g, ProgItem& pi, uint64_t* scan_blocks, uint64_t* markers, uint64_t* marker_bytes,
                             const TranscodeSpec& spec)
{
    const Frame& f  = spec.frame;
    const int ncomp = it.channels;
    int script[kProgScans][5], n_scans = 0;
    const auto add = [&](int comp, int ss, int se, int ah, int al) {
        const int row[5] = {comp, ss, se, ah, al};
        std::memcpy(script[n_scans++], row, sizeof row);
    };
    if (ncomp == 1) {
        std::memcpy(script, kScriptGrey, sizeof kScriptGrey), n_scans = 6;
    } else if (ncomp == 3 && spec.color_space == JPEGGPU_EXT_COLOR_YCBCR) {
        std::memcpy(script, kScriptRgb, sizeof kScriptRgb), n_scans = 10;
    } else {
        add(-1, 0, 0, 0, 1);
        for (int c = 0; c < ncomp; ++c) add(c, 1, 5, 0, 2);
        for (int c = 0; c < ncomp; ++c) add(c, 6, 63, 0, 2);
        for (int c = 0; c < ncomp; ++c) add(c, 1, 63, 2, 1);
        add(-1, 0, 0, 1, 0);
        for (int c = 0; c < ncomp; ++c) add(c, 1, 63, 1, 0);
    }
    int k0[4] = {0, 0, 0, 0}, ch[4], cv[4];
    for (int c = 0, at = 0; c < ncomp; ++c) {
        ch[c] = f.hv >> (8 * c) & 15, cv[c] = f.hv >> (8 * c + 4) & 15;
        k0[c] = at;
        at += ch[c] * cv[c];
    }
    const uint64_t mcus = uint64_t(g.mcus_x) * g.mcus_y;
    pi         = ProgItem{};
    pi.scans_n = uint32_t(n_scans);
    uint64_t first = 0, marks = 0, bound = 0;
    int slot = 0;
    *marker_bytes = 0;
    for (int s = 0; s < n_scans; ++s) {
        const int* row = script[s];
        ProgScan& sc   = pi.scans[s];
        sc.comp = row[0], sc.ss = row[1], sc.se = row[2], sc.ah = row[3], sc.al = row[4];
        const int c           = sc.comp < 0 ? 0 : sc.comp;
        const uint64_t blocks = sc.comp < 0 ? g.blocks : uint64_t(f.grid_w[c]) * f.grid_h[c];
        const uint64_t units  = sc.comp < 0 ? mcus : blocks;
        const uint64_t segs   = it.restart_interval ? (units + it.restart_interval - 1) / it.restart_interval : 1;
        sc.blocks = int(blocks), sc.blocks_x = f.grid_w[c];
        sc.h = ch[c], sc.v = cv[c], sc.k0 = k0[c];
        sc.first = uint32_t(first), sc.marks_before = uint32_t(marks);
        const bool two = f.select != 0; // the DC scan brings the tables its components select
        sc.tables = sc.ss == 0 ? (sc.ah ? 0 : sc.comp < 0 && two ? 2 : 1) : 1;
        sc.slot   = sc.tables ? slot : -1;
        for (int t = 0; t < sc.tables; ++t) pi.slot_class_id[slot++] = uint8_t(sc.ss == 0 ? t : 0x10 | spec.comp[c].select);
        const int band = sc.se - sc.ss + 1;
        const int bits = sc.ss == 0 ? (sc.ah ? kProgDcRefineBits : kProgDcFirstBits) : sc.ah ? prog_ac_refine_bits(band) : prog_ac_first_bits(band);
        bound += (blocks * uint64_t(bits) + 7) / 8 + segs;
        first += blocks;
        marks += segs - 1;
        uint32_t n = 0;
        if (s == 0 && it.restart_interval) {
            const uint8_t dri[6] = {0xFF, 0xDD, 0, 4, uint8_t(it.restart_interval >> 8), uint8_t(it.restart_interval)};
            std::memcpy(sc.sos, dri, 6);
            n = 6;
        }
        const int ns = sc.comp < 0 ? ncomp : 1;
        sc.sos[n++] = 0xFF, sc.sos[n++] = 0xDA, sc.sos[n++] = 0, sc.sos[n++] = uint8_t(6 + 2 * ns), sc.sos[n++] = uint8_t(ns);
        for (int a = 0; a < ns; ++a) {
            const int comp = sc.comp < 0 ? a : sc.comp;
            const int sel  = spec.comp[comp].select;
            sc.sos[n++]    = spec.comp[comp].id;
            sc.sos[n++]    = uint8_t(sc.ss == 0 ? (sc.ah == 0 ? sel << 4 : 0x00) : sel);
        }
        sc.sos[n++] = uint8_t(sc.ss), sc.sos[n++] = uint8_t(sc.se), sc.sos[n++] = uint8_t(sc.ah << 4 | sc.al);
        sc.sos_len  = n;
        *marker_bytes += uint64_t(sc.tables) * 277 + n;
    }
    pi.slots_n   = uint32_t(slot);
    *scan_blocks = first;
    *markers     = marks;
    return bound;
}

/// The scans of a progressive item, the tables they bring and their headers; returns the bound of its unstuffed stream:
/// per scan its blocks at their most bits (jg_encode_prog.hpp) and less than a byte of padding ones per restart segment.
uint64_t prog_script(const jpeggpu_ext_encode_item& it, const Geometry& g, ProgItem& pi, uint64_t* scan_blocks, uint64_t* markers, uint64_t* marker_bytes,
                     const TranscodeSpec* spec = nullptr)
{
    if (spec && spec->general) return general_prog_script(it, g, pi, scan_blocks, markers, marker_bytes, *spec);
    const bool grey  = it.channels == 1;
    const int grid_w = (it.width + 7) / 8, grid_h = (it.height + 7) / 8;
    const uint64_t mcus = uint64_t(g.mcus_x) * g.mcus_y;
    pi               = ProgItem{};
    pi.scans_n       = grey ? 6 : 10;
    uint64_t first = 0, marks = 0, bound = 0;
    int slot = 0;
    *marker_bytes = 0;
    for (uint32_t s = 0; s < pi.scans_n; ++s) {
        const int* row = grey ? kScriptGrey[s] : kScriptRgb[s];
        ProgScan& sc   = pi.scans[s];
        sc.comp = row[0], sc.ss = row[1], sc.se = row[2], sc.ah = row[3], sc.al = row[4];
        const uint64_t blocks = sc.comp < 0 ? g.blocks : sc.comp == 0 ? uint64_t(grid_w) * grid_h : mcus;
        const uint64_t units  = sc.comp < 0 ? mcus : blocks; // what the restart interval counts in this scan
        const uint64_t segs   = it.restart_interval ? (units + it.restart_interval - 1) / it.restart_interval : 1;
        sc.blocks       = int(blocks);
        sc.blocks_x     = sc.comp == 0 ? grid_w : g.mcus_x;
        sc.first        = uint32_t(first);
        sc.marks_before = uint32_t(marks);
        sc.tables       = sc.ss == 0 ? (sc.ah ? 0 : grey ? 1 : 2) : 1;
        sc.slot         = sc.tables ? slot : -1;
        for (int t = 0; t < sc.tables; ++t) pi.slot_class_id[slot++] = uint8_t(sc.ss == 0 ? t : 0x10 | (sc.comp > 0));
        const int band  = sc.se - sc.ss + 1;
        const int bits  = sc.ss == 0 ? (sc.ah ? kProgDcRefineBits : kProgDcFirstBits) : sc.ah ? prog_ac_refine_bits(band) : prog_ac_first_bits(band);
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
        const int ns = sc.comp < 0 ? 3 : 1;
        sc.sos[n++] = 0xFF, sc.sos[n++] = 0xDA, sc.sos[n++] = 0, sc.sos[n++] = uint8_t(6 + 2 * ns), sc.sos[n++] = uint8_t(ns);
        for (int c = 0; c < ns; ++c) {
            const int comp = sc.comp < 0 ? c : sc.comp;
            sc.sos[n++]    = uint8_t(comp + 1);
            sc.sos[n++]    = uint8_t(sc.ss == 0 ? (sc.ah == 0 && comp ? 0x10 : 0x00) : comp > 0);
        }
        sc.sos[n++] = uint8_t(sc.ss), sc.sos[n++] = uint8_t(sc.se), sc.sos[n++] = uint8_t(sc.ah << 4 | sc.al);
        sc.sos_len  = n;
        *marker_bytes += uint64_t(sc.tables) * 277 + n; // a DHT of 256 values: marker, length, class and id, 16 counts
    }
    pi.slots_n   = uint32_t(slot);
    *scan_blocks = first;
    *markers     = marks;
    return bound;
}
Geometry geometry(const jpeggpu_ext_encode_item& it, const TranscodeSpec* spec = nullptr)
{
    Geometry g;
    const bool grey = it.channels == 1;
    g.hs            = !grey && it.subsampling != JPEGGPU_EXT_SUBSAMPLING_444 ? 2 : 1;
    g.vs            = !grey && it.subsampling == JPEGGPU_EXT_SUBSAMPLING_420 ? 2 : 1;
    g.mcus_x        = (it.width + 8 * g.hs - 1) / (8 * g.hs);
    g.mcus_y        = (it.height + 8 * g.vs - 1) / (8 * g.vs);
    g.blocks_per_mcu = grey ? 1 : g.hs * g.vs + 2;
    if (spec && spec->general) { // the iMCU of the largest factors (a single component's MCU is one block); hs 0 marks the item
        int hmax = 1, vmax = 1;
        g.blocks_per_mcu = 0;
        for (int c = 0; c < it.channels; ++c) {
            const int h = spec->frame.hv >> (8 * c) & 15, v = spec->frame.hv >> (8 * c + 4) & 15;
            hmax = h > hmax ? h : hmax, vmax = v > vmax ? v : vmax;
            g.blocks_per_mcu += h * v;
        }
        g.mcus_x = (it.width + 8 * hmax - 1) / (8 * hmax);
        g.mcus_y = (it.height + 8 * vmax - 1) / (8 * vmax);
        g.hs = g.vs = 0;
    }
    const uint64_t mcus = uint64_t(g.mcus_x) * g.mcus_y;
    g.blocks        = mcus * g.blocks_per_mcu;
    g.segments      = it.restart_interval ? (mcus + it.restart_interval - 1) / it.restart_interval : 1;
    // every block at kMaxBlockBits (optimised tables: a DC code of 16 bits), and less than a byte of padding ones per segment
    g.stream_bound = (g.blocks * (it.optimize ? kMaxBlockBitsOptimized : kMaxBlockBits) + 7) / 8 + g.segments;
    g.scan_blocks = g.markers = g.marker_bytes = 0;
    g.slots       = 0;
    if (it.progressive) {
        ProgItem pi;
        g.stream_bound = prog_script(it, g, pi, &g.scan_blocks, &g.markers, &g.marker_bytes, spec);
        g.slots        = int(pi.slots_n);
    }
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

/// SOI .. SOFn of a transcode item that keeps its source's frame (jpeggpu_ext.h: jpeggpu_ext_set_transcode_frame).
void write_general_prefix(const jpeggpu_ext_encode_item& it, std::vector<uint8_t>& out, const TranscodeSpec& spec)
{
    out.clear();
    out.push_back(0xFF);
    out.push_back(0xD8);
    const int cs = spec.color_space;
    if (cs == JPEGGPU_EXT_COLOR_GRAY || cs == JPEGGPU_EXT_COLOR_YCBCR) {
        static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
        put_segment(out, 0xE0, jfif, sizeof jfif);
    } else if (cs == JPEGGPU_EXT_COLOR_RGB || cs == JPEGGPU_EXT_COLOR_CMYK || cs == JPEGGPU_EXT_COLOR_YCCK) {
        const uint8_t adobe[12] = {'A', 'd', 'o', 'b', 'e', 0, 100, 0, 0, 0, 0, uint8_t(cs == JPEGGPU_EXT_COLOR_YCCK ? 2 : 0)};
        put_segment(out, 0xEE, adobe, sizeof adobe);
    }
    bool sof1 = false;
    for (int t = 0; t < spec.tables_n; ++t) {
        uint8_t seg[1 + 128];
        size_t n = 0;
        seg[n++] = uint8_t((spec.table16[t] ? 0x10 : 0) | spec.table_id[t]);
        for (int k = 0; k < 64; ++k) {
            if (spec.table16[t]) seg[n++] = uint8_t(spec.table[t][k] >> 8);
            seg[n++] = uint8_t(spec.table[t][k]);
        }
        put_segment(out, 0xDB, seg, n);
        sof1 |= spec.table16[t];
    }
    const int ncomp     = it.channels;
    uint8_t sof[6 + 12] = {8, uint8_t(it.height >> 8), uint8_t(it.height), uint8_t(it.width >> 8), uint8_t(it.width), uint8_t(ncomp)};
    for (int c = 0; c < ncomp; ++c) {
        sof[6 + 3 * c] = spec.comp[c].id;
        sof[7 + 3 * c] = uint8_t(spec.comp[c].h << 4 | spec.comp[c].v);
        sof[8 + 3 * c] = spec.comp[c].tq;
    }
    put_segment(out, it.progressive ? 0xC2 : sof1 ? 0xC1 : 0xC0, sof, size_t(6 + 3 * ncomp));
}

/// The header as libjpeg writes it for Pillow, in the three parts an item with optimised tables needs: SOI .. SOF0 (the
/// prefix), the DHTs, which for such an item the device writes, and DRI if any and SOS (the suffix).
/// `spec`: a transcode item's -- the source's quantisation tables and the sampling byte of its first component.
void write_prefix(const jpeggpu_ext_encode_item& it, std::vector<uint8_t>& out, const TranscodeSpec* spec = nullptr)
{
    if (spec && spec->general) return write_general_prefix(it, out, *spec);
    const int ncomp = it.channels;
    // the factors that were asked for go into the frame header of a grey file too (Pillow sets them whatever the mode); with
    // one component they change nothing else
    const int hs = it.subsampling != JPEGGPU_EXT_SUBSAMPLING_444 ? 2 : 1, vs = it.subsampling == JPEGGPU_EXT_SUBSAMPLING_420 ? 2 : 1;
    out.clear();
    out.push_back(0xFF);
    out.push_back(0xD8);
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    put_segment(out, 0xE0, jfif, sizeof jfif);
    for (int t = 0; t < (ncomp == 1 ? 1 : 2); ++t) {
        uint8_t q[64], seg[65];
        quant_table(t, it.quality, q);
        seg[0] = uint8_t(t);
        for (int k = 0; k < 64; ++k) seg[1 + k] = spec ? spec->qtable[t][k] : q[kNatural[k]];
        put_segment(out, 0xDB, seg, sizeof seg);
    }
    uint8_t sof[6 + 9] = {8, uint8_t(it.height >> 8), uint8_t(it.height), uint8_t(it.width >> 8), uint8_t(it.width), uint8_t(ncomp)};
    for (int c = 0; c < ncomp; ++c) {
        sof[6 + 3 * c] = uint8_t(c + 1);
        sof[7 + 3 * c] = uint8_t(c ? 0x11 : spec ? spec->sampling0 : hs << 4 | vs);
        sof[8 + 3 * c] = uint8_t(c == 0 ? 0 : 1);
    }
    put_segment(out, it.progressive ? 0xC2 : 0xC0, sof, size_t(6 + 3 * ncomp));
}

void write_standard_dhts(const jpeggpu_ext_encode_item& it, std::vector<uint8_t>& out, const TranscodeSpec* spec = nullptr)
{
    const int ncomp          = it.channels;
    const HuffSpec* specs[4] = {&kDcLuma, &kAcLuma, &kDcChroma, &kAcChroma};
    const uint8_t ids[4]     = {0x00, 0x10, 0x01, 0x11};
    const bool one           = spec && spec->general ? spec->frame.select == 0 : ncomp == 1; // no component selects tables 1
    for (int t = 0; t < (one ? 2 : 4); ++t) {
        uint8_t seg[1 + 16 + 162];
        seg[0] = ids[t];
        std::memcpy(seg + 1, specs[t]->bits, 16);
        std::memcpy(seg + 17, specs[t]->values, size_t(specs[t]->count));
        put_segment(out, 0xC4, seg, size_t(17 + specs[t]->count));
    }
}

void write_suffix(const jpeggpu_ext_encode_item& it, std::vector<uint8_t>& out, const TranscodeSpec* spec = nullptr)
{
    const int ncomp = it.channels;
    if (it.restart_interval) {
        const uint8_t dri[2] = {uint8_t(it.restart_interval >> 8), uint8_t(it.restart_interval)};
        put_segment(out, 0xDD, dri, 2);
    }
    uint8_t sos[1 + 8 + 3] = {uint8_t(ncomp)};
    for (int c = 0; c < ncomp; ++c) {
        sos[1 + 2 * c] = uint8_t(c + 1);
        sos[2 + 2 * c] = uint8_t(c == 0 ? 0x00 : 0x11);
        if (spec && spec->general) sos[1 + 2 * c] = spec->comp[c].id, sos[2 + 2 * c] = uint8_t(spec->comp[c].select ? 0x11 : 0x00);
    }
    sos[1 + 2 * ncomp] = 0x00, sos[2 + 2 * ncomp] = 0x3F, sos[3 + 2 * ncomp] = 0x00;
    put_segment(out, 0xDA, sos, size_t(4 + 2 * ncomp));
}

/// SOI .. the end of SOS with the Annex K tables: the header of an item without optimised tables, and the longest an
/// optimised one can get (its DHTs list at most the symbols these list: 12 categories, 162 AC symbols).
void write_header(const jpeggpu_ext_encode_item& it, std::vector<uint8_t>& out, const TranscodeSpec* spec = nullptr)
{
    write_prefix(it, out, spec);
    write_standard_dhts(it, out, spec);
    write_suffix(it, out, spec);
}

/// The plan of a call: every offset in d_scratch. JPEGGPU_NOT_SUPPORTED for an item or a call beyond the kernels' 32-bit
/// bit offsets and block indices. headers[i]: what goes to the blob at the item's header_off -- its header, or for an item
/// with optimised tables its OptState with the two parts of the header that the host knows.
/// What a call's progressive items add to the blob.
struct ProgBlob {
    std::vector<Item> shadow; // and a sentinel
    std::vector<ProgItem> items;
};

/// `specs`: the call is a transcode call and items[i] is specs[i].item.
/// `fit`: the call is a budget call (jg_encode_fit.hpp) -- its FitItem[n] in the blob and each item's unquantised transform
/// behind the item's other arrays; `fit_items`, if not null, receives where those lie and each item's blocks.
jpeggpu_status make_plan(const jpeggpu_ext_encode_item* items, int n, Plan& plan, std::vector<Item>* out_items, std::vector<std::vector<uint8_t>>* headers,
                         ProgBlob* prog, const TranscodeSpec* specs = nullptr, bool fit = false, std::vector<FitItem>* fit_items = nullptr)
{
    if (!items || n <= 0 || n > 65535) return JPEGGPU_INVALID_ARGUMENT;
    uint64_t tiles = 0, chunks = 0, header_bytes = 0, prog_tiles = 0, prog_chunks = 0;
    plan.prog = ProgPlan{};
    std::vector<Geometry> geo(static_cast<size_t>(n));
    std::vector<uint8_t> header, part;
    plan.optimized = 0;
    plan.oriented  = 0;
    for (int i = 0; i < n; ++i) {
        if (specs && specs[i].src.oriented) ++plan.oriented;
        if (!valid(&items[i], specs ? specs + i : nullptr)) return JPEGGPU_INVALID_ARGUMENT;
        geo[i] = geometry(items[i], specs ? specs + i : nullptr);
        if (geo[i].stream_bound * 8 >= (uint64_t(1) << 32)) return JPEGGPU_NOT_SUPPORTED;
        tiles += (geo[i].blocks + kTileBlocks - 1) / kTileBlocks;
        if (items[i].progressive) { // no header and no chunks among the call's: its stream lies in the progressive spaces
            ++plan.prog.n;
            plan.prog.slots = geo[i].slots > plan.prog.slots ? geo[i].slots : plan.prog.slots;
            prog_tiles += (geo[i].scan_blocks + kTileBlocks - 1) / kTileBlocks;
            prog_chunks += (geo[i].stream_bound + kChunkBytes - 1) / kChunkBytes;
            header.clear();
            if (headers) headers->push_back(header);
            continue;
        }
        chunks += (geo[i].stream_bound + kChunkBytes - 1) / kChunkBytes;
        if (items[i].optimize) {
            ++plan.optimized;
            header.assign(sizeof(OptState), 0);
            if (specs && specs[i].general) header.resize(sizeof(OptState) + size_t(kLongPrefixBytes)); // (planned at its longest)
            if (headers) {
                header.resize(sizeof(OptState));
                OptState st{}; // (counts, lengths and statuses zero: the device adds to them)
                write_prefix(items[i], part, specs ? specs + i : nullptr);
                if (part.size() > size_t(kLongPrefixBytes)) return JPEGGPU_INTERNAL_ERROR;
                st.prefix_len = uint32_t(part.size());
                if (long_prefix(st.prefix_len)) header.insert(header.end(), part.begin(), part.end()); // behind the state
                else std::memcpy(st.prefix, part.data(), part.size());
                part.clear();
                write_suffix(items[i], part, specs ? specs + i : nullptr);
                if (part.size() > sizeof st.suffix) return JPEGGPU_INTERNAL_ERROR;
                st.suffix_len = uint32_t(part.size());
                std::memcpy(st.suffix, part.data(), part.size());
                std::memcpy(header.data(), &st, sizeof st);
                if (specs && specs[i].general) header.resize(sizeof(OptState) + size_t(kLongPrefixBytes));
            }
        } else {
            write_header(items[i], header, specs ? specs + i : nullptr);
        }
        header_bytes += align_up(header.size(), 16);
        if (headers) headers->push_back(header);
    }
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
    uint64_t header_off   = take(header_bytes);
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
    uint32_t tile = 0, chunk = 0, prog_tile = 0, prog_chunk = 0;
    if (out_items) out_items->resize(size_t(n) + 1);
    if (fit_items) fit_items->assign(size_t(n), FitItem{});
    for (int i = 0; i < n; ++i) {
        const Geometry& g       = geo[i];
        const uint64_t chunks_i = (g.stream_bound + kChunkBytes - 1) / kChunkBytes;
        const uint64_t coef     = take(g.blocks * 128);
        const uint64_t stream   = take(chunks_i * kChunkBytes);
        const uint64_t starts   = take(chunks_i * (kChunkBytes / 8));
        const bool progressive  = items[i].progressive != 0;
        const uint64_t work     = progressive ? take(sizeof(ProgWork)) : items[i].optimize ? take(sizeof(OptWork)) : 0;
        const uint64_t raw      = take(fit ? g.blocks * 128 : 0);
        if (fit_items) (*fit_items)[size_t(i)].raw_off = raw, (*fit_items)[size_t(i)].blocks = int32_t(g.blocks);
        if (out_items) {
            const jpeggpu_ext_encode_item& s = items[i];
            Item& d                          = (*out_items)[i];
            d                                = Item{};
            d.src = s.data, d.out = s.out, d.capacity = s.capacity;
            d.row_pitch = s.row_pitch, d.pixel_stride = s.pixel_stride, d.channel_stride = s.channel_stride;
            d.coef_off = coef, d.stream_off = stream, d.starts_off = starts;
            d.width = s.width, d.height = s.height, d.channels = s.channels;
            d.hs = g.hs, d.vs = g.vs, d.mcus_x = g.mcus_x, d.mcus_y = g.mcus_y;
            d.blocks_per_mcu = g.blocks_per_mcu, d.blocks = int(g.blocks);
            d.grid_w = (s.width + 7) / 8, d.grid_h = (s.height + 7) / 8;
            d.restart_interval = s.restart_interval;
            d.tile_start = tile, d.chunk_start = chunk;
            d.header_off = uint32_t(header_off), d.header_len = progressive ? kProgressiveHeader : s.optimize ? 0u : uint32_t((*headers)[i].size());
            if (s.optimize && !progressive) std::memcpy((*headers)[i].data() + offsetof(OptState, work_off), &work, sizeof work);
            uint8_t q[64];
            for (int t = 0; t < 2; ++t) {
                quant_table(t, s.quality, q);
                for (int k = 0; k < 64; ++k) d.divisor[t][k] = uint16_t(8 * q[kNatural[k]]);
            }
            if (specs && specs[i].general) { // nothing is quantised: the frame lies in the divisors' place
                std::memset(d.divisor, 0, sizeof d.divisor);
                d.frame  = specs[i].frame;
                d.grid_w = d.frame.grid_w[0], d.grid_h = d.frame.grid_h[0];
            }
            header_off += align_up((*headers)[i].size(), 16);
            if (progressive && prog) {
                Item sh        = d;
                sh.tile_start  = prog_tile;
                sh.chunk_start = prog_chunk;
                prog->shadow.push_back(sh);
                ProgItem pi;
                uint64_t a, b, c;
                prog_script(s, g, pi, &a, &b, &c, specs ? specs + i : nullptr);
                pi.work_off = work;
                pi.item     = uint32_t(i);
                std::vector<uint8_t> prefix;
                write_prefix(s, prefix, specs ? specs + i : nullptr);
                if (prefix.size() > sizeof pi.prefix) return JPEGGPU_INTERNAL_ERROR;
                pi.prefix_len = uint32_t(prefix.size());
                std::memcpy(pi.prefix, prefix.data(), prefix.size());
                prog->items.push_back(pi);
            }
        }
        tile += uint32_t((g.blocks + kTileBlocks - 1) / kTileBlocks);
        if (progressive) {
            prog_tile += uint32_t((g.scan_blocks + kTileBlocks - 1) / kTileBlocks);
            prog_chunk += uint32_t(chunks_i);
            continue;
        }
        chunk += uint32_t(chunks_i);
    }
    if (out_items) {
        Item& s       = (*out_items)[size_t(n)];
        s             = Item{};
        s.tile_start  = tile;
        s.chunk_start = chunk;
        if (prog && plan.prog.n) {
            s.tile_start  = prog_tile;
            s.chunk_start = prog_chunk;
            prog->shadow.push_back(s);
            s.tile_start  = tile;
            s.chunk_start = chunk;
        }
    }
    plan.total = off;
    return JPEGGPU_SUCCESS;
}

/// Page-locked staging of a call's blob: a ring of four per process, as the resize calls keep theirs. Never destroyed (the
/// HIP runtime may be gone when static objects are).
struct Staging {
    static constexpr int kRing = 4;
    std::mutex mu;
    StagingBuffer buf[kRing];
    hipEvent_t copied[kRing] = {};
    bool in_use[kRing]       = {};
    int next                 = 0;
};
Staging& staging()
{
    static Staging* s = new Staging;
    return *s;
}

} // namespace

/// jpeggpu_ext_read_coefficients_batch behind its checks: the items through the staging ring, one launch.
jpeggpu_status read_coefficients(const ReadItem* items, int n, int type, void* d_scratch, size_t scratch_size, hipStream_t stream)
{
    const size_t bytes = sizeof(ReadItem) * (size_t(n) + 1);
    uint8_t* base      = reinterpret_cast<uint8_t*>(jg::align_up(reinterpret_cast<uintptr_t>(d_scratch), 256));
    if (size_t(base - static_cast<uint8_t*>(d_scratch)) + bytes > scratch_size) return JPEGGPU_INVALID_ARGUMENT;
    Staging& rs = staging();
    std::lock_guard<std::mutex> lock(rs.mu);
    const int r = rs.next;
    if (rs.in_use[r] && hipEventSynchronize(rs.copied[r]) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    rs.in_use[r] = false;
    if (!rs.buf[r].reserve(bytes)) return JPEGGPU_OUT_OF_HOST_MEMORY;
    std::memcpy(rs.buf[r].ptr, items, bytes);
    if (!rs.copied[r] && hipEventCreateWithFlags(&rs.copied[r], hipEventDisableTiming) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    if (hipMemcpyAsync(base, rs.buf[r].ptr, bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    if (hipEventRecord(rs.copied[r], stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    rs.in_use[r] = true;
    rs.next      = (r + 1) % Staging::kRing;
    if (launch_read_blocks(reinterpret_cast<const ReadItem*>(base), n, items[n].tile_start[0], type, stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    return JPEGGPU_SUCCESS;
}

} // namespace enc
} // namespace jg

using namespace jg::enc;

extern "C" {

static jpeggpu_status header_of(const jpeggpu_ext_encode_item* item, const TranscodeSpec* spec, uint8_t* host_buf, size_t* size)
{
    if (!valid(item, spec) || !size) return JPEGGPU_INVALID_ARGUMENT;
    std::vector<uint8_t> header;
    try {
        write_header(*item, header, spec);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    const size_t room = *size;
    *size             = header.size();
    if (item->progressive) { // every scan brings its tables: SOI .. SOF2 and what the scans' marker segments can take at most
        write_prefix(*item, header, spec);
        *size = header.size() + size_t(geometry(*item, spec).marker_bytes);
        return JPEGGPU_NOT_SUPPORTED;
    }
    if (item->optimize) return JPEGGPU_NOT_SUPPORTED; // its DHTs depend on the pixels; no header is longer than this one
    if (!host_buf) return JPEGGPU_SUCCESS;
    if (room < header.size()) return JPEGGPU_INVALID_ARGUMENT;
    std::memcpy(host_buf, header.data(), header.size());
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_encode_header(const struct jpeggpu_ext_encode_item* item, uint8_t* host_buf, size_t* size)
{
    return header_of(item, nullptr, host_buf, size);
}

static size_t bound_of(const jpeggpu_ext_encode_item* item, const TranscodeSpec* spec)
{
    if (!valid(item, spec)) return 0;
    (void)tables(); // checks kMaxBlockBits against the tables
    const Geometry g = geometry(*item, spec);
    size_t header    = 0;
    const jpeggpu_status st = header_of(item, spec, nullptr, &header);
    if (st != JPEGGPU_SUCCESS && !((item->optimize || item->progressive) && st == JPEGGPU_NOT_SUPPORTED)) return 0;
    // the header; the stream with every byte 0xFF and stuffed; a marker between segments (of every scan); EOI
    return header + 2 * size_t(g.stream_bound) + 2 * size_t(item->progressive ? g.markers : g.segments - 1) + 2;
}

size_t jpeggpu_ext_encode_bound(const struct jpeggpu_ext_encode_item* item) { return bound_of(item, nullptr); }

size_t jpeggpu_ext_encode_scratch_size(const struct jpeggpu_ext_encode_item* items, int n)
{
    Plan plan;
    try {
        if (make_plan(items, n, plan, nullptr, nullptr, nullptr) != JPEGGPU_SUCCESS) return 0;
    } catch (const std::bad_alloc&) {
        return 0;
    }
    return size_t(plan.total) + 256; // room to align the caller's pointer
}

/// Where the 64 bytes of an item's DQT payloads lie in SOI .. SOF0 as write_prefix made it, 0: no such table.
static void dqt_payloads(const uint8_t* prefix, size_t len, uint32_t at[2])
{
    at[0] = at[1] = 0u;
    for (size_t p = 2; p + 4 <= len && prefix[p] == 0xFF;) { // marker, length, and for a DQT the precision / id byte
        if (prefix[p + 1] == 0xDB && prefix[p + 4] < 2) at[prefix[p + 4]] = uint32_t(p + 5);
        p += 2 + (size_t(prefix[p + 2]) << 8 | prefix[p + 3]);
    }
}

/// jpeggpu_ext_encode_batch, and with `specs` (items[i] is specs[i].item) jpeggpu_ext_transcode_batch; with `fit`
/// (items[i] is fit[i].item at quality_max) jpeggpu_ext_encode_fit_batch.
static jpeggpu_status batch_of(const jpeggpu_ext_encode_item* items, const TranscodeSpec* specs, int n, void* d_scratch, size_t scratch_size, size_t* d_sizes,
                               int* d_status, jpeggpu_stream_t stream, const jpeggpu_ext_encode_fit_item* fit = nullptr, int* d_quality = nullptr)
{
    if (!items || n <= 0 || !d_scratch || !d_sizes || !d_status) return JPEGGPU_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i)
        if (!valid(&items[i], specs ? specs + i : nullptr) || (!specs && !items[i].data) || (!items[i].out && items[i].capacity)) return JPEGGPU_INVALID_ARGUMENT;
    Plan plan;
    std::vector<Item> dev;
    std::vector<std::vector<uint8_t>> headers;
    ProgBlob prog;
    std::vector<FitItem> fits;
    try {
        const jpeggpu_status st = make_plan(items, n, plan, &dev, &headers, &prog, specs, fit != nullptr, fit ? &fits : nullptr);
        if (st != JPEGGPU_SUCCESS) return st;
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    uint8_t* base = reinterpret_cast<uint8_t*>(jg::align_up(reinterpret_cast<uintptr_t>(d_scratch), 256));
    if (size_t(base - static_cast<uint8_t*>(d_scratch)) + plan.total > scratch_size) return JPEGGPU_INVALID_ARGUMENT;

    Staging& rs = staging();
    std::lock_guard<std::mutex> lock(rs.mu);
    const int r = rs.next;
    // the staging buffer may still be the source of a copy enqueued kRing calls ago
    if (rs.in_use[r] && hipEventSynchronize(rs.copied[r]) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    rs.in_use[r] = false;
    if (!rs.buf[r].reserve(plan.blob_bytes)) return JPEGGPU_OUT_OF_HOST_MEMORY;
    uint8_t* h = rs.buf[r].ptr;
    std::memset(h, 0, plan.blob_bytes);
    std::memcpy(h + plan.tables_off, &tables(), sizeof(Tables));
    if (specs) { // each item's source behind the items, and where its capacity is kept a second time
        GatherSrc* srcs = reinterpret_cast<GatherSrc*>(h + plan.gather_off);
        for (int i = 0, k = 0; i < n; ++i) {
            srcs[i]            = specs[i].src;
            srcs[i].uncodable  = 0u;
            srcs[i].shadow_off = items[i].progressive ? uint32_t(plan.prog.shadow_off + sizeof(Item) * size_t(k++)) : 0u;
            dev[i].src         = base + plan.gather_off + sizeof(GatherSrc) * size_t(i);
        }
    }
    std::memcpy(h + plan.items_off, dev.data(), sizeof(Item) * dev.size());
    for (int i = 0; i < n; ++i) std::memcpy(h + dev[i].header_off, headers[i].data(), headers[i].size());
    if (plan.prog.n) {
        std::memcpy(h + plan.prog.shadow_off, prog.shadow.data(), sizeof(Item) * prog.shadow.size());
        std::memcpy(h + plan.prog.items_off, prog.items.data(), sizeof(ProgItem) * prog.items.size());
    }
    int probes = 0;
    if (fit) { // every search starts at quality_max, whose tables the items and headers above hold
        int widest = 1;
        for (int i = 0; i < n; ++i) {
            FitItem& f  = fits[size_t(i)];
            f.max_bytes = fit[i].max_bytes;
            f.lo = fit[i].quality_min, f.hi = f.q = fit[i].quality_max;
            f.phase = kFitHigh;
            // the header a standard item has in the blob begins with the prefix; an optimised one keeps it in its state
            const size_t prefix_at = items[i].optimize ? offsetof(OptState, prefix) : 0;
            const size_t prefix_n  = items[i].optimize ? size_t(kPrefixBytes) : headers[size_t(i)].size();
            dqt_payloads(headers[size_t(i)].data() + prefix_at, prefix_n, f.dqt_off);
            for (int t = 0; t < 2; ++t)
                if (f.dqt_off[t]) f.dqt_off[t] += dev[size_t(i)].header_off + uint32_t(prefix_at);
            widest = f.hi - f.lo + 1 > widest ? f.hi - f.lo + 1 : widest;
        }
        probes = fit_probes(widest);
        std::memcpy(h + plan.fit_off, fits.data(), sizeof(FitItem) * fits.size());
    }
    if (!rs.copied[r] && hipEventCreateWithFlags(&rs.copied[r], hipEventDisableTiming) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    if (hipMemcpyAsync(base, h, plan.blob_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    if (hipEventRecord(rs.copied[r], stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    rs.in_use[r] = true;
    rs.next      = (r + 1) % Staging::kRing;
    if (fit) {
        int launched = 0;
        if (launch_encode_fit(plan, probes, base, reinterpret_cast<unsigned long long*>(d_sizes), d_status, d_quality, stream, &launched) != hipSuccess ||
            launched != fit_launches(probes, plan.optimized != 0))
            return JPEGGPU_INTERNAL_ERROR;
        return JPEGGPU_SUCCESS;
    }
    if (launch_encode(plan, base, reinterpret_cast<unsigned long long*>(d_sizes), d_status, stream, specs != nullptr) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_encode_batch(
    const struct jpeggpu_ext_encode_item* items, int n, void* d_scratch, size_t scratch_size, size_t* d_sizes, int* d_status, jpeggpu_stream_t stream)
{
    return batch_of(items, nullptr, n, d_scratch, scratch_size, d_sizes, d_status, stream);
}

} // extern "C"

namespace jg {
namespace enc {

size_t encode_fit_scratch(const jpeggpu_ext_encode_item* items, int n)
{
    Plan plan;
    try {
        if (make_plan(items, n, plan, nullptr, nullptr, nullptr, nullptr, true) != JPEGGPU_SUCCESS) return 0;
    } catch (const std::bad_alloc&) {
        return 0;
    }
    return size_t(plan.total) + 256; // room to align the caller's pointer
}

jpeggpu_status encode_fit_batch(const jpeggpu_ext_encode_item* items, const jpeggpu_ext_encode_fit_item* fit, int n, void* d_scratch, size_t scratch_size,
                                size_t* d_sizes, int* d_status, int* d_quality, hipStream_t stream)
{
    return batch_of(items, nullptr, n, d_scratch, scratch_size, d_sizes, d_status, stream, fit, d_quality);
}

} // namespace enc
} // namespace jg

extern "C" {

/// The specs of a transcode call and their encoder items side by side.
static jpeggpu_status specs_of(const jpeggpu_ext_transcode_item* items, int n, bool need_device, std::vector<TranscodeSpec>& specs,
                               std::vector<jpeggpu_ext_encode_item>& enc)
{
    if (!items || n <= 0 || n > 65535) return JPEGGPU_INVALID_ARGUMENT;
    specs.resize(size_t(n));
    enc.resize(size_t(n));
    for (int i = 0; i < n; ++i) {
        const jpeggpu_status st = transcode_spec(items[i], need_device, specs[size_t(i)]);
        if (st != JPEGGPU_SUCCESS) return st;
        enc[size_t(i)] = specs[size_t(i)].item;
    }
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_transcode_header(const struct jpeggpu_ext_transcode_item* item, uint8_t* host_buf, size_t* size)
{
    if (!item || !size) return JPEGGPU_INVALID_ARGUMENT;
    TranscodeSpec spec;
    const jpeggpu_status st = transcode_spec(*item, false, spec);
    return st != JPEGGPU_SUCCESS ? st : header_of(&spec.item, &spec, host_buf, size);
}

size_t jpeggpu_ext_transcode_bound(const struct jpeggpu_ext_transcode_item* item)
{
    TranscodeSpec spec;
    if (!item || transcode_spec(*item, false, spec) != JPEGGPU_SUCCESS) return 0;
    return bound_of(&spec.item, spec.general ? &spec : nullptr); // (an encoder layout's header is as long whatever its tables hold)
}

size_t jpeggpu_ext_transcode_scratch_size(const struct jpeggpu_ext_transcode_item* items, int n)
{
    Plan plan;
    try {
        std::vector<TranscodeSpec> specs;
        std::vector<jpeggpu_ext_encode_item> enc;
        if (specs_of(items, n, false, specs, enc) != JPEGGPU_SUCCESS) return 0;
        if (make_plan(enc.data(), n, plan, nullptr, nullptr, nullptr, specs.data()) != JPEGGPU_SUCCESS) return 0;
    } catch (const std::bad_alloc&) {
        return 0;
    }
    return size_t(plan.total) + 256;
}

enum jpeggpu_status jpeggpu_ext_transcode_batch(
    const struct jpeggpu_ext_transcode_item* items, int n, void* d_scratch, size_t scratch_size, size_t* d_sizes, int* d_status, jpeggpu_stream_t stream)
{
    if (!d_scratch || !d_sizes || !d_status) return JPEGGPU_INVALID_ARGUMENT;
    try {
        std::vector<TranscodeSpec> specs;
        std::vector<jpeggpu_ext_encode_item> enc;
        const jpeggpu_status st = specs_of(items, n, true, specs, enc);
        if (st != JPEGGPU_SUCCESS) return st;
        return batch_of(enc.data(), specs.data(), n, d_scratch, scratch_size, d_sizes, d_status, stream);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
}

/// The specs of a jpeggpu_ext_write_coefficients_ call and their encoder items side by side (jg_coefficients.cpp: coefficient_spec).
static jpeggpu_status coefficient_specs_of(const jpeggpu_ext_coefficient_item* items, int n, bool need_device, std::vector<TranscodeSpec>& specs,
                                           std::vector<jpeggpu_ext_encode_item>& enc)
{
    if (!items || n <= 0 || n > 65535) return JPEGGPU_INVALID_ARGUMENT;
    specs.resize(size_t(n));
    enc.resize(size_t(n));
    for (int i = 0; i < n; ++i) {
        const jpeggpu_status st = coefficient_spec(items[i], need_device, specs[size_t(i)]);
        if (st != JPEGGPU_SUCCESS) return st;
        enc[size_t(i)] = specs[size_t(i)].item;
    }
    return JPEGGPU_SUCCESS;
}

enum jpeggpu_status jpeggpu_ext_write_coefficients_header(const struct jpeggpu_ext_coefficient_item* item, uint8_t* host_buf, size_t* size)
{
    if (!item || !size) return JPEGGPU_INVALID_ARGUMENT;
    TranscodeSpec spec;
    const jpeggpu_status st = coefficient_spec(*item, false, spec);
    return st != JPEGGPU_SUCCESS ? st : header_of(&spec.item, &spec, host_buf, size);
}

size_t jpeggpu_ext_write_coefficients_bound(const struct jpeggpu_ext_coefficient_item* item)
{
    TranscodeSpec spec;
    if (!item || coefficient_spec(*item, false, spec) != JPEGGPU_SUCCESS) return 0;
    return bound_of(&spec.item, spec.general ? &spec : nullptr);
}

size_t jpeggpu_ext_write_coefficients_scratch_size(const struct jpeggpu_ext_coefficient_item* items, int n)
{
    Plan plan;
    try {
        std::vector<TranscodeSpec> specs;
        std::vector<jpeggpu_ext_encode_item> enc;
        if (coefficient_specs_of(items, n, false, specs, enc) != JPEGGPU_SUCCESS) return 0;
        if (make_plan(enc.data(), n, plan, nullptr, nullptr, nullptr, specs.data()) != JPEGGPU_SUCCESS) return 0;
    } catch (const std::bad_alloc&) {
        return 0;
    }
    return size_t(plan.total) + 256;
}

enum jpeggpu_status jpeggpu_ext_write_coefficients_batch(
    const struct jpeggpu_ext_coefficient_item* items, int n, void* d_scratch, size_t scratch_size, size_t* d_sizes, int* d_status, jpeggpu_stream_t stream)
{
    if (!d_scratch || !d_sizes || !d_status) return JPEGGPU_INVALID_ARGUMENT;
    try {
        std::vector<TranscodeSpec> specs;
        std::vector<jpeggpu_ext_encode_item> enc;
        const jpeggpu_status st = coefficient_specs_of(items, n, true, specs, enc);
        if (st != JPEGGPU_SUCCESS) return st;
        return batch_of(enc.data(), specs.data(), n, d_scratch, scratch_size, d_sizes, d_status, stream);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
}

enum jpeggpu_status jpeggpu_ext_encode_tables_from_counts(const uint32_t* d_counts, int n_tables, uint8_t* d_bits_values, int* d_status, jpeggpu_stream_t stream)
{
    if (!d_counts || n_tables <= 0 || !d_bits_values || !d_status) return JPEGGPU_INVALID_ARGUMENT;
    if (launch_tables_from_counts(d_counts, n_tables, d_bits_values, d_status, stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    return JPEGGPU_SUCCESS;
}

} // extern "C"
