// jg_encode_prog.hpp -- what the host plans for a progressive item and what the kernels of jg_encode_prog.hip keep for it.
// The file is libjpeg's jpeg_simple_progression script coded by jcphuff.c's rules: ten scans for three-component YCbCr, six
// for grey, and for a transcode item that keeps another frame (jg_encode.hpp: Frame) the all-purpose script of 2 + 4 n scans;
// every scan with Huffman tables made from its own symbol counts.
//
// The parallel unit is the SCAN BLOCK: one block of one scan. An item's scan blocks are numbered scan after scan, each scan
// in its own order -- MCU order over the padded grid for the two interleaved DC scans, the component's real blocks row by
// row for every other scan -- and cut into tiles of kTileBlocks like the blocks of a baseline item, in a tile space of the
// progressive items' own. The item's unstuffed stream is its scans' entropy-coded data one after the other; a scan's first
// block starts on a byte like a restart segment's.
#ifndef JG_ENCODE_PROG_HPP_
#define JG_ENCODE_PROG_HPP_

#include "jg_encode.hpp"

namespace jg {
namespace enc {

constexpr int kProgScans = 18; // four components: 2 + 4 * 4
constexpr int kProgSlots = 18; // Huffman tables of a file: up to two DC tables of the first scan, one AC table per AC scan
constexpr int kProgSlotsEncoder = 10; // what the pixel encoder's scripts need: the kernels' LDS follows the call's items (ProgPlan::slots)
/// jcphuff.c: an end-of-band run is sent when it reaches kMaxEobRun blocks, and in a refinement scan when more than
/// kMaxPendingBits correction bits wait behind it (MAX_CORR_BITS - DCTSIZE2 + 1).
constexpr uint32_t kMaxEobRun      = 0x7FFF;
constexpr uint32_t kMaxPendingBits = 937;

/// The most bits a block adds to a scan (every Huffman code at most 16 bits long):
///   DC first        a code and 11 value bits
///   DC refinement   one bit
///   AC first        per coefficient of the band a code and 10 value bits; a ZRL stands for 16 coefficients, an EOBn
///                   symbol (a code and 14 bits of run length) for at least one
///   AC refinement   per coefficient a code and a sign bit, or one correction bit; ZRL and EOBn as above
constexpr int kProgDcFirstBits  = 16 + 11;
constexpr int kProgDcRefineBits = 1;
constexpr int kProgEobBits      = 16 + 14;
constexpr int prog_ac_first_bits(int band) { return band * (16 + 10) + kProgEobBits; }
constexpr int prog_ac_refine_bits(int band) { return band * (16 + 1) + kProgEobBits; }

struct ProgScan {
    int comp;              // the scan's component, -1: all of them, interleaved
    int ss, se, ah, al;
    int blocks, blocks_x;  // the scan's blocks and, for a scan of one component, the width of its grid
    int h, v, k0;          // a `Frame` item's scan of one component: its blocks in an MCU, and the first one's place there
    uint32_t first;        // its first scan block among the item's
    int slot, tables;      // its first table and how many it brings: 2 (the first scan of RGB: luma, chroma), 1 or 0
    uint32_t marks_before; // restart markers of the scans in front of it
    uint32_t sos_len;
    uint8_t sos[24];       // the scan header; the first scan's follows the DRI segment here
};

/// One progressive item, in the blob. shadow[i] beside it is the call's Item with tile_start, chunk_start, stream_off and
/// starts_off in the progressive spaces.
struct ProgItem {
    uint64_t work_off;          // ProgWork, in d_scratch
    uint32_t item;              // its index in the call: where its size and status go
    uint32_t scans_n, slots_n;
    uint32_t prefix_len;
    uint8_t slot_class_id[kProgSlots + 2]; // the DHT's Tc << 4 | Th
    ProgScan scans[kProgScans];            // (in front of the prefix: what every lane reads stays within the struct's first lines)
    uint8_t prefix[kLongPrefixBytes + 2];  // SOI .. SOF2
};

/// What the device makes for a progressive item.
struct ProgWork {
    uint32_t counts[kProgSlots][256]; // zeroed by the first launch
    uint32_t codes[kProgSlots][256];  // code << 8 | length
    uint8_t dht[kProgSlots][kDhtBytes];
    uint32_t dht_len[kProgSlots], status[kProgSlots];
    uint32_t scan_pos[kProgScans]; // the byte of the unstuffed stream at which each scan begins
};

/// The launches of a call's progressive items, around the table launch that jg_encode.hip owns (build_table lives there):
/// front -- facts of every scan block, the end-of-band runs, the symbol counts; back -- bit counts, the stream, the files.
hipError_t launch_prog_front(const Plan& plan, uint8_t* d_scratch, hipStream_t stream);
hipError_t launch_prog_tables(const Plan& plan, uint8_t* d_scratch, hipStream_t stream);
hipError_t launch_prog_back(const Plan& plan, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, hipStream_t stream);

/// Stages of jg_encode.hip that the progressive items run on their shadow items as they are.
hipError_t launch_scan_tiles(const Cursor* tile_sum, Cursor* tile_before, uint32_t tiles, hipStream_t stream);
hipError_t launch_clear_streams(const Item* items, int n, uint32_t chunks, uint8_t* d_scratch, const Cursor* tile_sum, const Cursor* tile_before, hipStream_t stream);
/// count_bytes and the scan of its counts
hipError_t launch_count_bytes(const Item* items, int n, uint32_t chunks, const uint8_t* d_scratch, const Cursor* tile_sum, const Cursor* tile_before, Count* counts,
                              Count* count_before, hipStream_t stream);

} // namespace enc
} // namespace jg

#endif // JG_ENCODE_PROG_HPP_
