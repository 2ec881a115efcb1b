// jg_encode_jobs.h -- the records of the encoder: what the host plan (jg_encode_plan.cpp) builds and the kernels
// (jg_encode.hip, jg_encode_prog.hip, jg_encode_fit.hip) read, with the tile and bound arithmetic both sides count by, and
// the hand-over of a transcode item (jg_transcode.cpp makes it, the plan reads it). Free of HIP: a plain C++ compiler reads
// it. The launch interfaces are in jg_encode.hpp, jg_encode_prog.hpp, jg_encode_fit.hpp and jg_transcode.hpp.
#ifndef JG_ENCODE_JOBS_H_
#define JG_ENCODE_JOBS_H_

#include <jpeggpu/jpeggpu.h>
#include <jpeggpu/jpeggpu_ext.h>

#include <cstddef>
#include <cstdint>

namespace jg {
namespace enc {

/// A workgroup of the block kernels owns a TILE of kTileBlocks consecutive blocks of ONE item's MCU stream (an item's first
/// tile starts a new tile: `tile_start`). A workgroup of the byte kernels owns a CHUNK of kChunkBytes bytes of one item's
/// unstuffed stream, kChunkLane bytes per lane. The two scans between the stages are one workgroup of kScanThreads lanes
/// each, every lane walking a run of consecutive tiles (chunks).
constexpr int kTileBlocks  = 256;
constexpr int kChunkLane   = 32;
constexpr int kChunkBytes  = 256 * kChunkLane;
constexpr int kScanThreads = 128;

/// The longest a block can get, from the longest codes of the four tables (Annex K.3 - K.6): a DC code of at most 11 bits
/// (chroma, category 11) with 11 value bits, and 63 AC coefficients of at most a 16-bit code with 10 value bits each. A
/// ZRL or an EOB replaces coefficients and is shorter than what it replaces (ZRL: 11 bits for 16 coefficients).
constexpr int kMaxDcCode    = 11;
constexpr int kMaxAcCode    = 16;
constexpr int kMaxBlockBits = kMaxDcCode + 11 + 63 * (kMaxAcCode + 10); // 1660
/// With optimised tables (jpeg_gen_optimal_table limits every code to 16 bits) a DC code can be 16 bits long as well.
constexpr int kMaxBlockBitsOptimized = 16 + 11 + 63 * (16 + 10); // 1665

/// Position in the unstuffed stream as a function of the position before: what a run of blocks does to the bit cursor.
/// A segment's first block starts on a byte, so the functions are  x + a  (kAdd),  roundup8(x + a) + b  (kRound) and the
/// constant b (kConst: an item's first tile, whatever came before). They are closed under composition, which makes the
/// segmented scan of the bit counts an ordinary scan.
enum CursorKind : uint32_t { kAdd = 0, kRound = 1, kConst = 2 };
struct Cursor {
    uint32_t kind, a, b;
};
/// 0xFF bytes and segment starts of a run of chunks; `reset`: the run begins a new item.
struct Count {
    uint32_t reset, ff, starts;
};

/// The frame of a transcode item that keeps its source's layout (jpeggpu_ext_set_transcode_frame), where the pixel encoder's
/// three layouts do not describe it: Item::hs == 0 marks such an item, and the description lies where a pixel item keeps its
/// divisors, so sizeof(Item) stays what it is. Components' blocks follow each other in the MCU, each component's row by row.
/// The two maps are whole 64-bit words: a uniform load reaches them, and a lane shifts out the entry of its block.
struct Frame {
    uint64_t map;        // 6 bits per block of the MCU: component | xo << 2 | yo << 4 (the block's place among its component's)
    uint64_t last;       // 4 bits per block of the MCU: the blocks of its component in an MCU, less one
    uint32_t hv;         // 8 bits per component: h | v << 4
    uint8_t ncomp;
    uint8_t select;      // bit c: component c is coded with Huffman tables 1 (else tables 0)
    uint8_t pad[2];
    int32_t grid_w[4], grid_h[4]; // each component's real blocks: beyond them a block of an MCU is a dummy
};
constexpr int kMaxMcuBlocks = 10;

/// One image of a call, as the kernels see it.
struct Item {
    const uint8_t* src;
    uint8_t* out;
    uint64_t capacity;
    int64_t row_pitch, pixel_stride, channel_stride;
    uint64_t coef_off;   // byte offsets in d_scratch: int16[blocks][64], zigzag order, MCU stream order
    uint64_t stream_off; // the unstuffed stream, chunks * kChunkBytes, zeroed up to its length by the device
    uint64_t starts_off; // one bit per byte of the unstuffed stream: a restart segment begins here
    int width, height, channels;
    int hs, vs;           // luma blocks per MCU, 1 x 1 for grey; 0, 0: the layout is `frame`'s
    int mcus_x, mcus_y;
    int blocks_per_mcu, blocks;
    int grid_w, grid_h;   // the luma component's real blocks: beyond them a block of an MCU is a dummy
    int restart_interval; // MCUs, 0: none
    uint32_t tile_start, chunk_start; // this item's first tile / chunk among the call's
    uint32_t header_off, header_len;  // in the blob. header_len 0: an item with optimised tables, header_off its OptState
    union {
        uint16_t divisor[2][64];      // 8 * quantiser, zigzag order: luma, chroma
        Frame frame;                  // hs == 0 (a transcode item: nothing is quantised)
    };
};
static_assert(sizeof(Item) == 392, "the scratch size of a call without optimised items is part of the interface");

/// Encoder tables in the blob: code << 8 | length, index = table * 256 + symbol (DC: the category), tables luma, chroma.
struct Tables {
    uint32_t dc[2 * 16];
    uint32_t ac[2 * 256];
};

/// Symbol counts of one table as the kernels keep them: 16 DC categories, then 256 AC symbols.
constexpr int kDcSymbols    = 16;
constexpr int kTableCounts  = kDcSymbols + 256;
constexpr int kDhtBytes     = 280; // a DHT segment of 256 values: marker and length (4), class / id, 16 bits, the values: 277
constexpr int kPrefixBytes  = 192; // SOI, APP0, two DQTs, SOF0 of three components: 177
constexpr int kSuffixBytes  = 32;  // DRI, SOS of three components: 20; of four: 22
/// What the device makes for an item with optimised tables, outside the blob: its own Tables and its DHT segments
/// (DC0, AC0, DC1, AC1; a grey item has the first two), each as it stands in the file.
struct OptWork {
    Tables tables;
    uint8_t dht[4][kDhtBytes];
};
/// The state of an item with optimised tables, in the blob: the host zeroes it and writes the two parts of the header
/// that do not depend on the pixels; count_symbols adds into `counts`, build_tables writes the rest.
struct OptState {
    uint32_t counts[2][kTableCounts]; // luma, chroma (Cb and Cr share a table)
    uint32_t dht_len[4];              // bytes of OptWork::dht[t], 0: no such table
    uint32_t table_status[4];         // jpeggpu_ext_encode_status of each table: 0, or 2 (a code length above 32)
    uint32_t prefix_len, suffix_len;
    uint64_t work_off;                // OptWork, in d_scratch
    uint8_t prefix[kPrefixBytes];     // SOI .. SOF0; a prefix_len above kPrefixBytes (a `frame` item: up to four DQTs of
                                      // 16-bit entries) lies in the blob behind this struct instead
    uint8_t suffix[kSuffixBytes];     // DRI if any, SOS
};
/// The longest SOI .. SOFn: APP0, four DQTs of 16-bit entries, four components.
constexpr int kLongPrefixBytes = 2 + 18 + 4 * 133 + 22;
/// Where an item's prefix lies: host (make_plan) and device (write_files) go through this one rule.
constexpr bool long_prefix(uint32_t prefix_len) { return prefix_len > uint32_t(kPrefixBytes); }
static_assert(kLongPrefixBytes > kPrefixBytes && kSuffixBytes >= 6 + 16, "a long prefix exists, and DRI with an SOS of four components fits the suffix");

/// Item::header_len of a progressive item. The baseline stages pass over it: its tiles hold only its coefficients, it has
/// no chunks among the call's, and jg_encode_prog.hip codes its scans in tiles and chunks of their own (ProgPlan).
constexpr uint32_t kProgressiveHeader = 0xFFFFFFFFu;

/// The progressive items of a call (ProgItem below): n of them, the tiles of their scan blocks and the chunks of their
/// streams, counted apart from the call's, and where their arrays sit in d_scratch. All zero without such an item.
struct ProgPlan {
    int n;
    int slots;              // the most Huffman tables an item has: what the scan-block kernels keep in LDS
    uint32_t tiles, chunks;
    uint64_t shadow_off, items_off; // in the blob: Item[n + 1] (tile_start, chunk_start and the stream in these spaces), ProgItem[n]
    uint64_t bits_off;              // uint32[tiles * kTileBlocks]
    uint64_t facts_off;             // uint8[tiles * kTileBlocks]
    uint64_t eobn_off;              // uint16[tiles * kTileBlocks]
    uint64_t tile_sum_off, tile_before_off, count_off, count_before_off; // as the Plan's
};

/// Where the parts of a call sit in d_scratch (byte offsets; the blob is copied from the host, the rest the device's).
struct Plan {
    int n;
    int optimized; // items with optimised tables: none, and the call is the eight launches it always was
    int oriented;  // a transcode call's items with an orientation (GatherSrc::oriented): none, and the gather is the one it always was
    ProgPlan prog;
    uint32_t tiles, chunks;
    uint64_t tables_off, items_off; // in the blob
    uint64_t gather_off;            // in the blob: GatherSrc[n] of a transcode call, nothing otherwise
    uint64_t fit_off;               // in the blob: FitItem[n] of a budget call, nothing otherwise
    uint64_t blob_bytes;
    uint64_t bits_off;        // uint32[tiles * kTileBlocks]
    uint64_t tile_sum_off;    // Cursor[tiles]: each tile's own function
    uint64_t tile_before_off; // Cursor[tiles]: everything before the tile, composed
    uint64_t count_off;       // Count[chunks]
    uint64_t count_before_off;
    uint64_t total;
};

// ---- progressive items (jg_encode_prog.hpp) ------------------------------------------------------

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

// ---- budget calls (jg_encode_fit.hpp) ------------------------------------------------------------

/// Where an item's search stands. In the blob, behind the call's other descriptors; the device moves it on.
enum FitPhase : int32_t {
    kFitHigh   = 0, // the probe under way is quality_max
    kFitLow    = 1, // .. quality_min
    kFitBisect = 2, // .. (a + b) / 2
    kFitDone   = 3  // `q` is the chosen quality
};
struct FitItem {
    uint64_t raw_off;    // in d_scratch: int16[blocks][64], the unquantised transform (8 times the DCT), zigzag order, MCU
                         // stream order, a dummy block's AC zero
    uint64_t max_bytes;
    uint32_t dqt_off[2]; // in the blob: the 64 bytes of the item's DQT payloads (luma, chroma), 0: the file has no such table
    int32_t lo, hi;      // quality_min, quality_max
    int32_t a, b, best;  // the bisection's state
    int32_t q;           // the quality of the probe under way: the item's divisors and DQT bytes are this quality's
    int32_t phase;       // FitPhase
    int32_t over;        // 1: even quality_min exceeds max_bytes
    int32_t blocks;      // Item::blocks, which is 0 while a finished item sits out the remaining probes
    int32_t pad;
};
static_assert(sizeof(FitItem) == 64, "FitItem[n] follows the blob's 256-byte grid");

/// Evaluations of size() that the rule needs at most for a range of `widest` qualities: 1 for one quality, 2 for two,
/// else quality_max, quality_min and the bisection of widest - 2 values: 2 + floor(log2(widest - 2)) + 1. 9 for 1..100.
inline int fit_probes(int widest)
{
    if (widest <= 2) return widest < 1 ? 1 : widest;
    int steps = 0;
    for (int m = widest - 2; m; m >>= 1) ++steps;
    return 2 + steps;
}

/// Launches of a budget call: the transform; per probe the requantiser, the table stages if an item has optimised tables
/// (2), the size stages (6) and the decision; then the final pass: requantiser, table stages, size stages, write_files and
/// the report. 10 + 8 probes, with optimised tables 12 + 10 probes -- whatever n and the image sizes are.
inline int fit_launches(int probes, bool optimized) { return optimized ? 12 + 10 * probes : 10 + 8 * probes; }

// ---- transcode items (jg_transcode.hpp) ----------------------------------------------------------

/// Where the blocks of one component of the source lie in the decoder's d_tmp.
///   baseline source     the symbol stream and data-unit table of the scan that codes the component (jg_defs.h): block
///                       (bx, by) of the component is data unit  mcu * du_per_mcu + k0 + dy * h + dx  of an interleaved scan
///                       (mcu over the frame's MCU grid, so dummy blocks are units like any other), and unit
///                       by * vis_x + bx  of a scan of the component alone, which codes the real blocks only; a mapped item
///                       counts both from GatherSrc::first_unit (a decode that kept only some restart segments)
///   progressive source  the component's coefficient array: int16[64] per block in natural order, raster over the MCU-padded
///                       grid `blocks_x` wide (jg_prog_core.h); the blocks no scan wrote are the zeros the decode began with
struct GatherComp {
    const uint16_t* sym;
    const void* du_tab;   // uint2_t[]: {first entry, count | flags}
    uint64_t sym_limit;   // a record's first entry is clamped to this: 127 + 8 entries from there stay inside the buffer
    const int16_t* coef;  // progressive source (then sym is NULL)
    int32_t blocks_x;     // progressive source: the array's row length in blocks
    int32_t interleaved;  // baseline source: the scan holds other components too
    int32_t du_per_mcu, k0, h, v, mcus_x;
    int32_t vis_x, vis_y; // the component's real blocks
    int32_t dst_x, dst_y; // the TARGET's real blocks of the component (a mapped item: the mirrors run over them)
    // jpeggpu_ext_set_transcode_crop: the block of that grid where the written file's grid begins (in what was padding: the
    // struct keeps its size, and a frame of 65535 pixels has 8192 blocks)
    int16_t off_x, off_y;
};
static_assert(sizeof(GatherComp) == 80, "GatherComp: the crop's offsets lie in its padding");

/// One item's source, in the call's blob behind the items (Item::src points at it, in d_scratch).
struct GatherSrc {
    GatherComp comp[4];
    // a progressive item's shadow Item in d_scratch (its capacity is what prog_write_files tests), else 0. 32 bits of a 64-bit
    // plan offset: the shadow items lie in the blob, which make_plan keeps below 4 GB (its test for Item::header_off)
    uint32_t shadow_off;
    uint32_t uncodable;  // set by the gather: the source holds a coefficient the target cannot code
    // jpeggpu_ext_set_transcode_orientation other than 1 or jpeggpu_ext_set_transcode_crop (`oriented`: the item is mapped):
    // block (bx, by) of the written component grid is block (bx + off_x, by + off_y) of the uncropped target's, and that is
    // the source's block at  x = mirror_x ? dst_x - 1 - bx : bx,  y = mirror_y ? dst_y - 1 - by : by  (the DISPLAYED axes of
    // jpeggpu_ext.h's table), x and y exchanged with `transpose`; the coefficients follow (gather_blocks). The target's
    // dummy blocks are then the encoder's (encode_blocks), whatever the source holds beyond its grid.
    uint8_t oriented, transpose, mirror_x, mirror_y;
    // a mapped item of a baseline source whose decode kept only some restart segments (jpeggpu_ext_set_crop; Scan::first_mcu):
    // the frame's data unit that is unit 0 of du_tab. Such a file has one scan, so one number serves its components.
    int32_t first_unit;
};
static_assert(sizeof(GatherSrc) == 4 * sizeof(GatherComp) + 16, "GatherSrc: four components and four words");

/// What jg_transcode.cpp says of one item: the encoder's item (geometry, options, slot; `data` and `quality` unused), the
/// header's tables and sampling byte, the source.
struct TranscodeSpec {
    jpeggpu_ext_encode_item item;
    uint8_t qtable[2][64]; // zigzag order, as a DQT segment holds them: luma, chroma
    uint8_t sampling0;     // the frame header's sampling-factor byte of component 0
    GatherSrc src;
    // jpeggpu_ext_set_transcode_frame(SOURCE) on a source outside the encoder's layouts: the file keeps the source's frame.
    // `item` then carries the component count in `channels`, and the header and the geometry are made of what follows.
    bool general;
    int color_space;       // enum jpeggpu_ext_color_space
    struct Comp {
        uint8_t id, h, v, tq, select; // as written: the factors exchanged by a transposing orientation
    } comp[4];
    int tables_n;          // the DQT segments, in the order written
    uint8_t table_id[4];
    bool table16[4];       // Pq = 1: an entry above 255
    uint16_t table[4][64]; // zigzag order (transposed by a transposing orientation)
    Frame frame;           // what the kernels get, over the TARGET's grids
};

/// The spec of a transcode item (jg_transcode.cpp): JPEGGPU_INVALID_ARGUMENT / JPEGGPU_NOT_SUPPORTED by the rules of
/// jpeggpu_ext.h. `need_device`: the pointers into d_tmp are wanted (the batch call), not only the geometry.
__attribute__((visibility("hidden"))) jpeggpu_status transcode_spec(const jpeggpu_ext_transcode_item& it, bool need_device, TranscodeSpec& spec);

/// The spec of a jpeggpu_ext_write_coefficients_ item (jg_coefficients.cpp): a transcode item whose source is the caller's
/// tensors -- GatherComp::coef over the REAL grids, blocks_x the real grid's width -- mapped with the identity, so that
/// gather_blocks<true> makes the dummy blocks the tensors do not hold.
__attribute__((visibility("hidden"))) jpeggpu_status coefficient_spec(const jpeggpu_ext_coefficient_item& it, bool need_device, TranscodeSpec& spec);

} // namespace enc
} // namespace jg

#endif // JG_ENCODE_JOBS_H_
