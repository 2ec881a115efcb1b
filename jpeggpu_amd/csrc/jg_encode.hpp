// jg_encode.hpp -- the encoder's tables and launch interface (jg_encode.hip; progressive items: jg_encode_prog.hpp; every launch is asynchronous on
// `stream`). The host (jg_encode.cpp) plans a call into one blob of descriptors that travels to the device in one copy; the
// kernels index everything by BLOCK (8 x 8 samples), the parallel unit of every stage.
#ifndef JG_ENCODE_HPP_
#define JG_ENCODE_HPP_

#include <hip/hip_runtime_api.h>

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

/// The progressive items of a call (jg_encode_prog.hpp): n of them, the tiles of their scan blocks and the chunks of their
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
    uint64_t gather_off;            // in the blob: GatherSrc[n] of a transcode call (jg_transcode.hpp), nothing otherwise
    uint64_t fit_off;               // in the blob: FitItem[n] of a budget call (jg_encode_fit.hpp), nothing otherwise
    uint64_t blob_bytes;
    uint64_t bits_off;        // uint32[tiles * kTileBlocks]
    uint64_t tile_sum_off;    // Cursor[tiles]: each tile's own function
    uint64_t tile_before_off; // Cursor[tiles]: everything before the tile, composed
    uint64_t count_off;       // Count[chunks]
    uint64_t count_before_off;
    uint64_t total;
};

/// `transcode`: every item's Item::src is its GatherSrc (jg_transcode.hpp); gather_blocks takes the place of encode_blocks and
/// finish_transcode follows the last launch.
hipError_t launch_encode(const Plan& plan, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, hipStream_t stream, bool transcode = false);

/// The parts of launch_encode behind its first launch, as a budget call enqueues them once per probe (jg_encode_fit.hip);
/// each returns the number of launches it enqueued. launch_table_stages: launches 1a and 1b if the call has an item with
/// optimised tables, else nothing. launch_size_stages: launches 2 - 7, after which every item's size is known on the
/// device. launch_write_files: launch 8.
int launch_table_stages(const Plan& plan, uint8_t* d_scratch, hipStream_t stream);
int launch_size_stages(const Plan& plan, uint8_t* d_scratch, hipStream_t stream);
int launch_write_files(const Plan& plan, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, hipStream_t stream);

/// jpeg_gen_optimal_table of n_tables x 256 counts: per table 16 `bits` bytes and 256 `values` bytes, and a status.
hipError_t launch_tables_from_counts(const uint32_t* d_counts, int n_tables, uint8_t* d_bits_values, int* d_status, hipStream_t stream);

} // namespace enc
} // namespace jg

#endif // JG_ENCODE_HPP_
