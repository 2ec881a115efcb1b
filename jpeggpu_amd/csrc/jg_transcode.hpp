// jg_transcode.hpp -- the lossless transcode's hand-over between the two halves of the library: what jg_transcode.cpp reads
// out of a decoded image (it knows the decoder) and what jg_encode.cpp and the gather kernel of jg_encode.hip need of it
// (they do not). A transcode item is an encoder Item whose coefficients come from the decoder's entropy stage instead of
// encode_blocks: everything behind the gather is the encoder as it is.
#ifndef JG_TRANSCODE_HPP_
#define JG_TRANSCODE_HPP_

#include <jpeggpu/jpeggpu.h>
#include <jpeggpu/jpeggpu_ext.h>

#include <cstdint>

#include "jg_encode.hpp"

namespace jg {
struct Decoder;
struct Scan;
namespace enc {

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
    Frame frame;           // what the kernels get (jg_encode.hpp), over the TARGET's grids
};

/// The spec of a transcode item: JPEGGPU_INVALID_ARGUMENT / JPEGGPU_NOT_SUPPORTED by the rules of jpeggpu_ext.h.
/// `need_device`: the pointers into d_tmp are wanted (the batch call), not only the geometry.
__attribute__((visibility("hidden"))) jpeggpu_status transcode_spec(const jpeggpu_ext_transcode_item& it, bool need_device, TranscodeSpec& spec);

/// jg_transcode.cpp: where component c of a parsed image lies in its d_tmp, for transcode_spec and the coefficient reader.
__attribute__((visibility("hidden"))) bool source_comp(const Decoder& d, uint8_t* tmp, int c, GatherComp& g, const Scan** scan);

/// The spec of a jpeggpu_ext_write_coefficients_ item (jg_coefficients.cpp): a transcode item whose source is the caller's
/// tensors -- GatherComp::coef over the REAL grids, blocks_x the real grid's width -- mapped with the identity, so that
/// gather_blocks<true> makes the dummy blocks the tensors do not hold.
__attribute__((visibility("hidden"))) jpeggpu_status coefficient_spec(const jpeggpu_ext_coefficient_item& it, bool need_device, TranscodeSpec& spec);

/// One item of jpeggpu_ext_read_coefficients_batch as read_blocks sees it: the source as a transcode item's, and per
/// component the caller's tensor over the real grid grid_w x grid_h, the component's first tile among the call's (a tile:
/// kReadTile consecutive blocks of ONE component's raster; tile_start[c] of a component the frame lacks, and [4], is the
/// item's end) and the factor of each coefficient in natural order: the quantisation table, or ones.
constexpr int kReadTile = kTileBlocks; // (64-block tiles were measured 4 % slower on 64 photographs: DESIGN.md section 7)
struct ReadItem {
    GatherSrc src;
    void* dst[4];
    uint32_t tile_start[5];
    int32_t grid_w[4], grid_h[4];
    uint32_t pad;
    uint16_t factor[4][64];
};
static_assert(sizeof(ReadItem) % 8 == 0, "ReadItem: an array of them keeps its pointers aligned");

/// jg_coefficients.cpp (it knows the decoder) makes the items, items[n] a sentinel whose tile_start[0] is the call's tile
/// count; jg_encode.cpp stages them through the encoder's ring and launches read_blocks (jg_encode.hip). `type`: enum
/// jpeggpu_ext_coefficient_type.
__attribute__((visibility("hidden"))) jpeggpu_status read_coefficients(const ReadItem* items, int n, int type, void* d_scratch, size_t scratch_size, hipStream_t stream);
hipError_t launch_read_blocks(const ReadItem* d_items, int n, uint32_t tiles, int type, hipStream_t stream);

} // namespace enc
} // namespace jg

#endif // JG_TRANSCODE_HPP_
