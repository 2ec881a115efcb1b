// jg_transcode.hpp -- the lossless transcode's hand-over between the two halves of the library: what jg_transcode.cpp reads
// out of a decoded image (it knows the decoder) and what the encoder's plan and the gather kernel of jg_encode.hip need of it
// (they do not; the records are in jg_encode_jobs.h). A transcode item is an encoder Item whose coefficients come from the decoder's entropy stage instead of
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

/// jg_transcode.cpp: where component c of a parsed image lies in its d_tmp, for transcode_spec and the coefficient reader.
__attribute__((visibility("hidden"))) bool source_comp(const Decoder& d, uint8_t* tmp, int c, GatherComp& g, const Scan** scan);

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
