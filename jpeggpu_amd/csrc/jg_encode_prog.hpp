// jg_encode_prog.hpp -- the launches of a call's progressive items (their records, ProgItem and ProgWork: jg_encode_jobs.h).
// The file is libjpeg's jpeg_simple_progression script coded by jcphuff.c's rules: ten scans for three-component YCbCr, six
// for grey, and for a transcode item that keeps another frame (jg_encode_jobs.h: Frame) the all-purpose script of 2 + 4 n scans;
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
