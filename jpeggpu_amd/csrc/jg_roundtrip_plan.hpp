// jg_roundtrip_plan.hpp -- the host plan of a JPEG round trip (jpeggpu_ext_roundtrip_batch; jg_roundtrip_plan.cpp): every
// check of a call's arguments, each item's geometry and quantisation tables, the tiles of the block kernel, the scratch
// layout, and the second stage as a batched conversion of jg_output_plan.hpp. Free of HIP: jg_output.cpp runs a plan on the
// device, tests/emu/roundtrip_plan_check_main.cpp runs the planning under sanitizers without one.
#ifndef JG_ROUNDTRIP_PLAN_HPP_
#define JG_ROUNDTRIP_PLAN_HPP_

#include "jg_output_plan.hpp"

#include <jpeggpu/jpeggpu.h>
#include <jpeggpu/jpeggpu_ext.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace jg {
namespace rt {

/// A workgroup of roundtrip_blocks owns a TILE of kTileBlocks consecutive blocks of ONE item, one lane per block; an item's
/// first tile starts a new tile (`tile_start`), as in the encoder.
constexpr int kTileBlocks = 256;

/// One image of a call, as the kernel sees it. Its blocks are counted component by component, each component's REAL blocks
/// row by row: luma's grid_w x grid_h, then (RGB) Cb's and Cr's mcus_x x mcus_y.
struct Item {
    const uint8_t* src;
    uint8_t* dst;         // grey: the item's output, pitch[0] bytes between rows; RGB: not read (the planes are the output)
    int64_t row_pitch, pixel_stride, channel_stride;
    uint64_t plane_off[3]; // RGB: byte offsets in d_scratch of the component planes, whole blocks of pitch[c > 0] bytes a row
    int pitch[2];          // luma, chroma: multiples of 16 (grey: [0] is the caller's dst_pitch)
    int width, height, channels;
    int hs, vs;           // input samples per chroma sample; 1 x 1 for grey
    int grid_w, grid_h;   // luma's real blocks: ceil(width / 8) x ceil(height / 8)
    int mcus_x, mcus_y;   // each chroma component's real blocks: ceil(width / 8 hs) x ceil(height / 8 vs)
    int blocks;
    uint32_t tile_start;  // this item's first tile among the call's
    uint16_t quant[2][64]; // jpeg_set_quality's tables, natural order: luma, chroma
};

/// Where everything of one call sits in d_scratch, counted from its 256-aligned start: the batched conversion's staged part
/// for the RGB items (RgbBatchLayout of their number; nothing without one), the Item[n] -- together `head` bytes, staged and
/// copied --, then the planes of each RGB item.
struct Plan {
    std::vector<Item> items;
    std::vector<jpeggpu_img_info> infos; // of the RGB items, in their order: three components, hs x vs, 1 x 1, 1 x 1
    std::vector<jpeggpu_img> imgs;       // their planes in d_scratch
    std::vector<jpeggpu_ext_rgb_item> rgb_items;
    RgbBatchPlan rgb;                    // the second stage (planned only with an RGB item)
    int n_rgb      = 0;
    uint32_t tiles = 0;
    size_t off_items = 0, head = 0, total = 0;
};

/// Geometry and tables of one item (checked: sides, channels, quality, subsampling); nothing of it depends on pointers.
void item_geometry(const jpeggpu_ext_roundtrip_item& s, Item& it);

/// Every check of a call, and its plan. `base`: the 256-aligned start of the scratch (the planes' addresses go into the
/// second stage's descriptors; the size call passes an address that nothing dereferences and `sizes_only`, which leaves out
/// the checks of pointers and pitches and the second stage's plan).
jpeggpu_status plan_roundtrip(const jpeggpu_ext_roundtrip_item* items, int n, int layout, uint8_t* base, Plan& p, bool sizes_only = false);
/// The plan's staged bytes, written to the `p.head` bytes at `h`.
void fill_roundtrip(const Plan& p, uint8_t* h);

} // namespace rt
} // namespace jg

#endif // JG_ROUNDTRIP_PLAN_HPP_
