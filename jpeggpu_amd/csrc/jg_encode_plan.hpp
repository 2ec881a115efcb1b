// jg_encode_plan.hpp -- the encoder's host side that launches nothing (jg_encode_plan.cpp): argument checks, the file
// header, the size bound, the plan of a call and the fill of its staged blob. Free of HIP, so that a stand-alone program
// can run it under a sanitizer (tests/emu/encode_plan_check_main.cpp). It knows nothing of the decoder: of a transcode
// item it sees the TranscodeSpec that jg_transcode.cpp made of it.
#ifndef JG_ENCODE_PLAN_HPP_
#define JG_ENCODE_PLAN_HPP_

#include "jg_encode_jobs.h"

#include <vector>

#pragma GCC visibility push(hidden)
namespace jg {
namespace enc {

/// What an item adds to a call. `header_bytes`: what it has in the blob at its header_off -- its header, for an item with
/// optimised tables its OptState (and the room of a long prefix), for a progressive item nothing.
struct Geometry {
    int hs, vs, mcus_x, mcus_y, blocks_per_mcu;
    uint64_t blocks, segments, stream_bound;
    uint32_t header_bytes;
    int slots;                                   // a progressive item's Huffman tables
    uint64_t scan_blocks, markers, marker_bytes; // a progressive item's: the blocks and restart markers of all its scans, DHTs + DRI + SOS at their longest
};

/// A planned call. A scratch-size query (`sizes_only`) fills `plan` and `geo` alone.
struct CallPlan {
    Plan plan;
    std::vector<Geometry> geo;
    std::vector<Item> items;      // and a sentinel
    uint64_t headers_off;         // in the blob: `headers`
    std::vector<uint8_t> headers; // every item's header or OptState, each on a multiple of 16 as Item::header_off says
    std::vector<Item> shadow;     // the progressive items' (and a sentinel, if there is one)
    std::vector<ProgItem> prog;
    std::vector<FitItem> fits;    // a budget call's: raw_off and blocks
};

/// The plan of a call: every offset in d_scratch. JPEGGPU_INVALID_ARGUMENT for an item outside the ranges of jpeggpu_ext.h,
/// JPEGGPU_NOT_SUPPORTED for an item or a call beyond the kernels' 32-bit bit offsets and block indices.
/// `specs`: the call is a transcode call and items[i] is specs[i].item. `fit`: the call is a budget call -- its FitItem[n]
/// in the blob and each item's unquantised transform behind the item's other arrays.
jpeggpu_status make_plan(const jpeggpu_ext_encode_item* items, const TranscodeSpec* specs, int n, bool fit, bool sizes_only, CallPlan& out);

/// The blob of a planned call into `h`, plan.blob_bytes of them; `base`: where d_scratch + 0 of the plan lies on the device.
/// `budgets`: a budget call's items (items[i] is budgets[i].item at quality_max, where every search starts).
void fill_blob(const CallPlan& call, const jpeggpu_ext_encode_item* items, const TranscodeSpec* specs, const jpeggpu_ext_encode_fit_item* budgets,
               const uint8_t* base, uint8_t* h);

/// make_plan(sizes_only) as the *_scratch_size calls report it: total and the room to align the caller's pointer, or 0.
size_t scratch_size_of(const jpeggpu_ext_encode_item* items, const TranscodeSpec* specs, int n, bool fit);

/// The TranscodeSpecs of a call's items through `make` (transcode_spec, coefficient_spec) and their encoder items side by side.
template <class SrcItem>
jpeggpu_status specs_of(const SrcItem* items, int n, bool need_device, jpeggpu_status (*make)(const SrcItem&, bool, TranscodeSpec&),
                        std::vector<TranscodeSpec>& specs, std::vector<jpeggpu_ext_encode_item>& enc)
{
    if (!items || n <= 0 || n > 65535) return JPEGGPU_INVALID_ARGUMENT;
    specs.resize(size_t(n));
    enc.resize(size_t(n));
    for (int i = 0; i < n; ++i) {
        const jpeggpu_status st = make(items[i], need_device, specs[size_t(i)]);
        if (st != JPEGGPU_SUCCESS) return st;
        enc[size_t(i)] = specs[size_t(i)].item;
    }
    return JPEGGPU_SUCCESS;
}

} // namespace enc
} // namespace jg
#pragma GCC visibility pop

#endif // JG_ENCODE_PLAN_HPP_
