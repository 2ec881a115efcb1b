// jg_encode_fit.hpp -- encoding to a byte budget (jpeggpu_ext_encode_fit_batch): the best quality whose file fits, found on
// the device without the host in the loop. The pixel stage runs ONCE and keeps the unquantised transform; every probe of
// the search requantises it with a quality that lives in device memory, runs the encoder's size stages (jg_encode.hip,
// launches 2 - 7) and lets one kernel per call compare each item's size with its budget and move its search on. The host
// only derives the number of probes from the widest range of the call.
//
// The rule (include/jpeggpu/jpeggpu_ext.h): with lo = quality_min, hi = quality_max, B = max_bytes
//
//     size(hi) <= B: hi.   size(lo) > B: over budget.   Otherwise bisection over lo + 1 .. hi - 1 from best = lo:
//     m = (a + b) / 2; size(m) <= B: best = m, a = m + 1; else b = m - 1; until a > b.
//
// size(q) is not monotone in q, so this rule, not "the largest quality that fits", is what the call computes.
#ifndef JG_ENCODE_FIT_HPP_
#define JG_ENCODE_FIT_HPP_

#include "jg_encode.hpp"

#include <jpeggpu/jpeggpu.h>
#include <jpeggpu/jpeggpu_ext.h>

namespace jg {
namespace enc {

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

/// Enqueues the call; *launched receives the number of launches.
hipError_t launch_encode_fit(const Plan& plan, int probes, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, int* d_quality, hipStream_t stream,
                             int* launched);

/// jg_encode.cpp: the plan and the descriptors of a budget call, behind the checks of jg_encode_fit.cpp. `items[i]` is
/// fit[i].item with quality_max as its quality.
size_t encode_fit_scratch(const jpeggpu_ext_encode_item* items, int n);
jpeggpu_status encode_fit_batch(const jpeggpu_ext_encode_item* items, const jpeggpu_ext_encode_fit_item* fit, int n, void* d_scratch, size_t scratch_size,
                                size_t* d_sizes, int* d_status, int* d_quality, hipStream_t stream);

} // namespace enc
} // namespace jg

#endif // JG_ENCODE_FIT_HPP_
