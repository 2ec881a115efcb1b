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

namespace jg {
namespace enc {

/// Enqueues the call; *launched receives the number of launches.
hipError_t launch_encode_fit(const Plan& plan, int probes, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, int* d_quality, hipStream_t stream,
                             int* launched);

/// jg_encode.cpp: a budget call behind the checks of jg_encode_fit.cpp. `items[i]` is fit[i].item with quality_max as its
/// quality. (Its scratch size: jg_encode_plan.hpp, scratch_size_of.)
jpeggpu_status encode_fit_batch(const jpeggpu_ext_encode_item* items, const jpeggpu_ext_encode_fit_item* fit, int n, void* d_scratch, size_t scratch_size,
                                size_t* d_sizes, int* d_status, int* d_quality, hipStream_t stream);

} // namespace enc
} // namespace jg

#endif // JG_ENCODE_FIT_HPP_
