// jg_roundtrip.hpp -- the launch interface of the round trip's block kernel (jg_roundtrip.hip; asynchronous on `stream`).
// The host plans a call in jg_roundtrip_plan.cpp; the second stage is launch_rgb_batch (jg_output.hpp).
#ifndef JG_ROUNDTRIP_HPP_
#define JG_ROUNDTRIP_HPP_

#include "jg_roundtrip_plan.hpp"

#include <hip/hip_runtime_api.h>

namespace jg {
namespace rt {

/// roundtrip_blocks over `tiles` tiles of the `n` items at `d_items`, whose plane offsets count from `d_scratch`.
hipError_t launch_roundtrip_blocks(const Item* d_items, int n, uint32_t tiles, uint8_t* d_scratch, hipStream_t stream);

} // namespace rt
} // namespace jg

#endif // JG_ROUNDTRIP_HPP_
