// jg_front.hpp -- launch interface of the device-side front end (jg_front.hip); its parameters: FrontParams, jg_defs.h.
#ifndef JG_FRONT_HPP_
#define JG_FRONT_HPP_

#include "jg_defs.h"

#include <hip/hip_runtime_api.h>

namespace jg {

/// One scan, parameters by value. `job` is stored to P.job by the first kernel (a kernel argument is captured at
/// launch, so the caller's copy may change as soon as this returns -- no staging buffer, no copy from pageable memory).
hipError_t launch_front(const FrontParams& P, const ScanJob& job, hipStream_t stream);
/// The same for `count` scans whose parameters sit in device memory (grid.y = scan).
hipError_t launch_front_batch(const FrontParams* d_params, int count, uint32_t max_windows, hipStream_t stream);

} // namespace jg

#endif // JG_FRONT_HPP_
