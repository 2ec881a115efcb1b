// jg_prog.hpp -- launch interface of the progressive (SOF2) kernels (jg_prog.hip; all launches are asynchronous on `stream`).
#ifndef JG_PROG_HPP_
#define JG_PROG_HPP_

#include "jg_prog_core.h"

#include <hip/hip_runtime_api.h>

namespace jg {

/// Work extents of the progressive launches of a call: the largest counts over its images (lanes beyond an image's own
/// count leave at once).
struct ProgExtent {
    uint32_t num_levels = 0;
    uint32_t max_items[kMaxProgScans] = {}; // work items (lanes) per level
    uint32_t max_units = 0;                 // visible blocks
};
void extend(ProgExtent& e, const ProgHeader& h);

/// The scans of ONE progressive image (passed by value), level by level, then the hand-over to the IDCT stage
/// (prog_pack_kernel). The coefficient buffers must have been zeroed on the stream.
hipError_t launch_prog(const ProgImage& img, const ProgExtent& e, hipStream_t stream);

/// The same for `num_images` images whose descriptors lie in device memory, one per blockIdx.y: one launch per level for
/// all of them, one pack launch.
hipError_t launch_prog_batch(const ProgImage* d_images, int num_images, const ProgExtent& e, hipStream_t stream);

} // namespace jg

#endif // JG_PROG_HPP_
