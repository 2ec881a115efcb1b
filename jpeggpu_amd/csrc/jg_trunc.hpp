// jg_trunc.hpp -- launch interface of the kernels that finish the decode of a file that ended early (jg_trunc.hip). A call
// that holds no such file launches none of them.
#ifndef JG_TRUNC_HPP_
#define JG_TRUNC_HPP_

#include "jg_defs.h"

#include <hip/hip_runtime_api.h>

namespace jg {

/// In front of the Huffman stages (any time before kStageSyncIntra): the subsequences of zeros the host walk appended to the
/// scan are zeroed and given their segment. One launch.
hipError_t launch_trunc_prepare(const ScanJob& job, const TruncParams& tp, hipStream_t stream);
hipError_t launch_trunc_prepare_batch(const TruncRef* d_refs, int num_refs, hipStream_t stream);

/// Behind the write pass, in front of the IDCT stage (or of whatever reads the symbol stream): find the MCU that is finished
/// from zero bits, then make every data unit behind it an empty block of DC 0. Two launches.
hipError_t launch_trunc_finish(const ScanJob& job, const TruncParams& tp, hipStream_t stream);
hipError_t launch_trunc_finish_batch(const TruncRef* d_refs, int num_refs, hipStream_t stream);

} // namespace jg

#endif // JG_TRUNC_HPP_
