// jg_idct.hpp -- launch interface of the IDCT stage (jg_idct.hip), for the stage launches of jg_kernels.hip.
#ifndef JG_IDCT_HPP_
#define JG_IDCT_HPP_

#include "jg_kernels.hpp"

namespace jg {

/// Data units a workgroup of the IDCT kernels takes: JobExtent::max_idct_blocks counts these groups (extend).
constexpr int kIdctDuPerWg = 256;

// (between two sources of the library only: not among the symbols it exports)
#pragma GCC visibility push(hidden)
/// kStageIdct for each way a launch holds its jobs (jg_kernels.hpp: launch_stage, launch_stage_scans,
/// launch_stage_device_job, launch_stage_batch), with the extents `e` of those jobs. Nothing is launched where
/// e.max_idct_blocks is 0.
hipError_t launch_idct_job(const ScanJob& job, const JobExtent& e, hipStream_t stream);
hipError_t launch_idct_scans(const ScanJob (&jobs)[kMaxScans], int num_jobs, const JobExtent& e, hipStream_t stream);
hipError_t launch_idct_device_job(const ScanJob* d_job, const JobExtent& e, hipStream_t stream);
hipError_t launch_idct_batch(const ScanJob* d_jobs, int num_jobs, const JobExtent& e, hipStream_t stream);
#pragma GCC visibility pop

} // namespace jg

#endif // JG_IDCT_HPP_
