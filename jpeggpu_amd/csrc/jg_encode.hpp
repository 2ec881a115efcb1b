// jg_encode.hpp -- the encoder's launch interface (jg_encode.hip; progressive items: jg_encode_prog.hpp; every launch is
// asynchronous on `stream`). The host (jg_encode_plan.cpp) plans a call into one blob of descriptors (jg_encode_jobs.h) that
// travels to the device in one copy; the kernels index everything by BLOCK (8 x 8 samples), the parallel unit of every stage.
#ifndef JG_ENCODE_HPP_
#define JG_ENCODE_HPP_

#include "jg_encode_jobs.h"

#include <hip/hip_runtime_api.h>

namespace jg {
namespace enc {

/// `transcode`: every item's Item::src is its GatherSrc; gather_blocks takes the place of encode_blocks and
/// finish_transcode follows the last launch.
hipError_t launch_encode(const Plan& plan, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, hipStream_t stream, bool transcode = false);

/// The parts of launch_encode behind its first launch, as a budget call enqueues them once per probe (jg_encode_fit.hip);
/// each returns the number of launches it enqueued. launch_table_stages: launches 1a and 1b if the call has an item with
/// optimised tables, else nothing. launch_size_stages: launches 2 - 7, after which every item's size is known on the
/// device. launch_write_files: launch 8.
int launch_table_stages(const Plan& plan, uint8_t* d_scratch, hipStream_t stream);
int launch_size_stages(const Plan& plan, uint8_t* d_scratch, hipStream_t stream);
int launch_write_files(const Plan& plan, uint8_t* d_scratch, unsigned long long* d_sizes, int* d_status, hipStream_t stream);

/// jpeg_gen_optimal_table of n_tables x 256 counts: per table 16 `bits` bytes and 256 `values` bytes, and a status.
hipError_t launch_tables_from_counts(const uint32_t* d_counts, int n_tables, uint8_t* d_bits_values, int* d_status, hipStream_t stream);

} // namespace enc
} // namespace jg

#endif // JG_ENCODE_HPP_
