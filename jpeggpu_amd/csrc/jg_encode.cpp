// jg_encode.cpp -- the encoder's entry points of the exported C ABI (include/jpeggpu/jpeggpu_ext.h) that touch the device:
// each checks its arguments, has jg_encode_plan.cpp plan the call, stages and copies the blob that the plan fills, and
// launches the kernels of jg_encode.hip. It knows nothing of the decoder: of a transcode item it sees the TranscodeSpec
// that jg_transcode.cpp made of it.
#include "jg_encode_fit.hpp"
#include "jg_encode_plan.hpp"
#include "jg_encode_prog.hpp"
#include "jg_staging.hpp"
#include "jg_transcode.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

namespace jg {
namespace enc {
namespace {

/// The encoder's staging ring (the output stage keeps its own: an encode call does not wait for a resize call's lock).
StagingRing& staging()
{
    static StagingRing* s = new StagingRing;
    return *s;
}

/// The 256-aligned start of a caller's scratch, what the plans' offsets count from; null if `bytes` from there do not fit.
uint8_t* scratch_base(void* d_scratch, size_t scratch_size, uint64_t bytes)
{
    uint8_t* base = reinterpret_cast<uint8_t*>(jg::align_up(reinterpret_cast<uintptr_t>(d_scratch), 256));
    return size_t(base - static_cast<uint8_t*>(d_scratch)) + bytes > scratch_size ? nullptr : base;
}

/// jpeggpu_ext_encode_batch, and with `specs` (items[i] is specs[i].item) jpeggpu_ext_transcode_batch; with `fit`
/// (items[i] is fit[i].item at quality_max) jpeggpu_ext_encode_fit_batch.
jpeggpu_status batch_of(const jpeggpu_ext_encode_item* items, const TranscodeSpec* specs, int n, void* d_scratch, size_t scratch_size, size_t* d_sizes,
                        int* d_status, jpeggpu_stream_t stream, const jpeggpu_ext_encode_fit_item* fit = nullptr, int* d_quality = nullptr)
{
    if (!items || n <= 0 || !d_scratch || !d_sizes || !d_status) return JPEGGPU_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i)
        if ((!specs && !items[i].data) || (!items[i].out && items[i].capacity)) return JPEGGPU_INVALID_ARGUMENT;
    CallPlan call;
    try {
        const jpeggpu_status st = make_plan(items, specs, n, fit != nullptr, false, call);
        if (st != JPEGGPU_SUCCESS) return st;
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
    const Plan& plan = call.plan;
    uint8_t* base    = scratch_base(d_scratch, scratch_size, plan.total);
    if (!base) return JPEGGPU_INVALID_ARGUMENT;
    const auto fill = [&](uint8_t* h) {
        fill_blob(call, items, specs, fit, base, h);
        return JPEGGPU_SUCCESS;
    };
    std::lock_guard<std::mutex> lock(staging().mu);
    const jpeggpu_status staged = staging().stage_and_copy(plan.blob_bytes, fill, base, stream);
    if (staged != JPEGGPU_SUCCESS) return staged;
    if (fit) {
        int widest = 1, launched = 0;
        for (int i = 0; i < n; ++i) widest = fit[i].quality_max - fit[i].quality_min + 1 > widest ? fit[i].quality_max - fit[i].quality_min + 1 : widest;
        const int probes = fit_probes(widest);
        if (launch_encode_fit(plan, probes, base, reinterpret_cast<unsigned long long*>(d_sizes), d_status, d_quality, stream, &launched) != hipSuccess ||
            launched != fit_launches(probes, plan.optimized != 0))
            return JPEGGPU_INTERNAL_ERROR;
        return JPEGGPU_SUCCESS;
    }
    if (launch_encode(plan, base, reinterpret_cast<unsigned long long*>(d_sizes), d_status, stream, specs != nullptr) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    return JPEGGPU_SUCCESS;
}

/// batch_of for a call whose items become TranscodeSpecs through `make`.
template <class SrcItem>
jpeggpu_status spec_batch(const SrcItem* items, int n, jpeggpu_status (*make)(const SrcItem&, bool, TranscodeSpec&), void* d_scratch, size_t scratch_size,
                          size_t* d_sizes, int* d_status, jpeggpu_stream_t stream)
{
    if (!d_scratch || !d_sizes || !d_status) return JPEGGPU_INVALID_ARGUMENT;
    try {
        std::vector<TranscodeSpec> specs;
        std::vector<jpeggpu_ext_encode_item> enc;
        const jpeggpu_status st = specs_of(items, n, true, make, specs, enc);
        if (st != JPEGGPU_SUCCESS) return st;
        return batch_of(enc.data(), specs.data(), n, d_scratch, scratch_size, d_sizes, d_status, stream);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
}

} // namespace

/// jpeggpu_ext_read_coefficients_batch behind its checks: the items through the staging ring, one launch.
jpeggpu_status read_coefficients(const ReadItem* items, int n, int type, void* d_scratch, size_t scratch_size, hipStream_t stream)
{
    const size_t bytes = sizeof(ReadItem) * (size_t(n) + 1);
    uint8_t* base      = scratch_base(d_scratch, scratch_size, bytes);
    if (!base) return JPEGGPU_INVALID_ARGUMENT;
    const auto fill = [&](uint8_t* h) {
        std::memcpy(h, items, bytes);
        return JPEGGPU_SUCCESS;
    };
    std::lock_guard<std::mutex> lock(staging().mu);
    const jpeggpu_status staged = staging().stage_and_copy(bytes, fill, base, stream);
    if (staged != JPEGGPU_SUCCESS) return staged;
    if (launch_read_blocks(reinterpret_cast<const ReadItem*>(base), n, items[n].tile_start[0], type, stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    return JPEGGPU_SUCCESS;
}

jpeggpu_status encode_fit_batch(const jpeggpu_ext_encode_item* items, const jpeggpu_ext_encode_fit_item* fit, int n, void* d_scratch, size_t scratch_size,
                                size_t* d_sizes, int* d_status, int* d_quality, hipStream_t stream)
{
    return batch_of(items, nullptr, n, d_scratch, scratch_size, d_sizes, d_status, stream, fit, d_quality);
}

} // namespace enc
} // namespace jg

using namespace jg::enc;

extern "C" {

enum jpeggpu_status jpeggpu_ext_encode_batch(
    const struct jpeggpu_ext_encode_item* items, int n, void* d_scratch, size_t scratch_size, size_t* d_sizes, int* d_status, jpeggpu_stream_t stream)
{
    return batch_of(items, nullptr, n, d_scratch, scratch_size, d_sizes, d_status, stream);
}

enum jpeggpu_status jpeggpu_ext_transcode_batch(
    const struct jpeggpu_ext_transcode_item* items, int n, void* d_scratch, size_t scratch_size, size_t* d_sizes, int* d_status, jpeggpu_stream_t stream)
{
    return spec_batch(items, n, transcode_spec, d_scratch, scratch_size, d_sizes, d_status, stream);
}

enum jpeggpu_status jpeggpu_ext_write_coefficients_batch(
    const struct jpeggpu_ext_coefficient_item* items, int n, void* d_scratch, size_t scratch_size, size_t* d_sizes, int* d_status, jpeggpu_stream_t stream)
{
    return spec_batch(items, n, coefficient_spec, d_scratch, scratch_size, d_sizes, d_status, stream);
}

enum jpeggpu_status jpeggpu_ext_encode_tables_from_counts(const uint32_t* d_counts, int n_tables, uint8_t* d_bits_values, int* d_status, jpeggpu_stream_t stream)
{
    if (!d_counts || n_tables <= 0 || !d_bits_values || !d_status) return JPEGGPU_INVALID_ARGUMENT;
    if (launch_tables_from_counts(d_counts, n_tables, d_bits_values, d_status, stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
    return JPEGGPU_SUCCESS;
}

} // extern "C"
