// jg_staging.hpp -- host staging memory and offset alignment: StagingBuffer, which the decoder (jg_decoder.cpp) keeps per
// handle, and StagingRing, the ring of four that the output stage (jg_output.cpp) and the encoder (jg_encode.cpp) each keep
// one of per process.
#ifndef JG_STAGING_HPP_
#define JG_STAGING_HPP_

#include <jpeggpu/jpeggpu.h>

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <mutex>

namespace jg {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/// Host staging memory for the table blob: page-locked when a HIP device is present (so the copy
/// enqueued by transfer is asynchronous), pageable otherwise (header parsing needs no GPU).
struct StagingBuffer {
    uint8_t* ptr  = nullptr;
    size_t cap    = 0;
    bool pinned   = false;

    bool reserve(size_t n)
    {
        if (n <= cap) return true;
        release();
        const size_t want = align_up(n + n / 2, 4096);
        void* p           = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) == hipSuccess && p) {
            pinned = true;
        } else {
            (void)hipGetLastError();
            p      = std::malloc(want);
            pinned = false;
        }
        if (!p) return false;
        ptr = static_cast<uint8_t*>(p);
        cap = want;
        return true;
    }
    void release()
    {
        if (ptr) {
            if (pinned) (void)hipHostFree(ptr);
            else std::free(ptr);
        }
        ptr = nullptr;
        cap = 0;
    }
};

/// Page-locked staging of a call's descriptors and tables: a ring of four buffers. An owner keeps one per process and
/// never destroys it (the HIP runtime may be gone when static objects are).
struct StagingRing {
    static constexpr int kRing = 4;
    std::mutex mu;

    /// What every batched call does with its plan's staged part: the ring's next buffer with room for `bytes`, once the
    /// copy that last read it has executed; `fill(pinned bytes)`, which writes them and returns a status; the copy to
    /// `d_dst` on `stream`; the ring moves on. A failure leaves the ring where it was. Called with `mu` held; the callers
    /// hold it until their kernels are enqueued too.
    template <class Fill>
    jpeggpu_status stage_and_copy(size_t bytes, Fill fill, void* d_dst, hipStream_t stream)
    {
        const int r = next;
        // the staging buffer may still be the source of a copy enqueued kRing calls ago
        if (in_use[r] && hipEventSynchronize(copied[r]) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
        in_use[r] = false;
        if (!buf[r].reserve(bytes)) return JPEGGPU_OUT_OF_HOST_MEMORY;
        const jpeggpu_status filled = fill(buf[r].ptr);
        if (filled != JPEGGPU_SUCCESS) return filled;
        if (!copied[r] && hipEventCreateWithFlags(&copied[r], hipEventDisableTiming) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
        if (hipMemcpyAsync(d_dst, buf[r].ptr, bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
        if (hipEventRecord(copied[r], stream) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
        in_use[r] = true;
        next      = (r + 1) % kRing;
        return JPEGGPU_SUCCESS;
    }

private:
    StagingBuffer buf[kRing];
    hipEvent_t copied[kRing] = {};
    bool in_use[kRing]       = {};
    int next                 = 0;
};

} // namespace jg

#endif // JG_STAGING_HPP_
