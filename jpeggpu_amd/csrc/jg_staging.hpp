// jg_staging.hpp -- host staging memory and offset alignment, shared by the decoder (jg_decoder.cpp) and the output
// stage (jg_output.cpp).
#ifndef JG_STAGING_HPP_
#define JG_STAGING_HPP_

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>

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

} // namespace jg

#endif // JG_STAGING_HPP_
