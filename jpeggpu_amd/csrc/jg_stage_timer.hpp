// jg_stage_timer.hpp -- optional stage timing (jpeggpu_ext_set_profiling, jpeggpu_ext_batch_set_profiling): events recorded
// between the launches of a decode, one timer for the decoder (jg_decoder.cpp) and for the batch (jg_batch.cpp).
#ifndef JG_STAGE_TIMER_HPP_
#define JG_STAGE_TIMER_HPP_

#include <jpeggpu/jpeggpu.h>
#include <jpeggpu/jpeggpu_ext.h>

#include <hip/hip_runtime_api.h>

#include <vector>

namespace jg {

#pragma GCC visibility push(hidden)
/// A ring of event sets, one set per decode, so that several decodes can be in flight before the times are read back. A
/// set holds as many events as its decode marks -- a lone decode's number varies, a batch call's is kNumStages + 1 -- and
/// every event carries the stage that ENDS at it.
class StageTimer {
  public:
    static constexpr int kSets = 64; // decodes a measurement window holds at the most

    StageTimer() = default;
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    ~StageTimer()
    {
        for (Set& s : sets_)
            for (hipEvent_t e : s.events) (void)hipEventDestroy(e);
    }

    bool enabled() const { return on_; }
    /// Switch the timing on or off; either way a new measurement window starts.
    void enable(bool on)
    {
        on_    = on;
        cur_   = -1;
        valid_ = 0;
    }

    /// A decode starts on `stream`: the next set of the ring, and its first event. `events`: so many are created up front.
    /// False if an event cannot be created (a failed record is not reported, here or by mark's caller of the batch).
    bool begin(hipStream_t stream, size_t events = 1)
    {
        if (!on_) return true;
        if (sets_.empty()) sets_.resize(kSets);
        cur_ = (cur_ + 1) % kSets;
        if (valid_ < kSets) ++valid_;
        Set& s = sets_[cur_];
        s.used = 0;
        while (s.events.size() < events)
            if (!s.add_event()) return false;
        (void)mark(-1, stream);
        return true;
    }

    /// `stage` ends here on `stream`. False if the event cannot be created or recorded.
    bool mark(int stage, hipStream_t stream)
    {
        if (!on_ || cur_ < 0) return true;
        Set& s = sets_[cur_];
        if (s.used == s.events.size() && !s.add_event()) return false;
        s.stage[s.used] = stage;
        return hipEventRecord(s.events[s.used++], stream) == hipSuccess;
    }

    /// ms[JPEGGPU_EXT_NUM_STAGES]: the mean over the decodes recorded since the window started, at most the last kSets; the
    /// events must have completed. Starts a new window. INVALID_ARGUMENT if the timing is off or nothing was recorded.
    jpeggpu_status mean_ms(float* ms)
    {
        for (int i = 0; i < JPEGGPU_EXT_NUM_STAGES; ++i) ms[i] = 0.f;
        if (!on_ || valid_ == 0) return JPEGGPU_INVALID_ARGUMENT;
        for (int k = 0; k < valid_; ++k) {
            const Set& s = sets_[k];
            for (size_t i = 1; i < s.used; ++i) {
                float t = 0.f;
                if (hipEventElapsedTime(&t, s.events[i - 1], s.events[i]) != hipSuccess) return JPEGGPU_INTERNAL_ERROR;
                if (s.stage[i] >= 0 && s.stage[i] < JPEGGPU_EXT_NUM_STAGES) ms[s.stage[i]] += t;
            }
        }
        for (int i = 0; i < JPEGGPU_EXT_NUM_STAGES; ++i) ms[i] /= static_cast<float>(valid_);
        enable(on_);
        return JPEGGPU_SUCCESS;
    }

  private:
    struct Set {
        std::vector<hipEvent_t> events;
        std::vector<int> stage; // stage that ENDS at event i (event 0 has none)
        size_t used = 0;
        bool add_event()
        {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return false;
            events.push_back(e);
            stage.push_back(-1);
            return true;
        }
    };
    bool on_ = false;
    std::vector<Set> sets_;
    int cur_ = -1, valid_ = 0;
};
#pragma GCC visibility pop

} // namespace jg

#endif // JG_STAGE_TIMER_HPP_
