// jg_encode_fit.cpp -- encoding to a byte budget, the host's part (include/jpeggpu/jpeggpu_ext.h: jpeggpu_ext_encode_fit_*):
// the checks of a call's ranges and the items the encoder's planner sees, each at its quality_max, where every search
// starts. The plan and the descriptors are jg_encode_plan.cpp's, the launches jg_encode.cpp's and jg_encode_fit.hip's.
#include "jg_encode_fit.hpp"
#include "jg_encode_plan.hpp"

#include <new>
#include <vector>

namespace {

/// JPEGGPU_SUCCESS and the items as the planner takes them; the planner checks everything an encode call checks.
jpeggpu_status plain_items(const jpeggpu_ext_encode_fit_item* items, int n, std::vector<jpeggpu_ext_encode_item>& plain)
{
    if (!items || n <= 0 || n > 65535) return JPEGGPU_INVALID_ARGUMENT;
    plain.resize(size_t(n));
    bool progressive = false;
    for (int i = 0; i < n; ++i) {
        const jpeggpu_ext_encode_fit_item& f = items[i];
        if (f.quality_min < 1 || f.quality_max > 100 || f.quality_min > f.quality_max) return JPEGGPU_INVALID_ARGUMENT;
        if (f.item.progressive != 0 && f.item.progressive != 1) return JPEGGPU_INVALID_ARGUMENT;
        progressive |= f.item.progressive == 1;
        plain[size_t(i)]         = f.item;
        plain[size_t(i)].quality = f.quality_max; // (item.quality is ignored)
    }
    return progressive ? JPEGGPU_NOT_SUPPORTED : JPEGGPU_SUCCESS;
}

} // namespace

extern "C" {

size_t jpeggpu_ext_encode_fit_scratch_size(const struct jpeggpu_ext_encode_fit_item* items, int n)
{
    try {
        std::vector<jpeggpu_ext_encode_item> plain;
        if (plain_items(items, n, plain) != JPEGGPU_SUCCESS) return 0;
        return jg::enc::scratch_size_of(plain.data(), nullptr, n, true);
    } catch (const std::bad_alloc&) {
        return 0;
    }
}

int jpeggpu_ext_encode_fit_launches(const struct jpeggpu_ext_encode_fit_item* items, int n)
{
    try {
        std::vector<jpeggpu_ext_encode_item> plain;
        if (plain_items(items, n, plain) != JPEGGPU_SUCCESS || jg::enc::scratch_size_of(plain.data(), nullptr, n, true) == 0) return 0;
    } catch (const std::bad_alloc&) {
        return 0;
    }
    int widest = 1;
    bool optimized = false;
    for (int i = 0; i < n; ++i) {
        const int range = items[i].quality_max - items[i].quality_min + 1;
        widest          = range > widest ? range : widest;
        optimized |= items[i].item.optimize == 1;
    }
    return jg::enc::fit_launches(jg::enc::fit_probes(widest), optimized);
}

enum jpeggpu_status jpeggpu_ext_encode_fit_batch(const struct jpeggpu_ext_encode_fit_item* items, int n, void* d_scratch, size_t scratch_size, size_t* d_sizes,
                                                 int* d_status, int* d_quality, jpeggpu_stream_t stream)
{
    try {
        std::vector<jpeggpu_ext_encode_item> plain;
        const jpeggpu_status st = plain_items(items, n, plain);
        if (st != JPEGGPU_SUCCESS) return st;
        if (!d_quality) return JPEGGPU_INVALID_ARGUMENT;
        return jg::enc::encode_fit_batch(plain.data(), items, n, d_scratch, scratch_size, d_sizes, d_status, d_quality, stream);
    } catch (const std::bad_alloc&) {
        return JPEGGPU_OUT_OF_HOST_MEMORY;
    }
}

} // extern "C"
