// jg_quant.h -- jpeg_set_quality's arithmetic (jcparam.c: jpeg_quality_scaling, jpeg_add_quant_table with force_baseline)
// on the Annex K.1 / K.2 tables, for host and device alike: the host planner writes an item's DQT segments and divisors with
// it (jg_encode_plan.cpp), the budget search derives them on the device from a quality that lives there (jg_encode_fit.hip).
// Plain C++: a host compiler reads it without the HIP headers.
#ifndef JG_QUANT_H_
#define JG_QUANT_H_

#include <cstdint>

#if defined(__HIPCC__)
#define JG_QUANT_HD __host__ __device__
#else
#define JG_QUANT_HD
#endif

namespace jg {
namespace enc {

/// jpeg_quality_scaling: the percentage the base tables are scaled by. `quality` 1..100.
JG_QUANT_HD inline int quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }

/// jpeg_add_quant_table: one entry, held to 1..255 (force_baseline).
JG_QUANT_HD inline int quant_value(int base, int scale)
{
    const int v = (base * scale + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

/// Annex K.1 (table 0, luminance) and K.2 (table 1, chrominance), entry `i` in natural order.
JG_QUANT_HD inline int quant_base(int table, int i)
{
    constexpr uint8_t kLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                   14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    // K.2 is 99 outside its upper left corner: rows 0..3, columns 0..3
    constexpr uint8_t kChromaCorner[4][4] = {{17, 18, 24, 47}, {18, 21, 26, 66}, {24, 26, 56, 99}, {47, 66, 99, 99}};
    if (table == 0) return kLuma[i];
    return (i >> 3) < 4 && (i & 7) < 4 ? kChromaCorner[i >> 3][i & 7] : 99;
}

/// The quantiser of table `table` at `quality`, entry `i` in natural order: what the DQT segment holds.
JG_QUANT_HD inline int quantizer(int table, int quality, int i) { return quant_value(quant_base(table, i), quality_scale(quality)); }

} // namespace enc
} // namespace jg

#endif // JG_QUANT_H_
