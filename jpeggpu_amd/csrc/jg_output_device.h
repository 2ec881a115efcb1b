// jg_output_device.h -- device code that the translation units of the output stage share: jg_output.hip (RGB) and
// jg_output_gray.hip (grey). The staged tile and the upsampled sample read from it, the clamp, the 24-bit multiply, the
// tensor element and its stores, the search of a batch's tile list. Everything is inlined: each unit has its own copy.
#ifndef JG_OUTPUT_DEVICE_H_
#define JG_OUTPUT_DEVICE_H_

#include "jg_output_jobs.h"

#include <hip/hip_runtime.h>

#include <type_traits>

namespace jg {

namespace {

constexpr int kFancyTileW = 256, kFancyTileH = 8;
constexpr int kFancyLdsW = kFancyTileW + 4, kFancyLdsH = kFancyTileH + 2; // samples under a tile at ratio 1, with the halo
using FancyTile = uint8_t[kFancyLdsH][kFancyLdsW];
/// The upsampled value of image pixel (x, y) of a staged component; (bx, by): full-plane coordinates of t[0][0].
__device__ __forceinline__ int fancy_sample(const FancyComp& c, const FancyTile& t, int bx, int by, int x, int y)
{
    switch (c.mode) {
    case kFancyH2V1: {
        const int i = (x >> 1) - bx, j = y - by, odd = x & 1;
        return (3 * t[j][i] + t[j][odd ? i + 1 : i - 1] + 1 + odd) >> 2;
    }
    case kFancyH2V2: {
        const int i = (x >> 1) - bx, j = (y >> 1) - by, odd = x & 1, dj = (y & 1) ? 1 : -1, di = odd ? 1 : -1;
        const int here = 3 * t[j][i] + t[j + dj][i];      // column sums: 3 near + far row
        const int side = 3 * t[j][i + di] + t[j + dj][i + di];
        return (3 * here + side + 8 - odd) >> 4;
    }
    case kFancyH1V2: {
        const int i = x - bx, j = (y >> 1) - by, below = y & 1;
        return (3 * t[j][i] + t[below ? j + 1 : j - 1][i] + 1 + below) >> 2;
    }
    default: return t[y / c.vr - by][x / c.hr - bx];
    }
}

__device__ __forceinline__ uint32_t clamp255(int v) { return static_cast<uint32_t>(min(max(v, 0), 255)); }

/// Taps per output column that a first-pass workgroup keeps in LDS (more: straight from the table).
constexpr int kResizeLdsTaps = 64;

/// The 24-bit multiply (v_mad_i32_i24 with its add) for the kernels added since resize_h_kernel. Not HIP's __mul24: that
/// is one `static` wrapper for the whole file, and a further call site of it changes how it is inlined into
/// resize_h_kernel's tap loop, whose code is to stay as it is (the compile check).
/// Plain C++: the product of two values sign-extended from 24 bits is what the compiler selects that instruction for.
__device__ __forceinline__ int mul24(int a, int b) { return ((a << 8) >> 8) * ((b << 8) >> 8); }

/// ToTensor + Normalize of byte u: ((float(u) / 255) - mean) / std. Three binary32 operations, each rounded to nearest
/// even on its own: no FMA, no reciprocal, no folded scale and bias (those differ from the CPU's result in the last bit
/// of hundreds of the 3 x 256 values). The division is the correctly rounded one (v_div_scale / v_div_fmas / v_div_fixup).
__device__ __forceinline__ float tensor_norm(uint32_t u, float mean, float std)
{
#pragma clang fp contract(off)
    return __fdiv_rn(__fsub_rn(__fdiv_rn(static_cast<float>(u), 255.0f), mean), std);
}

/// The bit pattern of float v as an element of the float type T: itself, or converted ONCE, round to nearest even, to half
/// or bfloat16 (never arithmetic in half precision). Also the coefficient reader's conversion (jg_encode.hip: read_blocks).
template <class T>
__device__ __forceinline__ uint32_t float_bits(float v)
{
    if constexpr (sizeof(T) == 4) {
        return __float_as_uint(v);
    } else if constexpr (std::is_same<T, _Float16>::value) {
        return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v)); // v_cvt_f16_f32 in the default rounding mode
    } else { // bfloat16: the upper half of the float, rounded to nearest even on the lower half
        const uint32_t b = __float_as_uint(v);
        if ((b & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
        return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
    }
}

/// The bit pattern of the element of type T made of byte u: the byte itself, or float_bits of tensor_norm's float.
template <class T>
__device__ __forceinline__ uint32_t tensor_bits(uint32_t u, float mean, float std)
{
    if constexpr (sizeof(T) == 1) return u;
    else return float_bits<T>(tensor_norm(u, mean, std));
}

/// N elements of S bytes (their bit patterns in e[0 .. N - 1]) as N S / 4 dwords in memory order.
template <int S, int N>
__device__ __forceinline__ void tensor_pack(const uint32_t (&e)[N], uint32_t (&d)[N * S / 4])
{
    constexpr int per = 4 / S;
#pragma unroll
    for (int k = 0; k < N / per; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < per; ++j) v |= e[per * k + j] << (8 * S * j);
        d[k] = v;
    }
}

template <int S>
__device__ __forceinline__ void tensor_store_elem(uint8_t* p, uint32_t bits)
{
    if constexpr (S == 1) *p = static_cast<uint8_t>(bits);
    else if constexpr (S == 2) *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(bits);
    else *reinterpret_cast<uint32_t*>(p) = bits;
}

/// Two and four dwords as one value that asks for dword alignment only: global_store_dwordx2 / x4 need no more on gfx950.
typedef uint32_t TensorDwords2 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t TensorDwords4 __attribute__((ext_vector_type(4), aligned(4)));

/// A lane's run of N contiguous elements of S bytes at p, of which it has the first `count`. The whole run where p lies on
/// a dword, as 16-byte stores, then an 8-byte one, then dwords (three of them: the compiler joins them, as in store_rgb4).
/// Written as vectors and not as dword stores in a row, which for float elements the compiler would take apart again: it
/// sinks the dword the element path below has in common with them. Branches by 8- and 16-byte alignment in front of the
/// wider stores bought nothing: the target's alignment rule is the dword, and the compiler sank their common dwords too.
/// Element by element otherwise.
template <int S, int N>
__device__ __forceinline__ void tensor_store_run(uint8_t* p, const uint32_t (&e)[N], int count)
{
    constexpr int ND = N * S / 4;
    if (count == N && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        uint32_t d[ND];
        tensor_pack<S, N>(e, d);
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
        int k = 0;
#pragma unroll
        for (; k + 4 <= ND; k += 4) *reinterpret_cast<TensorDwords4*>(q + k) = TensorDwords4{d[k], d[k + 1], d[k + 2], d[k + 3]};
        if (k + 2 == ND) *reinterpret_cast<TensorDwords2*>(q + k) = TensorDwords2{d[k], d[k + 1]};
        else
#pragma unroll
            for (; k < ND; ++k) q[k] = d[k];
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < count) tensor_store_elem<S>(p + k * S, e[k]);
    }
}

/// The last item whose first tile is <= b: the item of workgroup b (items without tiles in this list share their first
/// tile with the item behind them and are never found).
__device__ __forceinline__ int rgb_batch_item(const int* first_tile, int n, int b)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (first_tile[m] <= b) lo = m;
        else hi = m - 1;
    }
    return lo;
}

} // namespace

} // namespace jg

#endif // JG_OUTPUT_DEVICE_H_
