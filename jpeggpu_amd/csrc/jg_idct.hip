// jg_idct.hip -- gfx950 (CDNA4, wave64) kernels of the IDCT stage: from the symbol stream the write pass left
// (jg_kernels.hip) to the pixels of the component planes.
//
//   idct_kernel             gather + dequant + 8x8 fixed-point IDCT in stream order
//                                                                    (reference idct.cu:44-223 + decode_transpose.cu:41-132)
//   idct_scaled_kernel      the same at 1/2, 1/4, 1/8 size: libjpeg-turbo's reduced IDCTs (jidctred.c; jpeggpu_ext_set_scale)
//   idct_kernel<IslowJobs<..>>  full size with libjpeg-turbo's jpeg_idct_islow (jidctint.c; jpeggpu_ext_set_idct)
//   ..<CropJobs<..>>        the units of a job's MCU window only (jpeggpu_ext_set_crop)
//   ..<DraftJobs<..>>       the units of one block size of a job in libjpeg's scale mode, whose components differ in size
//                                                                    (jdmaster.c; jpeggpu_ext_set_scale_mode), and of a
//                                                                    luma-only job: component 0's (jpeggpu_ext_set_luma_only)
//   ..<LumaJobs<..>>        component 0's units of a full-size luma-only job with the reference transform
//
// Integer arithmetic throughout: no MFMA. Every kernel takes a job source (jg_jobs.h), as the kernels of the entropy pass
// do; the sources that only this stage knows (an array's full-size jobs, the jobs of one IDCT method) are defined here.
// A translation unit of its own: these kernels are a third of the library's instantiations and more than half of its
// code, and whoever changes one has only this file's assembly to read.
#include "jg_idct.hpp"

#include <hip/hip_runtime.h>

#include <type_traits>

#include "jg_huff_core.h" // the symbol stream's entries: sym_entry_index, sym_entry_value, kUnitHasEscape
#include "jg_jobs.h"

namespace jg {

namespace {

/// A batch's jobs as idct_kernel sees them when the batch mixes scales (jpeggpu_ext_set_scale): a scaled job reads as the
/// empty job below (no data units), so that only the full-size ones are decoded at full size.
__device__ ScanJob g_no_job;
struct JobArrayFullSize {
    const ScanJob* jobs;
    __device__ __forceinline__ const ScanJob& get() const
    {
        const ScanJob& j = jobs[blockIdx.y];
        return j.ip.scale_log2 == 0 ? j : g_no_job;
    }
};
/// The same when the batch's full-size jobs mix IDCT methods (jpeggpu_ext_set_idct): the instantiation of method kMethod
/// sees the full-size jobs of that method; every other job reads as g_no_job.
template <uint8_t kMethod>
struct JobArrayFullSizeOf {
    const ScanJob* jobs;
    __device__ __forceinline__ const ScanJob& get() const
    {
        const ScanJob& j = jobs[blockIdx.y];
        return j.ip.scale_log2 == 0 && j.ip.idct_method == kMethod ? j : g_no_job;
    }
};

// ------------------------------------------------------------------------------------------------
// dequantisation + inverse DCT
// ------------------------------------------------------------------------------------------------

__device__ __forceinline__ int unfixo(int x) { return (x + 0x1000) >> 13; }

/// 8-point fixed-point inverse DCT, the arithmetic of the reference's `idct_vector`
/// (src/idct.cu:49-95): Q15 even part, Q13 odd part, results rounded to int16.
/// kRound = 0x8000 is the reference's rounding; the row pass adds the level shift as well (128 in the high half:
/// the int16 the reference stores and then offsets, `(int16)(t + 128)`, src/idct.cu:218, wraps the same way).
template <int kRound = 0x8000>
__device__ __forceinline__ void idct8(int (&v)[8])
{
    constexpr int cos_1_4 = 0x5a82, sin_1_8 = 0x30fc, cos_1_8 = 0x7642;
    constexpr int osin_1_16 = 0x063e, osin_5_16 = 0x1a9b, ocos_1_16 = 0x1f63, ocos_5_16 = 0x11c7;

    const int e0 = (v[0] + v[4]) * cos_1_4;
    const int e1 = (v[0] - v[4]) * cos_1_4;
    // (a rotation as three products: x s - y c = (x + y) s - y (s + c), y s + x c = (x + y) s + x (c - s); the same
    // numbers in wrapping 32-bit arithmetic, and an addition issues faster than a multiplication)
    int z26 = (v[2] + v[6]) * sin_1_8;
    asm("" : "+v"(z26)); // one product with two users: left to itself the compiler multiplies it out again inside each of them
    const int e2  = z26 - v[6] * (sin_1_8 + cos_1_8);
    const int e3  = z26 + v[2] * (cos_1_8 - sin_1_8);
    const int a0 = e0 + e3, a1 = e1 + e2, a2 = e1 - e2, a3 = e0 - e3;

    const int m0 = unfixo((v[3] + v[5]) * cos_1_4);
    const int m1 = unfixo((v[3] - v[5]) * cos_1_4);
    // x4 written as a multiplication: `<<` on a negative int is undefined before C++20 and hipcc uses that
    const int q1 = v[1] * 4, q7 = v[7] * 4;
    const int o0 = q1 + m0, o1 = q7 + m1, o2 = q1 - m0, o3 = q7 - m1;
    int z01 = (o0 + o1) * osin_1_16;
    asm("" : "+v"(z01));
    const int b0  = z01 + o0 * (ocos_1_16 - osin_1_16); // o0 c + o1 s
    const int b1  = z01 - o1 * (ocos_1_16 + osin_1_16); // o0 s - o1 c
    int z23 = (o2 + o3) * osin_5_16;
    asm("" : "+v"(z23));
    const int b2  = z23 + o2 * (ocos_5_16 - osin_5_16); // o2 c + o3 s
    const int b3  = z23 - o3 * (ocos_5_16 + osin_5_16); // o2 s - o3 c

    // results rounded but NOT shifted: the int16 the reference stores (`unfixh`) is the high half
    v[0] = a0 + b0 + kRound;
    v[1] = a1 + b3 + kRound;
    v[2] = a2 + b2 + kRound;
    v[3] = a3 + b1 + kRound;
    v[4] = a3 - b1 + kRound;
    v[5] = a2 - b2 + kRound;
    v[6] = a1 - b3 + kRound;
    v[7] = a0 - b0 + kRound;
}

__device__ __forceinline__ uint32_t magic_quot(uint32_t n, uint32_t mul, uint32_t shift)
{
    return mul ? __umulhi(n, mul) >> shift : n;
}

/// Four finished samples from four row-pass results whose high halves already hold (int16)(t + 128): clamped to
/// 0..255 (reference src/idct.cu:218-220), one byte each.
__device__ __forceinline__ uint32_t finish_pixels(int w0, int w1, int w2, int w3)
{
    const uint32_t lo = __builtin_amdgcn_perm(static_cast<uint32_t>(w1), static_cast<uint32_t>(w0), 0x07060302u);
    const uint32_t hi = __builtin_amdgcn_perm(static_cast<uint32_t>(w3), static_cast<uint32_t>(w2), 0x07060302u);
    uint32_t a, b;
    asm("v_sat_pk_u8_i16 %0, %1" : "=v"(a) : "v"(lo)); // two bytes in the low half
    asm("v_sat_pk_u8_i16 %0, %1" : "=v"(b) : "v"(hi));
    return __builtin_amdgcn_perm(b, a, 0x05040100u);
}

constexpr int kIdctDuPerBlock = 32; // 8 lanes per data unit, 256 lanes
constexpr int kIdctDuStride   = 64 + 8; // int16 per staged data unit (+8: the 8 units of a wave start on different banks)

__device__ __forceinline__ void unpack8(const uint4& raw, int (&v)[8])
{
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = static_cast<int16_t>(w[i >> 1] >> (16 * (i & 1)));
}

constexpr int kIdctIters    = 8;                            // groups of 32 data units per workgroup
static_assert(kIdctDuPerWg == kIdctDuPerBlock * kIdctIters, "jg_idct.hpp"); // 256

/// Zig-zag index of the coefficient in `row`, `col` (T.81 figure A.6), worked out instead of looked up: a table in
/// memory is one more load for the prologue to wait for. Diagonal d = row + col holds the indices from d (d + 1) / 2
/// on, downwards for odd d; the lower right half mirrors the upper left.
__host__ __device__ constexpr int zigzag_of(int row, int col)
{
    const bool low = row + col > 7;
    const int r = low ? 7 - row : row, c = low ? 7 - col : col, d = r + c;
    const int z = d * (d + 1) / 2 + ((d & 1) ? r : c);
    return low ? 63 - z : z;
}
constexpr bool zigzag_of_matches_table()
{
    constexpr uint8_t nat[64] = JG_ORDER_NATURAL; // zig-zag index -> natural index
    for (int z = 0; z < 64; ++z)
        if (zigzag_of(nat[z] >> 3, nat[z] & 7) != z) return false;
    return true;
}
static_assert(zigzag_of_matches_table(), "zigzag_of");

/// Two 16-bit products at once (v_pk_mul_lo_u16): the low halves of coefficient * quantiser.
__device__ __forceinline__ uint32_t mul_lo_u16x2(uint32_t a, uint32_t b)
{
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, static_cast<u16x2>(__builtin_bit_cast(u16x2, a) * __builtin_bit_cast(u16x2, b)));
}

/// libjpeg's post-IDCT range limit (the sample_range_limit table indexed with x & RANGE_MASK, RANGE_MASK = 1023): x
/// wrapped to a 10-bit signed value, clamped to -128..127, plus 128.
__device__ __forceinline__ uint32_t range_limit(int x)
{
    const int w = static_cast<int>(static_cast<uint32_t>(x) << 22) >> 22;
    return static_cast<uint32_t>(min(max(w, -128), 127) + 128);
}

/// The transform idct_kernel applies is a policy of its job source: the reference's (idct8 above) for the plain sources,
/// libjpeg-turbo's jpeg_idct_islow (jidctint.c) for IslowJobs<JS>, which the launch picks for jobs of jpeggpu_ext_set_idct's
/// JPEGGPU_EXT_IDCT_ISLOW. Both share everything else of the kernel: the unit records, the entry gather and prefetch, the
/// zig-zag placement, the geometry and the coalesced pixel stores.
struct IdctReference {
    static constexpr bool kIslow = false;
};
struct IdctIslow {
    static constexpr bool kIslow = true;
};
template <class JS>
struct IslowJobs {
    JS js;
    __device__ __forceinline__ const ScanJob& get() const { return js.get(); }
};
template <class JS>
struct IdctOf {
    using type = IdctReference;
};
template <class JS>
struct IdctOf<IslowJobs<JS>> {
    using type = IdctIslow;
};

/// Which data units the IDCT kernels transform is a policy of the job source as well: every unit of the job in stream
/// order for the plain sources, the units of the job's MCU window (jpeggpu_ext_set_crop, IdctWindow) for CropJobs<JS>,
/// which the launch picks when a call holds a cropped job. That instantiation decodes a job without a window as the plain
/// one does, so one launch serves a batch of both kinds.
template <class JS>
struct CropJobs {
    JS js;
    __device__ __forceinline__ const ScanJob& get() const { return js.get(); }
};
template <class JS>
struct IsCropped : std::false_type {
};
template <class JS>
struct IsCropped<CropJobs<JS>> : std::true_type {
};
template <class JS>
struct IsCropped<IslowJobs<JS>> : IsCropped<JS> {
};

/// Unit w of a cropped job's window (IdctWindow): its index in the job's stream order (the data-unit table) and the
/// column and row of its MCU inside the window. A job without a window: unit w itself, and the MCU in the frame.
struct WindowUnit {
    int stream, mx, my, k;
};
__device__ __forceinline__ WindowUnit window_unit(const IdctParams& ip, const IdctWindow& win, int w)
{
    const int wm = static_cast<int>(magic_quot(w, ip.du_per_mcu_mul, ip.du_per_mcu_shift));
    const int k  = w - wm * ip.du_per_mcu;
    if (win.mcus_x == 0) {
        const int mcu = wm + ip.first_mcu;
        const int my  = static_cast<int>(magic_quot(mcu, ip.mcus_x_mul, ip.mcus_x_shift));
        return WindowUnit{w, mcu - my * ip.mcus_x, my, k};
    }
    const int my  = static_cast<int>(magic_quot(wm, win.mcus_x_mul, win.mcus_x_shift));
    const int mx  = wm - my * win.mcus_x;
    const int mcu = (win.my0 + my) * ip.mcus_x + win.mx0 + mx;
    return WindowUnit{(mcu - ip.first_mcu) * ip.du_per_mcu + k, mx, my, k};
}

/// The units of ONE block size of a JPEGGPU_EXT_SCALE_LIBJPEG job (IdctDraft, jg_defs.h) are what the IDCT kernels
/// transform for DraftJobs<JS>: idct_kernel<IslowJobs<DraftJobs<JS>>> the 8x8 ones, idct_scaled_kernel<DraftJobs<JS>, lg>
/// the reduced ones. Every other job counts no units of any size there (draft_num_du), so one launch per size serves a
/// batch of any mix; a job's MCU window is honoured whether the call holds cropped jobs or not. Only jobs of that mode
/// reach these instantiations.
template <class JS>
struct DraftJobs {
    JS js;
    __device__ __forceinline__ const ScanJob& get() const { return js.get(); }
};
template <class JS>
struct IsDraft : std::false_type {
};
template <class JS>
struct IsDraft<DraftJobs<JS>> : std::true_type {
};
template <class JS>
struct IsDraft<IslowJobs<JS>> : IsDraft<JS> {
};
/// Luma-only decoding (jpeggpu_ext_set_luma_only) needs no kernel of its own: build_jobs lists the units of component 0
/// alone in the job's classes, and the DraftJobs instantiations transform what is listed -- fewer units, no branch per
/// unit. One case they do not cover: 8x8 units with the REFERENCE transform (theirs are ISLOW). LumaJobs<JS> is that
/// instantiation of idct_kernel: class 0 of the jobs marked kDraftLumaReference, which the DraftJobs ones count no units
/// of. The launch picks it only when a call holds such a job.
template <class JS>
struct LumaJobs {
    JS js;
    __device__ __forceinline__ const ScanJob& get() const { return js.get(); }
};
template <class JS>
struct IsDraft<LumaJobs<JS>> : std::true_type {
};
/// IdctDraft::on of the jobs whose classes a job source takes.
template <class JS>
struct DraftOn : std::integral_constant<uint8_t, kDraftOn> {
};
template <class JS>
struct DraftOn<LumaJobs<JS>> : std::integral_constant<uint8_t, kDraftLumaReference> {
};
template <class JS>
struct DraftOn<IslowJobs<JS>> : DraftOn<JS> {
};
/// Units of class kLg in the job: its MCUs (the window's, for a cropped job: IdctParams::num_du counts those) times the
/// class's units per MCU. 0 for a job of another kind and for one the device front end refused (num_du == 0).
template <int kLg, uint8_t kOn = kDraftOn>
__device__ __forceinline__ int draft_num_du(const ScanJob& j)
{
    if (j.draft.on != kOn) return 0;
    return static_cast<int>(magic_quot(static_cast<uint32_t>(j.ip.num_du), j.ip.du_per_mcu_mul, j.ip.du_per_mcu_shift)) * j.draft.n[kLg];
}
/// Unit w of class kLg: window_unit's answer for data unit k[kLg][w % n] of MCU w / n.
template <int kLg>
__device__ __forceinline__ WindowUnit draft_unit(const ScanJob& j, int w)
{
    const IdctParams& ip  = j.ip;
    const IdctWindow& win = j.win;
    const int wm = static_cast<int>(magic_quot(w, j.draft.mul[kLg], j.draft.shift[kLg]));
    const int k  = j.draft.k[kLg][w - wm * j.draft.n[kLg]];
    if (win.mcus_x == 0) {
        const int mcu = wm + ip.first_mcu;
        const int my  = static_cast<int>(magic_quot(mcu, ip.mcus_x_mul, ip.mcus_x_shift));
        return WindowUnit{wm * ip.du_per_mcu + k, mcu - my * ip.mcus_x, my, k};
    }
    const int my  = static_cast<int>(magic_quot(wm, win.mcus_x_mul, win.mcus_x_shift));
    const int mx  = wm - my * win.mcus_x;
    const int mcu = (win.my0 + my) * ip.mcus_x + win.mx0 + mx;
    return WindowUnit{(mcu - ip.first_mcu) * ip.du_per_mcu + k, mx, my, k};
}

/// One 8-point pass of jpeg_idct_islow (jidctint.c, CONST_BITS = 13): the eight outputs before their DESCALE, in T (int:
/// wrapping 32-bit arithmetic, the library is built with -fwrapv; long long: jidctint.c's JLONG). Output i is row i of a
/// column (pass 1) or column i of a row (pass 2).
template <class T>
__device__ __forceinline__ void islow8(const T (&in)[8], T (&out)[8])
{
    // even part: the rotator is sqrt(2) c(-6)
    const T z1   = (in[2] + in[6]) * T(4433);       // FIX_0_541196100
    const T tmp2 = z1 + in[6] * T(-15137);           // FIX_1_847759065
    const T tmp3 = z1 + in[2] * T(6270);             // FIX_0_765366865
    const T tmp0 = (in[0] + in[4]) * T(1 << 13);     // LEFT_SHIFT(.., CONST_BITS)
    const T tmp1 = (in[0] - in[4]) * T(1 << 13);
    const T tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    // odd part
    T t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
    T o1 = t0 + t3, o2 = t1 + t2, o3 = t0 + t2, o4 = t1 + t3;
    const T z5 = (o3 + o4) * T(9633);                // FIX_1_175875602
    t0 = t0 * T(2446);                               // FIX_0_298631336
    t1 = t1 * T(16819);                              // FIX_2_053119869
    t2 = t2 * T(25172);                              // FIX_3_072711026
    t3 = t3 * T(12299);                              // FIX_1_501321110
    o1 = o1 * T(-7373);                              // FIX_0_899976223
    o2 = o2 * T(-20995);                             // FIX_2_562915447
    o3 = o3 * T(-16069) + z5;                        // FIX_1_961570560
    o4 = o4 * T(-3196) + z5;                         // FIX_0_390180644
    t0 += o1 + o3;
    t1 += o2 + o4;
    t2 += o2 + o3;
    t3 += o1 + o4;
    out[0] = tmp10 + t3, out[7] = tmp10 - t3;
    out[1] = tmp11 + t2, out[6] = tmp11 - t2;
    out[2] = tmp12 + t1, out[5] = tmp12 - t1;
    out[3] = tmp13 + t0, out[4] = tmp13 - t0;
}

/// Dequantised inputs a pass-1 column may hold for the 32-bit pass 1 to be exact. Every output of islow8 is a sum
/// sum_k c_k in[k] with integer coefficients c_k fixed by the constants above; the largest sum_k |c_k| over the eight
/// outputs is 61,214 (outputs 2 and 5: 8192 + 8192 from in[0], in[4] and 4,433 + 10,704 from in[2], in[6], the even
/// part's 31,521; 6,437 + 11,362 + 2,261 + 9,633 from in[1], in[3], in[5], in[7], the odd part's 29,693), and DESCALE
/// adds 2^10. With |in[k]| <= 32,767, |output| + 2^10 <= 61,214 * 32,767 + 1,024 = 2,005,800,162 < 2^31: the true sum fits
/// an int, and wrapping 32-bit arithmetic, exact modulo 2^32 whatever the order of its operations, gives it exactly.
/// (tests/test_libjpeg_ref.py checks the bound on every sign pattern at +-32,767.) Pass 2 never needs 64 bits: its
/// result goes through range_limit, which reads bits 18..27 of the sum only, and those are the same modulo 2^32.
constexpr int kIslowPass1Max = 32767;

/// One data unit per 8 lanes, kIdctIters groups of 32 units per workgroup. The unit's entries are
/// gathered from the symbol stream (aligned 4-byte reads of two entries) and de-zigzagged on the
/// way into LDS; everything else is zero. The lane of the column pass dequantises its column when it
/// reads it. Steps and int16 truncation points are those of the reference `idct_kernel`
/// (src/idct.cu:146-223): (int16)(coef * q) -> column pass -> row pass -> +128 -> clamp. The MCU
/// geometry (reference decode_transpose.cu:65-131) is applied when the 8x8 pixels are stored.
///
/// Two things bound a naive version: LDS instruction issue and the chain of dependent loads
/// (table entry -> symbol entries) paid once per tiny workgroup. So the block is staged TRANSPOSED
/// ([column][row]: zeroing is one 16-byte write, the column pass one 16-byte read), all table
/// entries of the workgroup are loaded up front, and the first entries of each lane are fetched two
/// iterations ahead.
///
/// With IslowJobs<JS> (IdctIslow) only the arithmetic differs: dequantisation in full int, jidctint.c's two passes
/// (islow8) with a 32-bit workspace between them, DESCALE by 11 and by 18, the range limit.
template <class JS>
__global__ __launch_bounds__(256) void idct_kernel(JS js)
{
    using X = typename IdctOf<JS>::type;
    constexpr bool kCrop = IsCropped<JS>::value;
    constexpr bool kDraft = IsDraft<JS>::value; // the 8x8 units of a JPEGGPU_EXT_SCALE_LIBJPEG job (draft_unit)
    static_assert(!kDraft || X::kIslow == (DraftOn<JS>::value == kDraftOn), "blocks of size 8 of that mode take the ISLOW arithmetic; LumaJobs: the reference's");
    __shared__ __attribute__((aligned(16))) int16_t s_blk[kIdctDuPerBlock][kIdctDuStride]; // [unit][col * 8 + row]
    // ISLOW: the int workspace between the passes, [unit][row * 8 + col] (+8: as s_blk)
    __shared__ __attribute__((aligned(16))) int s_ws[X::kIslow ? kIdctDuPerBlock : 1][X::kIslow ? kIdctDuStride : 4];
    // [quantisation table][column][row]: the 16 bytes a lane of the column pass multiplies its column with
    // ((int16)(coef * q), reference idct.cu:178-180: the low 16 bits of the product, whatever the signs)
    __shared__ __attribute__((aligned(16))) uint16_t s_qcol[4 * 64];
    // zig-zag index -> byte offset of the coefficient's transposed slot in a staged block. 64 bytes are 16 banks:
    // lanes that ask for different entries never collide (same word: broadcast).
    __shared__ __attribute__((aligned(16))) uint8_t s_slot[64];
    __shared__ uint2 s_px[2][kIdctDuPerBlock][9]; // finished pixel rows, [buffer][unit][row] (+1: bank spread)
    // Where the pixels of each of the workgroup's data units go, worked out ONCE per unit by lane = unit (reference
    // decode_transpose.cu:65-131 walks the same geometry): address of the unit's top-left pixel, pitch, how many of
    // its 8 columns / rows are inside the plane (0..8), and its quantisation table. The per-iteration code reads
    // 16 bytes instead of redoing two divisions and a dozen multiply-adds per lane and unit row.
    struct UnitGeo {
        uint32_t addr_lo, addr_hi;
        int pitch;
        // rows to store (0..8; 0 if no column is visible) | byte offset of the quantisation table in s_qcol (bits
        // 7-8) | visible columns << 12 | kGeoWhole: every field where one instruction picks it up
        uint32_t vis;
    };
    constexpr uint32_t kGeoWhole = 1u << 31; // all 8 columns visible and every row 8-byte aligned: one store per row
    __shared__ __attribute__((aligned(16))) UnitGeo s_geo[kIdctDuPerWg];

    const JobView J(js.get());
    const IdctParams& ip = J.ip;
    const int du0        = blockIdx.x * kIdctDuPerWg;
    const int num_du     = [&] {
        if constexpr (kDraft) return draft_num_du<0, DraftOn<JS>::value>(js.get());
        else return ip.num_du;
    }();
    if (du0 >= num_du) return;

    const int t  = threadIdx.x;
    const int r  = t & 7;  // column (pass 1) or row (pass 2) handled by this lane
    const int dl = t >> 3; // data unit inside the group

    // The records of the lane's units of all iterations, asked for before anything else and without a branch (a unit
    // past the end reads the last record and counts no entries): eight loads in flight at once. Behind an `if` each,
    // as up to round 4, the compiler waited for every one before it issued the next -- eight memory latencies in a
    // row in front of the first iteration, in a workgroup that lives for eight iterations.
    uint2_t rec[kIdctIters];
#pragma unroll
    for (int it = 0; it < kIdctIters; ++it) {
        const int w = min(du0 + it * kIdctDuPerBlock + dl, num_du - 1);
        if constexpr (kDraft) rec[it] = ld_global(J.du_tab + draft_unit<0>(js.get(), w).stream);
        else if constexpr (kCrop) rec[it] = ld_global(J.du_tab + window_unit(ip, js.get().win, w).stream); // (a window unit: its MCU's place in the stream)
        else rec[it] = ld_global(J.du_tab + w);
    }
    // (and the lane's byte and word of the job's geometry tables, below)
    const uint32_t unit_byte = reinterpret_cast<const uint8_t*>(ip.du_comp)[t & 31];
    const uint32_t comp_word = reinterpret_cast<const uint32_t*>(ip.comp_h)[t & 31];

    s_qcol[t] = J.qtables[(t & ~63) + (t & 7) * 8 + ((t >> 3) & 7)]; // [table][col][row] <- natural row * 8 + col
    if (t < 64) s_slot[zigzag_of(t >> 3, t & 7)] = static_cast<uint8_t>(((t & 7) * 8 + (t >> 3)) * 2); // natural row * 8 + col -> transposed slot col * 8 + row
    // Geometry, first half: which unit of which MCU, and the one load the rest depends on. Straight-line code (a unit
    // past the end works on the last one and is marked invisible): the loads of this prologue are then the
    // compiler's to count, and the first entries below travel while the geometry is worked out.
    const int gdu  = min(du0 + t, num_du - 1);
    const int grel = static_cast<int>(magic_quot(gdu, ip.du_per_mcu_mul, ip.du_per_mcu_shift));
    int gk         = gdu - grel * ip.du_per_mcu;
    // What the unit's place depends on sits in two small tables of the job: the MCU's units (component, block column,
    // block row: three arrays of 10 bytes) and the components (six arrays of 4 ints, then 4 plane pointers). Lane L of
    // every half wave loads byte L of the first and word L of the second -- loads that depend on nothing -- and a unit
    // then takes its values from the lanes that hold them (ds_bpermute: no memory behind it). Indexed loads, first
    // by the unit's place in the MCU, then by its component, were two more memory latencies in a row.
    static_assert(kMaxDuPerMcu == 10 && kMaxComp == 4 && sizeof(ip.plane[0]) == 8, "lane layout of the two tables");
    static_assert(offsetof(IdctParams, du_dx) == offsetof(IdctParams, du_comp) + 10 && offsetof(IdctParams, du_dy) == offsetof(IdctParams, du_comp) + 20 &&
                      offsetof(IdctParams, comp_h) >= offsetof(IdctParams, du_comp) + 32,
                  "32 bytes from du_comp on");
    static_assert(offsetof(IdctParams, comp_v) == offsetof(IdctParams, comp_h) + 16 && offsetof(IdctParams, size_x) == offsetof(IdctParams, comp_h) + 32 &&
                      offsetof(IdctParams, size_y) == offsetof(IdctParams, comp_h) + 48 && offsetof(IdctParams, pitch) == offsetof(IdctParams, comp_h) + 64 &&
                      offsetof(IdctParams, qidx) == offsetof(IdctParams, comp_h) + 80 && offsetof(IdctParams, plane) == offsetof(IdctParams, comp_h) + 96,
                  "32 words from comp_h on");
    const auto from_lane = [](int lane, uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(lane * 4, static_cast<int>(v))); };
    const int gmcu = grel + ip.first_mcu;
    int gmy        = static_cast<int>(magic_quot(gmcu, ip.mcus_x_mul, ip.mcus_x_shift));
    int gmx        = gmcu - gmy * ip.mcus_x;
    if constexpr (kCrop) { // the MCU's column and row in the window, whose top-left corner ip.plane is
        const WindowUnit u = window_unit(ip, js.get().win, gdu);
        gk = u.k, gmx = u.mx, gmy = u.my;
    }
    if constexpr (kDraft) {
        const WindowUnit u = draft_unit<0>(js.get(), gdu);
        gk = u.k, gmx = u.mx, gmy = u.my;
    }
    // a table entry that was never written (corrupt stream) must not lead out of the buffer
    uint32_t toff[kIdctIters], tcnt[kIdctIters];
    const uint64_t limit = J.sym_entries - 10 * kSymSectorStride; // a 128-entry gather from here stays inside
#pragma unroll
    for (int it = 0; it < kIdctIters; ++it) {
        const bool mine = du0 + it * kIdctDuPerBlock + dl < num_du;
        tcnt[it] = mine ? rec[it].y & 0xFFu : 0u; // entries (at most 127) | kUnitHasEscape
        toff[it] = static_cast<uint32_t>(rec[it].x < limit ? rec[it].x : limit);
    }
    // Nothing but the fetched words to place in any of this wave's units (no unit above 31 entries, none with an
    // escape: the record's flag sits above the count)? Asked once per wave, not once per iteration.
    uint32_t most = 0;
#pragma unroll
    for (int it = 0; it < kIdctIters; ++it) most = max(most, tcnt[it]);
    const bool plain = __ballot(most > 31u) == 0;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 zero4 = {0u, 0u, 0u, 0u};
    asm volatile("" : "+v"(zero4)); // four registers that stay zero: the compiler would set them up again in every iteration
    const uint2* const px_mine = &s_px[0][t & 31][t >> 5];
    const uint8_t* const qcol_mine = reinterpret_cast<const uint8_t*>(s_qcol) + r * 16;
    // Entry PAIRS per lane, fetched kDepth iterations ahead: the lane reads the aligned 32-bit words r, r + 8, ... of
    // the sector row its unit starts in, counted from the word that holds the unit's first entry. Eight words further
    // is the same word of the next sector (one 32-byte sector = 16 entries = 8 words): +2048 bytes. With an odd first
    // entry the low half of lane 0's first word belongs to the unit in front. The words are read whether the unit
    // reaches them or not (toff is clamped so that they lie inside the buffer; what is not the unit's is not placed):
    // without branches around the loads the compiler can count them, and the wait for one iteration's words leaves
    // the next one's in flight. (Up to round 4 the lanes read single entries under a compare and a branch each: twice
    // the loads, twice the address arithmetic, and one wait for everything.)
    constexpr int kPairs = 2;
    static_assert(kPairs * kSymSectorStride * 2 <= 4096 + 2048, "immediate offsets of the loads");
    constexpr int kDepth = 2; // iterations the fetches run ahead
    uint32_t pre[kIdctIters + kDepth][kPairs];
    const auto entry_at = [&](uint32_t index) -> uint32_t {
        return *reinterpret_cast<JG_GLOBAL const uint16_t*>(reinterpret_cast<JG_GLOBAL const uint8_t*>(J.sym) + index * 2u);
    };
    // Entry j of the unit sits in half (j + odd) & 1 of word (j + odd) / 2 counted as above; a lane's word k holds
    // the entries jb + 16 k and jb + 16 k + 1, jb = 2 r - odd.
    const auto prefetch = [&](uint32_t first, uint32_t (&out)[kPairs]) {
        // the word that holds the unit's first entry, r words on; past the end of the 8-word sector: the next sector
        const uint32_t word = first >> 1;
        const uint32_t over = ((word & 7u) + static_cast<uint32_t>(r)) & 8u;
        const uint32_t base = word * 4u + static_cast<uint32_t>(r) * 4u + over * ((kSymSectorStride * 2u - 32u) / 8u);
        JG_GLOBAL const uint8_t* stream = reinterpret_cast<JG_GLOBAL const uint8_t*>(J.sym);
#pragma unroll
        for (int k = 0; k < kPairs; ++k)
            out[k] = *reinterpret_cast<JG_GLOBAL const uint32_t*>(stream + (base + k * (kSymSectorStride * 2u)));
    };

    {
        // (the first entries: asked for behind the geometry's loads, so that waiting for those does not wait for these)
#pragma unroll
        for (int d = 0; d < kDepth; ++d) prefetch(toff[d], pre[d]);
        const int sc = static_cast<int>(from_lane(gk, unit_byte));
        const int dx = static_cast<int>(from_lane(10 + gk, unit_byte)), dy = static_cast<int>(from_lane(20 + gk, unit_byte));
        const int comp_h = static_cast<int>(from_lane(sc, comp_word)), comp_v = static_cast<int>(from_lane(4 + sc, comp_word));
        const int size_x = static_cast<int>(from_lane(8 + sc, comp_word)), size_y = static_cast<int>(from_lane(12 + sc, comp_word));
        const int pitch = static_cast<int>(from_lane(16 + sc, comp_word)), qidx = static_cast<int>(from_lane(20 + sc, comp_word));
        const uint64_t plane = static_cast<uint64_t>(from_lane(24 + 2 * sc, comp_word)) | static_cast<uint64_t>(from_lane(25 + 2 * sc, comp_word)) << 32;
        const int x0  = (gmx * comp_h + dx) * 8;
        const int y0  = (gmy * comp_v + dy) * 8;
        const int vx  = min(max(size_x - x0, 0), 8), vy = min(max(size_y - y0, 0), 8);
        const uint64_t a = plane + static_cast<uint64_t>(y0) * static_cast<uint32_t>(pitch) + static_cast<uint32_t>(x0);
        const bool whole = vx == 8 && ((a | static_cast<uint32_t>(pitch)) & 7u) == 0;
        const uint32_t vis = static_cast<uint32_t>(vx > 0 ? vy : 0) | static_cast<uint32_t>(qidx & 3) << 7 | static_cast<uint32_t>(vx) << 12 | (whole ? kGeoWhole : 0u);
        s_geo[t] = UnitGeo{static_cast<uint32_t>(a), static_cast<uint32_t>(a >> 32), pitch, du0 + t < num_du ? vis : 0u};
    }
    int16_t* blk = s_blk[dl];
    uint8_t* const blk_bytes = reinterpret_cast<uint8_t*>(blk);
    __syncthreads(); // s_qcol, s_slot, s_geo are loaded

#pragma unroll
    for (int it = 0; it < kIdctIters; ++it) {
        uint32_t ex[kPairs];
#pragma unroll
        for (int k = 0; k < kPairs; ++k) ex[k] = pre[it][k];
        if (it + kDepth < kIdctIters) prefetch(toff[it + kDepth], pre[it + kDepth]); // in flight while this one computes
        // The 8 lanes of a data unit sit in one wave and LDS executes a wave's instructions in order,
        // so the phases below need no workgroup barrier among themselves; only the pixel re-mapping
        // at the end crosses waves (one barrier per iteration, buffers alternate).
        *reinterpret_cast<u32x4*>(blk + r * 8) = zero4;

        const uint32_t qoff = s_geo[it * kIdctDuPerBlock + dl].vis & 0x180u;
        // place one coefficient, not yet dequantised: zig-zag index, value (its low 16 bits count)
        const auto put = [&](uint32_t zz, uint32_t value) { *reinterpret_cast<int16_t*>(blk_bytes + s_slot[zz]) = static_cast<int16_t>(value); };
        const uint32_t cnt = tcnt[it] & 0x7Fu;
        const bool odd     = (toff[it] & 1u) != 0;
        // Entry j of the unit (jg_defs.h): j == 0 is the DC value; an AC entry holds value << 6 | index; an entry
        // with index 0 behind one is the ESCAPE that carries the value's high bits. The unit's record says whether it
        // holds one (no photograph does).
        if (__builtin_expect(plain || __ballot((tcnt[it] & kUnitHasEscape) != 0) == 0, 1)) {
            // the look-ups first, all of them (an index of a word that was not loaded is 0): one LDS latency, not one per entry
            uint32_t slot[kPairs][2];
#pragma unroll
            for (int k = 0; k < kPairs; ++k) {
                slot[k][0] = s_slot[ex[k] & 63u];
                slot[k][1] = s_slot[(ex[k] >> 16) & 63u];
            }
            if (r == 0) blk[0] = static_cast<int16_t>(ex[0] >> ((toff[it] << 4) & 31u)); // DC: lane 0, the half the unit starts in
            // The lane's words hold the entries jb + c, c = 16 k + h, jb = 2 r - odd; an AC entry of the unit is one
            // with 1 <= jb + c < cnt: c < left, and for lane 0 not the DC or the entry in front of it.
            const int left = static_cast<int>(cnt) + static_cast<int>(toff[it] & 1u) - 2 * r;
#pragma unroll
            for (int k = 0; k < kPairs; ++k) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    bool mine = 16 * k + h < left;
                    if (k == 0 && h == 0) mine = mine && r != 0;
                    if (k == 0 && h == 1) mine = mine && !(r == 0 && odd);
                    if (mine)
                        *reinterpret_cast<int16_t*>(blk_bytes + slot[k][h]) = static_cast<int16_t>(static_cast<int32_t>(ex[k] << (16 - 16 * h)) >> 22);
                }
            }
            if (!plain) {
                for (uint32_t i = 16u * kPairs - (toff[it] & 1u) + static_cast<uint32_t>(r); i < cnt; i += 8) { // dense units only: entries behind the fetched words
                    const uint32_t e = entry_at(sym_advance(toff[it], i));
                    put(sym_entry_index(e), static_cast<uint32_t>(sym_entry_value(e)));
                }
            }
        } else {
            for (uint32_t i = r; i < cnt; i += 8) {
                const uint32_t e    = entry_at(sym_advance(toff[it], i));
                const uint32_t next = i + 1 < cnt ? entry_at(sym_advance(toff[it], i + 1)) : 1u;
                if (i == 0) put(0, e);
                else if (sym_entry_index(e) != 0)
                    put(sym_entry_index(e), static_cast<uint32_t>(sym_entry_index(next) == 0 ? sym_entry_value(e, next) : sym_entry_value(e)));
                asm volatile("" ::"v"(next)); // no load of this rare path is left in flight: the common path behind it would wait for it with everything else
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        uint2 o;
        if constexpr (X::kIslow) {
            int v[8];
            {
                int c[8], q[8];
                unpack8(*reinterpret_cast<const uint4*>(blk + r * 8), c); // column r
                const uint4 qc = *reinterpret_cast<const uint4*>(qcol_mine + qoff);
                const uint32_t qw[4] = {qc.x, qc.y, qc.z, qc.w};
#pragma unroll
                for (int i = 0; i < 8; ++i) q[i] = static_cast<int>((qw[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = c[i] * q[i]; // DEQUANTIZE in full int: |int16 * uint16| < 2^31
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // every column is read before the next iteration zeroes the block
            bool small = true;
#pragma unroll
            for (int i = 0; i < 8; ++i) small = small && static_cast<uint32_t>(v[i] + kIslowPass1Max) <= 2u * kIslowPass1Max;
            int* const ws = s_ws[dl];
            if (__builtin_expect(__ballot(!small) == 0, 1)) { // pass 1 in 32 bits: exact (kIslowPass1Max)
                int p[8];
                islow8(v, p);
#pragma unroll
                for (int i = 0; i < 8; ++i) ws[i * 8 + r] = (p[i] + (1 << 10)) >> 11; // DESCALE(.., CONST_BITS - PASS1_BITS), now [row][col]
            } else { // a coefficient the bound does not cover (16-bit quantisers, corrupt streams): jidctint.c's JLONG
                long long w[8], p[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) w[i] = v[i];
                islow8(w, p);
#pragma unroll
                for (int i = 0; i < 8; ++i) ws[i * 8 + r] = static_cast<int>((p[i] + (1ll << 10)) >> 11); // the int workspace keeps the low 32 bits
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            int w[8];
            {
                const uint4 a = *reinterpret_cast<const uint4*>(ws + r * 8), b = *reinterpret_cast<const uint4*>(ws + r * 8 + 4); // row r
                const uint32_t u[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int i = 0; i < 8; ++i) w[i] = static_cast<int>(u[i]);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // row reads precede the next iteration's workspace stores
            int p[8];
            islow8(w, p); // wrapping 32-bit: only bits 18..27 of each sum count (kIslowPass1Max)
            uint32_t px[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) px[i] = range_limit((p[i] + (1 << 17)) >> 18); // DESCALE(.., CONST_BITS + PASS1_BITS + 3)
            o.x = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
            o.y = px[4] | px[5] << 8 | px[6] << 16 | px[7] << 24;
        } else {
        int v[8];
        {
            uint4 col      = *reinterpret_cast<const uint4*>(blk + r * 8); // column r
            const uint4 qc = *reinterpret_cast<const uint4*>(qcol_mine + qoff);
            col.x = mul_lo_u16x2(col.x, qc.x), col.y = mul_lo_u16x2(col.y, qc.y), col.z = mul_lo_u16x2(col.z, qc.z), col.w = mul_lo_u16x2(col.w, qc.w);
            unpack8(col, v);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // every column is read before rows overwrite the block
        idct8(v);
#pragma unroll
        for (int i = 0; i < 8; ++i) blk[i * 8 + r] = static_cast<int16_t>(v[i] >> 16); // now [row][col]
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        unpack8(*reinterpret_cast<const uint4*>(blk + r * 8), v); // row r
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // row reads precede the next iteration's zeroing
        idct8<0x8000 + (128 << 16)>(v);

        o.x = finish_pixels(v[0], v[1], v[2], v[3]);
        o.y = finish_pixels(v[4], v[5], v[6], v[7]);
        }
        // A lane holds row r of unit dl; storing that directly makes every wave store touch ~40 cache
        // lines (8 units x 8 rows). Re-map through LDS: lane -> (row t / 32, unit t % 32), so that
        // consecutive lanes write the neighbouring 8-byte segments of one image row.
        s_px[it & 1][dl][r] = o;
        __syncthreads();
        // The next iteration's entries have had an iteration's time or more to arrive; asking for them HERE, in front
        // of the pixel stores, keeps those stores out of the wait (one counter counts loads and stores, and behind the
        // stores' branches the compiler can only wait for everything: with the wait at the first use every iteration
        // stood until its predecessor's pixels had reached L2 and its own entries had arrived, fetched a placement
        // phase earlier).
        if (it + 1 < kIdctIters) {
#pragma unroll
            for (int k = 0; k < kPairs; ++k) asm volatile("" : "+v"(pre[it + 1][k]));
        }
        {
            const int r2      = t >> 5;
            const int j       = t & 31;
            const UnitGeo g   = s_geo[it * kIdctDuPerBlock + j]; // all zero behind the last unit: nothing visible
            const int vx = (g.vis >> 12) & 15;
            if (r2 < static_cast<int>(g.vis & 15u)) {
                const uint2 w = px_mine[(it & 1) * (kIdctDuPerBlock * 9)];
                JG_GLOBAL uint8_t* row = reinterpret_cast<JG_GLOBAL uint8_t*>(
                    ((static_cast<uint64_t>(g.addr_hi) << 32) | g.addr_lo) + static_cast<uint64_t>(static_cast<uint32_t>(r2)) * static_cast<uint64_t>(static_cast<uint32_t>(g.pitch))); // one v_mad_u64_u32
                if (g.vis & kGeoWhole) {
                    st_global(reinterpret_cast<JG_GLOBAL uint2*>(row), w);
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        if (i < vx) row[i] = static_cast<uint8_t>((i < 4 ? w.x >> (8 * i) : w.y >> (8 * (i - 4))) & 0xFFu);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// scaled decoding (jpeggpu_ext_set_scale): the reduced inverse DCTs of libjpeg-turbo's jidctred.c
// ------------------------------------------------------------------------------------------------

/// jidctred.c's DESCALE: (x + 2^(n-1)) >> n, 64-bit (JLONG).
template <int n>
__device__ __forceinline__ long long descale(long long x)
{
    return (x + (1ll << (n - 1))) >> n;
}

constexpr int kRedConstBits = 13, kRedPass1Bits = 2; // jidctred.c CONST_BITS, PASS1_BITS

/// The 4-point part of jpeg_idct_4x4 (both passes), from the inputs of rows / columns 0, 1, 2, 3, 5, 6, 7:
/// outputs 0..3 before their DESCALE.
__device__ __forceinline__ void idct4_red(long long v0, long long v1, long long v2, long long v3, long long v5, long long v6, long long v7,
                                          long long (&o)[4])
{
    const long long t0 = v0 * (1ll << (kRedConstBits + 1));
    const long long t2 = v2 * 15137 - v6 * 6270;                       // FIX(1.847759065), FIX(0.765366865)
    const long long t10 = t0 + t2, t12 = t0 - t2;
    const long long a = -v7 * 1730 + v5 * 11893 - v3 * 17799 + v1 * 8697; // FIX(0.211164243), (1.451774981), (2.172734803), (1.061594337)
    const long long b = -v7 * 4176 - v5 * 4926 + v3 * 7373 + v1 * 20995;  // FIX(0.509795579), (0.601344887), (0.899976223), (2.562915447)
    o[0] = t10 + b;
    o[3] = t10 - b;
    o[1] = t12 + a;
    o[2] = t12 - a;
}

/// The 2-point part of jpeg_idct_2x2 (both passes), from the inputs of rows / columns 0, 1, 3, 5, 7: outputs 0, 1 before
/// their DESCALE.
__device__ __forceinline__ void idct2_red(long long v0, long long v1, long long v3, long long v5, long long v7, long long (&o)[2])
{
    const long long t10 = v0 * (1ll << (kRedConstBits + 2));
    const long long t0  = -v7 * 5906 + v5 * 6967 - v3 * 10426 + v1 * 29692; // FIX(0.720959822), (0.850430095), (1.272758580), (3.624509785)
    o[0] = t10 + t0;
    o[1] = t10 - t0;
}

constexpr int kScaledDuPerWg = kIdctDuPerWg; // one data unit per lane, the grid of idct_kernel

/// Scaled decode: one data unit per lane writes an N x N block, N = 8 >> kLg, at (block column * N, block row * N) of its
/// plane, clipped to the scaled plane size. One instantiation per scale, launched for the scales a call holds: jobs of
/// another scale (one job per blockIdx.y) leave at once. (One kernel that branched on the job's scale needed the
/// registers of its largest branch, 151 VGPRs, for the 1/8 path as well.)
///   * 1/8 (jpeg_idct_1x1): a gather and a store -- the unit's table record, its first (DC) entry, one quantiser. Units in
///     stream order are neighbouring blocks of an MCU row, so neighbouring lanes store neighbouring bytes of a few rows.
///   * 1/4, 1/2 (jpeg_idct_2x2, jpeg_idct_4x4): the unit's entries (and escapes, as in idct_kernel's rare path) are
///     de-zigzagged into the lane's own column of LDS, a mask of 64 bits says which slots hold one (nothing to zero),
///     and the two passes run in registers with jidctred.c's integer arithmetic: dequantisation in full int, 64-bit
///     products, a 32-bit workspace between the passes, the range limit above.
template <class JS, int kLg>
__global__ __launch_bounds__(256) void idct_scaled_kernel(JS js)
{
    __shared__ int16_t s_coef[64][kScaledDuPerWg]; // [natural index][lane]: coefficients as stored, not yet dequantised
    __shared__ uint16_t s_q[4 * 64];               // the quantisation tables, natural order
    __shared__ uint8_t s_nat[64];                  // zig-zag index -> natural index

    const JobView J(js.get());
    const IdctParams& ip = J.ip;
    constexpr int lg     = kLg;
    constexpr bool kDraft = IsDraft<JS>::value; // the units of this size of a JPEGGPU_EXT_SCALE_LIBJPEG job (draft_unit)
    const int du0        = blockIdx.x * kScaledDuPerWg;
    int num_du           = ip.num_du;
    if constexpr (kDraft) num_du = draft_num_du<kLg>(js.get());
    else if (ip.scale_log2 != kLg) return; // (uniform)
    if (du0 >= num_du) return;
    const int t  = threadIdx.x;
    int du = min(du0 + t, num_du - 1);

    // geometry (idct_kernel's, at N pixels per block side)
    int k, mx, my;
    if constexpr (kDraft) {
        const WindowUnit u = draft_unit<kLg>(js.get(), du);
        du = u.stream, k = u.k, mx = u.mx, my = u.my;
    } else if constexpr (IsCropped<JS>::value) { // a window unit (idct_kernel): its MCU's place in the stream, and in the window
        const WindowUnit u = window_unit(ip, js.get().win, du);
        du = u.stream, k = u.k, mx = u.mx, my = u.my;
    } else {
        const int rel = static_cast<int>(magic_quot(du, ip.du_per_mcu_mul, ip.du_per_mcu_shift));
        k             = du - rel * ip.du_per_mcu;
        const int mcu = rel + ip.first_mcu;
        my            = static_cast<int>(magic_quot(mcu, ip.mcus_x_mul, ip.mcus_x_shift));
        mx            = mcu - my * ip.mcus_x;
    }
    const int sc  = ip.du_comp[k];
    const int n   = 8 >> lg;
    const int x0  = (mx * ip.comp_h[sc] + ip.du_dx[k]) * n;
    const int y0  = (my * ip.comp_v[sc] + ip.du_dy[k]) * n;
    const int vx  = min(ip.size_x[sc] - x0, n), vy = min(ip.size_y[sc] - y0, n);
    const bool active = du0 + t < num_du && vx > 0 && vy > 0;
    const int pitch   = ip.pitch[sc];
    const int qbase   = (ip.qidx[sc] & 3) * 64;
    JG_GLOBAL uint8_t* const out = as_global(ip.plane[sc]) + static_cast<int64_t>(y0) * pitch + x0;

    const uint2_t rec = ld_global(J.du_tab + du);
    // a table entry that was never written (corrupt stream) must not lead out of the buffer: 127 entries from here stay inside
    const uint64_t limit = J.sym_entries - 10 * kSymSectorStride;
    const uint32_t first = static_cast<uint32_t>(rec.x < limit ? rec.x : limit);
    const uint32_t cnt   = rec.y & 0x7Fu;
    const auto entry_at  = [&](uint32_t index) -> uint32_t { return J.sym[index]; };
    const int dc         = static_cast<int16_t>(entry_at(first)); // the unit's first entry: its DC coefficient, absolute

    if constexpr (lg == 3) { // 1/8: jpeg_idct_1x1
        if (active) *out = static_cast<uint8_t>(range_limit(static_cast<int>(descale<3>(static_cast<long long>(dc) * J.qtables[qbase]))));
        return;
    }

    s_q[t] = J.qtables[t];
    if (t < 64) {
        constexpr uint8_t nat[64] = JG_ORDER_NATURAL;
        s_nat[t] = nat[t];
    }
    __syncthreads();
    if (!active) return;

    // the unit's AC entries, eight loads at a time (the clamp above keeps entries up to 127 + 8 inside the buffer)
    uint64_t mask  = 0;
    const bool esc = (rec.y & kUnitHasEscape) != 0;
    for (uint32_t i0 = 1; i0 < cnt; i0 += 8) {
        uint32_t e[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) { // (sym_advance, written out: a call here widens what the compiler knows of that function's
                                      // argument in idct_kernel, and its code there changed)
            const uint32_t w = (first & (kSymSectorEntries - 1u)) + i0 + j;
            e[j]             = entry_at((first & ~(kSymSectorEntries - 1u)) + (w / kSymSectorEntries) * kSymSectorStride + (w & (kSymSectorEntries - 1u)));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t zz = sym_entry_index(e[j]);
            if (i0 + j < cnt && zz != 0) { // index 0 behind the DC: the escape of the coefficient in front
                const int v       = esc && i0 + j + 1 < cnt && sym_entry_index(e[j + 1]) == 0 ? sym_entry_value(e[j], e[j + 1]) : sym_entry_value(e[j]);
                const uint32_t nt = s_nat[zz];
                s_coef[nt][t]     = static_cast<int16_t>(v);
                mask |= 1ull << nt;
            }
        }
    }
    // dequantised coefficient (row, col): DEQUANTIZE in full int
    const auto coef = [&](int row, int col) -> long long {
        const int i = row * 8 + col;
        const int c = i == 0 ? dc : ((mask >> i) & 1u) ? s_coef[i][t] : 0;
        return static_cast<long long>(c * static_cast<int>(s_q[qbase + i]));
    };

    if constexpr (lg == 1) { // 1/2: jpeg_idct_4x4 (column 4 and, in the second pass, workspace column 4 are never used)
        int ws[4][8];
#pragma unroll
        for (int col = 0; col < 8; ++col) {
            if (col == 4) continue;
            long long o[4];
            idct4_red(coef(0, col), coef(1, col), coef(2, col), coef(3, col), coef(5, col), coef(6, col), coef(7, col), o);
#pragma unroll
            for (int r = 0; r < 4; ++r) ws[r][col] = static_cast<int>(descale<kRedConstBits - kRedPass1Bits + 1>(o[r]));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            long long o[4];
            idct4_red(ws[r][0], ws[r][1], ws[r][2], ws[r][3], ws[r][5], ws[r][6], ws[r][7], o);
            uint32_t px = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) px |= range_limit(static_cast<int>(descale<kRedConstBits + kRedPass1Bits + 3 + 1>(o[c]))) << (8 * c);
            if (r < vy) {
                JG_GLOBAL uint8_t* row = out + static_cast<int64_t>(r) * pitch;
                if (vx == 4 && (reinterpret_cast<uintptr_t>(row) & 3u) == 0) {
                    *reinterpret_cast<JG_GLOBAL uint32_t*>(row) = px;
                } else {
                    for (int c = 0; c < vx; ++c) row[c] = static_cast<uint8_t>(px >> (8 * c));
                }
            }
        }
    } else { // 1/4: jpeg_idct_2x2 (rows and columns 0, 1, 3, 5, 7)
        int ws[2][8];
#pragma unroll
        for (int col = 0; col < 8; ++col) {
            if (col == 2 || col == 4 || col == 6) continue;
            long long o[2];
            idct2_red(coef(0, col), coef(1, col), coef(3, col), coef(5, col), coef(7, col), o);
#pragma unroll
            for (int r = 0; r < 2; ++r) ws[r][col] = static_cast<int>(descale<kRedConstBits - kRedPass1Bits + 2>(o[r]));
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            long long o[2];
            idct2_red(ws[r][0], ws[r][1], ws[r][3], ws[r][5], ws[r][7], o);
            const uint32_t p0 = range_limit(static_cast<int>(descale<kRedConstBits + kRedPass1Bits + 3 + 2>(o[0])));
            const uint32_t p1 = range_limit(static_cast<int>(descale<kRedConstBits + kRedPass1Bits + 3 + 2>(o[1])));
            if (r < vy) {
                JG_GLOBAL uint8_t* row = out + static_cast<int64_t>(r) * pitch;
                if (vx == 2 && (reinterpret_cast<uintptr_t>(row) & 1u) == 0) {
                    *reinterpret_cast<JG_GLOBAL uint16_t*>(row) = static_cast<uint16_t>(p0 | p1 << 8);
                } else {
                    row[0] = static_cast<uint8_t>(p0);
                    if (vx == 2) row[1] = static_cast<uint8_t>(p1);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------

/// The IDCT stage of a launch; G: the job sources' geometry (Plain: every unit in stream order, CropJobs: MCU windows).
template <class X>
using Plain = X;
template <template <class> class G, class JS>
hipError_t launch_idct(const JS& js, const JobExtent& e, int grid_y, hipStream_t stream)
{
    // every kernel of the stage on one grid: 256 data units per workgroup, a job per blockIdx.y
    static_assert(kScaledDuPerWg == kIdctDuPerWg, "one grid for both");
    const auto launch = [&](auto kernel, const auto& source) { kernel<<<dim3(e.max_idct_blocks, grid_y), 256, 0, stream>>>(source); };
    // full-size jobs: idct_kernel, one instantiation per IDCT method present (jpeggpu_ext_set_idct); scaled ones
    // (jpeggpu_ext_set_scale): idct_scaled_kernel, one launch per scale present. Only a batch can hold several kinds;
    // each instantiation then sees the other kinds' jobs as empty. A call without ISLOW jobs launches what it did before.
    if (e.scales & 1u) {
        const bool alone = e.scales == 1u; // no scaled job
        constexpr bool batch = std::is_same<JS, JobArray>::value;
        if (e.methods == (1u << kIdctReference)) {
            if (alone) {
                launch(idct_kernel<G<JS>>, G<JS>{js});
            } else {
                if constexpr (batch)
                    launch(idct_kernel<G<JobArrayFullSize>>, G<JobArrayFullSize>{JobArrayFullSize{js.jobs}});
                else
                    return hipErrorInvalidValue; // the scans of one image share its scale
            }
        } else if (e.methods == (1u << kIdctIslow) && alone) {
            launch(idct_kernel<IslowJobs<G<JS>>>, IslowJobs<G<JS>>{G<JS>{js}});
        } else {
            if constexpr (batch) {
                using Ref = G<JobArrayFullSizeOf<kIdctReference>>;
                using Islow = IslowJobs<G<JobArrayFullSizeOf<kIdctIslow>>>;
                if (e.methods & (1u << kIdctReference)) launch(idct_kernel<Ref>, Ref{{js.jobs}});
                launch(idct_kernel<Islow>, Islow{{{js.jobs}}});
            } else {
                return hipErrorInvalidValue; // the scans of one image share its scale and method
            }
        }
    }
    if (e.scales & 2u) launch(idct_scaled_kernel<G<JS>, 1>, G<JS>{js});
    if (e.scales & 4u) launch(idct_scaled_kernel<G<JS>, 2>, G<JS>{js});
    if (e.scales & 8u) launch(idct_scaled_kernel<G<JS>, 3>, G<JS>{js});
    // jobs of JPEGGPU_EXT_SCALE_LIBJPEG: one launch per block size their components have (IdctDraft; blocks past a class's
    // units leave at once: the grid is that of all units)
    using D = DraftJobs<JS>;
    if (e.draft_sizes & 1u) launch(idct_kernel<IslowJobs<D>>, IslowJobs<D>{D{js}});
    if (e.draft_sizes & 2u) launch(idct_scaled_kernel<D, 1>, D{js});
    if (e.draft_sizes & 4u) launch(idct_scaled_kernel<D, 2>, D{js});
    if (e.draft_sizes & 8u) launch(idct_scaled_kernel<D, 3>, D{js});
    if (e.luma_reference) launch(idct_kernel<LumaJobs<JS>>, LumaJobs<JS>{js});
    return hipGetLastError();
}

/// The stage for one job source: nothing to launch for jobs without data units; a call that holds a cropped job
/// (jpeggpu_ext_set_crop) launches the CropJobs instantiations, for all of its jobs.
template <class JS>
hipError_t launch_idct_any(const JS& js, const JobExtent& e, int grid_y, hipStream_t stream)
{
    if (e.max_idct_blocks == 0) return hipSuccess;
    return e.crop ? launch_idct<CropJobs>(js, e, grid_y, stream) : launch_idct<Plain>(js, e, grid_y, stream);
}

} // namespace

hipError_t launch_idct_job(const ScanJob& job, const JobExtent& e, hipStream_t stream)
{
    return launch_idct_any(JobByValue{job}, e, 1, stream);
}

hipError_t launch_idct_scans(const ScanJob (&jobs)[kMaxScans], int num_jobs, const JobExtent& e, hipStream_t stream)
{
    JobsByValue js{};
    for (int i = 0; i < num_jobs; ++i) js.jobs[i] = jobs[i];
    return launch_idct_any(js, e, num_jobs, stream);
}

hipError_t launch_idct_device_job(const ScanJob* d_job, const JobExtent& e, hipStream_t stream)
{
    return launch_idct_any(JobSingle{d_job}, e, 1, stream);
}

hipError_t launch_idct_batch(const ScanJob* d_jobs, int num_jobs, const JobExtent& e, hipStream_t stream)
{
    return launch_idct_any(JobArray{d_jobs}, e, num_jobs, stream);
}

} // namespace jg
