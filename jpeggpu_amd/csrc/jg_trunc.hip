// jg_trunc.hip -- the decode of a file that ended early (jpeggpu_ext_set_truncated), as libjpeg finishes it when Pillow hands it
// a fake EOI (ImageFile.LOAD_TRUNCATED_IMAGES; INTEGRATION.md, "Truncated files"):
//   * behind the last real bit the bit reader delivers zero bits; the first MCU that needs a bit that does not exist is
//     finished from them (jdhuff.c, jpeg_fill_bit_buffer: insufficient_data);
//   * every MCU behind that one, to the end of the scan, keeps the zeros it was cleared to: no coefficient, DC 0;
//   * a run of zeros that overshoots the block puts its coefficient at index 63 (jpeg_natural_order's padding).
// The host walk (jg_reader.cpp, walk_scan) appends subsequences of zeros to the segment the data ends in, and the next restart
// interval as a segment of zeros alone, so the Huffman stages decode "data, then zero bits" as they decode anything else, and
// their kernels are not touched. Three small kernels do the rest, for the truncated scans of a call only:
//   trunc_prepare  in front of the Huffman stages: zero those subsequences in the tiled destuffed buffer, mirrored slots
//                  included (jg_defs.h), and give them their segment (destuff_kernel does both for subsequences that hold data);
//   trunc_find     behind the write pass: one lane walks the symbols from the synchronised start state of the subsequence
//                  that holds the last real bit to the end of the MCU in flight there, finds the first symbol that ends behind
//                  that bit -- its MCU is the last one decoded -- and rewrites the entry of an overshooting coefficient, which
//                  the write pass's entry format cannot express (index >= 64);
//   trunc_fill     every data unit behind that MCU becomes {one entry: DC 0} in the data-unit table, whatever the write pass
//                  left there; the entry is one spare entry of the symbol stream that no subsequence's region covers.
// Nothing is handed to the host: the MCU stays in d_tmp (TruncParams::state).
#include "jg_trunc.hpp"

#include "jg_huff_core.h"

#include <hip/hip_runtime.h>

namespace jg {

namespace {

constexpr int kT = 256;          // lanes per workgroup: four waves of 64
constexpr int kFillBlocks = 64;  // workgroups of trunc_fill per scan (grid-stride over the data units)

struct TruncByValue {
    ScanJob job;
    TruncParams tp;
    __device__ __forceinline__ const ScanJob& get() const { return job; }
    __device__ __forceinline__ const TruncParams& params() const { return tp; }
};
struct TruncArray {
    const TruncRef* refs;
    __device__ __forceinline__ const ScanJob& get() const { return *refs[blockIdx.y].job; }
    __device__ __forceinline__ const TruncParams& params() const { return refs[blockIdx.y].tp; }
};

/// The spare entry of the symbol stream that holds the DC of an emptied data unit: the first of the 16 sector strides behind
/// the regions (sym_buffer_entries), in front of the IDCT's clamp (sym_entries - 10 strides).
__device__ __forceinline__ uint32_t zero_entry(const ScanJob& j) { return static_cast<uint32_t>(j.sym_entries - 16u * kSymSectorStride); }

/// Rows [r0, r1) of the tiled destuffed buffer zeroed, with the copies their words have in the neighbouring rows, and given
/// to segment `seg`.
__device__ void zero_rows(const ScanJob& j, int r0, int r1, int seg)
{
    const int W         = j.sp.subseq_words;
    const int log2w     = 31 - __clz(W);
    uint32_t* const dst = reinterpret_cast<uint32_t*>(j.destuffed);
    const int rows      = r1 - r0;
    if (rows <= 0) return;
    for (int i = static_cast<int>(threadIdx.x); i < rows * W; i += kT) {
        const uint32_t row = static_cast<uint32_t>(r0 + i / W), k = static_cast<uint32_t>(i % W);
        dst[tiled_slot(row, k + kRowLeadWords, log2w)] = 0u;
        if (k < static_cast<uint32_t>(kRowTailWords) && row > 0) dst[tiled_slot(row - 1, static_cast<uint32_t>(W) + kRowLeadWords + k, log2w)] = 0u;
        if (k == static_cast<uint32_t>(W) - 1u) dst[tiled_slot(row + 1, 0, log2w)] = 0u; // (behind the last subsequence: spare rows)
    }
    for (int i = static_cast<int>(threadIdx.x); i < rows; i += kT) j.seg_idx[r0 + i] = seg;
}

template <class JS>
__global__ __launch_bounds__(kT) void trunc_prepare(JS js)
{
    const ScanJob& j      = js.get();
    const TruncParams& tp = js.params();
    const int B           = j.sp.subseq_words * 4;
    const Segment cut     = j.segments[tp.cut_segment];
    const int data_rows   = static_cast<int>((tp.end_bit / 8u + static_cast<uint32_t>(B) - 1u) / static_cast<uint32_t>(B));
    zero_rows(j, cut.subseq_offset + data_rows, min(cut.subseq_offset + cut.subseq_count, j.sp.num_subseq), tp.cut_segment);
    if (tp.zero_segment >= 0) {
        const Segment z = j.segments[tp.zero_segment];
        zero_rows(j, z.subseq_offset, min(z.subseq_offset + z.subseq_count, j.sp.num_subseq), tp.zero_segment);
    }
}

/// The bits of one segment for the walk: words [w0, w0 + n) of it staged in LDS by the workgroup (a lone lane that fetched
/// every symbol's bits from memory took two dependent loads per symbol), anything else from the main copies of the tiled
/// buffer's words (stored most significant byte first). `buf` null: a segment of zeros, nothing is read.
constexpr int kWalkWords = 1024;
struct WalkBits {
    const uint32_t* buf; // the tiled destuffed buffer
    uint32_t word0;      // linear word of the segment's first one
    int log2w;
    const uint32_t* staged;
    int w0, n;
    __device__ __forceinline__ uint32_t word(int w) const
    {
        if (!buf) return 0u;
        if (w >= w0 && w < w0 + n) return staged[w - w0];
        return buf[tiled_word(word0 + static_cast<uint32_t>(w), log2w)];
    }
    /// 32 bits at bit `p` of the segment
    __device__ __forceinline__ uint32_t at(int p) const
    {
        const uint32_t hi = word(p >> 5), lo = word((p >> 5) + 1);
        const int sh      = p & 31;
        return sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
    }
};

/// One lane walks segment `seg_i` from state (p, c, z) with `du` data units of the segment complete, up to the end of the MCU
/// in which a symbol first ends behind bit `end_bit`, or to the segment's last data unit. Returns that MCU (segment-relative),
/// or -1 if every symbol of the segment's data units fits. Entries of overshooting coefficients met on the way are rewritten.
__device__ int walk_to_cut(const ScanJob& j, const uint8_t* tabs, const WalkBits& bits, int seg_i, int p, int c, int z, int du, uint32_t end_bit)
{
    const ScanParams& sp = j.sp;
    const Segment seg    = j.segments[seg_i];
    const int seg_mcu0   = seg_i * sp.mcus_per_segment;
    const int seg_mcus   = min(sp.mcus_per_segment, sp.total_mcus - seg_mcu0);
    int limit_du         = seg_mcus * sp.du_per_mcu;
    const int last_bit   = seg.subseq_count * sp.subseq_words * 32 - 64; // the walk stays inside the segment's subsequences
    const uint64_t clamp = j.sym_entries - 10u * kSymSectorStride;
    int cut_mcu          = -1;
    c = c < sp.du_per_mcu ? c : 0, z &= 63; // (a synchronised state holds nothing else)
    // a data unit is at most 64 symbols; the walk covers at most two subsequences and one MCU
    const int max_symbols = 2 * sp.subseq_words * 32 + 64 * kMaxDuPerMcu + 64;
    for (int it = 0; it < max_symbols && du < limit_du; ++it) {
        if (p > last_bit) { // (cannot happen while the host keeps truncation_tail_bytes of zeros: end the walk as a cut)
            if (cut_mcu < 0) cut_mcu = du / sp.du_per_mcu;
            break;
        }
        const CursorEntry cur = *reinterpret_cast<const CursorEntry*>(tabs + sp.cursor_off + 16u * static_cast<uint32_t>(c));
        const bool is_dc      = z == 0;
        const uint32_t peek   = bits.at(p);
        const TabPtr tab      = tabs + (is_dc ? (cur.tabs & 0xFFFFu) : (cur.tabs >> 16));
        uint32_t e            = ld_u16(tab + 2u * (peek >> (is_dc ? 32 - kLutBitsDc : 32 - kLutBitsAc))) & (kEntrySlow - 1u);
        if ((e & 31u) == 0) e = huff_second_level(tab, e, peek, is_dc);
        const int total = e & 31, s = (e >> 5) & 15;
        if (cut_mcu < 0 && static_cast<uint32_t>(p + total) > end_bit) { // the first symbol that needs a bit that does not exist
            cut_mcu  = du / sp.du_per_mcu;
            limit_du = min(limit_du, (cut_mcu + 1) * sp.du_per_mcu);
        }
        p += total;
        const int zp = z - 1 + static_cast<int>(e >> 9); // index of the symbol's coefficient
        if (cut_mcu >= 0 && !is_dc && s != 0 && zp >= 64) {
            // libjpeg stores it at index 63. The write pass stored {value << 6 | zp}, the unit's last entry (an escape entry
            // behind it from category 10 on): index zp - 64, and zp's bit 6 in the value.
            const uint2_t rec  = j.du_tab[seg_mcu0 * sp.du_per_mcu + du];
            const uint32_t cnt = rec.y & 0x7Fu, back = s >= kEscapeFromCategory ? 2u : 1u;
            if (cnt > back && rec.x < clamp) {
                const int v = extend_bits(bits_field(peek, total, s), s);
                j.sym[sym_advance(rec.x, cnt - back)] = static_cast<uint16_t>(sym_entry_ac(63, v));
            }
        }
        if (zp >= 63) {
            ++du;
            c = c + 1 == sp.du_per_mcu ? 0 : c + 1;
            z = 0;
        } else {
            z = zp + 1;
        }
    }
    return cut_mcu;
}

template <class JS>
__global__ __launch_bounds__(kT) void trunc_find(JS js)
{
    __shared__ uint32_t s_sum[kT];
    __shared__ uint32_t s_bits[kWalkWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[(kMaxTablePack + 3) / 4];
    const ScanJob& j      = js.get();
    const TruncParams& tp = js.params();
    const ScanParams& sp  = j.sp;
    const Segment cut     = j.segments[tp.cut_segment];
    const int sub_bits    = sp.subseq_words * 32;
    // the subsequence that holds the first missing bit; the walk starts at its synchronised start state, which lies at or
    // in front of that bit: the exit state of the subsequence before it, or the segment's start
    const int rel = min(static_cast<int>(tp.end_bit / static_cast<uint32_t>(sub_bits)), cut.subseq_count - 1);
    // coefficient slots of the segment in front of it: 64 per complete data unit, plus the index inside the open one
    uint32_t n = 0;
    for (int i = static_cast<int>(threadIdx.x); i < rel; i += kT) n += static_cast<uint32_t>(j.st_n[cut.subseq_offset + i]);
    s_sum[threadIdx.x] = n;
    __syncthreads();
    for (int d = kT / 2; d > 0; d >>= 1) {
        if (static_cast<int>(threadIdx.x) < d) s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
        __syncthreads();
    }
    int p = 0, c = 0, z = 0;
    if (rel > 0) {
        p            = j.st_p[cut.subseq_offset + rel - 1];
        const int cz = j.st_cz[cut.subseq_offset + rel - 1];
        c = cz & 0xFF, z = cz >> 8;
        p = max(p, 0);
    }
    // the scan's table pack and the bits from the start state on, into LDS: all the one lane then reads
    const int log2w = 31 - __clz(sp.subseq_words);
    WalkBits bits{reinterpret_cast<const uint32_t*>(j.destuffed), static_cast<uint32_t>(cut.subseq_offset) << log2w, log2w, s_bits, max(p, 0) >> 5, 0};
    bits.n = max(min(kWalkWords, cut.subseq_count * sp.subseq_words - bits.w0), 0);
    for (int i = static_cast<int>(threadIdx.x); i < bits.n; i += kT) s_bits[i] = bits.buf[tiled_word(bits.word0 + static_cast<uint32_t>(bits.w0 + i), log2w)];
    const int tab_words = static_cast<int>(min(sp.tab_bytes, kMaxTablePack) + 3u) / 4;
    for (int i = static_cast<int>(threadIdx.x); i < tab_words; i += kT) s_tab[i] = reinterpret_cast<const uint32_t*>(j.tables)[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint8_t* const tabs = reinterpret_cast<const uint8_t*>(s_tab);
    const int total_du = sp.total_mcus * sp.du_per_mcu;
    int mcu            = walk_to_cut(j, tabs, bits, tp.cut_segment, p, c, z, static_cast<int>(s_sum[0] >> 6), tp.end_bit);
    int first_empty    = total_du, cut_mcu = -1;
    if (mcu >= 0) {
        cut_mcu = tp.cut_segment * sp.mcus_per_segment + mcu;
    } else if (tp.zero_segment >= 0) {
        // the segment is complete and no bit was missing: the next interval's first MCU is decoded from zero bits alone
        (void)walk_to_cut(j, tabs, WalkBits{nullptr, 0u, log2w, s_bits, 0, 0}, tp.zero_segment, 0, 0, 0, 0, 0u);
        cut_mcu = tp.zero_segment * sp.mcus_per_segment;
    }
    if (cut_mcu >= 0) first_empty = min((cut_mcu + 1) * sp.du_per_mcu, total_du);
    tp.state[0] = static_cast<uint32_t>(first_empty);
    tp.state[1] = static_cast<uint32_t>(cut_mcu);
}

template <class JS>
__global__ __launch_bounds__(kT) void trunc_fill(JS js)
{
    const ScanJob& j      = js.get();
    const TruncParams& tp = js.params();
    const int total_du    = j.sp.total_mcus * j.sp.du_per_mcu;
    const uint32_t zero   = zero_entry(j);
    if (blockIdx.x == 0 && threadIdx.x == 0) j.sym[zero] = 0;
    const uint2_t empty{zero, 1u};
    for (int du = max(static_cast<int>(tp.state[0]), 0) + static_cast<int>(blockIdx.x) * kT + static_cast<int>(threadIdx.x); du < total_du; du += kFillBlocks * kT)
        j.du_tab[du] = empty;
}

} // namespace

hipError_t launch_trunc_prepare(const ScanJob& job, const TruncParams& tp, hipStream_t stream)
{
    hipLaunchKernelGGL(trunc_prepare<TruncByValue>, dim3(1), dim3(kT), 0, stream, TruncByValue{job, tp});
    return hipGetLastError();
}

hipError_t launch_trunc_prepare_batch(const TruncRef* d_refs, int num_refs, hipStream_t stream)
{
    if (num_refs <= 0) return hipSuccess;
    hipLaunchKernelGGL(trunc_prepare<TruncArray>, dim3(1, static_cast<unsigned>(num_refs)), dim3(kT), 0, stream, TruncArray{d_refs});
    return hipGetLastError();
}

hipError_t launch_trunc_finish(const ScanJob& job, const TruncParams& tp, hipStream_t stream)
{
    hipLaunchKernelGGL(trunc_find<TruncByValue>, dim3(1), dim3(kT), 0, stream, TruncByValue{job, tp});
    hipLaunchKernelGGL(trunc_fill<TruncByValue>, dim3(kFillBlocks), dim3(kT), 0, stream, TruncByValue{job, tp});
    return hipGetLastError();
}

hipError_t launch_trunc_finish_batch(const TruncRef* d_refs, int num_refs, hipStream_t stream)
{
    if (num_refs <= 0) return hipSuccess;
    hipLaunchKernelGGL(trunc_find<TruncArray>, dim3(1, static_cast<unsigned>(num_refs)), dim3(kT), 0, stream, TruncArray{d_refs});
    hipLaunchKernelGGL(trunc_fill<TruncArray>, dim3(kFillBlocks, static_cast<unsigned>(num_refs)), dim3(kT), 0, stream, TruncArray{d_refs});
    return hipGetLastError();
}

} // namespace jg
