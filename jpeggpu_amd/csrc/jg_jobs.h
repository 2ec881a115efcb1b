// jg_jobs.h -- what a kernel of the decode path sees of its job: the view of a ScanJob whose pointers are qualified as
// global memory, and the job sources (one job by value, the scans of one image, an array indexed by blockIdx.y, one job
// in device memory). Internal to the two device sources that run on ScanJobs, jg_kernels.hip (the entropy pass) and
// jg_idct.hip (the IDCT stage): everything sits in an unnamed namespace, so that each of them names its kernels as
// jg::(anonymous)::kernel<source>.
#ifndef JG_JOBS_H_
#define JG_JOBS_H_

#include "jg_defs.h"

#include <hip/hip_runtime.h>

namespace jg {

namespace {

/// Pointers read out of a job that lives in memory are generic to the compiler, and generic (flat) loads
/// and stores count against lgkmcnt as well as vmcnt: every wait for an LDS table read would also wait for
/// the bitstream word prefetched one refill ahead. The kernels therefore work on a view of the job whose
/// pointers are qualified as global memory (kernel arguments passed by value are inferred global anyway).
#define JG_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ JG_GLOBAL T* as_global(T* p)
{
    return (JG_GLOBAL T*)p;
}

/// Class types do not copy through address-space-qualified pointers: move them as vectors of dwords.
template <class T>
__device__ __forceinline__ T ld_global(JG_GLOBAL const T* p)
{
    static_assert(sizeof(T) % 4 == 0 && alignof(T) >= 4, "dword-sized objects only");
    typedef uint32_t V __attribute__((ext_vector_type(sizeof(T) / 4)));
    const V v = *reinterpret_cast<JG_GLOBAL const V*>(p);
    return __builtin_bit_cast(T, v);
}
template <class T>
__device__ __forceinline__ void st_global(JG_GLOBAL T* p, const T& value)
{
    static_assert(sizeof(T) % 4 == 0 && alignof(T) >= 4, "dword-sized objects only");
    typedef uint32_t V __attribute__((ext_vector_type(sizeof(T) / 4)));
    *reinterpret_cast<JG_GLOBAL V*>(p) = __builtin_bit_cast(V, value);
}

struct JobView {
    JG_GLOBAL const uint8_t* bytes;
    JG_GLOBAL const DestuffChunk* chunks;
    JG_GLOBAL const Segment* segments;
    JG_GLOBAL const uint8_t* tables;
    JG_GLOBAL const uint8_t* tables_sync;
    JG_GLOBAL const uint16_t* qtables;
    JG_GLOBAL uint8_t* destuffed;
    JG_GLOBAL int* seg_idx;
    JG_GLOBAL int* st_p;
    JG_GLOBAL int* st_n;
    JG_GLOBAL int* st_cz;
    JG_GLOBAL uint32_t* st_dc01;
    JG_GLOBAL uint32_t* st_dc23;
    JG_GLOBAL uint8_t* pending;
    JG_GLOBAL int* bnd_p;
    JG_GLOBAL int* bnd_cz;
    JG_GLOBAL int* flow_list;
    JG_GLOBAL const int* tail_parts;
    int num_tail_parts;
    JG_GLOBAL int* tails_n;
    JG_GLOBAL uint32_t* tails_dc01;
    JG_GLOBAL uint32_t* tails_dc23;
    JG_GLOBAL int* mh_p;
    JG_GLOBAL int* mh_cz;
    JG_GLOBAL uint32_t* mh_link;
    JG_GLOBAL uint2_t* mh_pool;
    JG_GLOBAL uint8_t* mh_known;
    JG_GLOBAL const MhBlock* mh_blocks;
    JG_GLOBAL uint16_t* mh_blk_exit;
    JG_GLOBAL uint16_t* mh_blk_entry;
    int num_mh_blocks;
    JG_GLOBAL uint16_t* sym;
    JG_GLOBAL uint2_t* du_tab;
    uint32_t sym_region;
    uint64_t sym_entries;
    int num_chunks;
    int num_seq;
    const ScanParams& sp;
    const IdctParams& ip;
    __device__ __forceinline__ explicit JobView(const ScanJob& j)
        : bytes(as_global(j.bytes)), chunks(as_global(j.chunks)), segments(as_global(j.segments)),
          tables(as_global(j.tables)), tables_sync(as_global(j.tables_sync)), qtables(as_global(j.qtables)), destuffed(as_global(j.destuffed)),
          seg_idx(as_global(j.seg_idx)), st_p(as_global(j.st_p)), st_n(as_global(j.st_n)), st_cz(as_global(j.st_cz)),
          st_dc01(as_global(j.st_dc01)), st_dc23(as_global(j.st_dc23)), pending(as_global(j.pending)),
          bnd_p(as_global(j.bnd_p)), bnd_cz(as_global(j.bnd_cz)), flow_list(as_global(j.flow_list)), tail_parts(as_global(j.tail_parts)), num_tail_parts(j.num_tail_parts),
          tails_n(as_global(j.tails_n)), tails_dc01(as_global(j.tails_dc01)), tails_dc23(as_global(j.tails_dc23)),
          mh_p(as_global(j.mh_p)), mh_cz(as_global(j.mh_cz)), mh_link(as_global(j.mh_link)), mh_pool(as_global(j.mh_pool)), mh_known(as_global(j.mh_known)),
          mh_blocks(as_global(j.mh_blocks)), mh_blk_exit(as_global(j.mh_blk_exit)), mh_blk_entry(as_global(j.mh_blk_entry)), num_mh_blocks(j.num_mh_blocks),
          sym(as_global(j.sym)), du_tab(as_global(j.du_tab)), sym_region(j.sym_region), sym_entries(j.sym_entries),
          num_chunks(j.num_chunks), num_seq(j.num_seq), sp(j.sp), ip(j.ip)
    {
    }
};

struct JobByValue {
    // One image: ~14 dependent flow iterations decide the time, the speculative pass is one of them.
    static constexpr bool kSpeculateStateOnly = false;
    static constexpr bool kRepackFlows = true; // huff_sync_intra: flows that outlive the first iteration are packed into the lowest lanes
    ScanJob job;
    __device__ __forceinline__ const ScanJob& get() const { return job; }
};
struct JobsByValue {
    // All scans of ONE image (a file with several scans decoded on its own): one launch per stage, a scan per
    // blockIdx.y -- the scans are independent, and a 39 MP file of three scans spends a third of the time of three
    // launch sequences one after the other.
    static constexpr bool kSpeculateStateOnly = false;
    static constexpr bool kRepackFlows = true;
    ScanJob jobs[kMaxScans];
    __device__ __forceinline__ const ScanJob& get() const { return jobs[blockIdx.y]; }
};
struct JobArray {
    // Batches run one flow iteration, so the speculative pass is half of the sequence kernel's work:
    // it tracks the exit state only (-10 % kernel time); single-image latency is 4 % better without.
    static constexpr bool kSpeculateStateOnly = true;
    // The sequence kernel of a batch is bound by how many workgroups a CU holds (LDS: the sync table pack): the 4 KB the
    // re-packing needs cost one in five (538 -> 680 us per 64 images), and follow-up iterations inside that kernel cost
    // more than the tail kernel's trips they replace (jg_batch.cpp, sync_iters): batches run huff_sync_intra_batch.
    static constexpr bool kRepackFlows = false;
    const ScanJob* jobs;
    __device__ __forceinline__ const ScanJob& get() const { return jobs[blockIdx.y]; }
};

struct JobArrayLow {
    // A batch that does not fill the chip (jpeggpu_ext_decode_batch with a handful of images): what such a call waits for is
    // the chain of dependent flow iterations, as a lone decode does, and LDS is not what bounds the sequence kernel then: the
    // lone decode's kernel (all flows kept in the workgroup, survivors re-packed), one job per blockIdx.y. Only
    // huff_sync_intra is instantiated for it; every other stage of such a batch runs with JobArray.
    static constexpr bool kSpeculateStateOnly = false;
    static constexpr bool kRepackFlows = true;
    const ScanJob* jobs;
    __device__ __forceinline__ const ScanJob& get() const { return jobs[blockIdx.y]; }
};

struct JobSingle {
    // One job that lives in device memory, whatever blockIdx.y is: the lone decode of a device-scanned image (the
    // second dimension of the multi-hypothesis kernels' grid is the hypothesis).
    static constexpr bool kSpeculateStateOnly = false;
    static constexpr bool kRepackFlows = true;
    const ScanJob* job;
    __device__ __forceinline__ const ScanJob& get() const { return *job; }
};

} // namespace

} // namespace jg

#endif // JG_JOBS_H_
