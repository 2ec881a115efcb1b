// jg_prog.hip -- gfx950 kernels of progressive (SOF2) decoding: the scan kernel (one lane per restart segment of a
// scan, one launch per level of the scan script) and the hand-over that presents the finished coefficients to the IDCT
// stage as the symbol stream of non-interleaved baseline scans. The decoding itself is jg_prog_core.h, which the host
// twin compiles as well.
#include "jg_prog.hpp"

#include <hip/hip_runtime.h>

namespace jg {

namespace {

/// Job sources, as in jg_kernels.hip: one image by value (a lone decode), or an array in device memory (a batch).
struct ProgOne {
    ProgImage img;
    __device__ __forceinline__ const ProgImage& get() const { return img; }
};
struct ProgMany {
    const ProgImage* imgs;
    __device__ __forceinline__ const ProgImage& get() const { return imgs[blockIdx.y]; }
};

constexpr int kScanLanes = kProgLaneGroup; // one wave per workgroup: a workgroup's lanes share nothing
constexpr int kPackLanes = 256;

/// All scans of one level. Lane i takes work item i of the level's list (jg_reader.cpp orders it: a scan of 64 segments
/// or more starts a wave of its own, the rest is grouped by scan kind). The lanes run prog_step in lock step, one
/// symbol (or block) per trip, each on its own segment. Tables are read from global memory: most progressive files have
/// no restart markers, so the lanes of a wave belong to different scans (and images) with different tables and LDS
/// copies would have to hold all of them; a table is 1.4 KB that every wave of its scan reads, which L2 serves.
template <class IS>
__global__ __launch_bounds__(kScanLanes) void prog_scan_kernel(IS is, uint32_t level)
{
    const ProgImage& img = is.get();
    uint8_t* tmp         = img.tmp;
    const ProgHeader& H  = *reinterpret_cast<const ProgHeader*>(tmp + img.hdr_off);
    if (level >= H.num_levels) return;
    const uint32_t first = H.level_item[level], count = H.level_item[level + 1] - first;
    const uint32_t i     = blockIdx.x * kScanLanes + threadIdx.x;
    if (i >= count) return;
    const ProgItem item = reinterpret_cast<const ProgItem*>(tmp + H.items_off)[first + i];
    if (item.scan >= H.num_scans) return; // an idle lane
    const ProgScanDesc& sd = reinterpret_cast<const ProgScanDesc*>(tmp + H.scans_off)[item.scan];
    if (item.seg >= static_cast<uint32_t>(sd.num_segments)) return;
    const uint2_t range = reinterpret_cast<const uint2_t*>(tmp + sd.seg_off)[item.seg];
    ProgLane L;
    prog_lane_init(sd, tmp + H.bytes_off, H.bytes_len, range, static_cast<int>(item.seg), L);
    for (int64_t left = prog_max_steps(sd, L); left > 0 && prog_step(sd, tmp, L); --left) {
    }
}

/// One lane per visible block of the image (all components): the block, staged through LDS so that the loads are
/// whole 128-byte lines, becomes the symbol stream of data unit `w` of its component's job, region `w` (jg_prog_core.h).
template <class IS>
__global__ __launch_bounds__(kPackLanes) void prog_pack_kernel(IS is)
{
    // 33 words per block: lane t reads its block's words while the other lanes read theirs, one bank apart
    __shared__ uint32_t s_blk[kPackLanes][33];
    __shared__ const uint32_t* s_src[kPackLanes];
    const ProgImage& img = is.get();
    uint8_t* tmp         = img.tmp;
    const ProgHeader& H  = *reinterpret_cast<const ProgHeader*>(tmp + img.hdr_off);
    const uint32_t u0    = blockIdx.x * kPackLanes;
    if (u0 >= H.pack_units) return;
    const int t      = threadIdx.x;
    const uint32_t u = u0 + t;
    int c            = -1;
    uint32_t w       = 0;
    if (u < H.pack_units) {
        c = 0;
        while (c + 1 < static_cast<int>(H.num_comp) && u >= H.comp[c + 1].unit0) ++c;
        w = u - H.comp[c].unit0;
    }
    const uint32_t* src = nullptr;
    if (c >= 0) {
        const ProgComp& pc = H.comp[c];
        const uint32_t by = w / static_cast<uint32_t>(pc.vis_x), bx = w - by * static_cast<uint32_t>(pc.vis_x);
        src = reinterpret_cast<const uint32_t*>(tmp + pc.coef_off) + (static_cast<uint64_t>(by) * pc.blocks_x + bx) * 32u;
    }
    s_src[t] = src;
    __syncthreads();
    for (int it = 0; it < 32; ++it) {
        const int b           = it * (kPackLanes / 32) + (t >> 5);
        const uint32_t* from = s_src[b];
        if (from) s_blk[b][t & 31] = from[t & 31];
    }
    __syncthreads();
    if (c < 0) return;
    const ProgComp& pc   = H.comp[c];
    uint16_t* sym        = reinterpret_cast<uint16_t*>(tmp + pc.sym_off);
    const uint32_t base  = sym_region_base(w, kProgRegionEntries);
    const uint2_t record = prog_pack_block(reinterpret_cast<const int16_t*>(s_blk[t]), base, [&](uint32_t at, uint16_t e) { sym[at] = e; });
    reinterpret_cast<uint2_t*>(tmp + pc.du_tab_off)[w] = record;
}

template <class IS>
hipError_t launch_all(const IS& is, int grid_y, const ProgExtent& e, hipStream_t stream)
{
    for (uint32_t level = 0; level < e.num_levels; ++level) {
        if (e.max_items[level] == 0) continue;
        prog_scan_kernel<IS><<<dim3((e.max_items[level] + kScanLanes - 1) / kScanLanes, grid_y), kScanLanes, 0, stream>>>(is, level);
    }
    if (e.max_units) prog_pack_kernel<IS><<<dim3((e.max_units + kPackLanes - 1) / kPackLanes, grid_y), kPackLanes, 0, stream>>>(is);
    return hipGetLastError();
}

} // namespace

void extend(ProgExtent& e, const ProgHeader& h)
{
    if (h.num_levels > e.num_levels) e.num_levels = h.num_levels;
    for (uint32_t l = 0; l < h.num_levels && l < static_cast<uint32_t>(kMaxProgScans); ++l) {
        const uint32_t n = h.level_item[l + 1] - h.level_item[l];
        if (n > e.max_items[l]) e.max_items[l] = n;
    }
    if (h.pack_units > e.max_units) e.max_units = h.pack_units;
}

hipError_t launch_prog(const ProgImage& img, const ProgExtent& e, hipStream_t stream) { return launch_all(ProgOne{img}, 1, e, stream); }

hipError_t launch_prog_batch(const ProgImage* d_images, int num_images, const ProgExtent& e, hipStream_t stream)
{
    if (num_images <= 0) return hipSuccess;
    return launch_all(ProgMany{d_images}, num_images, e, stream);
}

} // namespace jg
