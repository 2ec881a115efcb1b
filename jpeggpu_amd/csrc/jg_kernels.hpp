// jg_kernels.hpp -- launch interface of the gfx950 kernels (all launches are asynchronous on `stream`).
#ifndef JG_KERNELS_HPP_
#define JG_KERNELS_HPP_

#include "jg_defs.h"

#include <hip/hip_runtime_api.h>

namespace jg {

bool subseq_bytes_supported(int subseq_bytes);

/// Stages of one decode, in launch order (also the indices of jpeggpu_ext_get_stage_ms).
enum Stage {
    kStageFront     = 0, // device-side marker scan (jg_front.hip), launched by the decoder; nothing to launch here
    kStageDestuff   = 1,
    kStageSyncIntra = 2,
    kStageSyncInter = 3, // huff_sync_tail: sequence boundaries + flows the intra kernel left unfinished
    kStageTails     = 4,
    kStageWrite     = 5,
    kStageIdct      = 6,
    kNumStages      = 7
};

/// Work extents of a launch: the largest count over the jobs it covers (blocks beyond a job's own
/// count exit at once).
struct JobExtent {
    int max_chunks      = 0;
    int max_seq         = 0;
    int max_tail_parts  = 0;
    int max_tail_part   = 0; // subsequences in the largest tail part of any job
    int max_idct_blocks = 0;
    int subseq_words    = 0; // identical for every job of a launch
    uint32_t scales     = 0; // bit s: a job decodes at 1 / 2^s (IdctParams::scale_log2; bits kDraftScale + 1 ..: jobs of the next line)
    uint32_t draft_sizes = 0; // bit lg: a JPEGGPU_EXT_SCALE_LIBJPEG job has components of block size 8 >> lg (IdctDraft)
    uint32_t methods    = 0; // bit m: a full-size job takes IDCT method m (IdctParams::idct_method)
    bool crop           = false; // a job has an MCU window (jpeggpu_ext_set_crop, ScanJob::win): the IDCT's CropJobs instantiations
    uint32_t max_tab_bytes = 0;      // largest write-pass table pack
    uint32_t max_tab_bytes_sync = 0; // largest sync pack
    bool fuse_tail_write = false;    // batch launches: the tail kernel's parts and the write pass's sequences as ONE launch
                                     // (huff_tail_write), launched at kStageWrite; kStageSyncInter and kStageTails launch nothing
    bool repack_flows   = false;     // batch launches: the lone decode's sequence kernel (every flow kept in its workgroup), for
                                     // calls too small to fill the chip; the jobs then carry max_intra_iters = kSeqLanes, tail_marks = 0
};
void extend(JobExtent& e, const ScanJob& job);
/// Writers of huff_tail_write that gave up waiting (0 on a correct run), since the library was loaded.
hipError_t read_fuse_timeouts(unsigned int* count);

/// One stage for ONE job passed by value as a kernel argument (the drop-in single-image API).
hipError_t launch_stage(Stage stage, const ScanJob& job, hipStream_t stream);

/// One stage for ALL scans of one image (1..kMaxScans jobs, by value, one per blockIdx.y; the same subsequence size).
hipError_t launch_stage_scans(Stage stage, const ScanJob* jobs, int num_jobs, hipStream_t stream);

/// The three kernels of the multi-hypothesis speculation (jg_defs.h) for ONE job with sp.mh > 1, in front of
/// kStageSyncIntra. `max_seg_subseq`: subsequences of the job's largest restart segment (kMhMaxSegSubseq for a
/// device-scanned image, whose segments the host does not know: longer ones fall back on the device). `d_job`: the
/// job's copy in device memory if the device-side front end has filled in its counts, else null.
hipError_t launch_mh(const ScanJob& job, const ScanJob* d_job, int max_seg_subseq, hipStream_t stream);

/// One stage for ONE job stored in device memory (the lone decode of a device-scanned image: the device-side front end
/// has filled in its counts; `extent` holds the header's upper bounds), with the kernels' lone-decode variants.
hipError_t launch_stage_device_job(Stage stage, const ScanJob* d_job, const JobExtent& extent, hipStream_t stream);

/// One stage for `num_jobs` jobs stored in device memory, one per blockIdx.y (the batch API).
hipError_t launch_stage_batch(
    Stage stage, const ScanJob* d_jobs, int num_jobs, const JobExtent& extent, hipStream_t stream);

/// Nearest-neighbour replication of one plane: dst[y][x] = src[y * num_y / den_y][x * num_x / den_x]
/// (integer part of the reference's host helper util/util.h:62-91).
hipError_t launch_upsample(
    const uint8_t* src, int src_pitch, int src_w, int src_h,
    uint8_t* dst, int dst_pitch, int dst_w, int dst_h,
    int num_x, int den_x, int num_y, int den_y, hipStream_t stream);

/// Nearest-neighbour replication + YCbCr -> interleaved RGB8 (reference host helper util/util.h:62-104);
/// `ncomp` 1 (grey copied to R, G, B) or 3.
hipError_t launch_rgbi(
    const uint8_t* const* planes, const int* pitch, const int* w, const int* h, const int* num_x, const int* num_y,
    int den_x, int den_y, int ncomp, uint8_t* dst, int dst_pitch, int width, int height, hipStream_t stream);

/// libjpeg's fancy upsampling + integer YCbCr -> interleaved RGB8 (jdsample.c, jdcolor.c); same arguments as launch_rgbi.
/// hipErrorInvalidValue if a component's sampling factors do not divide the largest ones. `replicate`: every component is
/// replicated (libjpeg at 1/8 scale: jdsample.c turns fancy upsampling off when min_DCT_scaled_size is 1); the colour
/// conversion stays jdcolor.c's.
hipError_t launch_rgbi_fancy(
    const uint8_t* const* planes, const int* pitch, const int* w, const int* h, const int* num_x, const int* num_y,
    int den_x, int den_y, int ncomp, uint8_t* dst, int dst_pitch, int width, int height, hipStream_t stream, bool replicate = false);
/// launch_rgbi_fancy for a rectangle of the image at (x, y), width x height pixels, from the planes' WINDOWS of a cropped
/// decode (jpeggpu_ext_set_crop): window sizes, their origins in the full planes, and the full planes' widths (which choose
/// between fancy upsampling and replication, as for the whole image).
hipError_t launch_crop_rgbi_fancy(
    const uint8_t* const* planes, const int* pitch, const int* win_w, const int* win_h, const int* win_x, const int* win_y,
    const int* full_w, const int* num_x, const int* num_y, int den_x, int den_y, int ncomp, int x, int y,
    uint8_t* dst, int dst_pitch, int width, int height, hipStream_t stream, bool replicate = false);

/// launch_rgbi_fancy's per-component choice (FancyMode) for the ratios hr = h_max / h_c, vr = v_max / v_c and a full
/// plane `full_w` samples wide.
int fancy_mode(int hr, int vr, int full_w);

/// One item of a batched resize (launch_resize), in device memory: a rectangle of a decoded image, given as the planes'
/// windows the way launch_crop_rgbi_fancy takes them, resampled to out_w x out_h RGB by two separable passes whose weight
/// tables the host computed (jpeggpu_ext_resize_weights). A table of n output coordinates with `taps` taps each is
/// int32 {first, count}[n] followed by int32 weights[n][taps] (22 fraction bits).
struct ResizeJob {
    const uint8_t* plane[3]; // the windows (grey: every entry is component 0)
    int pitch[3], w[3], h[3];
    int hr[3], vr[3], mode[3]; // output pixels per sample, FancyMode
    int ox[3], oy[3];          // each window's origin in its full plane
    int x, y;                  // the rectangle's top-left pixel in the image
    int ncomp;                 // 1 or 3
    int row0, rows;            // rectangle rows row0 .. row0 + rows - 1: the rows the vertical taps read
    int taps_x, taps_y;
    const int* tab_x;          // out_w columns
    const int* tab_y;          // out_h rows
    uint8_t* mid;              // rows x out_w RGB of the horizontal pass, rows mid_pitch bytes apart
    int mid_pitch;             // a multiple of 16
    int pad_;
};
constexpr int kResizeHTileW = 32, kResizeHTileH = 8; // horizontal pass: output columns x rows per workgroup
constexpr int kResizeVTileW = 256, kResizeVTileH = 4; // vertical pass: output pixels x rows per workgroup
/// Horizontal-pass workgroups of one item.
inline int resize_h_tiles(int rows, int out_w)
{
    return ((rows + kResizeHTileH - 1) / kResizeHTileH) * ((out_w + kResizeHTileW - 1) / kResizeHTileW);
}
/// The two passes for `n` items: `d_jobs` ResizeJob[n] and `d_first_tile` int[n] (each item's first horizontal-pass
/// workgroup; `h_tiles` of them in all) in device memory. `layout` 0: dst is n x out_h x out_w x 3 (NHWC), 1: n x 3 x out_h
/// x out_w (NCHW).
hipError_t launch_resize(
    const ResizeJob* d_jobs, const int* d_first_tile, int n, int h_tiles, int out_w, int out_h, int layout,
    uint8_t* dst, hipStream_t stream);

} // namespace jg

#endif // JG_KERNELS_HPP_
