/*
 * jpeggpu_ext.h -- additive entry points next to the drop-in API of jpeggpu.h. Nothing here exists in
 * the reference; callers that only use jpeggpu.h never need this header.
 *
 *   jpeggpu_ext_set_subsequence_bytes  tuning knob the reference leaves as a compile-time constant
 *   jpeggpu_ext_set_batched            (src/decoder_defs.hpp:28-34 `chunk_size`); chosen per image by default
 *   jpeggpu_ext_get_layout             where the intermediate buffers of the last parsed image sit
 *   jpeggpu_ext_set_segment_shard      decode a share of one image's restart segments (one image over several GPUs)
 *                                      inside d_tmp, for stage-level parity tests and profiling
 *   jpeggpu_ext_set_profiling /        per-stage device time of a decode from HIP events recorded on the
 *   jpeggpu_ext_get_stage_ms           caller's stream (the reference has wall-clock timing only,
 *                                      benchmark/benchmark_jpeggpu.hpp:96-102)
 *   jpeggpu_ext_decode_batch           one launch per stage for many images; the
 *                                      reference decodes one image per call sequence
 *   jpeggpu_ext_set_device_scan        restart-marker scan and segment / work-list construction on the device
 *   jpeggpu_ext_parse_headers          parse_header of many images on a pool of host threads
 *   jpeggpu_ext_planes_to_rgbi         chroma replication + YCbCr -> interleaved RGB8 (util/util.h:62-104)
 *   jpeggpu_ext_upsample_planes        nearest-neighbour chroma replication on the device, the integer
 *                                      part of the reference's host helper util/util.h:62-91
 *   jpeggpu_ext_set_scale              decode at 1/2, 1/4 or 1/8 size (libjpeg's scale_num / scale_denom), bit-exact with
 *                                      libjpeg-turbo's reduced IDCTs
 *   jpeggpu_ext_set_idct               full-size IDCT: the reference's (default) or libjpeg-turbo's jpeg_idct_islow
 *   jpeggpu_ext_planes_to_rgbi_fancy   libjpeg's fancy chroma upsampling + integer YCbCr -> interleaved RGB8
 *   jpeggpu_ext_set_crop /             decode only a rectangle of the image: a window of each plane, the restart segments
 *   jpeggpu_ext_get_crop               outside it skipped (nvJPEG's ROI decode, libjpeg-turbo's jpeg_crop_scanline)
 *   jpeggpu_ext_crop_to_rgbi_fancy     the rectangle as interleaved RGB8, equal to that part of planes_to_rgbi_fancy's image
 *   jpeggpu_ext_resize_to_rgb          a batch of (cropped) images resized to one size, NHWC or NCHW, with the arithmetic
 *                                      of Pillow's BILINEAR / BICUBIC Image.resize (torchvision's RandomResizedCrop)
 *   jpeggpu_ext_get_color_space        the colour model of the parsed file -- grey, YCbCr, RGB, CMYK or YCCK -- by libjpeg's
 *                                      rules (JFIF and Adobe segments, component ids)
 *   jpeggpu_ext_*_cs                   the libjpeg-exact RGB calls above for a given colour model: the RGB Pillow's
 *                                      Image.convert("RGB") makes of files of all five
 *   jpeggpu_ext_set_progressive /      progressive JPEGs (SOF2), per decoder and off by default: their scans are decoded
 *   jpeggpu_ext_get_progressive_info   on the device into coefficient buffers and handed to the IDCT stage
 *   jpeggpu_ext_set_truncated /        files that end early, per decoder and off by default: decoded as libjpeg finishes them
 *   jpeggpu_ext_get_truncated          for Pillow under ImageFile.LOAD_TRUNCATED_IMAGES (the rows that are there, grey below)
 *   jpeggpu_ext_resize_to_tensor       the batched resize written as a model's input: uint8, float32, float16 or bfloat16,
 *                                      normalised as ToTensor + Normalize do, items flipped left to right where asked
 *   jpeggpu_ext_resize_view_to_tensor  the evaluation transform: a window of the resize of each item's WHOLE image, zero
 *                                      outside it -- torchvision's Resize + CenterCrop on Pillow, from a cropped decode
 *   jpeggpu_ext_encode_batch           the way back: uint8 images on the device to baseline or progressive JPEG files on the
 *                                      device, byte for byte what Pillow's Image.save writes on libjpeg-turbo (optimize=True
 *                                      and progressive=True included)
 *   jpeggpu_ext_transcode_batch        jpegtran on the GPU: decoded files' quantised coefficients to new files with optimised
 *                                      tables, as progressive or baseline, with other restart intervals; no IDCT, no loss
 *   jpeggpu_ext_set_transcode_orientation  ... turned, flipped or transposed on the way (jpegtran -rotate / -flip / -transpose),
 *                                      still without loss: an EXIF orientation baked into the file
 *   jpeggpu_ext_set_transcode_crop     ... or cut to a rectangle (jpegtran -crop), decoding only the restart segments it needs
 *   jpeggpu_ext_set_transcode_frame    ... keeping the source's own frame layout: any sampling, up to four components and tables
 *   jpeggpu_ext_roundtrip_batch        JPEG compression as an augmentation: the pixels of Pillow's save at quality q, then open,
 *                                      in two launches per call and without a file
 *   jpeggpu_ext_read_coefficients_batch   DCT-domain access (libjpeg's jpeg_read_coefficients / jpeg_write_coefficients): the
 *   jpeggpu_ext_write_coefficients_batch  quantised coefficients of decoded files as tensors, and files from such tensors
 */
#ifndef JPEGGPU_JPEGGPU_EXT_H_
#define JPEGGPU_JPEGGPU_EXT_H_

#include <jpeggpu/jpeggpu.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Subsequence size (the reference's compile-time `chunk_size`, 128, with the TODO "pick per image",
 * src/decoder_defs.hpp:28-34). By default the library picks it PER IMAGE at jpeggpu_decoder_parse_header from the size
 * of the scan, its restart density and the call type: 64 bytes for an image decoded on its own (the sequence kernel's
 * serial chain is what such a decode waits for), 256 for one that shares its launches with others, less where restart
 * segments are so short that padding them to whole subsequences would show (jpeggpu_ext_layout.subsequence_bytes says
 * what an image got). jpeggpu_ext_set_batched tells the decoder which call type its images are for;
 * jpeggpu_ext_set_subsequence_bytes fixes the size instead (32, 64, 128 or 256; 0 = back to the per-image choice), as
 * does the environment variable JPEGGPU_SUBSEQ_BYTES at startup. Both take effect at the next parse_header.
 * jpeggpu_ext_decode_batch accepts any mix of sizes (one group of launches per size). */
enum jpeggpu_status jpeggpu_ext_set_subsequence_bytes(jpeggpu_decoder_t decoder, int subseq_bytes);
enum jpeggpu_status jpeggpu_ext_set_batched(jpeggpu_decoder_t decoder, int batched);
/* The plan knows the batch size: tell the decoder ABOUT how many images of this kind share one jpeggpu_ext_decode_batch
 * call (0: decoded on its own, the default; jpeggpu_ext_set_batched(decoder, 1) is the hint 64, "the chip is full"). What
 * is chosen at the next parse_header -- subsequence size, multi-hypothesis tables -- is then made for a launch of that
 * size, and jpeggpu_ext_decode_batch picks its kernels from the subsequences a call REALLY holds. A wrong hint costs speed,
 * never correctness: any decoder may be passed to either decode call. */
enum jpeggpu_status jpeggpu_ext_set_batch_hint(jpeggpu_decoder_t decoder, int images_per_call);

struct jpeggpu_ext_scan_layout {
    int num_components;        /* components in this scan */
    int component_idx[JPEGGPU_MAX_COMP];
    int num_subsequences;
    int num_segments;
    int num_sequences;         /* workgroups of the Huffman kernels */
    int num_data_units;
    int data_units_per_mcu;
    int num_chunks;            /* destuff work items */
    /* byte offsets inside d_tmp */
    size_t off_segments;       /* {int subseq_offset, subseq_count}[num_segments] */
    size_t off_chunks;
    size_t off_destuffed;      /* destuffed bytes, TILED in rows of W + 3 words (W = subsequence_bytes / 4): slot s of
                                  subsequence t is 32-bit word ((t / R) * (W + 3) + s) * R + t % R, R = 32 rows per
                                  tile (16 for 256-byte subsequences); slots 1..W are
                                  the subsequence's own words, slot 0 mirrors the last word of subsequence t - 1,
                                  slots W + 1 and W + 2 the first two of t + 1; a word holds its four stream bytes
                                  most significant first (stream byte i is byte 3 - i % 4) */
    size_t off_segment_index;  /* int[num_subsequences] */
    size_t off_state_p;        /* int[num_subsequences] */
    size_t off_state_n;
    size_t off_state_cz;       /* c | z << 8 */
    size_t off_state_dc01;     /* uint32[num_subsequences]: wrapping 16-bit DC-difference sums of scan
                                  components 0 (low half) and 1 (high half) */
    size_t off_state_dc23;     /* same for scan components 2 and 3 */
    size_t off_symbols;        /* uint16 entries, contiguous per data unit: the unit's DC value (absolute) first, then
                                  one entry per non-zero AC coefficient, value << 6 | zig-zag index (value in
                                  -512..511); a coefficient of magnitude 512 or more (category >= 10) is followed by an escape entry with
                                  index 0 holding value >> 10 in its high bits. Logically one region of symbol_region_entries per
                                  subsequence; physically the regions of 64 consecutive subsequences are interleaved
                                  in sectors of 16 entries: sector j of subsequence s starts at entry
                                  ((s / 64) * (symbol_region_entries / 16) + j) * 1024 + (s % 64) * 16 */
    size_t off_du_table;       /* {uint32 physical index of the first entry, uint32 count (| 128 if the unit holds an
                                  escape)}[num_data_units], stream order; entry k of a unit: w = (first & 15) + k -> (first & ~15) + (w >> 4) * 1024 + (w & 15) */
    int symbol_region_entries;
    /* jpeggpu_ext_set_device_scan: num_subsequences / num_segments / num_chunks above are then capacities from the
     * header; the real counts are uint32 words 1.. at off_device_status (status, subsequences, segments, chunks,
     * tail parts), and off_segments / off_chunks point at tables the device has built. */
    int device_scan;
    size_t off_device_status;
    /* Candidates per subsequence of the multi-hypothesis speculation that a lone decode (jpeggpu_decoder_decode) of this
     * scan runs in front of its synchronisation -- one per data unit of the MCU --, 0 where it does not apply (one data
     * unit per MCU, a decoder for batches, a device-scanned image without restart markers, a scan of more than 256 blocks)
     * or JPEGGPU_MULTI_HYPOTHESIS=0 switched it off at startup. */
    int hypotheses;
    /* Blocks of the block-wise chain walk: 0 where every restart segment has at most 1024 subsequences (one workgroup
     * walks a segment), else the scan's segments cut into blocks of 1024 (a scan without restart markers is one segment). */
    int hypothesis_blocks;
};

struct jpeggpu_ext_layout {
    int subsequence_bytes;
    int subsequences_per_sequence; /* owned by one workgroup of the Huffman kernels */
    int num_scans;
    size_t transferred_bytes;  /* entropy-coded byte range copied by jpeggpu_decoder_transfer */
    size_t blob_bytes;         /* table blob copied by jpeggpu_decoder_transfer */
    size_t off_bytes;          /* stuffed bytes inside d_tmp */
    size_t off_qtables;        /* uint16[4][64], natural order */
    struct jpeggpu_ext_scan_layout scans[JPEGGPU_MAX_COMP];
    int shard_rank, shard_world; /* jpeggpu_ext_set_segment_shard as it applies to this image (0, 1: the whole image) */
};

enum jpeggpu_status jpeggpu_ext_get_layout(jpeggpu_decoder_t decoder, struct jpeggpu_ext_layout* layout);

/* Restart-interval sharding of ONE image (one large image over the GPUs of a node): after
 * jpeggpu_ext_set_segment_shard(decoder, rank, world) -- before parse_header -- the decoder transfers and decodes only
 * restart segments [rank * n / world, (rank + 1) * n / world) of the n the scan has, and writes only the rows of each
 * plane that those segments cover (jpeggpu_ext_get_shard_rows, after parse_header); `world` decoders, on `world`
 * devices or one, write disjoint bands that together are the image. Segments are independent for the Huffman decode
 * and for DC prediction (reference src/decode_dc.cu:119-144). parse_header returns JPEGGPU_NOT_SUPPORTED unless the
 * file has one scan with a restart interval of whole MCU rows; the host walk is used (no device scan).
 * world = 1 switches it off. */
enum jpeggpu_status jpeggpu_ext_set_segment_shard(jpeggpu_decoder_t decoder, int rank, int world);
enum jpeggpu_status jpeggpu_ext_get_shard_rows(jpeggpu_decoder_t decoder, int component, int* first_row, int* num_rows);

/* Device-side front end (enable != 0, before parse_header): parse_header stops at the header of the file's LAST scan
 * (the only one of most files) instead of walking the entropy-coded bytes for restart markers (the
 * reference does that walk on the host inside its timed loop, src/reader.cpp:447-489; here it is 0.2 of the
 * 0.87 ms of a 12 MP image). transfer then copies everything up to the end of the file, and decode first runs four
 * small kernels that find the markers and build the segment table and the destuff work list in device memory. What
 * the host walk reports at parse time -- a scan without terminating marker, a restart-marker count that does not
 * match the geometry, an FF FF 00 sequence: JPEGGPU_INVALID_JPEG in each case, from either walk -- is then known
 * only on the device: decode leaves the planes untouched, and jpeggpu_ext_get_device_status (which synchronises
 * `stream`) returns the status. If the file ends in an end-of-image marker, or in one followed by padding, the
 * copy stops there (a backwards search on the host); otherwise it runs to the end of the file.
 * In a file of several scans the LAST one is the device's if it holds at least as many bytes as the scans in front of it
 * (those are walked on the host: the next scan header lies behind their last byte); otherwise the host walks them all. A batch may mix both
 * kinds: the front end of its device-scanned images runs as four launches for the whole batch (grid.y = image). */
/* enable: 0 off (default); 1 on, the caller asks for the status as above; 2 on and CHECKED: jpeggpu_decoder_decode
 * itself waits for the stream and returns the device's status (it then blocks the host, unlike every other mode).
 * The environment variable JPEGGPU_DEVICE_SCAN switches the scan on at jpeggpu_decoder_startup for callers of the
 * drop-in API alone: "1", "2" or "checked" select the CHECKED mode -- such a caller cannot ask for the device's verdict,
 * so decode tells it, at the price of a blocking call --, "async" mode 1 (a truncated scan then shows as unwritten planes
 * only). Items of jpeggpu_ext_decode_batch are never waited
 * for: their status is read with the call below. A decoder in segment-shard mode (jpeggpu_ext_set_segment_shard with
 * world > 1) always takes the host walk -- its share is cut out of the host walk's tables -- and parse_header logs
 * that the device scan was not used (jpeggpu_ext_layout.scans[0].device_scan says which walk an image got). */
enum jpeggpu_status jpeggpu_ext_set_device_scan(jpeggpu_decoder_t decoder, int enable);
enum jpeggpu_status jpeggpu_ext_get_device_status(
    jpeggpu_decoder_t decoder, const void* d_tmp, jpeggpu_stream_t stream, enum jpeggpu_status* status);

/* Scaled decoding (libjpeg's scale_num = 1, scale_denom = d): scale_denom 1 (the default), 2, 4 or 8, anything else
 * JPEGGPU_INVALID_ARGUMENT. Takes effect at the next jpeggpu_decoder_parse_header, like jpeggpu_ext_set_device_scan. With
 * denominator d, parse_header reports sizes_x[c] = ceil(W * h_c / (h_max * d)) (libjpeg's downsampled_width at that
 * scale), likewise sizes_y, and jpeggpu_decoder_decode / jpeggpu_ext_decode_batch write planes of those sizes (the pitch
 * checks use them). Every entry point works on a scaled decoder: a batch may mix items of any scales, 1 included; the
 * device marker scan; jpeggpu_ext_set_segment_shard, whose jpeggpu_ext_get_shard_rows then reports rows of the scaled
 * plane (a band is whole MCU rows, 8 v_c / d rows each); jpeggpu_ext_upsample_planes and jpeggpu_ext_planes_to_rgbi given
 * the scaled img_info and the scaled width and height.
 *   - Every component is scaled by the same factor: the planes keep their native subsampling. (libjpeg-turbo's raw-data
 *     output may upscale chroma through its IDCT instead; only 4:4:4 and grayscale files are directly comparable with
 *     libjpeg's.)
 *   - The arithmetic is that of libjpeg-turbo's jidctred.c (jpeg_idct_4x4, jpeg_idct_2x2, jpeg_idct_1x1): dequantisation
 *     in full int, its range limit (a 10-bit wrap, then the clamp). Scale 1 is the full-size IDCT as before.
 *   - Only the IDCT stage changes: subsequence choice, transfer, the Huffman kernels and jpeggpu_decoder_get_buffer_size
 *     (d_tmp sizing) do not depend on the scale. */
enum jpeggpu_status jpeggpu_ext_set_scale(jpeggpu_decoder_t decoder, int scale_denom);

/* How a scaled decode sizes its components. JPEGGPU_EXT_SCALE_UNIFORM (the default) is the behaviour described above: every
 * component at 1/d. JPEGGPU_EXT_SCALE_LIBJPEG is libjpeg-turbo's own (jdmaster.c), which is what Pillow's
 * Image.draft("RGB", size) + convert("RGB") returns: each component has its own IDCT output size S_c, so that the IDCT
 * does as much of the chroma upsampling as it can. With S_min = 8 / d,
 *     S_c = S_min;  while (S_c < 8 && (h_max S_min) % (h_c S_c 2) == 0 && (v_max S_min) % (v_c S_c 2) == 0) S_c *= 2;
 * 4:2:0 at 1/2 is luma 4x4 and chroma 8x8 (at 1/4: 2x2 and 4x4, at 1/8: 1x1 and 2x2): chroma planes of the luma's size.
 * 4:4:4, 4:2:2 and 4:4:0 keep one size for all components. Any other value: JPEGGPU_INVALID_ARGUMENT. Takes effect at the
 * next jpeggpu_decoder_parse_header, like the scale; at scale 1 it changes nothing. At a scale below 1, in this mode:
 *   - sizes_x[c] = ceil(W h_c S_c / (8 h_max)), sizes_y likewise; subsampling.x[c] / y[c] report the EFFECTIVE factors
 *     h_c S_c / S_min and v_c S_c / S_min -- the subsampling the planes really have -- so that every consumer that forms
 *     max / factor (jpeggpu_ext_planes_to_rgbi_fancy, jpeggpu_ext_crop_to_rgbi_fancy, jpeggpu_ext_resize_to_rgb,
 *     jpeggpu_ext_upsample_planes) sees the ratio that is left.
 *   - blocks of size 8 are transformed with jpeg_idct_islow whatever jpeggpu_ext_set_idct says, the smaller ones with
 *     jidctred.c's transforms as in the uniform mode.
 *   - RGB equal to libjpeg's: jpeggpu_ext_planes_to_rgbi_fancy / jpeggpu_ext_crop_to_rgbi_fancy on the reported img_info
 *     at 1/2 and 1/4; at 1/8 libjpeg replicates what subsampling is left instead (jdsample.c: no fancy upsampling when
 *     min_DCT_scaled_size is 1): jpeggpu_ext_planes_to_rgbi_replicate / jpeggpu_ext_crop_to_rgbi_replicate below.
 *     jpeggpu_ext_get_scale_info says which applies.
 *   - jpeggpu_ext_set_crop: the rectangle is in pixels of the image at 1/d as before; window origins, sizes, halos and
 *     the MCU window are computed with each component's own block size and effective factors.
 *   - jpeggpu_ext_set_segment_shard works: a band is whole MCU rows, v_c S_c rows of component c each
 *     (jpeggpu_ext_get_shard_rows). The device marker scan and jpeggpu_ext_decode_batch (any mix of modes, scales, crops and
 *     IDCT methods) work as in the uniform mode, and jpeggpu_decoder_get_buffer_size does not depend on the mode.
 * The environment's JPEGGPU_SCALE_MODE=libjpeg, read at jpeggpu_decoder_startup, selects it for a caller of the drop-in
 * API alone. */
enum jpeggpu_ext_scale_mode { JPEGGPU_EXT_SCALE_UNIFORM = 0, JPEGGPU_EXT_SCALE_LIBJPEG = 1 };
enum jpeggpu_status jpeggpu_ext_set_scale_mode(jpeggpu_decoder_t decoder, enum jpeggpu_ext_scale_mode mode);
/* Of the parsed image: the scale, the mode, each component's block size S_c (8 / d for all in the uniform mode), and
 * whether libjpeg upsamples what subsampling is left with its fancy upsamplers (1) or replicates (0: the LIBJPEG mode at
 * 1/8). JPEGGPU_INVALID_ARGUMENT before parse_header. */
struct jpeggpu_ext_scale_info {
    int scale_denom;
    int mode; /* enum jpeggpu_ext_scale_mode */
    int block_size[JPEGGPU_MAX_COMP];
    int fancy_upsampling;
};
enum jpeggpu_status jpeggpu_ext_get_scale_info(jpeggpu_decoder_t decoder, struct jpeggpu_ext_scale_info* info);

/* The full-size inverse DCT. JPEGGPU_EXT_IDCT_REFERENCE (the default) is the reference's fixed-point transform;
 * JPEGGPU_EXT_IDCT_ISLOW is libjpeg-turbo's jpeg_idct_islow (jidctint.c), the IDCT of Pillow, torchvision and OpenCV:
 * dequantisation in full int, CONST_BITS = 13, PASS1_BITS = 2, a 32-bit workspace between the passes and its
 * 10-bit-wrapping range limit. Planes decoded with it equal libjpeg's (jpeg_read_raw_data) bit for bit; with
 * jpeggpu_ext_planes_to_rgbi_fancy on top, so does the RGB output (jpeg_read_scanlines, JCS_RGB). Any other value:
 * JPEGGPU_INVALID_ARGUMENT.
 *   - Takes effect at the next jpeggpu_decoder_parse_header, like jpeggpu_ext_set_scale, and only at scale 1 (the reduced
 *     IDCTs are libjpeg's already).
 *   - Only the IDCT stage changes: plane sizes, jpeggpu_decoder_get_buffer_size, transfer, the Huffman kernels, segment
 *     shards and the device marker scan behave as with the reference IDCT. A batch may mix methods and scales.
 *   - The environment's JPEGGPU_IDCT=islow, read at jpeggpu_decoder_startup, selects it for a caller of the drop-in API
 *     alone. */
enum jpeggpu_ext_idct { JPEGGPU_EXT_IDCT_REFERENCE = 0, JPEGGPU_EXT_IDCT_ISLOW = 1 };
enum jpeggpu_status jpeggpu_ext_set_idct(jpeggpu_decoder_t decoder, enum jpeggpu_ext_idct method);

/* Cropped decoding: decode only the rectangle x, y, width x height (>= 0; 0 x 0 clears it) of the image AT THE DECODER'S
 * SCALE -- the RGB image jpeggpu_ext_planes_to_rgbi_fancy makes of the scaled planes. Takes effect at the next
 * jpeggpu_decoder_parse_header, like jpeggpu_ext_set_scale. Negative values, or a zero in only one of width / height:
 * JPEGGPU_INVALID_ARGUMENT from the setter; a rectangle that does not lie inside the image: JPEGGPU_INVALID_ARGUMENT from
 * parse_header; together with jpeggpu_ext_set_segment_shard (world > 1): JPEGGPU_NOT_SUPPORTED from parse_header.
 *   - The decoder writes a WINDOW of each plane: the slice of the uncropped plane that holds every sample libjpeg's fancy
 *     upsampler reads for the rectangle. For component c, hr = h_max / h_c, vr = v_max / v_c, the needed columns are
 *     floor(x / hr) - 1 .. floor((x + width - 1) / hr) + 1 clipped to the plane (rows likewise with vr; every component gets
 *     this one-sample halo). The frame's MCU columns [mx0, mx1) and rows [my0, my1) are the fewest that hold the needed
 *     samples of every component (an MCU column is 8 h_c / scale_denom samples of component c); the window of c starts at
 *     (mx0 * 8 h_c / d, my0 * 8 v_c / d) and ends behind its last needed sample.
 *   - parse_header reports the windows' sizes in sizes_x / sizes_y, and decode (and jpeggpu_ext_decode_batch, whose items
 *     may mix cropped and uncropped decoders, scales and IDCT methods) writes planes of those sizes (the pitch checks use
 *     them). jpeggpu_ext_get_crop, after parse_header, says where the windows lie.
 *   - A file of one scan with restart markers (any interval), walked on the host: parse_header keeps only the restart
 *     segments that hold the window's MCUs, so transfer copies only their bytes and the Huffman kernels decode only them
 *     (jpeggpu_ext_get_layout: transferred_bytes, num_segments, num_subsequences; get_buffer_size may shrink). Without restart
 *     markers, with several scans or with the device scan the whole scan is Huffman-decoded; the IDCT always transforms
 *     the window's MCUs only. */
struct jpeggpu_ext_crop_info {
    int x, y, width, height;         /* the rectangle (without a crop: the whole image at the scale) */
    int origin_x[JPEGGPU_MAX_COMP];  /* each component's window origin in its full plane */
    int origin_y[JPEGGPU_MAX_COMP];
    int full_x[JPEGGPU_MAX_COMP];    /* each component's full plane size at the scale */
    int full_y[JPEGGPU_MAX_COMP];
};
enum jpeggpu_status jpeggpu_ext_set_crop(jpeggpu_decoder_t decoder, int x, int y, int width, int height);
enum jpeggpu_status jpeggpu_ext_get_crop(jpeggpu_decoder_t decoder, struct jpeggpu_ext_crop_info* info);

/* Luma-only decoding: libjpeg's out_color_space = JCS_GRAYSCALE, what Pillow's im.draft("L", size) asks for. Set before
 * jpeggpu_decoder_parse_header and held like the scale (enable 0 or 1, else JPEGGPU_INVALID_ARGUMENT); 0, the default, leaves
 * every call as it was: the same launches, the same bytes. With 1, by the colour model jpeggpu_ext_get_color_space reports:
 *   - GRAY: nothing changes.
 *   - YCBCR: the IDCT stage transforms the data units of component 0 only -- in an interleaved scan the units of each MCU
 *     that belong to it, of a scan that codes only other components none at all (non-interleaved baseline files, the
 *     finished coefficients of a progressive file) -- with every transform: the reference's, ISLOW, the reduced ones in
 *     both scale modes (in JPEGGPU_EXT_SCALE_LIBJPEG component 0 keeps the block size jpeggpu_ext_get_scale_info reports).
 *     Plane 0 holds what it holds without the setting, crops and scales included. The planes of the other components are
 *     never written, and their pointers in jpeggpu_img are not looked at: they may be NULL. parse_header's sizes, the
 *     buffer size and jpeggpu_ext_get_layout are unchanged; entropy decoding is unchanged (every scan is still decoded).
 *   - RGB (an RGB-coded file): its grey needs all three components; the decode is unchanged and the grey output calls
 *     below apply jdcolor.c's rgb_gray_convert.
 *   - CMYK, YCCK, UNKNOWN: parse_header returns JPEGGPU_NOT_SUPPORTED (Pillow's draft("L") leaves such files as they are).
 * A jpeggpu_ext_decode_batch call may mix luma-only and other decoders; a call without a luma-only one launches exactly
 * the kernels it launched before. */
enum jpeggpu_status jpeggpu_ext_set_luma_only(jpeggpu_decoder_t decoder, int enable);

/* Stage timing: when enabled, jpeggpu_decoder_decode records HIP events on the caller's stream
 * between its launches; after the stream has been synchronised jpeggpu_ext_get_stage_ms returns the
 * mean milliseconds per stage (summed over scans) of the decodes since the previous call (at most the
 * last 64), and starts a new measurement window. */
enum jpeggpu_ext_stage {
    JPEGGPU_EXT_STAGE_FRONT      = 0, /* device-side marker scan (jpeggpu_ext_set_device_scan), else ~0 */
    JPEGGPU_EXT_STAGE_DESTUFF    = 1,
    JPEGGPU_EXT_STAGE_SYNC_INTRA = 2,
    JPEGGPU_EXT_STAGE_SYNC_INTER = 3,
    JPEGGPU_EXT_STAGE_TAILS      = 4,
    JPEGGPU_EXT_STAGE_WRITE      = 5, /* also the progressive launches of a call: zeroing, one launch per level, the hand-over */
    JPEGGPU_EXT_STAGE_IDCT       = 6,
    JPEGGPU_EXT_NUM_STAGES       = 7
};
enum jpeggpu_status jpeggpu_ext_set_profiling(jpeggpu_decoder_t decoder, int enable);
enum jpeggpu_status jpeggpu_ext_get_stage_ms(jpeggpu_decoder_t decoder, float* ms /* [JPEGGPU_EXT_NUM_STAGES] */);

/* Batched decode: ONE launch per stage for all scans of all items (grid.y = scan), which is what fills
 * a 256-CU device; the drop-in jpeggpu_decoder_decode launches per image. Every item must have been
 * parsed and transferred (jpeggpu_decoder_transfer) into its own d_tmp; items whose images got different
 * subsequence sizes are launched as one group per size. `d_scratch` is caller-owned device memory of at least
 * jpeggpu_ext_batch_scratch_size(total number of scans) bytes (job descriptors and front-end parameters),
 * private to the stream. The batch handle owns page-locked host staging only: a ring of FOUR staging buffers for
 * the job descriptors. What a call launches follows from what it holds (round 5): a call of ONE image whose decoder was
 * planned for lone decodes (the default, or jpeggpu_ext_set_batch_hint(decoder, 0 or 1)) is decoded as
 * jpeggpu_decoder_decode would decode it -- multi-hypothesis speculation included, never blocking --; a call of fewer
 * than 220 000 subsequences (about nineteen 12 MP images at 256 bytes) keeps every synchronisation flow in its sequence
 * kernel, as a lone decode does; a larger one runs one flow iteration there and the rest in the tail kernel.
 * Like jpeggpu_decoder_decode the call only enqueues -- with one exception: the fifth call in
 * a row on one handle waits (hipEventSynchronize) until the copy of the first one has executed, i.e. the host can
 * run at most four batch calls ahead of the device per handle. */
struct jpeggpu_batch;
typedef struct jpeggpu_batch* jpeggpu_batch_t;
struct jpeggpu_ext_batch_item {
    jpeggpu_decoder_t decoder;
    struct jpeggpu_img* img;
    void* d_tmp;
    size_t tmp_size;
};
size_t jpeggpu_ext_batch_scratch_size(int max_scans);
enum jpeggpu_status jpeggpu_ext_batch_create(jpeggpu_batch_t* batch, int max_scans);
enum jpeggpu_status jpeggpu_ext_decode_batch(
    jpeggpu_batch_t batch,
    const struct jpeggpu_ext_batch_item* items,
    int num_items,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);
enum jpeggpu_status jpeggpu_ext_batch_destroy(jpeggpu_batch_t batch);
/* Lock-step flow iterations inside the per-sequence sync kernel (>= 1: the first one is what gives every
 * subsequence its coefficient count and DC sums) before unfinished flows are handed to the low-footprint,
 * re-packing tail kernel (default 1: measured, a second iteration inside the sequence kernel costs a batch more than
 * the tail kernel's trip it saves; the drop-in decode keeps all flows in the sequence kernel, re-packed into its
 * lowest lanes between iterations). */
enum jpeggpu_status jpeggpu_ext_batch_set_sync_iterations(jpeggpu_batch_t batch, int iterations);
/* For a caller that uses ONE stream: split every batch into `parts` (1..4, default 1) that run concurrently,
 * part 0 on the caller's stream and the others on internal streams forked from and joined back into it with
 * events, so that one part's latency-bound synchronisation tail overlaps another part's decode (+15 % with
 * 2-3 parts). A caller that already keeps several streams busy gains nothing. Stage timing then reports
 * part 0. */
enum jpeggpu_status jpeggpu_ext_batch_set_overlap(jpeggpu_batch_t batch, int parts);
/* A call that fills the chip (what jpeggpu_ext_decode_batch launches is described above) runs the parts of the
 * synchronisation's tail and the sequences of the write pass as ONE launch, huff_tail_write: the sequences of parts
 * that are done are written while the slow parts still run (default on, or the environment's JPEGGPU_FUSE_TAIL_WRITE=0
 * when the batch is created; off: the two kernels one after the other, as up to round 4). Stage timing then reports
 * the launch under "write" and nothing under "sync_inter". Not taken with a caller's cap of the sequence kernel's
 * iterations (jpeggpu_ext_batch_set_sync_iterations), nor by calls of more than 256 scans. */
enum jpeggpu_status jpeggpu_ext_batch_set_fused_tail(jpeggpu_batch_t batch, int enable);
/* Consecutive subsequences a lane of the batched sequence kernel owns: `r` is 1, 2 or 4 (anything else is refused), the
 * default 2 or the environment's JPEGGPU_SYNC_RUN when the batch is created. With r = 1 a lane speculates its subsequence
 * and flows into the next one, two state-only decodes per subsequence; with a run of r it speculates only the run's first
 * subsequence, flows through the others and on into the next lane's run: (r + 1) / r decodes per subsequence. The result
 * is the same bit for bit; only the sequence kernel's work changes (2: +2.5 % images/s on 12 MP batches; 4: slower than 1). Runs apply where a call fills the chip and runs the
 * sequence kernel's single iteration: not to a call too small for that (which keeps every flow in its sequence's
 * workgroup), not with a caller's jpeggpu_ext_batch_set_sync_iterations, never to lone decodes. */
enum jpeggpu_status jpeggpu_ext_batch_set_sync_run(jpeggpu_batch_t batch, int r);
/* Writers of huff_tail_write that gave up waiting for a sequence to become ready, since the library was loaded (their
 * wait is bounded so that a defect cannot hang the GPU; 0 on every correct run: tests and the soak assert it). */
enum jpeggpu_status jpeggpu_ext_fused_tail_timeouts(unsigned int* count);
/* Stage timing of batched decodes; same contract as jpeggpu_ext_set_profiling / _get_stage_ms. */
enum jpeggpu_status jpeggpu_ext_batch_set_profiling(jpeggpu_batch_t batch, int enable);
enum jpeggpu_status jpeggpu_ext_batch_get_stage_ms(jpeggpu_batch_t batch, float* ms /* [JPEGGPU_EXT_NUM_STAGES] */);

/* Replicate every plane of `src` (as produced by jpeggpu_decoder_decode for `info`) to the full
 * image resolution: dst[c][y][x] = src[c][y * sy_c / sy_max][x * sx_c / sx_max]. */
enum jpeggpu_status jpeggpu_ext_upsample_planes(
    const struct jpeggpu_img_info* info,
    const struct jpeggpu_img* src,
    struct jpeggpu_img* dst,
    int width,
    int height,
    jpeggpu_stream_t stream);

/* One small decode (a built-in 96 x 80 4:2:0 JPEG with restart markers, through the public calls above, device memory
 * from hipMalloc) whose planes are compared with stored hashes: JPEGGPU_SUCCESS if the running system -- library build,
 * driver, device -- decodes bit-exactly, JPEGGPU_INTERNAL_ERROR if not (or without a device). Synchronises `stream`.
 * Meant for an application's start-up checks; the library never calls it on its own. */
enum jpeggpu_status jpeggpu_ext_self_test(jpeggpu_stream_t stream);

/* jpeggpu_decoder_parse_header for many images on `num_threads` host threads (the calling thread is one
 * of them). A 12 MP scan costs ~0.2 ms of one core to walk (reference src/reader.cpp:447-489 does the
 * same walk inside its timed loop), so a serving loop at 18 k images/s needs about four cores of it.
 * Every decoder must appear once. statuses[i] receives the result of item i; the return value is the
 * first failure, or JPEGGPU_SUCCESS. */
struct jpeggpu_ext_parse_item {
    jpeggpu_decoder_t decoder;
    struct jpeggpu_img_info* img_info;
    const uint8_t* data;
    size_t size;
};
enum jpeggpu_status jpeggpu_ext_parse_headers(
    const struct jpeggpu_ext_parse_item* items, int num_items, int num_threads, enum jpeggpu_status* statuses);

/* Planes of a 1- or 3-component image -> interleaved RGB8 at the full image resolution: nearest-neighbour
 * chroma replication + the JFIF YCbCr matrix in float, rounded and clamped -- the arithmetic of the
 * reference's host helper conv_to_rgbi (util/util.h:62-104). dst[y * dst_pitch + 3 * x + {0,1,2}] = R,G,B.
 * JPEGGPU_NOT_SUPPORTED for 2 or 4 components, as the helper. */
enum jpeggpu_status jpeggpu_ext_planes_to_rgbi(
    const struct jpeggpu_img_info* info,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    int width,
    int height,
    jpeggpu_stream_t stream);

/* The same contract and return codes as jpeggpu_ext_planes_to_rgbi, with libjpeg's arithmetic: fancy upsampling
 * (jdsample.c, do_fancy_upsampling on) and the integer YCbCr -> RGB conversion of jdcolor.c. Per component, by the ratio
 * h_max / h_c, v_max / v_c: 1x1 a copy; 2x1 h2v1_fancy_upsample; 2x2 h2v2_fancy_upsample (both replication instead when
 * the plane is at most 2 samples wide); 1x2 h1v2_fancy_upsample; other integral ratios replication; a non-integral ratio
 * JPEGGPU_NOT_SUPPORTED. The plane's edges are those of info's sizes (libjpeg's downsampled_width / _height): the samples
 * beyond them are copies of the edge samples. R = Y + ((91881 Cr + 2^15) >> 16), G = Y + ((-22554 Cb - 46802 Cr + 2^15)
 * >> 16), B = Y + ((116130 Cb + 2^15) >> 16), Cb and Cr centred on 128, each clamped to 0..255; one component is copied
 * to R, G and B. On planes of a JPEGGPU_EXT_IDCT_ISLOW decode this is what libjpeg-turbo (and Pillow's
 * Image.convert("RGB")) returns. */
enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_fancy(
    const struct jpeggpu_img_info* info,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    int width,
    int height,
    jpeggpu_stream_t stream);

/* jpeggpu_ext_planes_to_rgbi_fancy for the rectangle of a cropped decode: `info` and `src` are the windows parse_header
 * reported and decode wrote, `crop` what jpeggpu_ext_get_crop returned. Writes crop->width x crop->height pixels, equal to
 * rows y.., columns x.. of what jpeggpu_ext_planes_to_rgbi_fancy makes of the uncropped planes (the fancy / replicate choice
 * is made on the full plane sizes). JPEGGPU_NOT_SUPPORTED for 2 or 4 components or non-integral sampling ratios;
 * JPEGGPU_INVALID_ARGUMENT if a window does not hold the samples the rectangle reads. */
enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_fancy(
    const struct jpeggpu_img_info* info,
    const struct jpeggpu_ext_crop_info* crop,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    jpeggpu_stream_t stream);

/* jpeggpu_ext_planes_to_rgbi_fancy and jpeggpu_ext_crop_to_rgbi_fancy with every component REPLICATED (jdsample.c's
 * int_upsample and its h2v1 / h2v2 special cases: sample x / hr, y / vr) and the same integer colour conversion: libjpeg's
 * output where fancy upsampling is off, i.e. for planes of a JPEGGPU_EXT_SCALE_LIBJPEG decode at 1/8 that have subsampling
 * left (4:2:2, 4:4:0, 4:1:1 ...; jpeggpu_ext_scale_info.fancy_upsampling == 0). Same contracts and return codes. This is
 * not jpeggpu_ext_planes_to_rgbi, whose colour arithmetic is the reference helper's. */
enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_replicate(
    const struct jpeggpu_img_info* info,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    int width,
    int height,
    jpeggpu_stream_t stream);
enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_replicate(
    const struct jpeggpu_img_info* info,
    const struct jpeggpu_ext_crop_info* crop,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    jpeggpu_stream_t stream);

/* Batched resize to one size (a training pipeline's RandomResizedCrop, or a Resize of whole images; Resize + CenterCrop
 * is jpeggpu_ext_resize_view_to_tensor further down): each item's RGB -- what
 * jpeggpu_ext_crop_to_rgbi_fancy makes of a cropped decode's windows, or jpeggpu_ext_planes_to_rgbi_fancy of whole
 * planes -- resampled to out_w x out_h with the arithmetic of Pillow's Image.resize((out_w, out_h), BILINEAR | BICUBIC),
 * into ONE uint8 tensor: n x out_h x out_w x 3 (JPEGGPU_EXT_NHWC) or n x 3 x out_h x out_w (JPEGGPU_EXT_NCHW). On planes
 * of a JPEGGPU_EXT_IDCT_ISLOW decode at scale 1 the result equals Image.open(f).convert("RGB").crop(box).resize(...).
 * Items may mix scales, IDCT methods, sampling layouts, cropped and whole images, 1 and 3 components.
 *   - Pillow's arithmetic, per direction of input size `in` and output size `out` (in double): scale = in / out,
 *     fs = max(scale, 1), support = fs (bilinear) or 2 fs (bicubic, a = -0.5); output coordinate x has center = (x + 0.5)
 *     scale, first = max((int)(center - support + 0.5), 0) and count = min((int)(center + support + 0.5), in) - first
 *     taps; tap j weighs filter((j + first - center + 0.5) * (1 / fs)), divided by the sum of the weights (in tap order)
 *     when it is not 0, then (int)(w 2^22 + 0.5) ((int)(w 2^22 - 0.5) if negative). A pass computes
 *     clamp_0..255((2^21 + sum w_j p_j) >> 22). The horizontal pass comes first, over the rows the vertical taps read
 *     only, and its result is clamped to 8 bits; a direction whose size does not change is skipped. Equality with Pillow
 *     is tested (tests/test_resize_host.py).
 *   - Two launches per call (not one per item), stream-ordered on `stream`: the horizontal pass reads the planes' windows
 *     directly -- the items' full-resolution RGB is never written to memory -- and leaves its rows in `d_scratch`; the
 *     vertical pass writes `dst`. `d_scratch`: caller-owned device memory of at least jpeggpu_ext_resize_scratch_size
 *     bytes, private to the stream until the call has executed. The host may reuse `items` (and what they point to) as
 *     soon as the call returns: their descriptors and the weight tables are copied from internal page-locked staging
 *     (a ring of four: the fifth call in a row waits until the copy of the first has executed). `stream` must belong to
 *     the current device.
 *   - Items of a JPEGGPU_EXT_SCALE_LIBJPEG decode are described by their img_info like any other. The item has no room for
 *     "replicate": an item of that mode at 1/8 with subsampling left gets fancy upsampling here, which is not libjpeg's
 *     output (jpeggpu_ext_get_scale_info: fancy_upsampling == 0); decode such an image at 1/4 instead, or use
 *     jpeggpu_ext_resize_view_to_tensor, whose view has the flag.
 *   - JPEGGPU_NOT_SUPPORTED: a filter other than the two, an item of 2 or 4 components or with non-integral sampling
 *     ratios. JPEGGPU_INVALID_ARGUMENT: NULL pointers, n, out_w or out_h <= 0 (or n > 65535), an unknown layout, an item
 *     whose windows do not hold its rectangle's samples (the checks of jpeggpu_ext_crop_to_rgbi_fancy), scratch_size too
 *     small. Every check is made before anything is enqueued; on an error nothing is written. */
struct jpeggpu_ext_resize_item {
    const struct jpeggpu_img_info* info;       /* as parse_header reported it (a cropped decode: the windows) */
    const struct jpeggpu_ext_crop_info* crop;  /* jpeggpu_ext_get_crop's result; NULL: the whole image */
    const struct jpeggpu_img* src;             /* the decoded planes */
};
enum jpeggpu_ext_filter { JPEGGPU_EXT_FILTER_BILINEAR = 0, JPEGGPU_EXT_FILTER_BICUBIC = 1 };
enum jpeggpu_ext_output_layout { JPEGGPU_EXT_NHWC = 0, JPEGGPU_EXT_NCHW = 1 };
/* Bytes of d_scratch a call needs (the descriptors, the weight tables, and per item the horizontal pass's rows:
 * out_w x 3 bytes, padded to 16, for each rectangle row the vertical taps read); 0 for arguments the call would refuse.
 * It only grows with n for the same items. */
size_t jpeggpu_ext_resize_scratch_size(
    const struct jpeggpu_ext_resize_item* items, int n, int out_w, int out_h, enum jpeggpu_ext_filter filter);
enum jpeggpu_status jpeggpu_ext_resize_to_rgb(
    const struct jpeggpu_ext_resize_item* items,
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter,
    enum jpeggpu_ext_output_layout layout,
    uint8_t* dst,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);
/* The weight table the kernels use for input size `in` -> output size `out` (host only, no device needed): for output
 * coordinate x, taps first[x] .. first[x] + count[x] - 1 with weights[x * max_taps + j] (22 fraction bits; entries beyond
 * count[x] are set to 0). max_taps must be at least 2 ceil(support) + 1 (support: fs for bilinear, 2 fs for bicubic, as
 * above). JPEGGPU_INVALID_ARGUMENT for NULL pointers, in or out <= 0 or too small a max_taps; JPEGGPU_NOT_SUPPORTED for
 * another filter. */
enum jpeggpu_status jpeggpu_ext_resize_weights(
    int in, int out, enum jpeggpu_ext_filter filter, int* first, int* count, int* weights, int max_taps);

/* Colour models. jpeggpu_decoder_parse_header looks at the application segments in front of the first scan and at the
 * frame's component ids, and jpeggpu_ext_get_color_space reports what libjpeg (jdapimin.c, default_decompress_parms) and
 * therefore Pillow take the file for (JPEGGPU_INVALID_ARGUMENT before parse_header):
 *   1 component   GRAY.
 *   3 components  a JFIF APP0 segment (length >= 16, "JFIF\0") says YCBCR, even beside an Adobe segment; otherwise an
 *                 Adobe APP14 segment (length >= 14, "Adobe"; its transform flag is data byte 11): 0 is RGB, anything else
 *                 YCBCR; otherwise the component ids 'R', 'G', 'B' are RGB, anything else YCBCR.
 *   4 components  an Adobe segment with transform 0, or none: CMYK; any other transform: YCCK.
 *   2 components  UNKNOWN: there is no RGB of such a file.
 * A short or malformed APPn segment is skipped like any other APPn and says nothing. Nothing of the decode depends on the
 * model: the planes are the file's components either way.
 *
 * The calls below are jpeggpu_ext_planes_to_rgbi_fancy, _replicate, jpeggpu_ext_crop_to_rgbi_fancy, _replicate,
 * jpeggpu_ext_resize_scratch_size and jpeggpu_ext_resize_to_rgb with the model as an argument (the resize: one per item,
 * colors[n]; a call may mix models) -- the same upsampling per component, the fourth included, the same contracts, checks
 * and return codes, and then per pixel, of the upsampled samples s_0 ..:
 *   GRAY   s_0 three times.                    YCBCR  jdcolor.c's ycc_rgb_convert, as above.
 *   RGB    s_0, s_1, s_2 as they are.
 *   CMYK   the samples are taken for Adobe's inverted ones, as Pillow always does: with the inks c_i = 255 - s_i and
 *          K = s_3, out_i = K - (((t >> 8) + t) >> 8), t = c_i K + 128 -- Pillow's cmyk2rgb, nk - MULDIV255(c, nk).
 *   YCCK   (r, g, b) = ycc_rgb_convert(s_0, s_1, s_2), then the CMYK rule with the inks c_i = r, g, b and K = s_3
 *          (libjpeg hands out 255 - r ... in place of the samples, and Pillow inverts those like any CMYK file's).
 * On planes of a JPEGGPU_EXT_IDCT_ISLOW decode with the model jpeggpu_ext_get_color_space reported, this is
 * Image.open(f).convert("RGB") for every file Pillow opens as L, RGB or CMYK (in the JPEGGPU_EXT_SCALE_LIBJPEG mode: after
 * draft()). Embedded ICC profiles are ignored, as convert("RGB") ignores them; so is EXIF orientation by these calls -- the
 * oriented calls further down apply it.
 * JPEGGPU_NOT_SUPPORTED: a model that does not fit info's component count (GRAY 1, YCBCR and RGB 3, CMYK and YCCK 4),
 * UNKNOWN, non-integral sampling ratios; nothing is written then. The entry points without a model are these with GRAY for
 * one component and YCBCR for three (so 2 or 4 components stay JPEGGPU_NOT_SUPPORTED there). A NULL `colors`:
 * JPEGGPU_INVALID_ARGUMENT (jpeggpu_ext_resize_scratch_size_cs: 0). */
enum jpeggpu_ext_color_space {
    JPEGGPU_EXT_COLOR_UNKNOWN = 0,
    JPEGGPU_EXT_COLOR_GRAY    = 1,
    JPEGGPU_EXT_COLOR_YCBCR   = 2,
    JPEGGPU_EXT_COLOR_RGB     = 3,
    JPEGGPU_EXT_COLOR_CMYK    = 4,
    JPEGGPU_EXT_COLOR_YCCK    = 5
};
enum jpeggpu_status jpeggpu_ext_get_color_space(jpeggpu_decoder_t decoder, enum jpeggpu_ext_color_space* color);
enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_fancy_cs(
    const struct jpeggpu_img_info* info,
    enum jpeggpu_ext_color_space color,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    int width,
    int height,
    jpeggpu_stream_t stream);
enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_replicate_cs(
    const struct jpeggpu_img_info* info,
    enum jpeggpu_ext_color_space color,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    int width,
    int height,
    jpeggpu_stream_t stream);
enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_fancy_cs(
    const struct jpeggpu_img_info* info,
    enum jpeggpu_ext_color_space color,
    const struct jpeggpu_ext_crop_info* crop,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    jpeggpu_stream_t stream);
enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_replicate_cs(
    const struct jpeggpu_img_info* info,
    enum jpeggpu_ext_color_space color,
    const struct jpeggpu_ext_crop_info* crop,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    jpeggpu_stream_t stream);
size_t jpeggpu_ext_resize_scratch_size_cs(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors,
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter);
enum jpeggpu_status jpeggpu_ext_resize_to_rgb_cs(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors,
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter,
    enum jpeggpu_ext_output_layout layout,
    uint8_t* dst,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);

/* Progressive JPEGs (SOF2; Huffman-coded, 8-bit samples, 1..4 components). OFF by default: a decoder that was not told
 * otherwise answers JPEGGPU_NOT_SUPPORTED to SOF2, as the reference does. jpeggpu_ext_set_progressive(decoder, 1) takes
 * effect from the next jpeggpu_decoder_parse_header; SOF3 and SOF5..SOF15 (lossless, hierarchical, arithmetic-coded)
 * stay JPEGGPU_NOT_SUPPORTED. Up to 64 scans; scan headers that break T.81 G.1.1.1.1 are JPEGGPU_INVALID_JPEG; a scan
 * that breaks the progression (a first scan of coefficients already coded, a refinement of coefficients that are not at
 * its bit position, an AC scan before the component's first DC scan) is JPEGGPU_NOT_SUPPORTED, where libjpeg warns and
 * decodes on. A file may stop early: coefficients no scan coded are 0, bits no scan refined stay 0 (libjpeg would smooth
 * the blocks of such a file, this decoder does not; files an encoder finished decode to libjpeg's pixels).
 *
 * The scans are decoded on the device, one lane per restart segment of a scan and one launch per LEVEL of the scan
 * script (a scan's level: 0 if no earlier scan touches its coefficients, else one more than the highest level among
 * those that do), into per-component coefficient buffers inside d_tmp: int16[blocks_y][blocks_x][64], block raster over
 * the MCU-padded grid, natural order inside a block, zeroed on the stream at the start of every decode. The finished
 * frame is then presented to the IDCT stage as one non-interleaved baseline scan per component: jpeggpu_ext_get_layout
 * reports num_components scans without subsequences, and every scale, scale mode, IDCT method, crop (all entropy-coded
 * data is decoded, only the IDCT is windowed), colour model and the batched calls work as for a baseline file.
 * jpeggpu_ext_set_device_scan is ignored for a progressive image (its scans are walked on the host);
 * jpeggpu_ext_set_segment_shard with more than one rank is refused at parse_header with JPEGGPU_NOT_SUPPORTED. Stage
 * timing counts the progressive launches in JPEGGPU_EXT_STAGE_WRITE. */
struct jpeggpu_ext_progressive_info {
    int progressive; /* 1: the last parsed image is a progressive frame (all else 0 otherwise) */
    int num_scans;   /* scans of the file */
    int num_levels;
    size_t off_coefficients[JPEGGPU_MAX_COMP]; /* byte offset of each component's coefficient buffer in d_tmp */
    int blocks_x[JPEGGPU_MAX_COMP];            /* the buffer's block grid (MCU-padded) */
    int blocks_y[JPEGGPU_MAX_COMP];
    int visible_blocks_x[JPEGGPU_MAX_COMP];    /* ceil(plane size / 8): the blocks the IDCT stage is handed */
    int visible_blocks_y[JPEGGPU_MAX_COMP];
};
enum jpeggpu_status jpeggpu_ext_set_progressive(jpeggpu_decoder_t decoder, int enable);
enum jpeggpu_status jpeggpu_ext_get_progressive_info(jpeggpu_decoder_t decoder, struct jpeggpu_ext_progressive_info* info);

/* Truncated files (baseline and extended-sequential Huffman frames). OFF by default: a decoder that was not told otherwise
 * answers a file that ends early as it always did (JPEGGPU_INVALID_JPEG from jpeggpu_decoder_parse_header).
 * jpeggpu_ext_set_truncated(decoder, 1) takes effect from the next jpeggpu_decoder_parse_header: a file that ends anywhere
 * behind its first SOS header then parses with JPEGGPU_SUCCESS and decodes to what Pillow returns for it with
 * ImageFile.LOAD_TRUNCATED_IMAGES set (libjpeg given a fake EOI), through every decode call of this library:
 *   - the entropy-coded data is what lies in front of the end of the file; a trailing FF -- half of a stuffed FF 00 pair or of
 *     a marker -- is not data;
 *   - behind the last real bit the bit reader delivers zero bits. The first MCU that needs a bit that does not exist is
 *     finished from them (a coefficient whose run of zeros overshoots the block goes to index 63, as in jdhuff.c);
 *   - every MCU behind that one, to the end of the scan, has no coefficients at all, DC included: samples of 128;
 *   - restart intervals without data are such MCUs. Where the data ends with an interval and no bit was missing yet -- in
 *     front of, inside or right behind the restart marker -- the NEXT interval's first MCU is the one decoded from zero bits,
 *     with the DC predictions reset, and the emptying starts behind it;
 *   - a file that lacks only its EOI, or only half of it, decodes as the whole file does.
 * Fewer restart markers than the frame asks for are accepted under the flag; more, or a file cut in front of the end of its
 * first SOS header, are refused as ever. A whole file parses and decodes under the flag exactly as without it.
 * Refused under the flag with JPEGGPU_NOT_SUPPORTED: progressive frames (SOF2), also whole ones (libjpeg smooths the blocks
 * of a progressive file that ends early); jpeggpu_ext_set_segment_shard with more than one rank; a file of
 * several scans that ends in front of a scan some component needs. jpeggpu_ext_set_device_scan is silently not used while
 * the flag is set: the host walk is what records where the data ends.
 *
 * On the device a truncated image costs THREE launches more per call, whatever the call holds (jg_trunc.hip): one in front
 * of the Huffman stages and two between the write pass and the IDCT stage, each covering every truncated image of the call
 * (of the part, where jpeggpu_ext_batch_set_overlap cuts the call into parts). A call without a truncated image launches
 * what it always launched. The MCU that was finished from zero bits is found on the device and stays there: nothing
 * synchronises. jpeggpu_ext_get_truncated reports what the host walk of the last parsed image knows. The coefficient routes
 * (jpeggpu_ext_read_coefficients_batch, jpeggpu_ext_transcode_batch) see the same data units as the IDCT stage: the blocks
 * behind the cut are all zero. */
struct jpeggpu_ext_truncated_info {
    int truncated;              /* 1: the file ended without an EOI marker (all else as below) */
    int scan;                   /* the scan whose entropy-coded data runs to the end of the file, or -1: the file ended
                                   behind a whole scan (only the EOI, or trailing segments, are missing) */
    size_t scan_bytes;          /* bytes of that scan that are present, stuffing and restart markers included; 0 if scan < 0 */
    int first_missing_interval; /* the first restart interval without any data, or -1: none, or no restart markers */
};
enum jpeggpu_status jpeggpu_ext_set_truncated(jpeggpu_decoder_t decoder, int enable);
enum jpeggpu_status jpeggpu_ext_get_truncated(jpeggpu_decoder_t decoder, struct jpeggpu_ext_truncated_info* info);

/* EXIF orientation. jpeggpu_decoder_parse_header reads the Exif APP1 segments in front of the first scan the way Pillow
 * 12 does and jpeggpu_ext_get_orientation reports the Orientation tag (0x0112) of the last parsed image, 1..8:
 *   - the data is the first segment's that begins "Exif\0\0", with that of every later such segment (behind its six
 *     bytes) appended; a TIFF header: "II" with 42 in either byte order, or "MM" with 42 in either order or 43, then the
 *     offset of IFD0; IFD0's 12-byte entries are read for as long as whole ones lie in the data;
 *   - an entry of tag 0x0112, a TIFF type 1..13 or 16, a non-empty value that lies in the data: the first of its values
 *     counts, and a later such entry replaces an earlier. Of types SHORT, LONG, SSHORT, SLONG the values 1..8 are the
 *     orientation. Everything else is orientation 1: no segment, a truncated or malformed one, an offset outside the data,
 *     another type, the values 0 and 9..; a bad Exif segment never fails parse_header. One difference from Pillow, on
 *     purpose: a tag of type RATIONAL, SRATIONAL, FLOAT, DOUBLE, IFD or LONG8 is not converted and is orientation 1,
 *     where Pillow's exif_transpose would honour a value that compares equal to 2..8 (a DOUBLE 6.0). No camera or
 *     editor is known to write the tag so; the EXIF standard fixes it as SHORT.
 *   - Pillow's fallback to an XMP tiff:Orientation attribute when EXIF has none is NOT read: such a file is orientation 1.
 * Nothing of the decode depends on it: planes, crops and every call above stay in STORED coordinates. With S the stored
 * image, W x H at the decoder's scale, the DISPLAYED image O (ImageOps.exif_transpose) is
 *   1  O[y][x] = S[y][x]            5  O[y][x] = S[x][y]           (5..8: O is H x W)
 *   2  S[y][W-1-x]                  6  S[H-1-x][y]
 *   3  S[H-1-y][W-1-x]              7  S[H-1-x][W-1-y]
 *   4  S[H-1-y][x]                  8  S[x][W-1-y]
 * jpeggpu_ext_orient_size and jpeggpu_ext_orient_rect are host-only and pure: the displayed size of a stored w x h image,
 * and the stored rectangle (in place, in *x, *y, *rw, *rh) of a rectangle given in displayed coordinates -- pass it to
 * jpeggpu_ext_set_crop, so a crop in displayed pixels still decodes only its restart segments. An orientation outside
 * 1..8, sizes below 1 or a rectangle that does not lie in the displayed image: JPEGGPU_INVALID_ARGUMENT.
 *
 * jpeggpu_ext_planes_to_rgbi_oriented and jpeggpu_ext_crop_to_rgbi_oriented are the _cs conversions (`replicate` 0: the
 * _fancy one, else the _replicate one) that write the DISPLAYED image: `width` x `height` and `crop` are stored, `dst`
 * holds width x height pixels for 1..4 and height x width for 5..8, and `dst_pitch` is at least 3 x the displayed width
 * (else, or with an orientation outside 1..8: JPEGGPU_INVALID_ARGUMENT). jpeggpu_ext_resize_to_rgb_oriented is
 * jpeggpu_ext_resize_to_rgb_cs with an orientation per item (NULL: JPEGGPU_INVALID_ARGUMENT; the scratch size call: 0):
 * each item's crop is the stored rectangle, and the result is what Pillow gives for the displayed rectangle resized to
 * out_w x out_h -- its horizontal, rounded pass runs along DISPLAYED x. With orientation 1 every one of these launches
 * exactly what its _cs counterpart launches; a resize call with items of 5..8 takes one launch more. */
enum jpeggpu_status jpeggpu_ext_get_orientation(jpeggpu_decoder_t decoder, int* orientation);
enum jpeggpu_status jpeggpu_ext_orient_size(int orientation, int w, int h, int* out_w, int* out_h);
enum jpeggpu_status jpeggpu_ext_orient_rect(int orientation, int w, int h, int* x, int* y, int* rw, int* rh);
enum jpeggpu_status jpeggpu_ext_planes_to_rgbi_oriented(
    const struct jpeggpu_img_info* info,
    enum jpeggpu_ext_color_space color,
    int orientation,
    int replicate,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    int width,
    int height,
    jpeggpu_stream_t stream);
enum jpeggpu_status jpeggpu_ext_crop_to_rgbi_oriented(
    const struct jpeggpu_img_info* info,
    enum jpeggpu_ext_color_space color,
    int orientation,
    int replicate,
    const struct jpeggpu_ext_crop_info* crop,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    jpeggpu_stream_t stream);
size_t jpeggpu_ext_resize_scratch_size_oriented(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors,
    const int* orientations,
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter);
enum jpeggpu_status jpeggpu_ext_resize_to_rgb_oriented(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors,
    const int* orientations,
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter,
    enum jpeggpu_ext_output_layout layout,
    uint8_t* dst,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);

/* The batched resize written as a model's input: jpeggpu_ext_resize_to_rgb_oriented (RandomResizedCrop equal to torchvision
 * on Pillow) followed, in the same vertical pass and before anything is stored, by what every training loader does next:
 * RandomHorizontalFlip, ToTensor and Normalize, and a cast to half precision. `colors` NULL: each item's model by its
 * component count (jpeggpu_ext_resize_to_rgb); `orientations` NULL: 1 for all. The first-pass launches are exactly those
 * of the uint8 call on the same arguments; the vertical pass is another kernel: at most three launches, two without items
 * of orientations 5..8.
 *   - `dst`: n x out_h x out_w x 3 (JPEGGPU_EXT_NHWC) or n x 3 x out_h x out_w (JPEGGPU_EXT_NCHW) elements of spec->type,
 *     rows unpadded. It must be aligned to the element (else JPEGGPU_INVALID_ARGUMENT) and need not be aligned further.
 *   - JPEGGPU_EXT_TENSOR_U8: the bytes of the uint8 call; `mean` and `std` are ignored.
 *   - The float types, THE CONTRACT: for byte u of channel c (0: R, 1: G, 2: B)
 *         y = ((float(u) / 255.0f) - mean[c]) / std[c]
 *     Every operation is an IEEE-754 binary32 operation, rounded to nearest even on its own. It is not contracted into an
 *     FMA, not computed with a reciprocal multiply and not folded into one scale and bias. This is what ToTensor and
 *     Normalize compute on the CPU: img.float().div(255), then sub_(mean).div_(std) with float32 tensors. (The reciprocal
 *     form differs from it in 322 of the 3 x 256 values for the ImageNet constants, the single-FMA form in 522.) mean 0
 *     and std 1 give ToTensor alone: - 0.0f and / 1.0f are exact. JPEGGPU_EXT_TENSOR_F16 and _BF16 are that float32
 *     value converted once, round to nearest even; they are NOT arithmetic done in half precision.
 *   - `flips`: host memory, n entries, read before the call returns; non-zero: item i is flipped left to right -- output
 *     column x is column out_w - 1 - x of the unflipped result (torch.flip of the resized image over its width, which is
 *     torchvision's flip AFTER the resize; a resize of the mirrored source differs from it in the last bit). NULL: no item
 *     is flipped. Flips compose with every orientation and colour model: they touch the vertical pass only.
 *   - `d_scratch`, `scratch_size`: those of the uint8 call on the same items, colours and orientations --
 *     jpeggpu_ext_resize_scratch_size_oriented, or jpeggpu_ext_resize_scratch_size_cs / jpeggpu_ext_resize_scratch_size where
 *     `orientations` / `colors` are NULL. There is no size call of its own.
 *   - JPEGGPU_INVALID_ARGUMENT: `spec` NULL, a type that is none of the four, and for a float type a std[c] that is zero
 *     or a mean[c] or std[c] that is not finite -- checked first; then everything the uint8 call refuses, with its statuses
 *     (n <= 0, an unknown filter: JPEGGPU_NOT_SUPPORTED, an item's checks, NULL dst or scratch, an unknown layout, a
 *     scratch too small), and a `dst` not aligned to the element. Every check is made before anything is staged or
 *     enqueued; on an error nothing is written. */
enum jpeggpu_ext_tensor_type { JPEGGPU_EXT_TENSOR_U8 = 0, JPEGGPU_EXT_TENSOR_F32 = 1, JPEGGPU_EXT_TENSOR_F16 = 2, JPEGGPU_EXT_TENSOR_BF16 = 3 };
struct jpeggpu_ext_tensor_spec {
    enum jpeggpu_ext_tensor_type type;
    float mean[3], std[3];      /* float types only */
    const unsigned char* flips; /* host, n entries, non-zero: flip item i; NULL: none */
};
enum jpeggpu_status jpeggpu_ext_resize_to_tensor(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors, /* NULL: by the component count */
    const int* orientations,                    /* NULL: all 1 */
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter,
    enum jpeggpu_ext_output_layout layout,
    const struct jpeggpu_ext_tensor_spec* spec,
    void* dst,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);

/* Resize + CenterCrop (the evaluation transform; torchvision's Resize(s) + CenterCrop(c) on Pillow images): the batched
 * resize above, generalised from "the item's rectangle resized to out_w x out_h" to "the out_w x out_h window at (x, y) of
 * the resize of the item's WHOLE image to resized_w x resized_h" -- each item with its own resized size and window, all
 * in the same two (with items of orientations 5..8: three) launches, by the same kernels: only the weight tables differ.
 * jpeggpu_ext_resize_view_to_tensor is jpeggpu_ext_resize_to_tensor with views[i] per item: `items`, `colors`,
 * `orientations` (either may be NULL as there), `spec` (JPEGGPU_EXT_TENSOR_U8 gives the bytes), `dst`, the scratch, the
 * staging ring and the statuses and their order are that call's. jpeggpu_ext_resize_view_scratch_size is its size call (0
 * for arguments the call would refuse, a NULL `views` among them).
 *   - The whole image of item i is the image's extent by its planes when `crop` is NULL, otherwise the full plane size of
 *     a component with the largest factors (crop->full_x / full_y): the image at the decoder's scale. It is turned for
 *     orientations 5..8: resized_w, resized_h, x and y are in DISPLAYED pixels.
 *   - A window pixel inside the resized image is Pillow's Image.resize((resized_w, resized_h), filter) pixel of the whole
 *     displayed image, by the arithmetic stated at jpeggpu_ext_resize_to_rgb with in = the whole image's size and out =
 *     the resized size -- the taps are NOT clamped at the item's rectangle. A pixel outside it (x or y negative, or the
 *     window reaching beyond resized_w / resized_h: CenterCrop's padding of an image smaller than the crop) is byte 0 in
 *     all three channels, which a float type carries through ((0 / 255) - mean) / std like any other byte.
 *   - The item's rectangle (the whole image, or the crop of a cropped decode) must hold every source pixel the window's
 *     taps read, else JPEGGPU_INVALID_ARGUMENT. jpeggpu_ext_resize_view_rect (host only, pure) returns exactly that
 *     rectangle in STORED coordinates for a stored full_w x full_h image: the union of the column and row tap ranges of
 *     the window's coordinates, mapped as jpeggpu_ext_orient_rect maps -- pass it to jpeggpu_ext_set_crop and only that part
 *     of the file is decoded. Any rectangle that contains it will do.
 *   - `replicate`: libjpeg replicates this item's chroma instead of fancy upsampling (an image of
 *     JPEGGPU_EXT_SCALE_LIBJPEG at 1/8 with subsampling left: jpeggpu_ext_get_scale_info's fancy_upsampling == 0), so such
 *     items are taken here and equal Pillow after draft().
 *   - The view {out_w, out_h, 0, 0, 0} of an item that is a whole image is jpeggpu_ext_resize_to_tensor's result byte for
 *     byte, from the same plan, scratch layout and launches.
 *   - JPEGGPU_INVALID_ARGUMENT besides what jpeggpu_ext_resize_to_tensor refuses: `views` NULL, resized_w or resized_h <=
 *     0, a window that overlaps no pixel of the resized image, a rectangle that does not hold the taps' pixels or does not
 *     lie in the whole image. The view's checks follow the item's own; every check is made before anything is staged or
 *     enqueued, and on an error nothing is written.
 * jpeggpu_ext_resize_view_weights (host only) is the table the kernels get for output coordinates x0 .. x0 + count_out - 1
 * of `in` -> `resized`: jpeggpu_ext_resize_weights' rows for the coordinates inside [0, resized), `first` minus `origin`
 * (the rectangle's first sample; it is not checked against any extent); a coordinate outside gets count 0, weights 0 and
 * a `first` that keeps first and first + count from decreasing along the table, which the horizontal pass relies on: in
 * front of the image the `first` of the first entry with taps, behind it first + count of the last (0 if no entry has
 * taps). JPEGGPU_INVALID_ARGUMENT for NULL pointers, in, resized or count_out <= 0 or max_taps below what
 * jpeggpu_ext_resize_weights asks for in -> resized; JPEGGPU_NOT_SUPPORTED for another filter. */
struct jpeggpu_ext_resize_view {
    int resized_w, resized_h;  /* what Image.resize is asked for, of the item's WHOLE displayed image at its scale */
    int x, y;                  /* the window's top-left corner in that resized image; may be negative (padding) */
    int replicate;             /* libjpeg replicates this item's chroma (scale_info.fancy_upsampling == 0) */
};
size_t jpeggpu_ext_resize_view_scratch_size(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors, /* NULL: by the component count */
    const int* orientations,                    /* NULL: all 1 */
    const struct jpeggpu_ext_resize_view* views,
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter);
enum jpeggpu_status jpeggpu_ext_resize_view_to_tensor(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors, /* NULL: by the component count */
    const int* orientations,                    /* NULL: all 1 */
    const struct jpeggpu_ext_resize_view* views,
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter,
    enum jpeggpu_ext_output_layout layout,
    const struct jpeggpu_ext_tensor_spec* spec,
    void* dst,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);
enum jpeggpu_status jpeggpu_ext_resize_view_rect(
    int full_w, /* the STORED image at its scale */
    int full_h,
    int orientation,
    const struct jpeggpu_ext_resize_view* view,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter,
    int* x,
    int* y,
    int* w,
    int* h);
enum jpeggpu_status jpeggpu_ext_resize_view_weights(
    int in,
    int resized,
    int x0,
    int count_out,
    int origin,
    enum jpeggpu_ext_filter filter,
    int* first,
    int* count,
    int* weights,
    int max_taps);

/* Thumbnails (a resize service, a thumbnail cache): Pillow's im.thumbnail((req_w, req_h), BILINEAR | BICUBIC, reducing_gap)
 * of many JPEG files at once, each with its own result size. That chain is not Image.resize: it has a size rule of its
 * own, decodes at a reduced scale (draft), averages integer boxes (Image.reduce) in front of the convolution, and resizes
 * from a box that may end inside a sample.
 *
 * jpeggpu_ext_thumbnail_plan (host only, pure) says what the chain does to a width x height file. `reducing_gap` <= 0 is
 * Pillow's None; otherwise it must be at least 1.
 *   1. The final size out_w x out_h: if req_w >= width and req_h >= height nothing happens -- the thumbnail is the
 *      full-scale decode (identity = 1, scale 1). Otherwise, in doubles, with aspect = width / height: if req_w / req_h >=
 *      aspect the width becomes round_aspect(req_h * aspect), else the height round_aspect(req_w / aspect), where
 *      round_aspect takes of floor and ceil the one whose ratio to the other side is nearer `aspect` (the floor on a tie;
 *      a height of 0 counts as exact) and then at least 1.
 *   2. With a gap: draft() for (int(req_w g), int(req_h g)): s = min(width / that, height / that) in integers, rounded down
 *      to 8, 4, 2 or 1 = `scale`. The decode -- JPEGGPU_EXT_SCALE_LIBJPEG at that scale -- has dec_w x dec_h = ceil(width /
 *      s) x ceil(height / s) pixels, and the box is width / s x height / s in doubles.
 *   3. If the decode has the final size it is the thumbnail (identity = 1), whatever the box.
 *   4. With a gap: fx = int(box_w / out_w / g) or 1, fy alike. If either exceeds 1 the decode is reduced by (fx, fy) to
 *      red_w x red_h = ceil(dec_w / fx) x ceil(dec_h / fy) and the box is divided by the factors; else red = dec.
 *   5. box_w, box_h: the box rounded to binary32, as it passes through Pillow's C code. The resize is of red_w x red_h
 *      pixels to out_w x out_h from the box (0, 0, box_w, box_h).
 *   6. JPEGGPU_NOT_SUPPORTED if red_h > 100 red_w and out_h < red_h: Pillow runs the vertical pass first on such an image.
 * `replicate` is set to 0; the caller sets it for an image whose chroma libjpeg replicates at `scale`
 * (jpeggpu_ext_get_scale_info: fancy_upsampling == 0). JPEGGPU_INVALID_ARGUMENT: a NULL plan, width or height outside
 * 1..65535, req_w or req_h < 1, a gap in (0, 1), not a number, or above 65536. JPEGGPU_NOT_SUPPORTED: another filter.
 *
 * jpeggpu_ext_resize_box_weights (host only) is jpeggpu_ext_resize_weights for `in` samples of which the resize covers
 * `extent`: scale = extent / out in double, everything else as stated there, the taps clamped at `in`; max_taps at least 2
 * ceil(support) + 1 with fs = max(extent / out, 1). extent == in gives jpeggpu_ext_resize_weights' table bit for bit.
 *
 * jpeggpu_ext_thumbnail_to_rgb makes the thumbnails of n decoded images: items[i] are the whole planes of a decode at
 * plans[i].scale (`crop` NULL), colors[i] their model (NULL: by the component count). `dst` is n x canvas_h x canvas_w x 3
 * uint8; item i's thumbnail, out_h x out_w, lies in the top-left corner of slot i, zeros elsewhere in the slot. A grey
 * file's thumbnail is its one channel three times. On planes of a JPEGGPU_EXT_IDCT_ISLOW, JPEGGPU_EXT_SCALE_LIBJPEG decode
 * the thumbnail equals np.asarray(im) after im.thumbnail(...) (for a grey file: each channel does).
 *   - The reduction: an output pixel over nx x ny source pixels (fx x fy, fewer in the last column and row) is, per
 *     channel, ((sum + n / 2) * m) >> 24 in 32-bit unsigned arithmetic with n = nx ny and m = (uint32)((float)(1 << 24) /
 *     (float)n) -- not a rounded mean. One launch for all items that reduce; it reads the planes as every conversion here
 *     does (fancy upsampling or replication, the colour model), so the decoded-size RGB is never written, and leaves
 *     reduced planes in `d_scratch` that the resize passes read as an RGB-coded (or grey) image.
 *   - The resize: jpeggpu_ext_resize_view_to_tensor's two launches with the view {out_w, out_h, 0, 0} of the canvas and the
 *     tables of jpeggpu_ext_resize_box_weights; an item with identity = 1 gets one tap of weight 1 per coordinate. At most
 *     three launches per call, two if no item reduces.
 *   - `d_scratch`: at least jpeggpu_ext_thumbnail_scratch_size bytes (0 for arguments the call would refuse; it only grows
 *     with n for the same items), private to the stream until the call has executed; the staging ring is the resize calls'.
 *   - JPEGGPU_NOT_SUPPORTED: another filter, a model that does not fit the component count, non-integral sampling ratios,
 *     a CMYK or YCCK item (Pillow's thumbnail of those is CMYK), a box of more than 2^23 pixels, a plan that 6. refuses.
 *     JPEGGPU_INVALID_ARGUMENT: NULL pointers, n, canvas_w or canvas_h <= 0 (or n > 65535), an item with a `crop`, a plan
 *     that does not fit its item (dec_w x dec_h is not the image's extent by its planes; red_w, red_h not the ceilings; fx
 *     or fy < 1; out_w or out_h < 1 or beyond the canvas; a box that is not positive and finite; identity with factors or
 *     with another final size), scratch_size too small. Every check is made before anything is staged or enqueued; on an
 *     error nothing is written. */
struct jpeggpu_ext_thumbnail {
    int scale;             /* 1, 2, 4 or 8: what to decode at (JPEGGPU_EXT_SCALE_LIBJPEG) */
    int dec_w, dec_h;      /* the decoded size */
    int fx, fy;            /* Image.reduce's factors; 1, 1: no reduction */
    int red_w, red_h;      /* the size after the reduction */
    float box_w, box_h;    /* how much of red_w x red_h the resize covers */
    int out_w, out_h;      /* the thumbnail's size */
    int identity;          /* the decode is the thumbnail */
    int replicate;         /* libjpeg replicates this item's chroma (set by the caller) */
};
enum jpeggpu_status jpeggpu_ext_thumbnail_plan(
    int width, int height, int req_w, int req_h, enum jpeggpu_ext_filter filter, double reducing_gap, struct jpeggpu_ext_thumbnail* plan);
enum jpeggpu_status jpeggpu_ext_resize_box_weights(
    int in, float extent, int out, enum jpeggpu_ext_filter filter, int* first, int* count, int* weights, int max_taps);
size_t jpeggpu_ext_thumbnail_scratch_size(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors, /* NULL: by the component count */
    const struct jpeggpu_ext_thumbnail* plans,
    int n,
    int canvas_w,
    int canvas_h,
    enum jpeggpu_ext_filter filter);
enum jpeggpu_status jpeggpu_ext_thumbnail_to_rgb(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors, /* NULL: by the component count */
    const struct jpeggpu_ext_thumbnail* plans,
    int n,
    int canvas_w,
    int canvas_h,
    enum jpeggpu_ext_filter filter,
    uint8_t* dst,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);

/* Batched conversion to RGB (a list of files in, a list of RGB images out, each at its own size -- a validation loader,
 * or torchvision.io.decode_jpeg on a list): what jpeggpu_ext_crop_to_rgbi_oriented makes of every item with a `crop`, and
 * jpeggpu_ext_planes_to_rgbi_oriented of every item without one at the image's own extent by its planes (the size of a
 * plane with the largest sampling factors), each into its own `dst`, with ONE launch for all items of orientations 1..4
 * and one for all of 5..8 -- at most two per call, not one per image. Planes of one jpeggpu_ext_decode_batch call are the
 * usual source. Items may mix sizes, scales, IDCT methods, sampling layouts, colour models, orientations, cropped and
 * whole images.
 *   - Per item: `info`, `crop` (NULL: the whole image) and `src` as in jpeggpu_ext_resize_item; `color` the planes' model
 *     (jpeggpu_ext_get_color_space); `orientation` 1..8 (1: stored order); `replicate` 0: fancy upsampling, else
 *     replication (an image of JPEGGPU_EXT_SCALE_LIBJPEG at 1/8 with subsampling left: jpeggpu_ext_get_scale_info's
 *     fancy_upsampling == 0) -- this item has room for the flag, so such images are converted here. `crop` and the
 *     planes are stored; `dst` holds the DISPLAYED rectangle, ow x oh = width x height for 1..4 and height x width for 5..8.
 *   - JPEGGPU_EXT_HWC: R, G, B of displayed pixel (x, y) at dst + y * dst_pitch + 3 x, dst_pitch >= 3 ow.
 *     JPEGGPU_EXT_CHW: channel c at dst + c * plane_stride + y * dst_pitch + x, dst_pitch >= ow and plane_stride >=
 *     dst_pitch * oh (plane_stride is not read for HWC). No alignment is asked of dst or the pitches; rows that start on a
 *     dword are written in dwords. Outputs that overlap each other are the caller's error and are not checked.
 *   - `d_scratch`: caller-owned device memory of at least jpeggpu_ext_batch_rgb_scratch_size(n) bytes (the items'
 *     descriptors and tile lists; host only, 0 for n <= 0 or n > 65535, never smaller for a larger n), private to the
 *     stream until the call has executed. The host may reuse `items` (and what they point to) as soon as the call
 *     returns: the descriptors are copied from the page-locked staging ring of the resize calls (of four: the fifth call
 *     in a row waits until the copy of the first has executed). `stream` must belong to the current device.
 *   - Each item is checked like the per-image calls, with their statuses in their order (a window outside its plane is
 *     refused before non-integral ratios): JPEGGPU_NOT_SUPPORTED for a model that does not fit the component count,
 *     UNKNOWN, non-integral sampling ratios; JPEGGPU_INVALID_ARGUMENT for NULL pointers in an item, windows that do not
 *     hold the rectangle's samples and their halo. JPEGGPU_INVALID_ARGUMENT as well: NULL `items` or `d_scratch`, n <= 0 or
 *     n > 65535, a NULL `dst`, an orientation outside 1..8, a dst_pitch or plane_stride too small, an unknown layout,
 *     scratch_size too small. The first item that fails decides. Every check is made before anything is enqueued and
 *     without touching the device; on an error nothing is written. */
enum jpeggpu_ext_image_layout { JPEGGPU_EXT_HWC = 0, JPEGGPU_EXT_CHW = 1 };
struct jpeggpu_ext_rgb_item {
    const struct jpeggpu_img_info* info;       /* as parse_header reported it (a cropped decode: the windows) */
    const struct jpeggpu_ext_crop_info* crop;  /* jpeggpu_ext_get_crop's result; NULL: the whole image */
    const struct jpeggpu_img* src;             /* the decoded planes */
    enum jpeggpu_ext_color_space color;
    int orientation;                           /* 1..8 */
    int replicate;
    uint8_t* dst;                              /* the displayed rectangle */
    int dst_pitch;
    size_t plane_stride;                       /* JPEGGPU_EXT_CHW only */
};
size_t jpeggpu_ext_batch_rgb_scratch_size(int n);
enum jpeggpu_status jpeggpu_ext_batch_to_rgb(
    const struct jpeggpu_ext_rgb_item* items,
    int n,
    enum jpeggpu_ext_image_layout layout,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);

/* Grey output: one 8-bit channel, what libjpeg hands a caller of out_color_space = JCS_GRAYSCALE and Pillow's
 * np.asarray(im) shows after im.draft("L", size). The grey of a pixel: for GRAY and YCBCR sources component 0, upsampled
 * only where its sampling factors are below the frame's largest (by the fancy or the replicating rule of the RGB calls);
 * for RGB sources (RGB-coded files) (19595 R + 38470 G + 7471 B + 32768) >> 16 of the three upsampled samples, jdcolor.c's
 * rgb_gray_convert. CMYK, YCCK and UNKNOWN: JPEGGPU_NOT_SUPPORTED. Of a GRAY or YCBCR source only component 0's plane is read:
 * src->image[1..] may be NULL, as after a decode with jpeggpu_ext_set_luma_only; `info` (and `crop`) are parse_header's
 * (jpeggpu_ext_get_crop's) as they are, all components of them. Three calls, the grey forms of three RGB calls, with their
 * validation rules, statuses and the same contract that nothing is written on an error:
 *   - jpeggpu_ext_crop_to_gray_oriented: jpeggpu_ext_crop_to_rgbi_oriented for one channel, displayed pixel (x, y) at
 *     dst + y * dst_pitch + x, dst_pitch >= the displayed width. `crop` NULL: the whole image, at its extent by its planes
 *     (jpeggpu_ext_planes_to_rgbi_oriented). One launch.
 *   - jpeggpu_ext_batch_to_gray: jpeggpu_ext_batch_to_rgb for one channel; the items are jpeggpu_ext_rgb_item, of which
 *     plane_stride is not read and dst_pitch >= the displayed width. Scratch: jpeggpu_ext_batch_gray_scratch_size(n), with
 *     that call's rules. At most two launches. An item of orientation 1 whose component 0 has the largest factors is a
 *     pitched copy of a window of plane 0: it is made by the same launch, in 16-byte pieces.
 *   - jpeggpu_ext_resize_view_to_gray_tensor: jpeggpu_ext_resize_view_to_tensor for one channel -- views, orientations,
 *     per-item flips, the four element types -- with `views` NULL meaning whole rectangles resized to out_w x out_h, which
 *     makes it the grey form of jpeggpu_ext_resize_to_rgb and jpeggpu_ext_resize_to_tensor too. The arithmetic is Pillow's
 *     ImagingResample on one 8-bit band: the weights of jpeggpu_ext_resize_weights, the rounding and the clamp to 8 bits
 *     after the first pass are those of the RGB calls. Normalisation uses spec->mean[0] and spec->std[0] alone. `dst` is n
 *     x out_h x out_w x 1 (NHWC) or n x 1 x out_h x out_w (NCHW): the same bytes. Scratch:
 *     jpeggpu_ext_resize_view_to_gray_scratch_size of the same arguments (0 for arguments the call would refuse); the rows
 *     between the passes hold one byte per pixel, out_w padded to 16, a third of the RGB call's. Two launches, three
 *     when items of orientations 5..8 stand beside others.
 * Thumbnails stay RGB-only: jpeggpu_ext_thumbnail_plan, jpeggpu_ext_thumbnail_to_rgb and the Python thumbnail calls have no
 * grey form. */
enum jpeggpu_status jpeggpu_ext_crop_to_gray_oriented(
    const struct jpeggpu_img_info* info,
    enum jpeggpu_ext_color_space color,
    int orientation,
    int replicate,
    const struct jpeggpu_ext_crop_info* crop,
    const struct jpeggpu_img* src,
    uint8_t* dst,
    int dst_pitch,
    jpeggpu_stream_t stream);
size_t jpeggpu_ext_batch_gray_scratch_size(int n);
enum jpeggpu_status jpeggpu_ext_batch_to_gray(
    const struct jpeggpu_ext_rgb_item* items,
    int n,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);
size_t jpeggpu_ext_resize_view_to_gray_scratch_size(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors,
    const int* orientations,
    const struct jpeggpu_ext_resize_view* views,
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter);
enum jpeggpu_status jpeggpu_ext_resize_view_to_gray_tensor(
    const struct jpeggpu_ext_resize_item* items,
    const enum jpeggpu_ext_color_space* colors,
    const int* orientations,
    const struct jpeggpu_ext_resize_view* views,
    int n,
    int out_w,
    int out_h,
    enum jpeggpu_ext_filter filter,
    enum jpeggpu_ext_output_layout layout,
    const struct jpeggpu_ext_tensor_spec* spec,
    void* dst,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);

/* Encoding: grey or RGB uint8 images in device memory to baseline JPEG files in device memory, many per call. The file is
 * the one Pillow writes on libjpeg-turbo -- Image.fromarray(x).save(f, "JPEG", quality=, subsampling=,
 * restart_marker_blocks=) -- byte for byte (tests/golden/encode_pins.npz): jccolor.c's fixed-point RGB -> YCbCr, jcsample.c's
 * h2v1 / h2v2 downsampling without smoothing and its edge rules, jpeg_fdct_islow, the quantiser's rounded division,
 * jpeg_set_quality's tables, jccoefct.c's dummy blocks, jchuff.c with the Annex K tables, a JFIF header without
 * density; with `optimize` set, jchuff.c's statistics pass and jpeg_gen_optimal_table, the file of save(..., optimize=True)
 * (tests/golden/encode_opt_pins.npz); with `progressive` set, jpeg_simple_progression's script coded by jcphuff.c, the file of
 * save(..., progressive=True) (tests/golden/encode_prog_pins.npz). Not written: other samplings, four components, other scan
 * scripts, EXIF / ICC.
 *   - An item: `data` the device pointer of sample (0, 0) of channel 0; sample (x, y) of channel c is the byte at
 *     data + y * row_pitch + x * pixel_stride + c * channel_stride, so an HWC tensor (pixel_stride 3, channel_stride 1), a CHW
 *     tensor (pixel_stride 1, channel_stride H * W) and any view of either are one struct, without a copy. `channels` 1 (grey)
 *     or 3 (RGB). `quality` 1..100. `subsampling` of the chroma; a grey file has no chroma, and the value only sets the
 *     sampling factors its frame header names (as Pillow does). `restart_interval` in MCUs, 0..65535, 0: no restart markers.
 *     `out`, `capacity`: the item's output slot (out may be NULL with capacity 0: the call then only reports the size).
 *   - jpeggpu_ext_encode_header (host only, needs no device): SOI up to the end of the scan header. `*size` is the room in
 *     host_buf on entry and the header's length on return; host_buf NULL only asks for the length.
 *   - jpeggpu_ext_encode_bound (host only): the size no file of the item's geometry can exceed. A block takes at most 22 bits
 *     of DC (the longest DC code of the tables, 11 bits, and 11 value bits) and 63 x 26 bits of AC (a 16-bit code and 10 value
 *     bits per coefficient; a ZRL or EOB is shorter than the coefficients it stands for): 1660 bits. So the stream has at
 *     most ceil(1660 blocks / 8) + segments bytes with the padding of each restart segment; every byte may be 0xFF and
 *     doubled by stuffing; then the header, two bytes per restart marker and EOI. 0 for an invalid item.
 *   - jpeggpu_ext_encode_batch encodes items[0..n) on `stream` with EIGHT launches (TEN: `optimize`) and one copy of descriptors whatever n and
 *     the sizes are, and does not synchronise. d_sizes[i] receives the file's length and d_status[i] JPEGGPU_EXT_ENCODE_OK,
 *     or JPEGGPU_EXT_ENCODE_TOO_SMALL if that length exceeds `capacity`: then d_sizes[i] is the capacity it needs and not one
 *     byte of its slot is written; the other items are not affected. Sizes are known on the device before anything is written
 *     to a slot. `d_scratch`: caller-owned device memory of at least jpeggpu_ext_encode_scratch_size(items, n) bytes,
 *     private to the stream until the call has executed; it holds the coefficients (2 bytes per padded sample) and the
 *     unstuffed stream at its bound. The host may reuse `items` when the call returns: descriptors and headers travel
 *     through a page-locked ring of four (the fifth call in a row waits until the copy of the first has executed).
 *   - `optimize` 1: the item's Huffman tables are made from its own symbol counts, as libjpeg makes them (a call may mix items
 *     with and without). Its DHT segments, and so its header, depend on the pixels: jpeggpu_ext_encode_header returns
 *     JPEGGPU_NOT_SUPPORTED for it and sets `*size` to the length of the header with the Annex K tables, which no optimised
 *     header exceeds (its DHTs list at most the same 12 + 162 symbols, twice). An optimised DC code can take 16 bits, so
 *     jpeggpu_ext_encode_bound counts 16 + 11 + 63 x 26 = 1665 bits per block for such an item, with that header length, and
 *     the scratch size follows; for items without the flag both are what they were. A call with at least one such item
 *     enqueues TEN launches (the symbol counts and the tables, behind the first), still with one copy and no
 *     synchronisation. d_status[i] JPEGGPU_EXT_ENCODE_TABLE_OVERFLOW: a code of the item would be longer than 32 bits before
 *     limiting, where libjpeg raises JERR_HUFF_CLEN_OVERFLOW (a table of more than 32 symbols whose counts grow like
 *     Fibonacci numbers: millions of blocks); d_sizes[i] is 0, the slot is not written, the other items are not affected.
 *   - `progressive` 1 (`optimize` is then ignored: libjpeg always optimises a progressive file, and the bytes are the same
 *     with either value): a frame header SOF2 and ten scans for RGB, six for grey -- DC first, the low and the high AC band
 *     of luma, the chroma AC bands, then the refinements --, each scan behind the DHTs of the tables made from its own symbol
 *     counts (none for a DC refinement), one DRI before the first SOS, restart intervals counted in MCUs of the scan at
 *     hand (one block in a scan of one component, which walks the component's real blocks only). A call may mix such items
 *     with the others. They add ELEVEN launches to the call, whatever their number, their sizes and the number of their
 *     scans; a call without one enqueues what it always did. jpeggpu_ext_encode_header returns JPEGGPU_NOT_SUPPORTED for such
 *     an item and sets `*size` to a bound on ALL its marker segments: SOI .. SOF2, ten (grey: five) DHTs of 277 bytes, DRI and
 *     every SOS. jpeggpu_ext_encode_bound counts per block of a scan, every code 16 bits long: DC first 16 + 11 bits, DC
 *     refinement 1, AC first 26 per coefficient of the band (a code and 10 value bits; a ZRL stands for 16 of them) and 30
 *     for an EOBn symbol with its 14 bits of run length, AC refinement 17 per coefficient (a code and a sign, or one
 *     correction bit) and 30; per scan ceil(bits / 8) bytes and one byte of padding per restart segment of that scan; all
 *     of it doubled by stuffing; two bytes per restart marker of every scan; the marker segments; EOI. The scratch size
 *     follows. JPEGGPU_EXT_ENCODE_TOO_SMALL and _TABLE_OVERFLOW (any table of any scan) are reported as for `optimize`.
 *   - jpeggpu_ext_encode_tables_from_counts runs only the table kernel, on `stream`: d_counts holds 256 counts per table,
 *     d_bits_values receives per table the 16 `bits` bytes and 256 `values` bytes of a DHT segment (values behind the last
 *     symbol are 0), d_status[t] JPEGGPU_EXT_ENCODE_OK, _TABLE_OVERFLOW, or _EMPTY_TABLE for counts that are all zero (libjpeg
 *     does not define that table) or beyond what libjpeg's search covers (a count of 2^28, a sum of 10^9); then bits and
 *     values are zeros. JPEGGPU_INVALID_ARGUMENT for a NULL pointer or n_tables <= 0.
 *   - JPEGGPU_INVALID_ARGUMENT, before anything is enqueued: NULL items, d_scratch, d_sizes, d_status or data, a NULL out with
 *     a capacity, n <= 0 or > 65535, width or height outside 1..65535, channels other than 1 or 3, quality outside 1..100, an
 *     unknown subsampling, a restart interval outside 0..65535, an `optimize` or `progressive` other than 0 or 1, scratch_size too small. JPEGGPU_NOT_SUPPORTED: an item whose
 *     stream bound reaches 2^32 bits (about 2.5 million blocks: 160 megapixels grey), or a call of 2^31 blocks. */
enum jpeggpu_ext_subsampling { JPEGGPU_EXT_SUBSAMPLING_444 = 0, JPEGGPU_EXT_SUBSAMPLING_422 = 1, JPEGGPU_EXT_SUBSAMPLING_420 = 2 };
enum jpeggpu_ext_encode_status {
    JPEGGPU_EXT_ENCODE_OK             = 0,
    JPEGGPU_EXT_ENCODE_TOO_SMALL      = 1,
    JPEGGPU_EXT_ENCODE_TABLE_OVERFLOW = 2, /* an optimised code longer than 32 bits before limiting */
    JPEGGPU_EXT_ENCODE_EMPTY_TABLE    = 3, /* jpeggpu_ext_encode_tables_from_counts only */
    JPEGGPU_EXT_ENCODE_UNCODABLE      = 4, /* jpeggpu_ext_transcode_batch only: a coefficient the target cannot code */
    JPEGGPU_EXT_ENCODE_OVER_BUDGET    = 5  /* jpeggpu_ext_encode_fit_batch only: even quality_min exceeds max_bytes */
};
struct jpeggpu_ext_encode_item {
    const uint8_t* data;
    int width, height;
    int channels;
    int progressive; /* 0: one baseline scan, 1: libjpeg's progressive script (where LP64 had padding: size and offsets are unchanged) */
    int64_t row_pitch, pixel_stride, channel_stride; /* bytes */
    int quality;
    int subsampling; /* enum jpeggpu_ext_subsampling */
    int restart_interval;
    int optimize; /* 0: the Annex K tables, 1: tables made for the image (where LP64 had padding: size and offsets are unchanged) */
    uint8_t* out;
    size_t capacity;
};
enum jpeggpu_status jpeggpu_ext_encode_header(const struct jpeggpu_ext_encode_item* item, uint8_t* host_buf, size_t* size);
size_t jpeggpu_ext_encode_bound(const struct jpeggpu_ext_encode_item* item);
size_t jpeggpu_ext_encode_scratch_size(const struct jpeggpu_ext_encode_item* items, int n);
enum jpeggpu_status jpeggpu_ext_encode_batch(
    const struct jpeggpu_ext_encode_item* items,
    int n,
    void* d_scratch,
    size_t scratch_size,
    size_t* d_sizes,
    int* d_status,
    jpeggpu_stream_t stream);
enum jpeggpu_status jpeggpu_ext_encode_tables_from_counts(
    const uint32_t* d_counts,
    int n_tables,
    uint8_t* d_bits_values,
    int* d_status,
    jpeggpu_stream_t stream);

/* Encoding to a byte budget: for every item the best quality of a range whose file is no longer than `max_bytes`, found on
 * the device, and that file -- byte for byte the one jpeggpu_ext_encode_batch writes for the item at the chosen quality.
 *   - The chosen quality, exactly. Let size(q) be the length of jpeggpu_ext_encode_batch's file of the item at quality q (its
 *     subsampling, restart interval and `optimize` flag are the item's own; with `optimize` 1 every q has its own tables and
 *     size(q) counts their DHTs). With lo = quality_min, hi = quality_max, B = max_bytes:
 *         if size(hi) <= B:     chosen = hi
 *         else if size(lo) > B: JPEGGPU_EXT_ENCODE_OVER_BUDGET
 *         else: best = lo, a = lo + 1, b = hi - 1; while a <= b: m = (a + b) / 2;
 *               if size(m) <= B: best = m, a = m + 1; else b = m - 1;     chosen = best
 *     size(q) is NOT monotone in q (on small images a step down by a byte or two from q to q + 1 is common), so this rule, not
 *     "the largest quality that fits", is the contract: the file always fits, and the chosen quality is the largest fitting
 *     one wherever size grows with quality.
 *   - An item: `item` as for jpeggpu_ext_encode_batch, except that item.quality is ignored and item.progressive must be 0;
 *     1 <= quality_min <= quality_max <= 100. `out`, `capacity`: the slot of the chosen file; `max_bytes` limits the file, not
 *     the slot (out may be NULL with capacity 0: the call then only reports quality and size).
 *   - d_quality[i] receives the chosen quality, for an item over budget quality_min. d_status[i]: JPEGGPU_EXT_ENCODE_OK;
 *     JPEGGPU_EXT_ENCODE_TOO_SMALL as for jpeggpu_ext_encode_batch -- `capacity` is smaller than the chosen file, d_sizes[i] is
 *     what it needs, the slot is untouched; JPEGGPU_EXT_ENCODE_OVER_BUDGET -- even quality_min is larger than max_bytes,
 *     d_sizes[i] is size(quality_min), the slot is untouched; _TABLE_OVERFLOW as for `optimize` (a probe whose tables
 *     overflow has no file and counts as size 0). An item's status never affects its neighbours.
 *   - The pixel stage (colour conversion, downsampling, FDCT) runs once per call and keeps the unquantised transform; each
 *     evaluation of size() requantises it with a quality that lives in device memory and runs the encoder's size stages. The
 *     items of a call search in lockstep; the host derives the number of evaluations P from the widest range of the call
 *     (w = quality_max - quality_min + 1: P = 1 for w = 1, 2 for w = 2, else 3 + floor(log2(w - 2)); 9 for 1..100) and
 *     enqueues everything at once: the call does not synchronise, no evaluation makes the host wait for the device, and
 *     descriptors and headers travel through the encoder's page-locked ring in one copy. An item whose search has ended
 *     sits out the remaining evaluations (its tiles and chunks leave every kernel at their first test).
 *   - Launches: 10 + 8 P, and 12 + 10 P for a call with at least one `optimize` item -- one for the transform, per
 *     evaluation the requantiser, launches 2 - 7 of jpeggpu_ext_encode_batch (with `optimize`: 1a, 1b as well) and the
 *     decision, then the final pass at the chosen qualities: requantiser, the eight (ten) launches less the first, and the
 *     report. Whatever n and the image sizes are; jpeggpu_ext_encode_fit_launches (host only) returns the number for a
 *     call's items, 0 for invalid ones. 82 launches for the range 1..100.
 *   - `d_scratch`: at least jpeggpu_ext_encode_fit_scratch_size(items, n) bytes: what jpeggpu_ext_encode_scratch_size counts
 *     for the same items, and beyond it the unquantised transform (int16, 2 bytes per padded sample: jpeg_fdct_islow's
 *     output stays within +-8192 and a few units of rounding) and 64 bytes of search state per item. 0 for invalid items.
 *   - JPEGGPU_INVALID_ARGUMENT as for jpeggpu_ext_encode_batch, and for quality_min > quality_max, either outside 1..100, or a
 *     NULL d_quality. JPEGGPU_NOT_SUPPORTED, before anything is enqueued: an item with `progressive` 1 (a progressive search
 *     is not offered), and the limits of jpeggpu_ext_encode_batch. */
struct jpeggpu_ext_encode_fit_item {
    struct jpeggpu_ext_encode_item item; /* item.quality is ignored; item.progressive must be 0 */
    size_t max_bytes;
    int quality_min, quality_max;
};
size_t jpeggpu_ext_encode_fit_scratch_size(const struct jpeggpu_ext_encode_fit_item* items, int n);
int jpeggpu_ext_encode_fit_launches(const struct jpeggpu_ext_encode_fit_item* items, int n);
enum jpeggpu_status jpeggpu_ext_encode_fit_batch(
    const struct jpeggpu_ext_encode_fit_item* items,
    int n,
    void* d_scratch,
    size_t scratch_size,
    size_t* d_sizes,
    int* d_status,
    int* d_quality,
    jpeggpu_stream_t stream);

/* Lossless transcoding: a decoded JPEG's quantised coefficients, as the decoder's entropy stage leaves them in d_tmp, to a
 * new file with the encoder's entropy stages -- what jpegtran -optimize, -progressive and -restart N do: optimised Huffman
 * tables, a progressive file from a baseline one or the other way round, other restart intervals. No IDCT, no colour
 * conversion, no FDCT and no quantiser run; the output holds the source's coefficients exactly, so for a source Pillow wrote
 * the file is, byte for byte, the one Pillow writes with the other options (tests/golden/transcode_pins.npz).
 *   - An item: `decoder` has parsed the source (jpeggpu_decoder_parse_header), its bytes were transferred into `d_tmp`
 *     (jpeggpu_decoder_transfer) and jpeggpu_ext_decode_batch has decoded it there ON THE SAME STREAM, with
 *     jpeggpu_ext_batch_set_coefficients_only or without; d_tmp is read when the call executes. `progressive`, `optimize`, `out`
 *     and `capacity` as in jpeggpu_ext_encode_item. `restart_interval` in MCUs, 0: none, -1: the source's (the DRI in force at
 *     its first scan).
 *   - The file's layout is the encoder's: SOI, a JFIF APP0 without density, DQT 0 and for colour DQT 1 with the SOURCE's tables,
 *     SOF0 or SOF2, DHTs, DRI, SOS ... Markers are NOT copied: EXIF, ICC and COM segments are dropped, like jpegtran -copy none.
 *   - Dummy blocks (blocks of an MCU beyond a component's real grid): where a scan of the source codes them -- an interleaved
 *     scan, a progressive file's interleaved DC scans -- they keep the source's values; where none does (a component coded in
 *     a scan of its own) they are 64 zeros, as libjpeg's zeroed coefficient arrays leave them.
 *   - What can be transcoded is what the encoder writes: 8-bit samples; one component (its frame header keeps the sampling
 *     byte the source names), or three that jpeggpu_ext_get_color_space calls YCbCr with chroma 1x1 and luma 1x1, 2x1 or 2x2,
 *     8-bit quantisation tables (Pq = 0), Cb and Cr on one table. JPEGGPU_NOT_SUPPORTED, before anything is enqueued, for
 *     anything else (4:4:0, 4:1:1, RGB-coded, CMYK, YCCK, Pq = 1, Cb and Cr on different tables), for a decoder with a crop
 *     (unless jpeggpu_ext_set_transcode_crop is set too, below), a scale other than 1 or a segment shard, and at the encoder's size limits. JPEGGPU_INVALID_ARGUMENT as for
 *     jpeggpu_ext_encode_batch, for a decoder that has parsed nothing and a restart interval outside -1..65535.
 *   - jpeggpu_ext_transcode_header (host only): the header of an item without `optimize` and `progressive`, as
 *     jpeggpu_ext_encode_header; _bound and _scratch_size reuse the encoder's arithmetic per block.
 *   - jpeggpu_ext_transcode_batch enqueues what jpeggpu_ext_encode_batch enqueues, with a gather kernel in place of the pixel
 *     stage and one small launch behind the last: NINE launches (ELEVEN: `optimize`, ELEVEN more: `progressive`), one copy of
 *     descriptors, no synchronisation; a call may mix the three output kinds. d_status[i] as for encoding, and
 *     JPEGGPU_EXT_ENCODE_UNCODABLE for a source that holds an AC coefficient of category above 10 or a DC difference of
 *     category above 11 (a crafted file; nothing an 8-bit encoder writes): d_sizes[i] is 0, the slot is not written, the
 *     other items are not affected.
 *   - jpeggpu_ext_batch_set_coefficients_only(batch, 1): jpeggpu_ext_decode_batch stops in front of the IDCT stage (a
 *     transcode never reads the planes); the plane pointers of its items may then be NULL, and a call planned as lone decodes
 *     takes the batch's kernels. Default 0: the calls launch what they always did.
 *   - jpeggpu_ext_set_transcode_orientation(decoder, orientation, trim): jpegtran -flip / -rotate / -transpose / -transverse.
 *     The new file's STORED image is the displayed image O of the source's stored image S under `orientation`, 1..8 by the
 *     table at jpeggpu_ext_get_orientation, made in the coefficient domain without loss. Only the four jpeggpu_ext_transcode_
 *     calls read the setting, when they are called; it may be set any time after the decoder's creation and holds until it
 *     is set again; decodes to pixels ignore it. An orientation outside 1..8 or a `trim` other than 0 or 1:
 *     JPEGGPU_INVALID_ARGUMENT. With orientation 1 (the default) every call is what it was, launch for launch and byte for
 *     byte, dummy blocks included. Otherwise:
 *       - a real block of the target is the source's block of the same component under the table, taken on the component's
 *         own block grid; 5..8 transpose each block (natural index 8 v + u takes the source's 8 u + v); a mirrored displayed
 *         x (2, 3, 6, 7) negates the coefficients of odd horizontal frequency u, a mirrored displayed y (3, 4, 7, 8) those
 *         of odd v;
 *       - for 5..8 the size becomes H x W, both quantisation tables are transposed, and the sampling byte of component 0
 *         has its nibbles exchanged (a grey file's too, where it changes nothing else). 4:2:2 would become 4:4:0, which the
 *         encoder does not write: JPEGGPU_NOT_SUPPORTED;
 *       - a mirror is exact over whole iMCUs of the source only (8 hs x 8 vs pixels; 8 x 8 for grey). The stored x is
 *         mirrored for 2, 3, 7, 8: W must be a multiple of 8 hs. The stored y is mirrored for 3, 4, 6, 7: H must be a
 *         multiple of 8 vs. Orientation 5 needs neither. Otherwise, with `trim` 0 (jpegtran -perfect):
 *         JPEGGPU_NOT_SUPPORTED from all four calls, before anything is enqueued; with `trim` 1 (jpegtran -trim) the stored
 *         image is first cut at its right and / or bottom edge to the largest such multiple, and an axis shorter than one
 *         iMCU stays JPEGGPU_NOT_SUPPORTED;
 *       - the dummy blocks of the target (luma blocks of an MCU beyond the target's real grid) are the encoder's: 63 zeros
 *         and the DC of the real block in front of them in the MCU's order, as jctrans.c regenerates them. The source's own
 *         dummy blocks are never read;
 *       - the coding limits are the target's: the DC-difference rule runs in the target's prediction order.
 *         `restart_interval` -1 keeps the source's NUMBER of MCUs.
 *     A call with such an item launches another instantiation of the gather kernel; the number of launches is the same.
 *   - jpeggpu_ext_set_transcode_crop(decoder, x, y, width, height): jpegtran -crop. The new file holds the rectangle of the
 *     image the transcode would write without it -- the image AFTER the orientation and its trim, so with an orientation
 *     the rectangle is in displayed pixels, as jpegtran applies -crop to its transformed output. Read by the four
 *     jpeggpu_ext_transcode_ calls only, when they are called, and held until it is set again, like the orientation.
 *     (0, 0, 0, 0), the default, switches it off: every call is then what it was, launch for launch and byte for byte. A
 *     negative value, or a `width` or `height` of 0 beside any other value: JPEGGPU_INVALID_ARGUMENT at once. Checked by all
 *     four calls before anything is enqueued, on the uncropped target W' x H' with luma factors hs' x vs' (exchanged for
 *     5..8; 1 x 1 for grey):
 *       - x + width <= W' and y + height <= H', else JPEGGPU_INVALID_ARGUMENT;
 *       - x a multiple of 8 hs' and y of 8 vs', else JPEGGPU_NOT_SUPPORTED (jpegtran -perfect; round down and grow the size
 *         for jpegtran's own behaviour, as transcode_jpeg(expand=True) does). `width` and `height` may be anything from 1 up;
 *       - the orientation's edge and trim rules stay on the WHOLE source, as they are.
 *     The target is width x height. Its real blocks are the uncropped target's from block (x / 8, y / 8) of luma and
 *     (x / (8 hs'), y / (8 vs')) of chroma on; the mirrors run over the UNCROPPED target's grid (written block -> plus
 *     offset -> mirror -> exchange -> source block). Its dummy blocks are the encoder's, as for an orientation, also for a
 *     crop of the whole image (a cropped item, not "off"). Tables, sampling byte, restart interval (-1: the source's number
 *     of MCUs) and the coding limits in the target's prediction order are as without a crop -- the left edge of a crop is
 *     predicted from the right edge of its row above; header, bound and scratch size are the encoder's arithmetic on
 *     width x height. Where the rectangle starts on an iMCU boundary and each extent is a multiple of the iMCU or reaches
 *     the image's edge, the file of a source Pillow wrote is the file Pillow writes for the cropped pixels; an extent that
 *     ends inside the image keeps the source's real samples beyond it in its last blocks (Pillow would replicate the edge).
 *     A call with such an item launches the mapped instantiation of the gather kernel, also at orientation 1.
 *     With a transcode crop the decoder may carry a decode window (jpeggpu_ext_set_crop), so that only the restart segments
 *     that hold the window are transferred and entropy-decoded (a single scan with restart markers; any other file is
 *     decoded whole, a progressive one into whole coefficient arrays, and transcodes all the same): the window's frame MCUs
 *     must hold every source block the target reads, the DC sources of its dummy blocks included, else
 *     JPEGGPU_NOT_SUPPORTED. A rectangle of pixels that covers the source pixels of the target does (the window adds a
 *     sample of halo). A decode window WITHOUT a transcode crop, a scale and a segment shard stay JPEGGPU_NOT_SUPPORTED.
 *   - jpeggpu_ext_set_transcode_frame(decoder, mode): which frame layout the new file has. Read by the four
 *     jpeggpu_ext_transcode_ calls only, when they are called, and held until it is set again, like the orientation and the
 *     crop. A value other than the two below: JPEGGPU_INVALID_ARGUMENT, and the setting stays as it was.
 *       JPEGGPU_EXT_TRANSCODE_FRAME_ENCODER (0, the default): the layout the pixel encoder writes, and every refusal above.
 *       JPEGGPU_EXT_TRANSCODE_FRAME_SOURCE (1): the new file keeps the SOURCE's frame layout, as the file libjpeg writes
 *         after jpeg_copy_critical_parameters (jpegtran). Accepted: every file the parser accepts with one to four
 *         components -- any sampling factors (at most 10 blocks per MCU), up to four quantisation tables with 8- or 16-bit
 *         entries, every colour model jpeggpu_ext_get_color_space tells apart and two components; baseline, multi-scan and
 *         progressive sources. A scale, a segment shard, a decode window without a transcode crop, the encoder's size
 *         limits and the coding limits are refused as in the other mode. A file the other mode accepts gives the same
 *         bytes with every option (so such a file's tables are numbered 0 and 1 as there, whatever the source calls them).
 *         The file written, for every other source:
 *           - colour space: the source's. Component ids 1, 2, 3 (YCbCr), 'R' 'G' 'B', 'C' 'M' 'Y' 'K', 1..4 (YCCK), 0..n-1
 *             (unknown); APP0 for YCbCr only, in the other mode's bytes; an Adobe APP14 segment (version 100, flags 0,
 *             transform 0 / 0 / 2) for RGB, CMYK and YCCK; Huffman tables 1 for components 1 and 2 of YCbCr and YCCK,
 *             tables 0 for everything else (jpeg_set_colorspace);
 *           - each component keeps its sampling factors and its quantisation-table number: one DQT segment per table a
 *             component names, in component order, Pq = 1 for a table with an entry above 255, and then SOF1 for SOF0;
 *           - without `optimize` the Annex K tables the selectors name (DC 0 and AC 0 alone where no component selects
 *             tables 1); with `optimize` one optimised table per class and selector in use;
 *           - a dummy block (a block of an MCU beyond its component's real grid, in any component whose factors exceed 1)
 *             of an item without orientation and crop keeps the source's values where a scan of the source codes it and
 *             is zero where none does; of a mapped item it is the encoder's: 63 zeros and the DC of the block in front of
 *             it among its component's blocks of the MCU;
 *           - orientations 5..8 exchange the factors of EVERY component (4:2:2 becomes 4:4:0). The edge, trim and crop-origin
 *             rules use the iMCU of the target, 8 h_max x 8 v_max, in place of luma's factors; 4:2:2 takes every orientation.
 *           - `progressive`: SOF2. Three-component YCbCr keeps the ten scans of the other mode; every other case gets
 *             jpeg_simple_progression's all-purpose script of 2 + 4 n scans: the DC of all components interleaved (Al 1); per
 *             component AC 1-5 (Al 2), then AC 6-63 (Al 2), then AC 1-63 (Ah 2, Al 1); the DC refinement; per component
 *             AC 1-63 (Ah 1, Al 0). A component's own scan runs over its real blocks; the first scan brings the DC tables
 *             its components select, every AC scan one table under its component's selector. */
struct jpeggpu_ext_transcode_item {
    jpeggpu_decoder_t decoder;
    void* d_tmp;
    int progressive, optimize;
    int restart_interval;
    uint8_t* out;
    size_t capacity;
};
enum jpeggpu_status jpeggpu_ext_transcode_header(const struct jpeggpu_ext_transcode_item* item, uint8_t* host_buf, size_t* size);
size_t jpeggpu_ext_transcode_bound(const struct jpeggpu_ext_transcode_item* item);
size_t jpeggpu_ext_transcode_scratch_size(const struct jpeggpu_ext_transcode_item* items, int n);
enum jpeggpu_status jpeggpu_ext_transcode_batch(
    const struct jpeggpu_ext_transcode_item* items,
    int n,
    void* d_scratch,
    size_t scratch_size,
    size_t* d_sizes,
    int* d_status,
    jpeggpu_stream_t stream);
enum jpeggpu_status jpeggpu_ext_batch_set_coefficients_only(jpeggpu_batch_t batch, int enable);
enum jpeggpu_status jpeggpu_ext_set_transcode_orientation(jpeggpu_decoder_t decoder, int orientation, int trim);
enum jpeggpu_status jpeggpu_ext_set_transcode_crop(jpeggpu_decoder_t decoder, int x, int y, int width, int height);
enum jpeggpu_ext_transcode_frame {
    JPEGGPU_EXT_TRANSCODE_FRAME_ENCODER = 0,
    JPEGGPU_EXT_TRANSCODE_FRAME_SOURCE  = 1
};
enum jpeggpu_status jpeggpu_ext_set_transcode_frame(jpeggpu_decoder_t decoder, int mode);

/* JPEG round trip (JPEG compression as an augmentation or degradation: torchvision.transforms.v2.JPEG, albumentations'
 * ImageCompression, DALI's jpeg_compression_distortion): the pixels an image has after it was saved as a baseline JPEG of
 * quality q and opened again, on the device, without the file. For an H x W (grey) or H x W x 3 (RGB) uint8 array `a` the
 * result is, byte for byte (tests/golden/roundtrip_pins.npz),
 *     buf = BytesIO(); Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling=s); np.asarray(Image.open(buf))
 * of Pillow on libjpeg-turbo. Entropy coding is lossless, so none is done: one launch takes every block of the call from
 * pixels through jpeggpu_ext_encode_batch's first stage (jccolor.c, jcsample.c, jpeg_fdct_islow, the quantiser with
 * jpeg_set_quality's tables) and, on the quantised values still in registers, the decoder's ISLOW transform (dequantisation,
 * jpeg_idct_islow, the range limit); a second launch, jpeggpu_ext_batch_to_rgb's, makes RGB of the component planes (fancy
 * upsampling, YCbCr -> RGB). Optimised or progressive coding and restart intervals change no pixel and have no field here.
 * The range limit is jidctint.c's table lookup, as in the decoder: a sample that overshoots the 8-bit range by more than 384
 * wraps, where libjpeg-turbo's SIMD IDCT saturates. No input gets there with quantisers up to 100, and none of the pinned
 * ones at any quality; tests/roundtrip_ref.py holds a block built to (WRAP_BLOCK, quality 1).
 *   - An item: `data`, `width`, `height`, `channels` (1 or 3), the three strides, `quality` 1..100 and `subsampling` as in
 *     jpeggpu_ext_encode_item (`subsampling` is not read for a grey item). `dst`, `dst_pitch` and `plane_stride` as in
 *     jpeggpu_ext_rgb_item with `layout`: an RGB item's R, G, B of pixel (x, y) at dst + y * dst_pitch + 3 x (HWC) or channel c
 *     at dst + c * plane_stride + y * dst_pitch + x (CHW); a grey item's sample at dst + y * dst_pitch + x whatever the
 *     layout, dst_pitch >= width, plane_stride not read. No alignment is asked of any pointer or pitch.
 *   - `dst` may be the very view `data` describes (same pointer, same strides): an RGB item's source is read completely by
 *     the first launch before the second writes, and a grey block is read only by the lane that then stores it. Any other
 *     overlap of an output with an input or another output is the caller's error and is not checked.
 *   - A call may mix grey and RGB items, sizes, qualities and subsamplings. With an RGB item it is TWO launches whatever n
 *     is, of grey items only ONE; one copy of descriptors through the page-locked staging ring of the resize calls (of four:
 *     the fifth call in a row waits until the copy of the first has executed), and nothing synchronises. The host may reuse
 *     `items` as soon as the call returns.
 *   - `d_scratch`: caller-owned device memory of at least jpeggpu_ext_roundtrip_scratch_size(items, n) bytes (host only; 0
 *     for items the call would refuse for their geometry, never smaller for a longer list), private to the stream until the
 *     call has executed: the descriptors and, per RGB item, its three component planes padded to whole blocks.
 *   - JPEGGPU_INVALID_ARGUMENT, before anything is enqueued and without touching the device: NULL items, d_scratch, data or
 *     dst, n <= 0 or > 65535, width or height outside 1..65535, channels other than 1 or 3, quality outside 1..100, an
 *     unknown subsampling (RGB items) or layout, a dst_pitch or plane_stride too small, scratch_size too small.
 *     JPEGGPU_NOT_SUPPORTED: a call of 2^31 blocks. On an error nothing is written. */
struct jpeggpu_ext_roundtrip_item {
    const uint8_t* data;
    int width, height;
    int channels;    /* 1 or 3 */
    int64_t row_pitch, pixel_stride, channel_stride; /* bytes, as jpeggpu_ext_encode_item */
    int quality;     /* 1..100 */
    int subsampling; /* enum jpeggpu_ext_subsampling; not read for grey */
    uint8_t* dst;
    int dst_pitch;
    size_t plane_stride; /* RGB items of JPEGGPU_EXT_CHW only */
};
size_t jpeggpu_ext_roundtrip_scratch_size(const struct jpeggpu_ext_roundtrip_item* items, int n);
enum jpeggpu_status jpeggpu_ext_roundtrip_batch(
    const struct jpeggpu_ext_roundtrip_item* items,
    int n,
    enum jpeggpu_ext_image_layout layout,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);

/* DCT-domain access: libjpeg's jpeg_read_coefficients and jpeg_write_coefficients (what jpegio.read,
 * torchjpeg.codec.read_coefficients / write_coefficients and jpeglib wrap on the CPU), batched and on the device.
 *
 * READING. A component's coefficients are a tensor [blocks_y][blocks_x][64] over its REAL block grid -- libjpeg's
 * width_in_blocks x height_in_blocks, blocks_x = ceil(ceil(width * h_c / h_max) / 8) and likewise for y (one component: h_c /
 * h_max is 1 whatever its frame header says), not the MCU-padded grid -- with natural order inside a block (8 v + u), so
 * that it views as [by][bx][8][8]. The DC is absolute.
 *   - jpeggpu_ext_get_coefficient_info (host only; after jpeggpu_decoder_parse_header, else JPEGGPU_INVALID_ARGUMENT): the
 *     frame's size and component count, its colour model (jpeggpu_ext_get_color_space) and whether it is progressive; per
 *     component the grid, the sampling factors of the frame header, the quantisation table in natural order and whether
 *     one of its entries is above 255. Entries of components the frame does not have are zero.
 *   - jpeggpu_ext_read_coefficients_batch: an item is a decoder, its d_tmp and one destination per component, with a
 *     transcode item's precondition: parsed, transferred and decoded by jpeggpu_ext_decode_batch on the same stream, with
 *     jpeggpu_ext_batch_set_coefficients_only or without; d_tmp is read when the call executes. dst[c]: caller-owned device
 *     memory of blocks_y * blocks_x * 64 elements, aligned to 16 bytes; entries beyond the component count are not read.
 *     Every file the decoder reads: baseline (interleaved scans, and a component's own scan, whose units are its real
 *     blocks) and progressive (out of the padded coefficient array, its rows cut to the real grid), 1..4 components, any
 *     sampling, 8- and 16-bit tables, restart markers, device scan or not. A real block that no scan codes is 64 zeros.
 *   - spec->type: JPEGGPU_EXT_COEF_I16 gives the quantised values exactly. JPEGGPU_EXT_COEF_F32 / _F16 give float(value),
 *     and with spec->dequantize = 1 that times float(table entry): ONE IEEE-754 binary32 multiply, rounded to nearest even,
 *     and for _F16 then one conversion, rounded to nearest even -- never arithmetic in half precision (as
 *     jpeggpu_ext_resize_to_tensor converts). Dequantised _I16 is JPEGGPU_INVALID_ARGUMENT: a 16-bit table overflows it.
 *   - One copy of descriptors (the encoder's page-locked staging ring), ONE launch whatever the call holds -- a workgroup
 *     owns 256 consecutive blocks of one component's raster, so its stores are whole 128-byte lines of one tensor -- and
 *     nothing synchronises. The host may reuse `items` as soon as the call returns.
 *   - d_scratch: caller-owned, at least jpeggpu_ext_read_coefficients_scratch_size(n) bytes (host only, never smaller for
 *     a larger n; 0 for n <= 0 or n > 65535), private to the stream until the call has executed.
 *   - JPEGGPU_INVALID_ARGUMENT, before anything is enqueued: NULL items, spec or d_scratch, n <= 0 or > 65535, a NULL or
 *     unparsed decoder, a d_tmp that is NULL or not aligned to 256 bytes, a dst[c] that is NULL or not aligned to 16 bytes, an
 *     unknown type, a dequantize other than 0 or 1, a scratch too small. JPEGGPU_NOT_SUPPORTED, as a transcode refuses them:
 *     a decoder with a scale other than 1 or a segment shard, and one with a decode window (jpeggpu_ext_set_crop) --
 *     windowed reading is not offered --, and a call of 2^31 blocks. On an error nothing is written.
 *
 * WRITING. An item describes a frame and names one int16 tensor per component, laid out as above over the REAL grids:
 * `width`, `height`, `components` 1..4, sampling factors h[c], v[c] in 1..4 (of a single component they go into the frame
 * header as they are and change nothing else), qtable[c]: the component's table in natural order, entries 1..65535,
 * `color_space` (enum jpeggpu_ext_color_space; GRAY 1 component, YCBCR and RGB 3, CMYK and YCCK 4, UNKNOWN any count),
 * coef[c]: contiguous device memory aligned to 16 bytes, read when the call executes; `progressive`, `optimize`,
 * `restart_interval` 0..65535 (MCUs), `out`, `capacity` as in jpeggpu_ext_encode_item. Everything behind the first launch
 * is jpeggpu_ext_transcode_batch: the item is a transcode item whose source is the caller's tensors.
 *   - The file. A layout the pixel encoder writes -- one component, or YCbCr with chroma 1 x 1, luma 1 x 1, 2 x 1 or 2 x 2,
 *     equal tables for Cb and Cr and no entry above 255 -- gets the encoder's header (tables 0 and 1, APP0), and is then byte
 *     for byte what jpeggpu_ext_transcode_batch makes of a source with these coefficients. Everything else gets the header
 *     of jpeggpu_ext_set_transcode_frame(SOURCE) by the rules stated there (ids and APP0 / APP14 by the colour model,
 *     Huffman tables 1 for components 1 and 2 of YCbCr and YCCK, SOF1 where a table has an entry above 255, the all-purpose
 *     progressive script), with the quantisation tables numbered by first appearance: components whose tables are equal
 *     share one DQT segment.
 *   - Dummy blocks (blocks of an MCU beyond a component's real grid) are not in the tensors. They are the encoder's
 *     (jctrans.c): AC zero and the DC of the block in front of them among the component's blocks of the MCU.
 *   - d_status as jpeggpu_ext_transcode_batch: JPEGGPU_EXT_ENCODE_UNCODABLE for an item alone that holds an AC coefficient
 *     of magnitude 1024 or more, or a DC difference of 2048 or more in the file's prediction order (per component, from 0
 *     at every restart): its size is 0 and its slot is not written; the other items are not touched by it.
 *   - The launches are those of jpeggpu_ext_transcode_batch for the same mix of output kinds (its mapped gather first), one
 *     copy of descriptors, nothing synchronises. d_scratch: jpeggpu_ext_write_coefficients_scratch_size(items, n) (host
 *     only; 0 for items the call refuses; never smaller for a longer list).
 *   - jpeggpu_ext_write_coefficients_header / _bound (host only; `coef`, `out` and `capacity` are not read): as
 *     jpeggpu_ext_encode_header / jpeggpu_ext_encode_bound serve the pixel encoder.
 *   - JPEGGPU_INVALID_ARGUMENT, before anything is enqueued: width or height outside 1..65535, components outside 1..4, a
 *     factor outside 1..4, an MCU of more than 10 blocks, a table entry of 0, a colour model that does not fit the component
 *     count, a coef[c] that is NULL or not aligned to 16 bytes (the batch call), options out of range, `out` NULL with a
 *     capacity. (A grid that does not fit the frame cannot be expressed: the grids follow from the frame. The Python
 *     wrapper checks each tensor's shape against them.) JPEGGPU_NOT_SUPPORTED: the encoder's size limits. */
struct jpeggpu_ext_coefficient_info {
    int width, height, num_components;
    int color_space; /* enum jpeggpu_ext_color_space */
    int progressive;
    int blocks_x[JPEGGPU_MAX_COMP], blocks_y[JPEGGPU_MAX_COMP];
    int h[JPEGGPU_MAX_COMP], v[JPEGGPU_MAX_COMP];
    int table16[JPEGGPU_MAX_COMP];         /* the component's table has an entry above 255 */
    uint16_t qtable[JPEGGPU_MAX_COMP][64]; /* natural order */
};
enum jpeggpu_status jpeggpu_ext_get_coefficient_info(jpeggpu_decoder_t decoder, struct jpeggpu_ext_coefficient_info* info);
enum jpeggpu_ext_coefficient_type { JPEGGPU_EXT_COEF_I16 = 0, JPEGGPU_EXT_COEF_F32 = 1, JPEGGPU_EXT_COEF_F16 = 2 };
struct jpeggpu_ext_coefficient_spec {
    enum jpeggpu_ext_coefficient_type type;
    int dequantize; /* float types only */
};
struct jpeggpu_ext_coefficient_read_item {
    jpeggpu_decoder_t decoder;
    void* d_tmp;
    void* dst[JPEGGPU_MAX_COMP];
};
size_t jpeggpu_ext_read_coefficients_scratch_size(int n);
enum jpeggpu_status jpeggpu_ext_read_coefficients_batch(
    const struct jpeggpu_ext_coefficient_read_item* items,
    int n,
    const struct jpeggpu_ext_coefficient_spec* spec,
    void* d_scratch,
    size_t scratch_size,
    jpeggpu_stream_t stream);
struct jpeggpu_ext_coefficient_item {
    int width, height, components;
    int h[JPEGGPU_MAX_COMP], v[JPEGGPU_MAX_COMP];
    uint16_t qtable[JPEGGPU_MAX_COMP][64]; /* natural order, entries 1..65535 */
    int color_space;                       /* enum jpeggpu_ext_color_space */
    const int16_t* coef[JPEGGPU_MAX_COMP];
    int progressive, optimize;
    int restart_interval;
    uint8_t* out;
    size_t capacity;
};
enum jpeggpu_status jpeggpu_ext_write_coefficients_header(const struct jpeggpu_ext_coefficient_item* item, uint8_t* host_buf, size_t* size);
size_t jpeggpu_ext_write_coefficients_bound(const struct jpeggpu_ext_coefficient_item* item);
size_t jpeggpu_ext_write_coefficients_scratch_size(const struct jpeggpu_ext_coefficient_item* items, int n);
enum jpeggpu_status jpeggpu_ext_write_coefficients_batch(
    const struct jpeggpu_ext_coefficient_item* items,
    int n,
    void* d_scratch,
    size_t scratch_size,
    size_t* d_sizes,
    int* d_status,
    jpeggpu_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* JPEGGPU_JPEGGPU_EXT_H_ */
