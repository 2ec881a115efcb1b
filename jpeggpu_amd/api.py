"""ctypes mirror of include/jpeggpu/jpeggpu.h (+ jpeggpu_ext.h).

Call order is the reference's (example/example_tool.c:101-128):
    startup -> parse_header -> get_buffer_size -> transfer(d_tmp) -> decode(d_tmp) -> cleanup.
Device memory and streams are the caller's: pass raw device pointers (e.g. torch tensors'
data_ptr()) and a hipStream_t handle (torch.cuda.Stream.cuda_stream). There is no CPU fallback: if
the HIP library is missing, importing the binding fails.
"""
import ctypes as C
import enum
import os

from . import build as _build

MAX_COMP = 4
STAGES = ("front", "destuff", "sync_intra", "sync_inter", "tails", "write", "idct")
IDCT_METHODS = {"reference": 0, "islow": 1}  # enum jpeggpu_ext_idct
FILTERS = {"bilinear": 0, "bicubic": 1}  # enum jpeggpu_ext_filter
LAYOUTS = {"NHWC": 0, "NCHW": 1}  # enum jpeggpu_ext_output_layout
IMAGE_LAYOUTS = {"HWC": 0, "CHW": 1}  # enum jpeggpu_ext_image_layout
SCALE_MODES = {"uniform": 0, "libjpeg": 1}  # enum jpeggpu_ext_scale_mode
SUBSAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}  # enum jpeggpu_ext_subsampling (Pillow's numbers)
TENSOR_TYPE_NAMES = {"uint8": 0, "float32": 1, "float16": 2, "bfloat16": 3}  # enum jpeggpu_ext_tensor_type, by torch dtype name


def _tensor_types():
    import torch

    return {getattr(torch, name): v for name, v in TENSOR_TYPE_NAMES.items()}


class _TensorTypes(dict):
    """TENSOR_TYPES: torch dtype -> enum jpeggpu_ext_tensor_type. Filled at first use, so importing the binding does not
    import torch."""

    def _fill(self):
        if not len(self):
            self.update(_tensor_types())
        return self

    def __getitem__(self, k):
        return dict.__getitem__(self._fill(), k)

    def __contains__(self, k):
        return dict.__contains__(self._fill(), k)

    def __iter__(self):
        return dict.__iter__(self._fill())


TENSOR_TYPES = _TensorTypes()


class ColorSpace(enum.IntEnum):
    """enum jpeggpu_ext_color_space: what libjpeg and Pillow take a file's components for (Decoder.color_space)."""
    UNKNOWN = 0
    GRAY = 1
    YCBCR = 2
    RGB = 3
    CMYK = 4
    YCCK = 5


class Status(enum.IntEnum):
    SUCCESS = 0
    INVALID_ARGUMENT = 1
    INVALID_JPEG = 2
    INTERNAL_ERROR = 3
    NOT_SUPPORTED = 4
    OUT_OF_HOST_MEMORY = 5
    INCOMPLETE_BITSTREAM = 6


class Subsampling(C.Structure):
    _fields_ = [("x", C.c_int * MAX_COMP), ("y", C.c_int * MAX_COMP)]


class ImgInfo(C.Structure):
    _fields_ = [("sizes_x", C.c_int * MAX_COMP), ("sizes_y", C.c_int * MAX_COMP),
                ("num_components", C.c_int), ("subsampling", Subsampling)]


class Img(C.Structure):
    _fields_ = [("image", C.c_void_p * MAX_COMP), ("pitch", C.c_int * MAX_COMP)]


class CropInfo(C.Structure):
    """struct jpeggpu_ext_crop_info: the rectangle, each component's window origin in its full plane, the full plane sizes
    (all at the decoder's scale)."""
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("origin_x", C.c_int * MAX_COMP), ("origin_y", C.c_int * MAX_COMP),
                ("full_x", C.c_int * MAX_COMP), ("full_y", C.c_int * MAX_COMP)]


class ScaleInfo(C.Structure):
    """struct jpeggpu_ext_scale_info: the scale and mode of the parsed image, each component's block size, and whether
    libjpeg upsamples what subsampling is left with its fancy upsamplers (0: it replicates -- the libjpeg mode at 1/8)."""
    _fields_ = [("scale_denom", C.c_int), ("mode", C.c_int), ("block_size", C.c_int * MAX_COMP), ("fancy_upsampling", C.c_int)]


class ProgressiveInfo(C.Structure):
    """struct jpeggpu_ext_progressive_info: whether the last parsed image is a progressive frame, its scans and levels, and
    each component's coefficient buffer in d_tmp: int16 [blocks_y, blocks_x, 64] over the MCU-padded grid, of which the
    IDCT stage is handed the visible blocks."""
    _fields_ = [("progressive", C.c_int), ("num_scans", C.c_int), ("num_levels", C.c_int),
                ("off_coefficients", C.c_size_t * MAX_COMP), ("blocks_x", C.c_int * MAX_COMP), ("blocks_y", C.c_int * MAX_COMP),
                ("visible_blocks_x", C.c_int * MAX_COMP), ("visible_blocks_y", C.c_int * MAX_COMP)]


class TruncatedInfo(C.Structure):
    """struct jpeggpu_ext_truncated_info: whether the last parsed file ended without its EOI, the scan it ends in (-1: behind
    a whole scan), that scan's bytes that are present, and the first restart interval without data (-1: none)."""
    _fields_ = [("truncated", C.c_int), ("scan", C.c_int), ("scan_bytes", C.c_size_t), ("first_missing_interval", C.c_int)]


class ResizeItem(C.Structure):
    """struct jpeggpu_ext_resize_item: a decoded image's info and planes, and its crop (NULL: the whole image)."""
    _fields_ = [("info", C.POINTER(ImgInfo)), ("crop", C.POINTER(CropInfo)), ("src", C.POINTER(Img))]


class TensorSpec(C.Structure):
    """struct jpeggpu_ext_tensor_spec: the element type of jpeggpu_ext_resize_to_tensor's output, Normalize's mean and std
    per channel (float types only) and the items to flip left to right (host bytes, one per item; NULL: none)."""
    _fields_ = [("type", C.c_int), ("mean", C.c_float * 3), ("std", C.c_float * 3), ("flips", C.POINTER(C.c_ubyte))]


class ResizeView(C.Structure):
    """struct jpeggpu_ext_resize_view: the size an item's WHOLE displayed image is resized to, the window's corner in that
    resized image (negative: zero padding), and whether libjpeg replicates the item's chroma."""
    _fields_ = [("resized_w", C.c_int), ("resized_h", C.c_int), ("x", C.c_int), ("y", C.c_int), ("replicate", C.c_int)]


class Thumbnail(C.Structure):
    """struct jpeggpu_ext_thumbnail: what Pillow's Image.thumbnail does to one file (thumbnail_plan)."""
    _fields_ = [("scale", C.c_int), ("dec_w", C.c_int), ("dec_h", C.c_int), ("fx", C.c_int), ("fy", C.c_int), ("red_w", C.c_int),
                ("red_h", C.c_int), ("box_w", C.c_float), ("box_h", C.c_float), ("out_w", C.c_int), ("out_h", C.c_int), ("identity", C.c_int),
                ("replicate", C.c_int)]

    def astuple(self):
        """(scale, dec_w, dec_h, fx, fy, red_w, red_h, box_w, box_h, out_w, out_h, identity)"""
        return (self.scale, self.dec_w, self.dec_h, self.fx, self.fy, self.red_w, self.red_h, self.box_w, self.box_h, self.out_w, self.out_h,
                self.identity)


class RgbItem(C.Structure):
    """struct jpeggpu_ext_rgb_item: a decoded image's info, crop (NULL: the whole image) and planes, its colour model, EXIF
    orientation and whether libjpeg replicates its chroma, and where its displayed RGB goes."""
    _fields_ = [("info", C.POINTER(ImgInfo)), ("crop", C.POINTER(CropInfo)), ("src", C.POINTER(Img)),
                ("color", C.c_int), ("orientation", C.c_int), ("replicate", C.c_int),
                ("dst", C.c_void_p), ("dst_pitch", C.c_int), ("plane_stride", C.c_size_t)]


class EncodeItem(C.Structure):
    """struct jpeggpu_ext_encode_item (`progressive` lies where LP64 had padding behind `channels`)"""
    _fields_ = [("data", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int), ("progressive", C.c_int), ("row_pitch", C.c_int64),
                ("pixel_stride", C.c_int64), ("channel_stride", C.c_int64), ("quality", C.c_int), ("subsampling", C.c_int),
                ("restart_interval", C.c_int), ("optimize", C.c_int), ("out", C.c_void_p), ("capacity", C.c_size_t)]


class EncodeFitItem(C.Structure):
    """struct jpeggpu_ext_encode_fit_item"""
    _fields_ = [("item", EncodeItem), ("max_bytes", C.c_size_t), ("quality_min", C.c_int), ("quality_max", C.c_int)]


class EncodeStatus(enum.IntEnum):
    """enum jpeggpu_ext_encode_status: what the encoder's calls leave per item in their status tensor."""
    OK = 0
    TOO_SMALL = 1
    TABLE_OVERFLOW = 2
    EMPTY_TABLE = 3
    UNCODABLE = 4
    OVER_BUDGET = 5


class RoundtripItem(C.Structure):
    """struct jpeggpu_ext_roundtrip_item"""
    _fields_ = [("data", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int), ("row_pitch", C.c_int64),
                ("pixel_stride", C.c_int64), ("channel_stride", C.c_int64), ("quality", C.c_int), ("subsampling", C.c_int),
                ("dst", C.c_void_p), ("dst_pitch", C.c_int), ("plane_stride", C.c_size_t)]


class TranscodeItem(C.Structure):
    """struct jpeggpu_ext_transcode_item"""
    _fields_ = [("decoder", C.c_void_p), ("d_tmp", C.c_void_p), ("progressive", C.c_int), ("optimize", C.c_int), ("restart_interval", C.c_int),
                ("out", C.c_void_p), ("capacity", C.c_size_t)]


class CoefficientInfo(C.Structure):
    """struct jpeggpu_ext_coefficient_info"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("num_components", C.c_int), ("color_space", C.c_int), ("progressive", C.c_int),
                ("blocks_x", C.c_int * MAX_COMP), ("blocks_y", C.c_int * MAX_COMP), ("h", C.c_int * MAX_COMP), ("v", C.c_int * MAX_COMP),
                ("table16", C.c_int * MAX_COMP), ("qtable", (C.c_uint16 * 64) * MAX_COMP)]


class CoefficientSpec(C.Structure):
    """struct jpeggpu_ext_coefficient_spec"""
    _fields_ = [("type", C.c_int), ("dequantize", C.c_int)]


class CoefficientReadItem(C.Structure):
    """struct jpeggpu_ext_coefficient_read_item"""
    _fields_ = [("decoder", C.c_void_p), ("d_tmp", C.c_void_p), ("dst", C.c_void_p * MAX_COMP)]


class CoefficientItem(C.Structure):
    """struct jpeggpu_ext_coefficient_item"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("components", C.c_int), ("h", C.c_int * MAX_COMP), ("v", C.c_int * MAX_COMP),
                ("qtable", (C.c_uint16 * 64) * MAX_COMP), ("color_space", C.c_int), ("coef", C.c_void_p * MAX_COMP),
                ("progressive", C.c_int), ("optimize", C.c_int), ("restart_interval", C.c_int), ("out", C.c_void_p), ("capacity", C.c_size_t)]


class ExtScanLayout(C.Structure):
    _fields_ = [
        ("num_components", C.c_int), ("component_idx", C.c_int * MAX_COMP),
        ("num_subsequences", C.c_int), ("num_segments", C.c_int), ("num_sequences", C.c_int),
        ("num_data_units", C.c_int), ("data_units_per_mcu", C.c_int), ("num_chunks", C.c_int),
        ("off_segments", C.c_size_t), ("off_chunks", C.c_size_t), ("off_destuffed", C.c_size_t),
        ("off_segment_index", C.c_size_t), ("off_state_p", C.c_size_t), ("off_state_n", C.c_size_t),
        ("off_state_cz", C.c_size_t), ("off_state_dc01", C.c_size_t), ("off_state_dc23", C.c_size_t),
        ("off_symbols", C.c_size_t), ("off_du_table", C.c_size_t), ("symbol_region_entries", C.c_int),
        ("device_scan", C.c_int), ("off_device_status", C.c_size_t),
        ("hypotheses", C.c_int), ("hypothesis_blocks", C.c_int),
    ]


class ExtLayout(C.Structure):
    _fields_ = [
        ("subsequence_bytes", C.c_int), ("subsequences_per_sequence", C.c_int), ("num_scans", C.c_int),
        ("transferred_bytes", C.c_size_t), ("blob_bytes", C.c_size_t),
        ("off_bytes", C.c_size_t), ("off_qtables", C.c_size_t),
        ("scans", ExtScanLayout * MAX_COMP),
        ("shard_rank", C.c_int), ("shard_world", C.c_int),
    ]


class ParseItem(C.Structure):
    _fields_ = [("decoder", C.c_void_p), ("img_info", C.POINTER(ImgInfo)), ("data", C.c_void_p), ("size", C.c_size_t)]


class BatchItem(C.Structure):
    _fields_ = [("decoder", C.c_void_p), ("img", C.POINTER(Img)), ("d_tmp", C.c_void_p), ("tmp_size", C.c_size_t)]


class JpegGpuError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = Status(status)
        super().__init__("%s: %s" % (where, status_string(status)))


_lib = None


def lib():
    """Load the C-ABI library (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64 (SONAME libamdhip64.so.7, loaded via RPATH under the file name
    # libamdhip64.so). Import it first so our NEEDED libamdhip64.so.7 resolves to that same runtime:
    # two HIP runtimes in one process do not know each other's allocations and streams.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = os.environ.get("JPEGGPU_LIB", _build.LIB_PATH)  # override: A/B runs of experimental builds
    if not os.path.exists(path):
        raise ImportError(
            "jpeggpu_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    L = C.CDLL(path)
    dec = C.c_void_p
    L.jpeggpu_get_status_string.restype = C.c_char_p
    L.jpeggpu_get_status_string.argtypes = [C.c_int]
    L.jpeggpu_decoder_startup.argtypes = [C.POINTER(dec)]
    L.jpeggpu_set_logging.argtypes = [dec, C.c_int]
    L.is_css_444.argtypes = [Subsampling, C.c_int]
    L.jpeggpu_decoder_parse_header.argtypes = [dec, C.POINTER(ImgInfo), C.c_void_p, C.c_size_t]
    L.jpeggpu_decoder_get_buffer_size.argtypes = [dec, C.POINTER(C.c_size_t)]
    L.jpeggpu_decoder_transfer.argtypes = [dec, C.c_void_p, C.c_size_t, C.c_void_p]
    L.jpeggpu_decoder_decode.argtypes = [dec, C.POINTER(Img), C.c_void_p, C.c_size_t, C.c_void_p]
    L.jpeggpu_decoder_cleanup.argtypes = [dec]
    L.jpeggpu_ext_set_subsequence_bytes.argtypes = [dec, C.c_int]
    L.jpeggpu_ext_set_batched.argtypes = [dec, C.c_int]
    L.jpeggpu_ext_set_batch_hint.argtypes = [dec, C.c_int]
    L.jpeggpu_ext_get_layout.argtypes = [dec, C.POINTER(ExtLayout)]
    L.jpeggpu_ext_set_profiling.argtypes = [dec, C.c_int]
    L.jpeggpu_ext_get_stage_ms.argtypes = [dec, C.POINTER(C.c_float)]
    L.jpeggpu_ext_batch_scratch_size.restype = C.c_size_t
    L.jpeggpu_ext_batch_scratch_size.argtypes = [C.c_int]
    L.jpeggpu_ext_batch_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.jpeggpu_ext_decode_batch.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.jpeggpu_ext_batch_destroy.argtypes = [C.c_void_p]
    L.jpeggpu_ext_batch_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.jpeggpu_ext_batch_set_sync_iterations.argtypes = [C.c_void_p, C.c_int]
    L.jpeggpu_ext_batch_set_overlap.argtypes = [C.c_void_p, C.c_int]
    for name, args in (("jpeggpu_ext_batch_set_fused_tail", [C.c_void_p, C.c_int]), ("jpeggpu_ext_batch_set_sync_run", [C.c_void_p, C.c_int]),
                       ("jpeggpu_ext_fused_tail_timeouts", [C.POINTER(C.c_uint)])):
        if hasattr(L, name):  # (a library loaded through JPEGGPU_LIB may be older than this file: _newer_symbol)
            getattr(L, name).argtypes = args
    L.jpeggpu_ext_batch_get_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.jpeggpu_ext_upsample_planes.argtypes = [
        C.POINTER(ImgInfo), C.POINTER(Img), C.POINTER(Img), C.c_int, C.c_int, C.c_void_p]
    L.jpeggpu_ext_set_segment_shard.argtypes = [dec, C.c_int, C.c_int]
    L.jpeggpu_ext_get_shard_rows.argtypes = [dec, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.jpeggpu_ext_self_test.argtypes = [C.c_void_p]
    L.jpeggpu_ext_set_device_scan.argtypes = [dec, C.c_int]
    L.jpeggpu_ext_set_scale.argtypes = [dec, C.c_int]
    L.jpeggpu_ext_set_idct.argtypes = [dec, C.c_int]
    L.jpeggpu_ext_set_scale_mode.argtypes = [dec, C.c_int]
    L.jpeggpu_ext_get_scale_info.argtypes = [dec, C.POINTER(ScaleInfo)]
    L.jpeggpu_ext_get_device_status.argtypes = [dec, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.jpeggpu_ext_parse_headers.argtypes = [C.POINTER(ParseItem), C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.jpeggpu_ext_planes_to_rgbi.argtypes = [
        C.POINTER(ImgInfo), C.POINTER(Img), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.jpeggpu_ext_planes_to_rgbi_fancy.argtypes = [
        C.POINTER(ImgInfo), C.POINTER(Img), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.jpeggpu_ext_planes_to_rgbi_replicate.argtypes = L.jpeggpu_ext_planes_to_rgbi_fancy.argtypes
    L.jpeggpu_ext_set_crop.argtypes = [dec, C.c_int, C.c_int, C.c_int, C.c_int]
    L.jpeggpu_ext_get_crop.argtypes = [dec, C.POINTER(CropInfo)]
    L.jpeggpu_ext_crop_to_rgbi_fancy.argtypes = [
        C.POINTER(ImgInfo), C.POINTER(CropInfo), C.POINTER(Img), C.c_void_p, C.c_int, C.c_void_p]
    L.jpeggpu_ext_crop_to_rgbi_replicate.argtypes = L.jpeggpu_ext_crop_to_rgbi_fancy.argtypes
    L.jpeggpu_ext_resize_scratch_size.restype = C.c_size_t
    L.jpeggpu_ext_resize_scratch_size.argtypes = [C.POINTER(ResizeItem), C.c_int, C.c_int, C.c_int, C.c_int]
    L.jpeggpu_ext_resize_to_rgb.argtypes = [
        C.POINTER(ResizeItem), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.jpeggpu_ext_get_color_space.argtypes = [dec, C.POINTER(C.c_int)]
    L.jpeggpu_ext_planes_to_rgbi_fancy_cs.argtypes = [
        C.POINTER(ImgInfo), C.c_int, C.POINTER(Img), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.jpeggpu_ext_planes_to_rgbi_replicate_cs.argtypes = L.jpeggpu_ext_planes_to_rgbi_fancy_cs.argtypes
    L.jpeggpu_ext_crop_to_rgbi_fancy_cs.argtypes = [
        C.POINTER(ImgInfo), C.c_int, C.POINTER(CropInfo), C.POINTER(Img), C.c_void_p, C.c_int, C.c_void_p]
    L.jpeggpu_ext_crop_to_rgbi_replicate_cs.argtypes = L.jpeggpu_ext_crop_to_rgbi_fancy_cs.argtypes
    L.jpeggpu_ext_resize_scratch_size_cs.restype = C.c_size_t
    L.jpeggpu_ext_resize_scratch_size_cs.argtypes = [C.POINTER(ResizeItem), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int]
    L.jpeggpu_ext_resize_to_rgb_cs.argtypes = [
        C.POINTER(ResizeItem), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
        C.c_void_p]
    L.jpeggpu_ext_set_progressive.argtypes = [dec, C.c_int]
    L.jpeggpu_ext_get_progressive_info.argtypes = [dec, C.POINTER(ProgressiveInfo)]
    if hasattr(L, "jpeggpu_ext_set_truncated"):  # (a library loaded through JPEGGPU_LIB may be older than this file)
        L.jpeggpu_ext_set_truncated.argtypes = [dec, C.c_int]
        L.jpeggpu_ext_get_truncated.argtypes = [dec, C.POINTER(TruncatedInfo)]
    L.jpeggpu_ext_get_orientation.argtypes = [dec, C.POINTER(C.c_int)]
    L.jpeggpu_ext_orient_size.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.jpeggpu_ext_orient_rect.argtypes = [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4
    L.jpeggpu_ext_planes_to_rgbi_oriented.argtypes = [
        C.POINTER(ImgInfo), C.c_int, C.c_int, C.c_int, C.POINTER(Img), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.jpeggpu_ext_crop_to_rgbi_oriented.argtypes = [
        C.POINTER(ImgInfo), C.c_int, C.c_int, C.c_int, C.POINTER(CropInfo), C.POINTER(Img), C.c_void_p, C.c_int, C.c_void_p]
    L.jpeggpu_ext_resize_scratch_size_oriented.restype = C.c_size_t
    L.jpeggpu_ext_resize_scratch_size_oriented.argtypes = [
        C.POINTER(ResizeItem), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int]
    L.jpeggpu_ext_resize_to_rgb_oriented.argtypes = [
        C.POINTER(ResizeItem), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
        C.c_void_p, C.c_size_t, C.c_void_p]
    L.jpeggpu_ext_resize_to_tensor.argtypes = [
        C.POINTER(ResizeItem), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(TensorSpec),
        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.jpeggpu_ext_resize_view_scratch_size.restype = C.c_size_t
    L.jpeggpu_ext_resize_view_scratch_size.argtypes = [
        C.POINTER(ResizeItem), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(ResizeView), C.c_int, C.c_int, C.c_int, C.c_int]
    L.jpeggpu_ext_resize_view_to_tensor.argtypes = [
        C.POINTER(ResizeItem), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(ResizeView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
        C.POINTER(TensorSpec), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.jpeggpu_ext_resize_view_rect.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(ResizeView), C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4
    L.jpeggpu_ext_resize_view_weights.argtypes = [
        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    L.jpeggpu_ext_batch_rgb_scratch_size.restype = C.c_size_t
    L.jpeggpu_ext_batch_rgb_scratch_size.argtypes = [C.c_int]
    L.jpeggpu_ext_batch_to_rgb.argtypes = [C.POINTER(RgbItem), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    if hasattr(L, "jpeggpu_ext_encode_batch"):  # (a library loaded through JPEGGPU_LIB may be older than this file)
        L.jpeggpu_ext_encode_header.argtypes = [C.POINTER(EncodeItem), C.c_void_p, C.POINTER(C.c_size_t)]
        L.jpeggpu_ext_encode_bound.argtypes = [C.POINTER(EncodeItem)]
        L.jpeggpu_ext_encode_bound.restype = C.c_size_t
        L.jpeggpu_ext_encode_scratch_size.argtypes = [C.POINTER(EncodeItem), C.c_int]
        L.jpeggpu_ext_encode_scratch_size.restype = C.c_size_t
        L.jpeggpu_ext_encode_batch.argtypes = [C.POINTER(EncodeItem), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "jpeggpu_ext_encode_fit_batch"):  # encoding to a byte budget (_newer_symbol)
        L.jpeggpu_ext_encode_fit_scratch_size.argtypes = [C.POINTER(EncodeFitItem), C.c_int]
        L.jpeggpu_ext_encode_fit_scratch_size.restype = C.c_size_t
        L.jpeggpu_ext_encode_fit_launches.argtypes = [C.POINTER(EncodeFitItem), C.c_int]
        L.jpeggpu_ext_encode_fit_batch.argtypes = [C.POINTER(EncodeFitItem), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "jpeggpu_ext_roundtrip_batch"):
        L.jpeggpu_ext_roundtrip_scratch_size.argtypes = [C.POINTER(RoundtripItem), C.c_int]
        L.jpeggpu_ext_roundtrip_scratch_size.restype = C.c_size_t
        L.jpeggpu_ext_roundtrip_batch.argtypes = [C.POINTER(RoundtripItem), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    if hasattr(L, "jpeggpu_ext_transcode_batch"):
        L.jpeggpu_ext_transcode_header.argtypes = [C.POINTER(TranscodeItem), C.c_void_p, C.POINTER(C.c_size_t)]
        L.jpeggpu_ext_transcode_bound.argtypes = [C.POINTER(TranscodeItem)]
        L.jpeggpu_ext_transcode_bound.restype = C.c_size_t
        L.jpeggpu_ext_transcode_scratch_size.argtypes = [C.POINTER(TranscodeItem), C.c_int]
        L.jpeggpu_ext_transcode_scratch_size.restype = C.c_size_t
        L.jpeggpu_ext_transcode_batch.argtypes = [C.POINTER(TranscodeItem), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.jpeggpu_ext_batch_set_coefficients_only.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "jpeggpu_ext_read_coefficients_batch"):  # DCT-domain access (_newer_symbol)
        L.jpeggpu_ext_get_coefficient_info.argtypes = [dec, C.POINTER(CoefficientInfo)]
        L.jpeggpu_ext_read_coefficients_scratch_size.argtypes = [C.c_int]
        L.jpeggpu_ext_read_coefficients_scratch_size.restype = C.c_size_t
        L.jpeggpu_ext_read_coefficients_batch.argtypes = [C.POINTER(CoefficientReadItem), C.c_int, C.POINTER(CoefficientSpec), C.c_void_p, C.c_size_t, C.c_void_p]
        L.jpeggpu_ext_write_coefficients_header.argtypes = [C.POINTER(CoefficientItem), C.c_void_p, C.POINTER(C.c_size_t)]
        L.jpeggpu_ext_write_coefficients_bound.argtypes = [C.POINTER(CoefficientItem)]
        L.jpeggpu_ext_write_coefficients_bound.restype = C.c_size_t
        L.jpeggpu_ext_write_coefficients_scratch_size.argtypes = [C.POINTER(CoefficientItem), C.c_int]
        L.jpeggpu_ext_write_coefficients_scratch_size.restype = C.c_size_t
        L.jpeggpu_ext_write_coefficients_batch.argtypes = [C.POINTER(CoefficientItem), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "jpeggpu_ext_set_transcode_orientation"):
        L.jpeggpu_ext_set_transcode_orientation.argtypes = [dec, C.c_int, C.c_int]
    if hasattr(L, "jpeggpu_ext_set_transcode_crop"):
        L.jpeggpu_ext_set_transcode_crop.argtypes = [dec, C.c_int, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "jpeggpu_ext_set_transcode_frame"):
        L.jpeggpu_ext_set_transcode_frame.argtypes = [dec, C.c_int]
    if hasattr(L, "jpeggpu_ext_encode_tables_from_counts"):
        L.jpeggpu_ext_encode_tables_from_counts.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.jpeggpu_ext_resize_weights.argtypes = [
        C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    if hasattr(L, "jpeggpu_ext_thumbnail_to_rgb"):
        L.jpeggpu_ext_thumbnail_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(Thumbnail)]
        L.jpeggpu_ext_resize_box_weights.argtypes = [
            C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
        L.jpeggpu_ext_thumbnail_scratch_size.restype = C.c_size_t
        L.jpeggpu_ext_thumbnail_scratch_size.argtypes = [
            C.POINTER(ResizeItem), C.POINTER(C.c_int), C.POINTER(Thumbnail), C.c_int, C.c_int, C.c_int, C.c_int]
        L.jpeggpu_ext_thumbnail_to_rgb.argtypes = [
            C.POINTER(ResizeItem), C.POINTER(C.c_int), C.POINTER(Thumbnail), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
            C.c_size_t, C.c_void_p]
    if hasattr(L, "jpeggpu_ext_set_luma_only"):  # grey output (_newer_symbol)
        L.jpeggpu_ext_set_luma_only.argtypes = [dec, C.c_int]
        L.jpeggpu_ext_crop_to_gray_oriented.argtypes = L.jpeggpu_ext_crop_to_rgbi_oriented.argtypes
        L.jpeggpu_ext_batch_gray_scratch_size.restype = C.c_size_t
        L.jpeggpu_ext_batch_gray_scratch_size.argtypes = [C.c_int]
        L.jpeggpu_ext_batch_to_gray.argtypes = [C.POINTER(RgbItem), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.jpeggpu_ext_resize_view_to_gray_scratch_size.restype = C.c_size_t
        L.jpeggpu_ext_resize_view_to_gray_scratch_size.argtypes = L.jpeggpu_ext_resize_view_scratch_size.argtypes
        L.jpeggpu_ext_resize_view_to_gray_tensor.argtypes = L.jpeggpu_ext_resize_view_to_tensor.argtypes
    _lib = L
    return L


def status_string(status) -> str:
    return lib().jpeggpu_get_status_string(int(status)).decode()


def _check(status, where):
    if status != 0:
        raise JpegGpuError(status, where)


def _newer_symbol(name):
    """lib()'s function `name`, one of those a library loaded through JPEGGPU_LIB may predate: a RuntimeError that names it
    where it is missing."""
    if not hasattr(lib(), name):
        raise RuntimeError("this libjpeggpu has no %s" % name)
    return getattr(lib(), name)


def _img(planes, pitches=None):
    """An Img of plane pointers and their pitches, or (no pitches) of the planes as 2-D tensors."""
    if pitches is None:
        planes, pitches = [p.data_ptr() for p in planes], [p.stride(0) for p in planes]
    img = Img()
    for c, (p, pitch) in enumerate(zip(planes, pitches)):
        img.image[c], img.pitch[c] = p, pitch
    return img


def _host_buffer(data):
    """(address, size, object to keep alive) of a bytes / bytearray input. The decoder borrows the address until
    the copy enqueued by transfer() has executed, so the address must belong to the object that is kept: the
    bytes object itself, or a ctypes view of the bytearray's own storage (no temporary copy)."""
    if isinstance(data, bytearray):
        view = (C.c_char * len(data)).from_buffer(data) if len(data) else (C.c_char * 1)()
        return C.addressof(view), len(data), (data, view)
    return C.cast(C.c_char_p(data), C.c_void_p).value, len(data), data


class Decoder:
    """One jpeggpu_decoder_t. Not thread-safe; one decoder per host thread / stream."""

    def __init__(self, subseq_bytes=None):
        self._h = C.c_void_p()
        _check(lib().jpeggpu_decoder_startup(C.byref(self._h)), "jpeggpu_decoder_startup")
        self._keep = None
        if subseq_bytes is not None:
            self.set_subsequence_bytes(subseq_bytes)

    def set_logging(self, on: bool):
        _check(lib().jpeggpu_set_logging(self._h, int(on)), "jpeggpu_set_logging")

    def set_subsequence_bytes(self, n: int):
        _check(lib().jpeggpu_ext_set_subsequence_bytes(self._h, n), "jpeggpu_ext_set_subsequence_bytes")

    def set_batched(self, on: bool = True):
        """This decoder's images share their launches with others (jpeggpu_ext_decode_batch): the per-image choice
        of the subsequence size is made for throughput instead of for the latency of one image."""
        _check(lib().jpeggpu_ext_set_batched(self._h, int(on)), "jpeggpu_ext_set_batched")

    def set_batch_hint(self, images_per_call: int):
        """About how many images of this kind share one jpeggpu_ext_decode_batch call (0: decoded on its own). The plan
        of the next parsed images -- subsequence size, multi-hypothesis speculation -- is made for a launch of that size."""
        _check(lib().jpeggpu_ext_set_batch_hint(self._h, int(images_per_call)), "jpeggpu_ext_set_batch_hint")

    def parse_header(self, data, size=None) -> ImgInfo:
        """`data`: bytes, a numpy uint8 array, or an integer host address (then `size` is required).
        The buffer is borrowed until the copy enqueued by transfer() has executed."""
        info = ImgInfo()
        if isinstance(data, int):
            ptr, n = data, size
        elif isinstance(data, (bytes, bytearray)):
            ptr, n, self._keep = _host_buffer(data)
        else:  # numpy / torch-like with ctypes or data_ptr
            self._keep = data
            ptr = data.ctypes.data if hasattr(data, "ctypes") else data.data_ptr()
            n = data.nbytes if hasattr(data, "nbytes") else data.numel()
        _check(lib().jpeggpu_decoder_parse_header(self._h, C.byref(info), ptr, n), "jpeggpu_decoder_parse_header")
        self.info = info  # of the last parsed image
        return info

    def set_device_scan(self, on=True):
        """False / 0: host walk; True / 1: marker scan on the device, status via device_status(); 2: checked --
        decode() waits for the stream and raises the device's status (what JPEGGPU_DEVICE_SCAN=2 selects)."""
        _check(lib().jpeggpu_ext_set_device_scan(self._h, int(on)), "jpeggpu_ext_set_device_scan")

    def set_scale(self, scale_denom: int):
        """Decode the next parsed images at 1 / scale_denom (1, 2, 4 or 8): planes of ceil(size / scale_denom), the
        arithmetic of libjpeg-turbo's reduced IDCTs (jpeggpu_ext_set_scale)."""
        _check(lib().jpeggpu_ext_set_scale(self._h, int(scale_denom)), "jpeggpu_ext_set_scale")

    def set_scale_mode(self, mode: str):
        """How the next parsed images are scaled: "uniform" (the default: every component at 1 / scale) or "libjpeg" --
        libjpeg-turbo's per-component IDCT sizes, what Pillow's draft() decodes (jpeggpu_ext_set_scale_mode)."""
        if mode not in SCALE_MODES:
            raise ValueError("scale mode %r is not one of %s" % (mode, ", ".join(SCALE_MODES)))
        _check(lib().jpeggpu_ext_set_scale_mode(self._h, SCALE_MODES[mode]), "jpeggpu_ext_set_scale_mode")

    def scale_info(self) -> ScaleInfo:
        """jpeggpu_ext_get_scale_info of the last parsed image."""
        si = ScaleInfo()
        _check(lib().jpeggpu_ext_get_scale_info(self._h, C.byref(si)), "jpeggpu_ext_get_scale_info")
        return si

    def color_space(self) -> ColorSpace:
        """jpeggpu_ext_get_color_space of the last parsed image: GRAY, YCBCR, RGB, CMYK or YCCK by libjpeg's rules (JFIF and
        Adobe segments, component ids), UNKNOWN for two components."""
        cs = C.c_int()
        _check(lib().jpeggpu_ext_get_color_space(self._h, C.byref(cs)), "jpeggpu_ext_get_color_space")
        return ColorSpace(cs.value)

    def orientation(self) -> int:
        """jpeggpu_ext_get_orientation of the last parsed image: its EXIF Orientation as Pillow reads it, 1..8 (1: none)."""
        o = C.c_int()
        _check(lib().jpeggpu_ext_get_orientation(self._h, C.byref(o)), "jpeggpu_ext_get_orientation")
        return o.value

    def set_transcode_orientation(self, orientation: int = 1, trim: bool = False):
        """jpeggpu_ext_set_transcode_orientation: what the transcode calls make of this decoder's files from now on -- the
        stored image of the new file is the displayed image under `orientation` (1..8); `trim` cuts partial iMCUs at a
        mirrored edge instead of refusing them. Decodes to pixels ignore it."""
        _check(_newer_symbol("jpeggpu_ext_set_transcode_orientation")(self._h, int(orientation), int(trim)), "jpeggpu_ext_set_transcode_orientation")

    def set_transcode_frame(self, mode: int = 0):
        """jpeggpu_ext_set_transcode_frame: 0 -- the transcode calls write the encoder's frame layouts and refuse every other
        source; 1 -- the new file keeps the source's own layout (any sampling, up to four components and tables)."""
        _check(_newer_symbol("jpeggpu_ext_set_transcode_frame")(self._h, int(mode)), "jpeggpu_ext_set_transcode_frame")

    def set_transcode_crop(self, x: int = 0, y: int = 0, w: int = 0, h: int = 0):
        """jpeggpu_ext_set_transcode_crop: the transcode calls write only the rectangle (x, y, w, h) of the image they would
        write without it (after the orientation and its trim) from now on; (0, 0, 0, 0): the whole image again. x and y are
        multiples of the target's iMCU. Decodes to pixels ignore it."""
        _check(_newer_symbol("jpeggpu_ext_set_transcode_crop")(self._h, int(x), int(y), int(w), int(h)), "jpeggpu_ext_set_transcode_crop")

    def coefficient_info(self) -> CoefficientInfo:
        """jpeggpu_ext_get_coefficient_info of the last parsed image: the real block grids, factors and tables."""
        ci = CoefficientInfo()
        _check(_newer_symbol("jpeggpu_ext_get_coefficient_info")(self._h, C.byref(ci)), "jpeggpu_ext_get_coefficient_info")
        return ci

    def set_progressive(self, on: bool = True):
        """Read progressive JPEGs (SOF2) from the next parse_header on; off by default, when they are NOT_SUPPORTED
        (jpeggpu_ext_set_progressive)."""
        _check(lib().jpeggpu_ext_set_progressive(self._h, int(on)), "jpeggpu_ext_set_progressive")

    def progressive_info(self) -> ProgressiveInfo:
        """jpeggpu_ext_get_progressive_info of the last parsed image."""
        pi = ProgressiveInfo()
        _check(lib().jpeggpu_ext_get_progressive_info(self._h, C.byref(pi)), "jpeggpu_ext_get_progressive_info")
        return pi

    def set_truncated(self, on: bool = True):
        """Read files that end early from the next parse_header on, decoded as Pillow does with
        ImageFile.LOAD_TRUNCATED_IMAGES; off by default, when they are INVALID_JPEG (jpeggpu_ext_set_truncated). Progressive
        files are NOT_SUPPORTED while it is on."""
        _check(lib().jpeggpu_ext_set_truncated(self._h, int(on)), "jpeggpu_ext_set_truncated")

    def truncated(self) -> TruncatedInfo:
        """jpeggpu_ext_get_truncated of the last parsed image."""
        ti = TruncatedInfo()
        _check(lib().jpeggpu_ext_get_truncated(self._h, C.byref(ti)), "jpeggpu_ext_get_truncated")
        return ti

    def set_idct(self, method: str):
        """The full-size IDCT of the next parsed images: "reference" (the default) or "islow", libjpeg-turbo's
        jpeg_idct_islow, the transform of Pillow, torchvision and OpenCV (jpeggpu_ext_set_idct)."""
        if method not in IDCT_METHODS:
            raise ValueError("idct method %r is not one of %s" % (method, ", ".join(IDCT_METHODS)))
        _check(lib().jpeggpu_ext_set_idct(self._h, IDCT_METHODS[method]), "jpeggpu_ext_set_idct")

    def set_luma_only(self, on: bool = True):
        """jpeggpu_ext_set_luma_only: from the next parse_header on, only component 0 of a YCbCr file is transformed and
        written (libjpeg's JCS_GRAYSCALE; the other planes' pointers may be 0); grey and RGB-coded files are decoded as
        ever, CMYK and YCCK ones refused by parse_header (NOT_SUPPORTED)."""
        _check(_newer_symbol("jpeggpu_ext_set_luma_only")(self._h, 1 if on else 0), "jpeggpu_ext_set_luma_only")

    def set_crop(self, x: int, y: int, w: int, h: int):
        """Decode only the rectangle (x, y, w, h) of the image at the decoder's scale from the next parse_header on
        (0, 0, 0, 0: the whole image again). The planes are then windows of the full planes (crop_info says where)."""
        _check(lib().jpeggpu_ext_set_crop(self._h, int(x), int(y), int(w), int(h)), "jpeggpu_ext_set_crop")

    def crop_info(self) -> CropInfo:
        """jpeggpu_ext_get_crop of the last parsed image."""
        ci = CropInfo()
        _check(lib().jpeggpu_ext_get_crop(self._h, C.byref(ci)), "jpeggpu_ext_get_crop")
        return ci

    def set_segment_shard(self, rank: int, world: int):
        """Decode only restart segments [rank * n / world, (rank + 1) * n / world) of the next parsed images."""
        _check(lib().jpeggpu_ext_set_segment_shard(self._h, rank, world), "jpeggpu_ext_set_segment_shard")

    def shard_rows(self, component: int):
        """(first_row, num_rows) of the plane rows this decoder writes."""
        a, n = C.c_int(), C.c_int()
        _check(lib().jpeggpu_ext_get_shard_rows(self._h, component, C.byref(a), C.byref(n)), "jpeggpu_ext_get_shard_rows")
        return a.value, n.value

    def device_status(self, d_tmp: int, stream: int = 0) -> Status:
        st = C.c_int()
        _check(lib().jpeggpu_ext_get_device_status(self._h, d_tmp, stream, C.byref(st)), "jpeggpu_ext_get_device_status")
        return Status(st.value)

    def get_buffer_size(self) -> int:
        n = C.c_size_t()
        _check(lib().jpeggpu_decoder_get_buffer_size(self._h, C.byref(n)), "jpeggpu_decoder_get_buffer_size")
        return n.value

    def transfer(self, d_tmp: int, tmp_size: int, stream: int = 0):
        _check(lib().jpeggpu_decoder_transfer(self._h, d_tmp, tmp_size, stream), "jpeggpu_decoder_transfer")

    def decode(self, planes, pitches, d_tmp: int, tmp_size: int, stream: int = 0):
        _check(lib().jpeggpu_decoder_decode(self._h, C.byref(_img(planes, pitches)), d_tmp, tmp_size, stream), "jpeggpu_decoder_decode")

    def set_profiling(self, on: bool):
        _check(lib().jpeggpu_ext_set_profiling(self._h, int(on)), "jpeggpu_ext_set_profiling")

    def stage_ms(self):
        """Per-stage milliseconds of the last decode (after the stream was synchronised)."""
        ms = (C.c_float * len(STAGES))()
        _check(lib().jpeggpu_ext_get_stage_ms(self._h, ms), "jpeggpu_ext_get_stage_ms")
        return dict(zip(STAGES, ms))

    def layout(self) -> ExtLayout:
        lay = ExtLayout()
        _check(lib().jpeggpu_ext_get_layout(self._h, C.byref(lay)), "jpeggpu_ext_get_layout")
        return lay

    def cleanup(self):
        if self._h:
            lib().jpeggpu_decoder_cleanup(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass


class Batch:
    """jpeggpu_ext_decode_batch: one launch per stage for many parsed + transferred images."""

    def __init__(self, max_scans: int):
        self._h = C.c_void_p()
        self.max_scans = max_scans
        _check(lib().jpeggpu_ext_batch_create(C.byref(self._h), max_scans), "jpeggpu_ext_batch_create")
        self.scratch_size = lib().jpeggpu_ext_batch_scratch_size(max_scans)
        self._items = None
        self._keep = None

    def set_items(self, entries):
        """entries: list of (Decoder, plane_ptrs, pitches, d_tmp, tmp_size). Built once, reused per call."""
        n = len(entries)
        arr = (BatchItem * n)()
        imgs = []
        for i, (dec, ptrs, pitches, d_tmp, tmp_size) in enumerate(entries):
            imgs.append(_img(ptrs, pitches))
            arr[i].decoder = dec._h
            arr[i].img = C.pointer(imgs[i])
            arr[i].d_tmp = d_tmp
            arr[i].tmp_size = tmp_size
        self._items, self._keep = arr, (imgs, entries)

    def decode(self, d_scratch: int, stream: int = 0):
        _check(lib().jpeggpu_ext_decode_batch(self._h, self._items, len(self._items), d_scratch, self.scratch_size, stream),
               "jpeggpu_ext_decode_batch")

    def set_overlap(self, parts: int):
        _check(lib().jpeggpu_ext_batch_set_overlap(self._h, parts), "jpeggpu_ext_batch_set_overlap")

    def set_fused_tail(self, enable: bool):
        _check(_newer_symbol("jpeggpu_ext_batch_set_fused_tail")(self._h, 1 if enable else 0), "jpeggpu_ext_batch_set_fused_tail")

    def set_sync_run(self, r: int):
        """Consecutive subsequences a lane of the batched sequence kernel owns: 1, 2 or 4 (jpeggpu_ext.h)."""
        _check(_newer_symbol("jpeggpu_ext_batch_set_sync_run")(self._h, int(r)), "jpeggpu_ext_batch_set_sync_run")

    def set_coefficients_only(self, enable: bool):
        """The calls stop in front of the IDCT stage, and the items' plane pointers may be NULL (jpeggpu_ext.h): what a
        transcode needs of a decode."""
        _check(_newer_symbol("jpeggpu_ext_batch_set_coefficients_only")(self._h, 1 if enable else 0), "jpeggpu_ext_batch_set_coefficients_only")

    def set_sync_iterations(self, n: int):
        _check(lib().jpeggpu_ext_batch_set_sync_iterations(self._h, n), "jpeggpu_ext_batch_set_sync_iterations")

    def set_profiling(self, on: bool):
        _check(lib().jpeggpu_ext_batch_set_profiling(self._h, int(on)), "jpeggpu_ext_batch_set_profiling")

    def stage_ms(self):
        ms = (C.c_float * len(STAGES))()
        _check(lib().jpeggpu_ext_batch_get_stage_ms(self._h, ms), "jpeggpu_ext_batch_get_stage_ms")
        return dict(zip(STAGES, ms))

    def destroy(self):
        if self._h:
            lib().jpeggpu_ext_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def fused_tail_timeouts() -> int:
    """Writers of the fused tail + write launch that gave up waiting, since the library was loaded (0 on a correct run)."""
    n = C.c_uint(0)
    _check(_newer_symbol("jpeggpu_ext_fused_tail_timeouts")(C.byref(n)), "jpeggpu_ext_fused_tail_timeouts")
    return n.value


def self_test(stream: int = 0) -> None:
    """jpeggpu_ext_self_test: one small built-in decode checked against stored plane hashes; raises JpegGpuError if the
    running system does not decode bit-exactly."""
    _check(lib().jpeggpu_ext_self_test(stream), "jpeggpu_ext_self_test")


def draft_scale(width, height, requested):
    """The scale Pillow's JpegImageFile.draft(mode, requested) picks for a width x height JPEG: min(width // rw,
    height // rh) rounded down to 8, 4, 2 or 1 (requested = (rw, rh), each clamped to the image). Pure Python."""
    rw, rh = requested
    rw, rh = min(int(rw), width), min(int(rh), height)
    if rw < 1 or rh < 1:
        raise ValueError("requested size must be positive")
    s = min(width // rw, height // rh)
    return 8 if s >= 8 else 4 if s >= 4 else 2 if s >= 2 else 1


def orient_size(orientation, w, h):
    """jpeggpu_ext_orient_size (host only): the displayed (width, height) of a stored w x h image."""
    ow, oh = C.c_int(), C.c_int()
    _check(lib().jpeggpu_ext_orient_size(int(orientation), int(w), int(h), C.byref(ow), C.byref(oh)), "jpeggpu_ext_orient_size")
    return ow.value, oh.value


def orient_rect(orientation, w, h, rect):
    """jpeggpu_ext_orient_rect (host only): the stored rectangle (x, y, w, h) of `rect`, given in displayed coordinates of a
    stored w x h image -- what Decoder.set_crop takes."""
    v = [C.c_int(int(a)) for a in rect]
    _check(lib().jpeggpu_ext_orient_rect(int(orientation), int(w), int(h), *[C.byref(a) for a in v]), "jpeggpu_ext_orient_rect")
    return tuple(a.value for a in v)


def _frame_size(info):
    """(width, height) of the image an ImgInfo's planes make: img_info has no frame size, but the plane of a component
    with the largest factor has exactly the frame's extent."""
    n = info.num_components
    hmax, vmax = max(info.subsampling.x[:n]), max(info.subsampling.y[:n])
    return (info.sizes_x[[c for c in range(n) if info.subsampling.x[c] == hmax][0]],
            info.sizes_y[[c for c in range(n) if info.subsampling.y[c] == vmax][0]])


def decode_to_planes(data: bytes, device="cuda:0", subseq_bytes=None, return_tmp=False, device_scan=False, scale=1,
                     idct="reference", crop=None, scale_mode="uniform", return_color=False, progressive=False,
                     displayed_crop=False, return_orientation=False, luma_only=False, truncated=False):
    """Convenience wrapper used by tests: full call sequence on torch's current stream, returns the
    planes as torch uint8 tensors on `device` (torch is only the allocator / stream provider). With
    `device_scan` the restart markers are found on the device and a status it reports there is raised.
    `scale`: 1, 2, 4 or 8 -- planes at 1 / scale (Decoder.set_scale). `idct`: "reference" or "islow" (Decoder.set_idct).
    `crop`: (x, y, w, h) -- only the planes' windows for that rectangle are decoded (Decoder.set_crop), and the CropInfo
    is returned as well: (planes, info, crop_info). `scale_mode`: "uniform" or "libjpeg" (Decoder.set_scale_mode); the
    returned info then carries the planes' effective sampling factors. `return_color`: the file's ColorSpace
    (Decoder.color_space) is appended to what is returned. `progressive`: progressive files are decoded
    (Decoder.set_progressive); with `return_tmp` the ProgressiveInfo follows the layout. `displayed_crop`: `crop` is in
    displayed coordinates of the file's EXIF orientation (the header is parsed once more to learn it; orient_rect).
    `return_orientation`: Decoder.orientation is appended last. `luma_only`: Decoder.set_luma_only -- of a YCbCr file only
    plane 0 is allocated, decoded and returned (`planes` has one entry; `info` still describes all components).
    `truncated`: Decoder.set_truncated -- a file that ends early is decoded as Pillow does with LOAD_TRUNCATED_IMAGES."""
    import torch

    dec = Decoder(subseq_bytes)
    try:
        if truncated:
            dec.set_truncated(True)
        if luma_only:
            dec.set_luma_only(True)
        if scale != 1:
            dec.set_scale(scale)
        if scale_mode != "uniform":
            dec.set_scale_mode(scale_mode)
        if idct != "reference":
            dec.set_idct(idct)
        if device_scan:
            dec.set_device_scan(True)
        if progressive:
            dec.set_progressive(True)
        if crop is not None and displayed_crop:
            w, h = _frame_size(dec.parse_header(data))
            crop = orient_rect(dec.orientation(), w, h, crop)
        if crop is not None:
            dec.set_crop(*crop)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp = torch.empty(n + 256, dtype=torch.uint8, device=device)
        base = (tmp.data_ptr() + 255) // 256 * 256
        stream = torch.cuda.current_stream(torch.device(device)).cuda_stream
        planes = [torch.empty((info.sizes_y[c], info.sizes_x[c]), dtype=torch.uint8, device=device)
                  for c in range(1 if luma_only and dec.color_space() == ColorSpace.YCBCR else info.num_components)]
        dec.transfer(base, n, stream)
        dec.decode([p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n, stream)
        torch.cuda.synchronize(torch.device(device))
        if device_scan:
            _check(int(dec.device_status(base, stream)), "device-side marker scan")
        out = (planes, info)
        if crop is not None:
            out += (dec.crop_info(),)
        if return_tmp:
            out += (tmp, base, dec.layout())
            if progressive:
                out += (dec.progressive_info(),)
        if return_color:
            out += (dec.color_space(),)
        if return_orientation:
            out += (dec.orientation(),)
        return out
    finally:
        dec.cleanup()


def _to_rgb(stem, planes, info, crop_info, device, fancy, replicate, color, orientation):
    """planes_to_rgb's and crop_to_rgb's body. The entry point is `stem` + _oriented with an orientation, else `stem` +
    _replicate / _fancy / nothing, + _cs with a colour; without `crop_info` it converts the whole image and is told its size."""
    import torch

    n = info.num_components
    device = planes[0].device if device is None else torch.device(device)
    src = _img(planes[:n])
    w, h = _frame_size(info) if crop_info is None else (crop_info.width, crop_info.height)
    if not (fancy or replicate) and (orientation is not None or color is not None):
        raise ValueError("the reference's helper (fancy=False) takes no %s" % ("orientation" if orientation is not None else "colour model"))
    if orientation is not None:
        name = stem + "_oriented"
        cs = int(color) if color is not None else int(_item_colors(None, [info])[0])
        model = (cs, int(orientation), int(bool(replicate)))
        ow, oh = (h, w) if 5 <= int(orientation) <= 8 else (w, h)
    else:
        name = stem + ("_replicate" if replicate else "_fancy" if fancy else "") + ("_cs" if color is not None else "")
        model = (int(color),) if color is not None else ()
        ow, oh = w, h
    # the C signatures, by what `stem` and `name` select (jpeggpu_ext.h):
    #   planes_to_rgbi[_fancy|_replicate]     (info,                             src, out, pitch, width, height, stream)
    #   planes_to_rgbi_{fancy,replicate}_cs   (info, color,                      src, out, pitch, width, height, stream)
    #   planes_to_rgbi_oriented               (info, color, orientation, repl.,  src, out, pitch, width, height, stream)
    #   crop_to_rgbi_{fancy,replicate}        (info,                       crop, src, out, pitch, stream)
    #   crop_to_rgbi_{fancy,replicate}_cs     (info, color,                crop, src, out, pitch, stream)
    #   crop_to_rgbi_oriented                 (info, color, orientation, repl., crop, src, out, pitch, stream)
    source, size = ((C.byref(src),), (w, h)) if crop_info is None else ((C.byref(crop_info), C.byref(src)), ())
    out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=device)
    _check(getattr(lib(), name)(C.byref(info), *model, *source, out.data_ptr(), 3 * ow, *size, torch.cuda.current_stream(device).cuda_stream), name)
    return out


def planes_to_rgb(planes, info, fancy=True, device=None, replicate=False, color=None, orientation=None):
    """Planes of a 1- or 3-component image (as decode_to_planes returns them) -> (H, W, 3) uint8 tensor at the full image
    size, on torch's current stream: jpeggpu_ext_planes_to_rgbi_fancy (libjpeg's fancy upsampling and integer colour
    conversion) or, with fancy=False, jpeggpu_ext_planes_to_rgbi (the reference's helper). `replicate`:
    jpeggpu_ext_planes_to_rgbi_replicate -- libjpeg's conversion with replication, its output at 1/8 in the libjpeg scale
    mode. `color`: the planes' ColorSpace (Decoder.color_space) -- the _cs form of the fancy or replicating call, which also
    converts RGB-, CMYK- and YCCK-coded files (four planes); None: grey or YCbCr by the number of components.
    `orientation`: an EXIF orientation 1..8 (Decoder.orientation) -- jpeggpu_ext_planes_to_rgbi_oriented, the displayed
    image: (W, H, 3) for 5..8."""
    return _to_rgb("jpeggpu_ext_planes_to_rgbi", planes, info, None, device, fancy, replicate, color, orientation)


def crop_to_rgb(planes, info, crop_info, device=None, replicate=False, color=None, orientation=None):
    """The window planes of a cropped decode (decode_to_planes(..., crop=...)) -> (h, w, 3) uint8 tensor of the rectangle,
    equal to that part of planes_to_rgb's image of the uncropped planes (jpeggpu_ext_crop_to_rgbi_fancy, or with
    `replicate` jpeggpu_ext_crop_to_rgbi_replicate). `color`: as in planes_to_rgb. `orientation`: as in planes_to_rgb --
    crop_info is the STORED rectangle (orient_rect), the result the displayed one (jpeggpu_ext_crop_to_rgbi_oriented)."""
    return _to_rgb("jpeggpu_ext_crop_to_rgbi", planes, info, crop_info, device, True, replicate, color, orientation)


def _max_factors(info):
    n = info.num_components
    return max(info.subsampling.x[:n]), max(info.subsampling.y[:n])


def _needs_replication(info, scale):
    """libjpeg replicates instead of fancy upsampling at 1/8 (jdsample.c); it matters where subsampling is left."""
    n = info.num_components
    return scale == 8 and (len(set(info.subsampling.x[:n])) > 1 or len(set(info.subsampling.y[:n])) > 1)


def decode_to_rgb(data: bytes, device="cuda:0", device_scan=False, crop=None, scale=1, exif_transpose=False, truncated=False):
    """Decode a JPEG to an (H, W, 3) uint8 tensor on `device` the way libjpeg-turbo does: the ISLOW IDCT at full size, then
    fancy upsampling and the conversion of the file's colour model (Decoder.color_space): grey, YCbCr (jdcolor.c's integer
    conversion), RGB-coded files as they are, CMYK and YCCK by Pillow's rule for Adobe's inverted samples. Meant to equal
    np.asarray(PIL.Image.open(f).convert("RGB")) ("Matching Pillow / torchvision"). With `crop` = (x, y,
    w, h) only that rectangle is decoded: an (h, w, 3) tensor equal to decode_to_rgb(data)[y:y + h, x:x + w].
    `scale` = d in 2, 4, 8: the image at 1/d as libjpeg-turbo scales it (the libjpeg scale mode: per-component IDCT sizes,
    replication instead of fancy upsampling at 1/8), equal to im.draft("RGB", (W // d, H // d)); im.convert("RGB") in
    Pillow; `crop` is then in pixels of that image. Progressive files are decoded too (Decoder.set_progressive).
    `exif_transpose`: the file's EXIF orientation (Decoder.orientation) is applied -- the result is the DISPLAYED image,
    (W, H, 3) for orientations 5..8, and `crop` is in displayed pixels at the scale: what ImageOps.exif_transpose(im) put
    after draft() and before convert("RGB") and crop() gives. The XMP orientation Pillow falls back to is not read.
    `truncated`: a file that ends early gives what Pillow gives with ImageFile.LOAD_TRUNCATED_IMAGES set -- the rows that are
    there, grey below (Decoder.set_truncated; INTEGRATION.md, "Truncated files"); progressive files are then NOT_SUPPORTED."""
    import torch

    kw = dict(device=device, device_scan=device_scan, idct="islow", scale=scale, scale_mode="libjpeg", return_color=True, progressive=True,
              truncated=truncated)
    if exif_transpose:
        kw.update(displayed_crop=True, return_orientation=True)
    if crop is not None:
        planes, info, crop_info, color, *o = decode_to_planes(data, crop=crop, **kw)
        rgb = crop_to_rgb(planes, info, crop_info, replicate=_needs_replication(info, scale), color=color, orientation=o[0] if o else None)
        torch.cuda.synchronize(torch.device(device))
        return rgb
    planes, info, color, *o = decode_to_planes(data, **kw)
    rgb = planes_to_rgb(planes, info, fancy=True, replicate=_needs_replication(info, scale), color=color, orientation=o[0] if o else None)
    torch.cuda.synchronize(torch.device(device))
    return rgb


def planes_to_gray(planes, info, crop_info=None, device=None, replicate=False, color=None, orientation=1):
    """jpeggpu_ext_crop_to_gray_oriented on torch's current stream: the planes of a decode (the windows of a cropped one, with
    its `crop_info`; of a luma-only decode plane 0 alone) -> the (h, w) uint8 grey of the image or rectangle as `orientation`
    displays it, (w, h) for 5..8. The grey is component 0 of grey and YCbCr files, upsampled where its sampling factors are
    below the largest, and jdcolor.c's rgb_gray_convert of RGB-coded ones. `color`: the planes' ColorSpace; None: grey or
    YCbCr by the number of components. `replicate`: as in planes_to_rgb."""
    import torch

    device = planes[0].device if device is None else torch.device(device)
    src = _img(planes[:info.num_components])
    w, h = _frame_size(info) if crop_info is None else (crop_info.width, crop_info.height)
    ow, oh = (h, w) if 5 <= int(orientation) <= 8 else (w, h)
    cs = int(color) if color is not None else int(_item_colors(None, [info])[0])
    out = torch.empty((oh, ow), dtype=torch.uint8, device=device)
    name = "jpeggpu_ext_crop_to_gray_oriented"
    _check(_newer_symbol(name)(C.byref(info), cs, int(orientation), int(bool(replicate)), C.byref(crop_info) if crop_info is not None else None,
                               C.byref(src), out.data_ptr(), ow, torch.cuda.current_stream(device).cuda_stream), name)
    return out


def decode_to_gray(data: bytes, device="cuda:0", crop=None, scale=1, exif_transpose=False, truncated=False):
    """Decode a JPEG to an (H, W) uint8 grey tensor on `device` the way libjpeg-turbo does for out_color_space =
    JCS_GRAYSCALE: of a YCbCr file only the luma component goes through the IDCT (Decoder.set_luma_only: ISLOW at full size,
    the reduced IDCTs at `scale` = d in 2, 4, 8 in the libjpeg scale mode), a grey file is its one component, an RGB-coded
    file is decoded whole and converted by jdcolor.c's rgb_gray_convert. Meant to equal np.asarray(im) after
    im.draft("L", (W // d, H // d)) in Pillow; CMYK and YCCK files, which Pillow's draft("L") leaves as they are, raise
    JpegGpuError (NOT_SUPPORTED). `crop` = (x, y, w, h) in pixels of the image at the scale and `exif_transpose` as in
    decode_to_rgb: ImageOps.exif_transpose(im) and im.crop applied after the draft. `truncated` as in decode_to_rgb."""
    import torch

    kw = dict(device=device, idct="islow", scale=scale, scale_mode="libjpeg", return_color=True, progressive=True, luma_only=True,
              return_orientation=True, displayed_crop=bool(exif_transpose), truncated=truncated)
    if crop is not None:
        planes, info, crop_info, color, o = decode_to_planes(data, crop=crop, **kw)
    else:
        (planes, info, color, o), crop_info = decode_to_planes(data, **kw), None
    gray = planes_to_gray(planes, info, crop_info, replicate=_needs_replication(info, scale), color=color, orientation=o if exif_transpose else 1)
    torch.cuda.synchronize(torch.device(device))
    return gray


def parse_headers(decoders, buffers, num_threads=4):
    """jpeggpu_ext_parse_headers: parse `buffers[i]` (bytes or numpy uint8; kept alive by the decoder object)
    into `decoders[i]` on a pool of host threads. Returns the list of ImgInfo; raises on the first failure."""
    n = len(decoders)
    items = (ParseItem * n)()
    infos = [ImgInfo() for _ in range(n)]
    for i, (d, b) in enumerate(zip(decoders, buffers)):
        d._keep = b
        if isinstance(b, (bytes, bytearray)):
            ptr, size, d._keep = _host_buffer(b)
        else:
            ptr = b.ctypes.data if hasattr(b, "ctypes") else b.data_ptr()
            size = b.nbytes if hasattr(b, "nbytes") else b.numel()
        items[i].decoder, items[i].img_info, items[i].data, items[i].size = d._h.value, C.pointer(infos[i]), ptr, size
    st = (C.c_int * n)()
    _check(lib().jpeggpu_ext_parse_headers(items, n, num_threads, st), "jpeggpu_ext_parse_headers")
    return infos


def _size_hw(size):
    """torchvision's convention: an int is a square, a pair is (height, width)."""
    if isinstance(size, int):
        return size, size
    h, w = size
    return int(h), int(w)


def resize_max_taps(in_size, out_size, filt="bilinear"):
    """The row stride jpeggpu_ext_resize_weights needs: 2 ceil(support) + 1 (Pillow's ksize)."""
    import math

    return 2 * int(math.ceil({"bilinear": 1.0, "bicubic": 2.0}[filt] * max(in_size / out_size, 1.0))) + 1


def resize_weights(in_size, out_size, filt="bilinear"):
    """jpeggpu_ext_resize_weights (host only): the table the resize kernels use for in_size -> out_size, as numpy int32
    (first[out], count[out], weights[out, max_taps]) with 22 fraction bits."""
    import numpy as np

    if filt not in FILTERS:
        raise ValueError("filter %r is not one of %s" % (filt, ", ".join(FILTERS)))
    k = resize_max_taps(in_size, out_size, filt)
    first, count = np.zeros(max(out_size, 1), np.int32), np.zeros(max(out_size, 1), np.int32)
    w = np.zeros((max(out_size, 1), k), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _check(lib().jpeggpu_ext_resize_weights(int(in_size), int(out_size), FILTERS[filt], ptr(first), ptr(count), ptr(w), k),
           "jpeggpu_ext_resize_weights")
    return first, count, w


def _resize_items(planes_list, infos, crop_infos):
    """(ResizeItem array, objects to keep alive) of decoded images; crop_infos[i] None: the whole image."""
    n = len(planes_list)
    items = (ResizeItem * n)()
    keep = []
    for i in range(n):
        src = _img(planes_list[i])
        ci = crop_infos[i] if crop_infos is not None else None
        items[i].info = C.pointer(infos[i])
        items[i].crop = C.pointer(ci) if ci is not None else None
        items[i].src = C.pointer(src)
        keep.append((src, infos[i], ci))
    return items, keep


def _color_array(colors, n):
    if len(colors) != n:
        raise ValueError("colors must have one entry per image")
    return (C.c_int * n)(*[int(c) for c in colors])


def _item_colors(colors, infos):
    """`colors`, or grey / YCbCr by each item's component count (what the calls without a model assume)."""
    if colors is not None:
        return colors
    return [ColorSpace.GRAY if i.num_components == 1 else ColorSpace.YCBCR if i.num_components == 3 else ColorSpace.UNKNOWN for i in infos]


def _channel_triple(v, default, name):
    """Normalize's per-channel argument as three floats: None (the default), one number for all, or three."""
    if v is None:
        return [default] * 3
    try:
        v = [float(a) for a in v]
    except TypeError:
        v = [float(v)] * 3
    if len(v) != 3:
        raise ValueError("%s must be one number or three" % name)
    return v


def _channel_single(v, name):
    """A grey call's `mean` or `std`: one number, or a sequence of one."""
    try:
        v = list(v)
    except TypeError:
        return float(v)
    if len(v) != 1:
        raise ValueError("%s must be one number for mode \"L\"" % name)
    return float(v[0])


def _resize_plan(planes_list, infos, size, crop_infos, filt, layout="NHWC", colors=None, orientations=None, views=None, replicates=None,
                 dtype=None, flips=None):
    """What the batched resize wrappers share ahead of a launch. The arguments are checked before a device or `infos` is
    touched: the filter, the layout, the dtype (None: a uint8 RGB call), then that every per-image list has one entry per
    image. Returns (sizer, call, lead, dims, keep): the scratch-size function and the uint8 entry point paired with it --
    jpeggpu_ext_resize_scratch_size / jpeggpu_ext_resize_to_rgb, their _cs forms with `colors`, their _oriented forms with
    `orientations`; with `views` jpeggpu_ext_resize_view_scratch_size / jpeggpu_ext_resize_view_to_tensor --, the arrays both
    take first, (n, w, h, filter) that follow them, and what must outlive the call."""
    if filt not in FILTERS:
        raise ValueError("filter %r is not one of %s" % (filt, ", ".join(FILTERS)))
    if layout not in LAYOUTS:
        raise ValueError("layout %r is not one of %s" % (layout, ", ".join(LAYOUTS)))
    if dtype is not None and dtype not in TENSOR_TYPES:
        raise ValueError("dtype %r is not one of %s" % (dtype, ", ".join(TENSOR_TYPE_NAMES)))
    n = len(planes_list)
    for name, v in (("infos", infos), ("views", views), ("crop_infos", crop_infos), ("colors", colors), ("orientations", orientations),
                    ("replicates", replicates), ("flips", flips)):
        if v is not None and len(v) != n:
            raise ValueError("%s must have one entry per image" % name)
    h, w = _size_hw(size)
    items, keep = _resize_items(planes_list, infos, crop_infos)
    if orientations is not None and views is None:
        colors = _item_colors(colors, infos)  # (the oriented calls take no NULL for the colours)
    cs = _color_array(colors, n) if colors is not None else None
    os_ = _color_array(orientations, n) if orientations is not None else None
    if views is not None:
        vs = (ResizeView * n)(*[_view_struct(views[i], replicates[i] if replicates is not None else False) for i in range(n)])
        sizer, call, lead = "jpeggpu_ext_resize_view_scratch_size", "jpeggpu_ext_resize_view_to_tensor", (items, cs, os_, vs)
    else:
        form = "_oriented" if os_ is not None else "_cs" if cs is not None else ""
        sizer, call = "jpeggpu_ext_resize_scratch_size" + form, "jpeggpu_ext_resize_to_rgb" + form
        lead = tuple(a for a in (items, cs, os_) if a is not None)  # (each form takes the arrays it is named for)
    return sizer, call, lead, (n, w, h, FILTERS[filt]), keep


def _resize(planes_list, infos, size, crop_infos, filt, layout, colors=None, orientations=None, views=None, replicates=None, tensor=None,
            out=None, gray=False):
    """The one launch path of the batched resize calls, on torch's current stream. `tensor`: None -- the uint8 RGB call
    _resize_plan names -- or (dtype, mean, std, flips): jpeggpu_ext_resize_to_tensor (with `views`
    jpeggpu_ext_resize_view_to_tensor), whose scratch is the uint8 call's, by the arguments given. `gray` (with `tensor`): one
    channel -- jpeggpu_ext_resize_view_to_gray_tensor and its own scratch size, `views` or not; `mean` and `std` are one number."""
    import torch

    dtype, mean, std, flips = tensor if tensor is not None else (None, None, None, None)
    if gray:
        mean, std = (None if v is None else _channel_single(v, name) for v, name in ((mean, "mean"), (std, "std")))
    sizer, call, lead, dims, _keep = _resize_plan(planes_list, infos, size, crop_infos, filt, layout, colors, orientations, views, replicates,
                                                  dtype, flips)
    n, w, h, _ = dims
    spec, args = (), lead  # (the uint8 and the view calls take the arrays their sizer takes)
    if tensor is not None:
        ts = TensorSpec()
        ts.type = TENSOR_TYPES[dtype]
        ts.mean[:] = _channel_triple(mean, 0.0, "mean")
        ts.std[:] = _channel_triple(std, 1.0, "std")
        if flips is not None:
            flip_bytes = (C.c_ubyte * n)(*[1 if f else 0 for f in flips])
            ts.flips = C.cast(flip_bytes, C.POINTER(C.c_ubyte))
        spec = (C.byref(ts),)
        if gray:  # (items, colours or NULL, orientations or NULL, views or NULL) for the call and its sizer alike
            sizer, call = "jpeggpu_ext_resize_view_to_gray_scratch_size", "jpeggpu_ext_resize_view_to_gray_tensor"
            _newer_symbol(call)
            lead = args = lead if views is not None else (lead + (None, None))[:3] + (None,)
        elif views is None:
            call, args = "jpeggpu_ext_resize_to_tensor", (lead + (None, None))[:3]  # (items, colours or NULL, orientations or NULL)
    else:
        dtype = torch.uint8
    device = planes_list[0][0].device
    chans = 1 if gray else 3
    shape = (n, h, w, chans) if layout == "NHWC" else (n, chans, h, w)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s tensor of shape %s" % ("uint8" if tensor is None else dtype, shape))
    need = getattr(lib(), sizer)(*lead, *dims)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    _check(getattr(lib(), call)(*args, *dims, LAYOUTS[layout], *spec, out.data_ptr(), scratch.data_ptr(), need,
                                torch.cuda.current_stream(device).cuda_stream), call)
    # the scratch tensor is freed by torch's caching allocator in stream order: it is not reused before the launches ran
    return out


def resize_scratch_size(planes_list, infos, size, crop_infos=None, filt="bilinear", colors=None, orientations=None):
    """jpeggpu_ext_resize_scratch_size of these items (0 if the call would refuse them); with `colors` (one ColorSpace
    per item) jpeggpu_ext_resize_scratch_size_cs; with `orientations` jpeggpu_ext_resize_scratch_size_oriented."""
    sizer, _, lead, dims, _keep = _resize_plan(planes_list, infos, size, crop_infos, filt, colors=colors, orientations=orientations)
    return getattr(lib(), sizer)(*lead, *dims)


def resize_to_rgb(planes_list, infos, size, crop_infos=None, filt="bilinear", layout="NHWC", out=None, colors=None, orientations=None):
    """jpeggpu_ext_resize_to_rgb on torch's current stream: every decoded image i
    (planes_list[i], infos[i], and crop_infos[i] from a cropped decode, or None for the whole image) resampled to `size`
    (int: square; (h, w)) with Pillow's BILINEAR or BICUBIC arithmetic. Returns a uint8 tensor of n x h x w x 3 ("NHWC")
    or n x 3 x h x w ("NCHW"), `out` if given (contiguous, of that shape). `colors`: each image's ColorSpace
    (Decoder.color_space; jpeggpu_ext_resize_to_rgb_cs -- a call may mix grey, YCbCr, RGB, CMYK and YCCK items); None: grey
    or YCbCr by the number of components. `orientations`: each image's EXIF orientation 1..8
    (jpeggpu_ext_resize_to_rgb_oriented): crop_infos are the STORED rectangles (orient_rect), and the result is the
    DISPLAYED rectangle resized, as Pillow resizes ImageOps.exif_transpose's image."""
    return _resize(planes_list, infos, size, crop_infos, filt, layout, colors, orientations, out=out)


def resize_to_tensor(planes_list, infos, size, crop_infos=None, filt="bilinear", layout="NHWC", colors=None, orientations=None, dtype=None,
                     mean=None, std=None, flips=None, out=None):
    """jpeggpu_ext_resize_to_tensor on torch's current stream: resize_to_rgb's result (same items, `size`, `filt`, `layout`,
    `colors`, `orientations`) written as a model's input, by the same launches but for the last. `dtype`: torch.float32 (the
    default), float16, bfloat16 or uint8. For the float types element u of channel c becomes ((float(u) / 255) - mean[c]) /
    std[c], each operation in float32 on its own -- bit for bit torchvision's ToTensor followed by Normalize(mean, std) on
    the CPU; `mean` / `std`: three numbers, one, or None (0 and 1: ToTensor alone); float16 and bfloat16 are that float32
    value converted once. uint8: the bytes (mean and std are ignored). `flips`: one truth value per item -- where true,
    the item is flipped left to right after the resize (torch.flip over the width, RandomHorizontalFlip with the caller's
    draws); None: no item. Returns a tensor of `dtype`, n x h x w x 3 ("NHWC") or n x 3 x h x w ("NCHW"); `out` if given
    (contiguous, of that shape and dtype)."""
    import torch

    return _resize(planes_list, infos, size, crop_infos, filt, layout, colors, orientations,
                   tensor=(torch.float32 if dtype is None else dtype, mean, std, flips), out=out)


def resize_to_gray(planes_list, infos, size, crop_infos=None, filt="bilinear", layout="NHWC", colors=None, orientations=None, views=None,
                   replicates=None, dtype=None, mean=None, std=None, flips=None, out=None):
    """jpeggpu_ext_resize_view_to_gray_tensor on torch's current stream: resize_to_tensor (or, with `views`,
    resize_views_to_tensor) for ONE channel -- the grey of every item (planes_to_gray; of a luma-only decode plane 0 alone)
    resampled with Pillow's arithmetic on an "L" image. Returns n x h x w x 1 ("NHWC") or n x 1 x h x w ("NCHW") of `dtype`
    (uint8 unless `dtype`, `mean` or `std` says otherwise); `mean` and `std` are one number each."""
    import torch

    if dtype is None:
        dtype = torch.uint8 if mean is None and std is None else torch.float32
    return _resize(planes_list, infos, size, crop_infos, filt, layout, colors, orientations, views, replicates, (dtype, mean, std, flips), out,
                   gray=True)


class BatchDecode:
    """The front half of every batched pipeline: a list of JPEGs decoded to planes by ONE jpeggpu_ext_decode_batch call on
    torch's current stream of `device`. Construction gives every file its Decoder with the settings below, parses its
    header, allocates its planes and its 256-aligned tmp buffer and enqueues its transfer at once (the copies overlap the
    parsing of the files behind it); then it creates the Batch for the summed num_scans with its scratch. decode() enqueues
    the one batch call; transfer() enqueues the copies again, for a caller that decodes repeatedly. Nothing synchronises.
    close() cleans up the decoders and destroys the batch (again: no effect), after which decode() and transfer() raise a
    RuntimeError and only the planes and records remain of use; `with` closes, and a construction that fails part-way
    closes what it made before the exception leaves. An empty `datas` is refused by jpeggpu_ext_batch_create
    (JpegGpuError, INVALID_ARGUMENT).

    `hint`: Decoder.set_batch_hint (default: the number of files). `idct`: "islow" (libjpeg-turbo's) or "reference".
    `progressive`: progressive files are taken. `scales[i]` in 1, 2, 4, 8 (default 1) with `scale_mode` ("libjpeg", or
    "uniform") where the scale is not 1. `crops[i]`: the STORED rectangle (x, y, w, h) at the scale to decode, or None for
    the whole image. `crop_hooks[i]`: a function for the rectangles that depend on the header -- the file is parsed once
    for it, hook(i, decoder, stored_w, stored_h) returns the stored rectangle or None (in place of crops[i]), and the
    header is parsed again with it; None: no first parse.

    Per file, in order: `decoders`, `planes` (lists of uint8 tensors), `infos`, `crop_infos` (None where no rectangle was
    set), `colors`, `orientations` (the file's own EXIF orientation), `replicates` (where libjpeg replicates instead of
    fancy upsampling) and `tmps`; `transferred_bytes` is what one round of transfers copies, `batch` the Batch.
    `coefficients_only`: no planes are allocated (`planes[i]` is empty) and the batch stops in front of the IDCT stage
    (Batch.set_coefficients_only): the front half of transcode_jpeg. `luma_only`: a truth value for all files or one per
    file -- Decoder.set_luma_only; of a YCbCr file only plane 0 is allocated and decoded (`planes[i]` has one entry).
    `device_scan`: a truth value for all files or one per file -- Decoder.set_device_scan(True): the device finds the
    file's restart markers. `truncated`: Decoder.set_truncated for every file -- files that end early are decoded as Pillow
    does with ImageFile.LOAD_TRUNCATED_IMAGES, whole ones as ever, and `truncated` (the attribute) is then the list of
    per-file flags: True where the file ended without its EOI (Decoder.truncated), so a loader can count or log them;
    progressive files are NOT_SUPPORTED under the flag. `subseq_bytes`: None (chosen per file), or 32, 64, 128 or 256 for
    all files or one per file (Decoder's `subseq_bytes`: what tests fix)."""

    def __init__(self, datas, device="cuda:0", hint=None, idct="islow", progressive=True, scales=None, scale_mode="libjpeg", crops=None,
                 crop_hooks=None, coefficients_only=False, luma_only=False, device_scan=False, truncated=False, subseq_bytes=None):
        import torch

        dev = torch.device(device)
        self._stream = torch.cuda.current_stream(dev).cuda_stream
        self.decoders, self.planes, self.infos, self.crop_infos, self.tmps, self._entries = [], [], [], [], [], []
        self.colors, self.orientations, self.replicates, self.truncated = [], [], [], []
        self.transferred_bytes, self.batch = 0, None
        try:
            scans = 0
            for i, data in enumerate(datas):
                dec = Decoder(subseq_bytes[i] if isinstance(subseq_bytes, (list, tuple)) else subseq_bytes)
                self.decoders.append(dec)
                dec.set_batch_hint(len(datas) if hint is None else hint)
                dec.set_idct(idct)
                dec.set_progressive(progressive)
                if truncated:
                    dec.set_truncated(True)
                luma = bool(luma_only[i] if isinstance(luma_only, (list, tuple)) else luma_only)
                if luma:
                    dec.set_luma_only(True)
                if device_scan[i] if isinstance(device_scan, (list, tuple)) else device_scan:
                    dec.set_device_scan(True)
                scale = 1 if scales is None else scales[i]
                if scale != 1:
                    dec.set_scale(scale)
                    dec.set_scale_mode(scale_mode)
                crop = crops[i] if crops is not None else None
                if crop_hooks is not None and crop_hooks[i] is not None:
                    crop = crop_hooks[i](i, dec, *_frame_size(dec.parse_header(data)))
                if crop is not None:
                    dec.set_crop(*crop)
                info = dec.parse_header(data)
                lay = dec.layout()
                scans += lay.num_scans
                self.transferred_bytes += lay.transferred_bytes
                nb = dec.get_buffer_size()
                tmp = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
                base = _align256(tmp.data_ptr())
                ncomp = 1 if luma and dec.color_space() == ColorSpace.YCBCR else info.num_components
                planes = [] if coefficients_only else [torch.empty((info.sizes_y[c], info.sizes_x[c]), dtype=torch.uint8, device=dev)
                                                       for c in range(ncomp)]
                dec.transfer(base, nb, self._stream)
                self.tmps.append(tmp)
                self._entries.append((dec, [p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, nb))
                self.planes.append(planes)
                self.infos.append(info)
                self.crop_infos.append(dec.crop_info() if crop is not None else None)
                self.colors.append(dec.color_space())
                self.orientations.append(dec.orientation())
                self.replicates.append(_needs_replication(info, scale))
                self.truncated.append(bool(truncated and dec.truncated().truncated))
            self.batch = Batch(scans)
            if coefficients_only:
                self.batch.set_coefficients_only(True)
            self._scratch = torch.empty(self.batch.scratch_size, dtype=torch.uint8, device=dev)
            self.batch.set_items(self._entries)
        except BaseException:
            self.close()
            raise

    def _open(self):
        if not self.batch._h:
            raise RuntimeError("this BatchDecode is closed")

    def transfer(self):
        self._open()
        for dec, _, _, base, nb in self._entries:
            dec.transfer(base, nb, self._stream)

    def decode(self):
        self._open()
        self.batch.decode(self._scratch.data_ptr(), self._stream)

    def close(self):
        if self.batch is not None:
            self.batch.destroy()
        for dec in self.decoders:
            dec.cleanup()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _displayed_crops(crops):
    """BatchDecode's crop_hooks for crops given in DISPLAYED coordinates: orient_rect by the file's orientation."""
    return [None if crop is None else lambda i, dec, w, h, crop=crop: orient_rect(dec.orientation(), w, h, crop) for crop in crops]


def _per_image_args(n, crops, scales):
    """The pipelines' `crops` and `scales` as lists of n entries."""
    crops = [None] * n if crops is None else list(crops)
    if len(crops) != n:
        raise ValueError("crops must have one entry per image")
    scales = [1] * n if scales is None else [int(s) for s in scales]
    if len(scales) != n or any(s not in (1, 2, 4, 8) for s in scales):
        raise ValueError("scales must have one entry of 1, 2, 4 or 8 per image")
    return crops, scales


def decode_resized(datas, size, crops=None, filt="bilinear", layout="NHWC", device="cuda:0", scales=None, exif_transpose=False,
                   dtype=None, mean=None, std=None, flips=None, mode="RGB", truncated=False):
    """A training pipeline's decode: every JPEG of `datas` (of any colour model: decode_to_rgb) decoded with libjpeg-turbo's
    arithmetic (ISLOW IDCT, fancy upsampling), only the rectangle crops[i] = (x, y, w, h) of it (None: the whole image), in ONE jpeggpu_ext_decode_batch
    call, then resized to `size` (int: square; (h, w)) with Pillow's BILINEAR or BICUBIC arithmetic by one
    jpeggpu_ext_resize_to_rgb call. Returns an n x h x w x 3 ("NHWC") or n x 3 x h x w ("NCHW") uint8 tensor equal to
    Pillow's Image.open(f).convert("RGB").crop((x, y, x + w, y + h)).resize((w_out, h_out), filter) of every image
    ("RandomResizedCrop equal to torchvision on Pillow"). `scales[i]` in 1, 2, 4, 8 (default 1): image i is
    decoded at that scale the way libjpeg-turbo does (decode_to_rgb's `scale`; draft_scale gives Pillow's choice), crops[i]
    is in pixels of the image at that scale, and the result equals im.draft("RGB", ...); im.convert("RGB").crop(...)
    .resize(...). A ValueError for an image that libjpeg would upsample by replication (1/8 with subsampling left, e.g.
    4:2:2): the batched resize does not reproduce that; use scale 4 for it (raised before the decode call, once every
    header is parsed and every transfer enqueued). `exif_transpose`: every file's EXIF
    orientation is applied -- crops[i] is in DISPLAYED pixels at the scale, and the result equals
    ImageOps.exif_transpose(im) put after draft() and before convert("RGB"), crop() and resize().
    `dtype`, `mean`, `std`, `flips`: with any of them the second step is one jpeggpu_ext_resize_to_tensor call
    (resize_to_tensor) and the result is a training loader's whole transform -- RandomResizedCrop + RandomHorizontalFlip +
    ToTensor + Normalize(mean, std), with the draws (crops[i], flips[i]) supplied by the caller -- as a tensor of `dtype`:
    torch.float32 if `mean` or `std` is given, torch.uint8 (the bytes, flipped where asked) if only `flips` is; float16 and
    bfloat16 are the float32 result converted once. With all four None the call is what it was, call for call. An empty
    `datas` is refused where the batch is created: a JpegGpuError from jpeggpu_ext_batch_create (INVALID_ARGUMENT).
    `mode`: "RGB", or "L" -- one channel, n x h x w x 1 or n x 1 x h x w: the files are decoded luma-only (decode_to_gray)
    and resized by one jpeggpu_ext_resize_view_to_gray_tensor call, equal to im.draft("L", ...) in place of draft("RGB") and
    convert("RGB") above; `mean` and `std` are then one number each (or 1-tuples). `truncated`: files that end early are
    decoded as Pillow does with ImageFile.LOAD_TRUNCATED_IMAGES (BatchDecode)."""
    import torch

    if mode not in ("RGB", "L"):
        raise ValueError("mode %r is not one of RGB, L" % (mode,))
    crops, scales = _per_image_args(len(datas), crops, scales)
    crop_args = dict(crop_hooks=_displayed_crops(crops)) if exif_transpose else dict(crops=crops)
    with BatchDecode(datas, device, scales=scales, luma_only=mode == "L", truncated=truncated, **crop_args) as bd:
        replicates = bd.replicates
        if mode == "L":  # only component 0 is upsampled, and nearly always it has the largest factors: nothing to replicate
            replicates = [r and (i.subsampling.x[0], i.subsampling.y[0]) != _max_factors(i) for r, i in zip(replicates, bd.infos)]
        if any(replicates):
            i = replicates.index(True)
            info = bd.infos[i]
            raise ValueError("image %d at scale 1/8 has subsampling left (%s x %s): libjpeg replicates there, which the "
                             "batched resize does not reproduce" % (i, list(info.subsampling.x[:info.num_components]),
                                                                  list(info.subsampling.y[:info.num_components])))
        bd.decode()
        orients = bd.orientations if exif_transpose else None
        if mode == "L":
            out = resize_to_gray(bd.planes, bd.infos, size, bd.crop_infos, filt, layout, colors=bd.colors, orientations=orients, dtype=dtype,
                                 mean=mean, std=std, flips=flips)
        elif dtype is None and mean is None and std is None and flips is None:
            out = resize_to_rgb(bd.planes, bd.infos, size, bd.crop_infos, filt, layout, colors=bd.colors, orientations=orients)
        else:
            if dtype is None:
                dtype = torch.uint8 if mean is None and std is None else torch.float32
            out = resize_to_tensor(bd.planes, bd.infos, size, bd.crop_infos, filt, layout, colors=bd.colors, orientations=orients,
                                   dtype=dtype, mean=mean, std=std, flips=flips)
        torch.cuda.synchronize(torch.device(device))
        return out


def resized_size(w, h, size):
    """torchvision's Resize(size) of a w x h image, as (resized_w, resized_h): an int makes the shorter side `size` and the
    longer one int(size * long / short) (true division, truncated); a pair is (height, width) and used as given. Pure
    Python. (500, 375, 256) -> (341, 256); (640, 227, 256) -> (721, 256)."""
    if not isinstance(size, int):
        rh, rw = size
        return int(rw), int(rh)
    if w < 1 or h < 1 or size < 1:
        raise ValueError("sizes must be positive")
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (size, new_long) if w <= h else (new_long, size)


def center_crop_window(rw, rh, crop):
    """torchvision's CenterCrop(crop) of an rw x rh image, as the window's corner (x, y) in it (`crop`: int, or (height,
    width)): int(round((rw - cw) / 2.0)) -- Python's round, half to even -- where the image is at least the crop; where it
    is smaller it is padded with (cw - rw) // 2 zero columns on the left (and (cw - rw + 1) // 2 on the right), so
    x = -((cw - rw) // 2). The same for y. Pure Python."""
    ch, cw = _size_hw(crop)

    def corner(r, c):
        return int(round((r - c) / 2.0)) if c <= r else -((c - r) // 2)

    return corner(rw, cw), corner(rh, ch)


def _view_struct(view, replicate=False):
    rw, rh, x, y = (int(v) for v in view)
    return ResizeView(rw, rh, x, y, int(bool(replicate)))


def resize_view_rect(w, h, view, out_size, filt="bilinear", orientation=1):
    """jpeggpu_ext_resize_view_rect (host only): the STORED rectangle (x, y, w, h) of a stored w x h image whose pixels the
    window `view` = (resized_w, resized_h, x, y) of `out_size` (int: square; (h, w)) reads -- the view is in displayed
    pixels of `orientation`. What Decoder.set_crop takes so that only that part is decoded."""
    if filt not in FILTERS:
        raise ValueError("filter %r is not one of %s" % (filt, ", ".join(FILTERS)))
    oh, ow = _size_hw(out_size)
    v = [C.c_int() for _ in range(4)]
    vs = _view_struct(view)
    _check(lib().jpeggpu_ext_resize_view_rect(int(w), int(h), int(orientation), C.byref(vs), ow, oh, FILTERS[filt], *[C.byref(a) for a in v]),
           "jpeggpu_ext_resize_view_rect")
    return tuple(a.value for a in v)


def resize_view_weights(in_size, resized, x0, count_out, origin=0, filt="bilinear"):
    """jpeggpu_ext_resize_view_weights (host only): the table the kernels get for output coordinates x0 .. x0 + count_out - 1
    of in_size -> resized, `first` relative to `origin`, as numpy int32 (first[count_out], count[count_out],
    weights[count_out, max_taps]); coordinates outside [0, resized) have count 0."""
    import numpy as np

    if filt not in FILTERS:
        raise ValueError("filter %r is not one of %s" % (filt, ", ".join(FILTERS)))
    k = resize_max_taps(in_size, resized, filt)
    m = max(int(count_out), 1)
    first, count, w = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, k), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _check(lib().jpeggpu_ext_resize_view_weights(int(in_size), int(resized), int(x0), int(count_out), int(origin), FILTERS[filt], ptr(first),
                                                 ptr(count), ptr(w), k), "jpeggpu_ext_resize_view_weights")
    return first, count, w


def resize_views_to_tensor(planes_list, infos, views, size, crop_infos=None, filt="bilinear", layout="NHWC", colors=None, orientations=None,
                           replicates=None, dtype=None, mean=None, std=None, flips=None, out=None):
    """jpeggpu_ext_resize_view_to_tensor on torch's current stream: resize_to_tensor where image i contributes not its
    rectangle resized to `size` but the `size` window at (x, y) of the resize of its WHOLE displayed image to resized_w x
    resized_h -- views[i] = (resized_w, resized_h, x, y), from resized_size and center_crop_window: torchvision's Resize +
    CenterCrop on Pillow. Pixels of the window outside the resized image are byte 0 (normalised like any byte).
    crop_infos[i], if given, must hold what resize_view_rect returns for the view. `replicates`: where libjpeg replicates
    instead of fancy upsampling (1/8 in the libjpeg scale mode with subsampling left); None: nowhere. `dtype` defaults to
    torch.uint8 unless `mean` or `std` is given (then float32); everything else as in resize_to_tensor."""
    import torch

    if dtype is None:
        dtype = torch.uint8 if mean is None and std is None else torch.float32
    return _resize(planes_list, infos, size, crop_infos, filt, layout, colors, orientations, views, replicates, (dtype, mean, std, flips), out)


def decode_center_cropped(datas, resize=256, crop=224, filt="bilinear", layout="NHWC", device="cuda:0", scales=None, exif_transpose=False,
                          dtype=None, mean=None, std=None, mode="RGB", truncated=False):
    """An evaluation pipeline's decode: torchvision's Resize(resize) + CenterCrop(crop) (+ ToTensor + Normalize with `dtype`,
    `mean`, `std` as in decode_resized) of every JPEG of `datas`, equal to Pillow's
    Image.open(f).convert("RGB").resize((rw, rh), filter) cropped (or zero-padded, where the resized image is smaller than
    the crop) to the centre window, with (rw, rh) = resized_size and the window from center_crop_window -- in ONE
    jpeggpu_ext_decode_batch call and ONE jpeggpu_ext_resize_view_to_tensor call, however the images' sizes differ. Only the
    rectangle of each file that the window's taps read is decoded (resize_view_rect). `resize`: int (the shorter side) or
    (h, w); `crop`: int or (h, w). `scales[i]` in 1, 2, 4, 8: image i is decoded at that scale as libjpeg-turbo does
    (draft_scale gives Pillow's choice) and the resized size is computed from its size at that scale; 1/8 with subsampling
    left is taken (libjpeg's replication). `exif_transpose`: the transform runs on the displayed image
    (ImageOps.exif_transpose after draft()). Files of every colour model and progressive files are taken. Returns n x ch x
    cw x 3 ("NHWC") or n x 3 x ch x cw ("NCHW"), uint8 unless `dtype`, `mean` or `std` says otherwise. `mode`: "RGB", or "L" as in
    decode_resized: one channel of luma-only decodes, `mean` and `std` one number each."""
    import torch

    if mode not in ("RGB", "L"):
        raise ValueError("mode %r is not one of RGB, L" % (mode,))
    n = len(datas)
    _, scales = _per_image_args(n, None, scales)
    if n == 0:
        raise ValueError("datas is empty")
    ch, cw = _size_hw(crop)
    views = []

    def window(i, dec, w0, h0):  # from the first parse: the size at the scale and the orientation
        o = dec.orientation() if exif_transpose else 1
        rw, rh = resized_size(*orient_size(o, w0, h0), resize)
        views.append((rw, rh) + center_crop_window(rw, rh, (ch, cw)))  # (the hooks run in the files' order)
        return resize_view_rect(w0, h0, views[-1], (ch, cw), filt, o)

    with BatchDecode(datas, device, scales=scales, crop_hooks=[window] * n, luma_only=mode == "L", truncated=truncated) as bd:
        bd.decode()
        kw = dict(colors=bd.colors, orientations=bd.orientations if exif_transpose else [1] * n, replicates=bd.replicates, dtype=dtype,
                  mean=mean, std=std)
        if mode == "L":
            out = resize_to_gray(bd.planes, bd.infos, (ch, cw), bd.crop_infos, filt, layout, views=views, **kw)
        else:
            out = resize_views_to_tensor(bd.planes, bd.infos, views, (ch, cw), bd.crop_infos, filt, layout, **kw)
        torch.cuda.synchronize(torch.device(device))
        return out


def _thumbnail_request(size):
    """Pillow's (width, height) request after math.floor, each at least 1."""
    import math

    rw, rh = (int(math.floor(v)) for v in size)
    if rw < 1 or rh < 1:
        raise ValueError("a thumbnail's requested width and height must be at least 1")
    return rw, rh


def thumbnail_plan(width, height, size, resample="bicubic", reducing_gap=2.0) -> Thumbnail:
    """jpeggpu_ext_thumbnail_plan (host only, pure): what Pillow's im.thumbnail(size, resample, reducing_gap) does to a
    width x height JPEG -- the scale to decode at, the decoded size, Image.reduce's factors and the reduced size, the box
    the resize covers (as binary32), the thumbnail's size, and whether the decode already is the thumbnail. `size`: Pillow's
    (width, height) request; `reducing_gap`: None, or at least 1. A JpegGpuError (NOT_SUPPORTED) for an image more than 100
    times taller than wide at the resize, which Pillow resizes in the other order."""
    if resample not in FILTERS:
        raise ValueError("filter %r is not one of %s" % (resample, ", ".join(FILTERS)))
    rw, rh = _thumbnail_request(size)
    plan = Thumbnail()
    _check(_newer_symbol("jpeggpu_ext_thumbnail_plan")(int(width), int(height), rw, rh, FILTERS[resample],
                                                       0.0 if reducing_gap is None else float(reducing_gap), C.byref(plan)),
           "jpeggpu_ext_thumbnail_plan")
    return plan


def resize_box_weights(in_size, extent, out_size, filt="bilinear"):
    """jpeggpu_ext_resize_box_weights (host only): resize_weights for `in_size` samples of which the resize covers `extent`
    (rounded to binary32), as numpy int32 (first[out], count[out], weights[out, max_taps])."""
    import math

    import numpy as np

    if filt not in FILTERS:
        raise ValueError("filter %r is not one of %s" % (filt, ", ".join(FILTERS)))
    extent = C.c_float(extent).value
    k = 2 * int(math.ceil({"bilinear": 1.0, "bicubic": 2.0}[filt] * max(extent / out_size, 1.0))) + 1 if extent > 0 and out_size > 0 else 1
    first, count = np.zeros(max(out_size, 1), np.int32), np.zeros(max(out_size, 1), np.int32)
    w = np.zeros((max(out_size, 1), k), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _check(_newer_symbol("jpeggpu_ext_resize_box_weights")(int(in_size), extent, int(out_size), FILTERS[filt], ptr(first), ptr(count), ptr(w), k),
           "jpeggpu_ext_resize_box_weights")
    return first, count, w


def thumbnails_to_rgb(planes_list, infos, plans, canvas, filt="bicubic", colors=None, out=None):
    """jpeggpu_ext_thumbnail_to_rgb on torch's current stream: the thumbnails of decoded images -- planes_list[i] and infos[i]
    of a whole-image decode at plans[i].scale, plans[i] from thumbnail_plan (with `replicate` set where libjpeg replicates
    the chroma), colors[i] the ColorSpace (None: by the component count). `canvas`: (height, width), at least every plan's
    out_h x out_w. Returns the n x height x width x 3 uint8 canvas (`out` if given): thumbnail i in the top-left corner of
    slot i, zeros around it."""
    import torch

    if filt not in FILTERS:
        raise ValueError("filter %r is not one of %s" % (filt, ", ".join(FILTERS)))
    n = len(planes_list)
    for name, v in (("infos", infos), ("plans", plans), ("colors", colors)):
        if v is not None and len(v) != n:
            raise ValueError("%s must have one entry per image" % name)
    ch, cw = _size_hw(canvas)
    items, _keep = _resize_items(planes_list, infos, None)
    cs = _color_array(colors, n) if colors is not None else None
    ps = (Thumbnail * n)(*plans)
    device = planes_list[0][0].device
    shape = (n, ch, cw, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=device)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of shape %s" % (shape,))
    need = _newer_symbol("jpeggpu_ext_thumbnail_scratch_size")(items, cs, ps, n, cw, ch, FILTERS[filt])
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    _check(lib().jpeggpu_ext_thumbnail_to_rgb(items, cs, ps, n, cw, ch, FILTERS[filt], out.data_ptr(), scratch.data_ptr(), need,
                                              torch.cuda.current_stream(device).cuda_stream), "jpeggpu_ext_thumbnail_to_rgb")
    # the scratch tensor is freed by torch's caching allocator in stream order: it is not reused before the launches ran
    return out


def _exif_transposed(view, orientation):
    """ImageOps.exif_transpose of a small (h, w[, 3]) tensor, with torch: the eight orientations as flips and a transpose."""
    o = int(orientation)
    if o >= 5:  # 5: transpose, 6: rotate 270, 7: transverse, 8: rotate 90 -- a transpose, then the flips of 1, 2, 3, 4
        view = view.transpose(0, 1)
    flips = {1: (), 2: (1,), 3: (0, 1), 4: (0,), 5: (), 6: (1,), 7: (0, 1), 8: (0,)}[o]
    return view.flip(flips) if flips else view


def _header_frame_size(data):
    """(width, height) of a JPEG from its frame header, without parsing anything else: the thumbnail plans come before the
    decoders are set up, because the scale to decode at depends on the size. Bytes are walked marker by marker up to the
    frame header; any other buffer, and a file this walk does not understand, goes through a Decoder's parse_header, which
    raises what the file deserves."""
    if isinstance(data, (bytes, bytearray)) and data[:2] == b"\xff\xd8":
        i, n = 2, len(data)
        while i + 4 <= n and data[i] == 0xFF:
            m = data[i + 1]
            if m == 0xFF:  # a fill byte
                i += 1
            elif m == 0x01 or 0xD0 <= m <= 0xD8:  # markers without a segment
                i += 2
            elif m == 0xDA or m == 0xD9:
                break
            else:
                if m in (0xC0, 0xC1, 0xC2) and i + 9 <= n:
                    w, h = data[i + 7] << 8 | data[i + 8], data[i + 5] << 8 | data[i + 6]
                    if w and h:
                        return w, h
                    break
                i += 2 + (data[i + 2] << 8 | data[i + 3])
    probe = Decoder()
    try:
        probe.set_progressive(True)
        return _frame_size(probe.parse_header(data))
    finally:
        probe.cleanup()


def decode_thumbnails(datas, size, resample="bicubic", reducing_gap=2.0, exif_transpose=False, device="cuda:0", truncated=False):
    """Pillow's im.thumbnail(size, resample, reducing_gap) of every JPEG of `datas`, on the GPU: one BatchDecode at the
    scales draft() would pick (thumbnail_plan), then ONE jpeggpu_ext_thumbnail_to_rgb call -- Image.reduce's box averages and
    the resize from Pillow's fractional box -- with nothing on the host in between. `size`: Pillow's (width, height) request;
    `resample`: "bilinear" or "bicubic"; `reducing_gap`: None, or at least 1. Returns a list of uint8 tensors, views of one
    canvas: h x w x 3, or h x w for a grey file, each equal to np.asarray(im) after im.thumbnail(...). `exif_transpose`: each
    view is turned as ImageOps.exif_transpose turns the thumbnail (applied AFTER the thumbnail, with torch, on the small
    tensor). CMYK and YCCK files, and images more than 100 times taller than wide at the resize, raise a JpegGpuError
    (NOT_SUPPORTED)."""
    import torch

    if resample not in FILTERS:
        raise ValueError("filter %r is not one of %s" % (resample, ", ".join(FILTERS)))
    _thumbnail_request(size)
    n = len(datas)
    if n == 0:
        raise ValueError("datas is empty")
    plans = [thumbnail_plan(*_header_frame_size(data), size, resample, reducing_gap) for data in datas]
    with BatchDecode(datas, device, scales=[p.scale for p in plans], truncated=truncated) as bd:
        for p, rep in zip(plans, bd.replicates):
            p.replicate = int(bool(rep))
        bd.decode()
        canvas = thumbnails_to_rgb(bd.planes, bd.infos, plans, (max(p.out_h for p in plans), max(p.out_w for p in plans)), resample, bd.colors)
        torch.cuda.synchronize(torch.device(device))
        views = []
        for i, p in enumerate(plans):
            v = canvas[i, :p.out_h, :p.out_w] if bd.infos[i].num_components != 1 else canvas[i, :p.out_h, :p.out_w, 0]
            views.append(_exif_transposed(v, bd.orientations[i]) if exif_transpose else v)
        return views


def thumbnail_jpeg(datas, size, resample="bicubic", reducing_gap=2.0, exif_transpose=False, device="cuda:0", quality=75, subsampling=None,
                   optimize=False, progressive=False, restart_interval=0, max_bytes=None, min_quality=1, truncated=False):
    """JPEG in, smaller JPEG out: decode_thumbnails' views encoded by encode_jpeg (one decode batch, one thumbnail call, one
    encode call; the pixels never visit the host). Returns a list of bytes: encode_jpeg's file of each thumbnail, which for a
    source without a COM segment is byte for byte what im.save(f, "JPEG", quality=..., ...) writes after
    im.thumbnail(size, resample, reducing_gap) (Pillow copies only the comment across). `subsampling` None is save()'s
    default: "4:2:0" for a colour file, and factors 1 x 1 in a grey file's frame header (which an explicit subsampling
    would change, in Pillow as here). `max_bytes` (one value or one per file): a size limit -- the encode step is then
    encode_jpeg_fit's search over min_quality..quality, and the function returns (files, qualities); progressive=True is
    not offered with it."""
    views = decode_thumbnails(datas, size, resample, reducing_gap, exif_transpose, device, truncated=truncated)
    if subsampling is None:
        subsampling = ["4:4:4" if v.dim() == 2 else "4:2:0" for v in views]
    if max_bytes is not None:
        if progressive:
            raise JpegGpuError(Status.NOT_SUPPORTED, "thumbnail_jpeg: max_bytes with progressive=True")
        return encode_jpeg_fit(views, max_bytes, quality=quality, min_quality=min_quality, subsampling=subsampling, restart_interval=restart_interval,
                               optimize=optimize)
    return encode_jpeg(views, quality=quality, subsampling=subsampling, restart_interval=restart_interval, optimize=optimize,
                       progressive=progressive)


def _align256(v):
    return (v + 255) // 256 * 256


def batch_to_rgb(planes_list, infos, crop_infos=None, colors=None, orientations=None, replicates=None, layout="HWC"):
    """jpeggpu_ext_batch_to_rgb on torch's current stream: every decoded image i (planes_list[i], infos[i], and
    crop_infos[i] from a cropped decode, or None for the whole image) converted to RGB at its own size -- one launch for all
    images of orientations 1..4 and one for all of 5..8, not one per image. `colors`: each image's ColorSpace (None: grey or
    YCbCr by the number of components); `orientations`: each image's EXIF orientation 1..8 (None: 1, the stored image;
    crop_infos are always STORED rectangles, orient_rect); `replicates`: where libjpeg replicates instead of fancy
    upsampling (None: nowhere). Returns a list of uint8 tensors, (oh, ow, 3) for "HWC" or (3, oh, ow) for "CHW", of the
    displayed rectangles: views into ONE allocation, each image starting on a multiple of 256 bytes, its rows unpadded."""
    import torch

    if layout not in IMAGE_LAYOUTS:
        raise ValueError("layout %r is not one of %s" % (layout, ", ".join(IMAGE_LAYOUTS)))
    n = len(planes_list)
    for name, v in (("infos", infos), ("crop_infos", crop_infos), ("colors", colors), ("orientations", orientations), ("replicates", replicates)):
        if v is not None and len(v) != n:
            raise ValueError("%s must have one entry per image" % name)
    if n == 0:
        return []
    device = planes_list[0][0].device
    colors = _item_colors(colors, infos)
    orientations = [1] * n if orientations is None else [int(o) for o in orientations]
    if any(not 1 <= o <= 8 for o in orientations):
        raise ValueError("orientations must be 1..8")
    items, _keep = _resize_items(planes_list, infos, crop_infos)  # info, crop and src are the resize item's
    sizes, offsets, total = [], [], 0
    for i in range(n):
        ci = crop_infos[i] if crop_infos is not None else None
        w, h = (ci.width, ci.height) if ci is not None else _frame_size(infos[i])
        sizes.append((h, w) if orientations[i] >= 5 else (w, h))
        offsets.append(total)
        total = _align256(total + 3 * w * h)
    out = torch.empty(total + 256, dtype=torch.uint8, device=device)
    start = _align256(out.data_ptr()) - out.data_ptr()  # torch's allocations are aligned far beyond this; kept for any allocator
    rgb = (RgbItem * n)()
    for i, (ow, oh) in enumerate(sizes):
        rgb[i].info, rgb[i].crop, rgb[i].src = items[i].info, items[i].crop, items[i].src
        rgb[i].color, rgb[i].orientation = int(colors[i]), orientations[i]
        rgb[i].replicate = int(bool(replicates[i])) if replicates is not None else 0
        rgb[i].dst = out.data_ptr() + start + offsets[i]
        rgb[i].dst_pitch = 3 * ow if layout == "HWC" else ow
        rgb[i].plane_stride = ow * oh
    need = lib().jpeggpu_ext_batch_rgb_scratch_size(n)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    _check(lib().jpeggpu_ext_batch_to_rgb(rgb, n, IMAGE_LAYOUTS[layout], scratch.data_ptr(), need, torch.cuda.current_stream(device).cuda_stream),
           "jpeggpu_ext_batch_to_rgb")
    # the scratch tensor is freed by torch's caching allocator in stream order: it is not reused before the launches ran
    views = []
    for (ow, oh), off in zip(sizes, offsets):
        flat = out[start + off:start + off + 3 * ow * oh]
        views.append(flat.view(oh, ow, 3) if layout == "HWC" else flat.view(3, oh, ow))
    return views


def decode_batch_to_rgb(datas, device="cuda:0", crops=None, scales=None, exif_transpose=False, layout="HWC", truncated=False, subseq_bytes=None,
                        hint=None):
    """A list of JPEGs in, a list of RGB tensors out, each at its own size (torchvision.io.decode_jpeg on a list; a validation
    loader): every file of `datas` (of any colour model, baseline or progressive) decoded with libjpeg-turbo's arithmetic
    in ONE jpeggpu_ext_decode_batch call and converted by ONE jpeggpu_ext_batch_to_rgb call, with one synchronise at the
    end. Element i equals decode_to_rgb(datas[i], crop=crops[i], scale=scales[i], exif_transpose=exif_transpose) -- (h, w,
    3) uint8 for "HWC"; for "CHW" that result after .permute(2, 0, 1), (3, h, w). `crops[i]`: (x, y, w, h) or None;
    `scales[i]` in 1, 2, 4, 8 (default 1), crops in pixels of the image at that scale; images libjpeg upsamples by
    replication (1/8 with subsampling left) are taken, unlike decode_resized. `exif_transpose`: every file's EXIF
    orientation is applied, crops[i] is in DISPLAYED pixels. The tensors are views into one allocation (batch_to_rgb). An
    empty list gives []."""
    import torch

    if layout not in IMAGE_LAYOUTS:
        raise ValueError("layout %r is not one of %s" % (layout, ", ".join(IMAGE_LAYOUTS)))
    n = len(datas)
    crops, scales = _per_image_args(n, crops, scales)
    if n == 0:
        return []
    crop_args = dict(crop_hooks=_displayed_crops(crops)) if exif_transpose else dict(crops=crops)
    with BatchDecode(datas, device, scales=scales, truncated=truncated, subseq_bytes=subseq_bytes, hint=hint, **crop_args) as bd:
        bd.decode()
        out = batch_to_rgb(bd.planes, bd.infos, bd.crop_infos, bd.colors, bd.orientations if exif_transpose else [1] * n, bd.replicates, layout)
        torch.cuda.synchronize(torch.device(device))
        return out


def batch_to_gray(planes_list, infos, crop_infos=None, colors=None, orientations=None, replicates=None):
    """jpeggpu_ext_batch_to_gray on torch's current stream: batch_to_rgb for one channel -- every decoded image i (of a
    luma-only decode plane 0 alone) as its (oh, ow) uint8 grey (planes_to_gray), at most two launches for the list. The
    tensors are views into ONE allocation, each image starting on a multiple of 256 bytes, its rows unpadded."""
    import torch

    n = len(planes_list)
    for name, v in (("infos", infos), ("crop_infos", crop_infos), ("colors", colors), ("orientations", orientations), ("replicates", replicates)):
        if v is not None and len(v) != n:
            raise ValueError("%s must have one entry per image" % name)
    if n == 0:
        return []
    device = planes_list[0][0].device
    colors = _item_colors(colors, infos)
    orientations = [1] * n if orientations is None else [int(o) for o in orientations]
    if any(not 1 <= o <= 8 for o in orientations):
        raise ValueError("orientations must be 1..8")
    items, _keep = _resize_items(planes_list, infos, crop_infos)  # info, crop and src are the resize item's
    sizes, offsets, total = [], [], 0
    for i in range(n):
        ci = crop_infos[i] if crop_infos is not None else None
        w, h = (ci.width, ci.height) if ci is not None else _frame_size(infos[i])
        sizes.append((h, w) if orientations[i] >= 5 else (w, h))
        offsets.append(total)
        total = _align256(total + w * h)
    out = torch.empty(total + 256, dtype=torch.uint8, device=device)
    start = _align256(out.data_ptr()) - out.data_ptr()
    it = (RgbItem * n)()
    for i, (ow, oh) in enumerate(sizes):
        it[i].info, it[i].crop, it[i].src = items[i].info, items[i].crop, items[i].src
        it[i].color, it[i].orientation = int(colors[i]), orientations[i]
        it[i].replicate = int(bool(replicates[i])) if replicates is not None else 0
        it[i].dst = out.data_ptr() + start + offsets[i]
        it[i].dst_pitch = ow
    need = _newer_symbol("jpeggpu_ext_batch_gray_scratch_size")(n)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    _check(_newer_symbol("jpeggpu_ext_batch_to_gray")(it, n, scratch.data_ptr(), need, torch.cuda.current_stream(device).cuda_stream),
           "jpeggpu_ext_batch_to_gray")
    # the scratch tensor is freed by torch's caching allocator in stream order: it is not reused before the launches ran
    return [out[start + off:start + off + ow * oh].view(oh, ow) for (ow, oh), off in zip(sizes, offsets)]


def decode_batch_to_gray(datas, device="cuda:0", crops=None, scales=None, exif_transpose=False, truncated=False):
    """A list of JPEGs in, a list of (h, w) uint8 grey tensors out, each at its own size: every file decoded luma-only in ONE
    jpeggpu_ext_decode_batch call and written by ONE jpeggpu_ext_batch_to_gray call, with one synchronise at the end. Element
    i equals decode_to_gray(datas[i], crop=crops[i], scale=scales[i], exif_transpose=exif_transpose); the arguments are
    decode_batch_to_rgb's. A CMYK or YCCK file raises JpegGpuError (NOT_SUPPORTED). An empty list gives []."""
    import torch

    n = len(datas)
    crops, scales = _per_image_args(n, crops, scales)
    if n == 0:
        return []
    crop_args = dict(crop_hooks=_displayed_crops(crops)) if exif_transpose else dict(crops=crops)
    with BatchDecode(datas, device, scales=scales, luma_only=True, truncated=truncated, **crop_args) as bd:
        bd.decode()
        out = batch_to_gray(bd.planes, bd.infos, bd.crop_infos, bd.colors, bd.orientations if exif_transpose else [1] * n, bd.replicates)
        torch.cuda.synchronize(torch.device(device))
        return out


def encode_item(width, height, channels=3, quality=75, subsampling="4:2:0", restart_interval=0, optimize=False, progressive=False):
    """A struct jpeggpu_ext_encode_item of this geometry without pointers: what encode_header and encode_bound need.
    `optimize`: Huffman tables made for the image (Pillow's optimize=True) instead of the Annex K tables. `progressive`:
    libjpeg's progressive script (Pillow's progressive=True), whose tables are always made for the image."""
    if subsampling not in SUBSAMPLINGS:
        raise ValueError("subsampling %r is not one of %s" % (subsampling, ", ".join(SUBSAMPLINGS)))
    it = EncodeItem()
    it.width, it.height, it.channels = int(width), int(height), int(channels)
    it.quality, it.subsampling, it.restart_interval = int(quality), SUBSAMPLINGS[subsampling], int(restart_interval)
    it.optimize = int(optimize)  # (2 stays 2: the library refuses it)
    it.progressive = int(progressive)
    return it


def encode_header(width, height, channels=3, quality=75, subsampling="4:2:0", restart_interval=0, optimize=False, progressive=False) -> bytes:
    """jpeggpu_ext_encode_header (host only): SOI up to the end of the scan header of the file encode_jpeg writes. With
    optimize=True or progressive=True it raises JpegGpuError (NOT_SUPPORTED): that header holds tables made from the pixels."""
    it = encode_item(width, height, channels, quality, subsampling, restart_interval, optimize, progressive)
    size = C.c_size_t(1024)
    buf = C.create_string_buffer(1024)
    _check(lib().jpeggpu_ext_encode_header(C.byref(it), buf, C.byref(size)), "jpeggpu_ext_encode_header")
    return buf.raw[:size.value]


def encode_bound(width, height, channels=3, quality=75, subsampling="4:2:0", restart_interval=0, optimize=False, progressive=False) -> int:
    """jpeggpu_ext_encode_bound (host only): the size no file of this geometry exceeds."""
    it = encode_item(width, height, channels, quality, subsampling, restart_interval, optimize, progressive)
    n = lib().jpeggpu_ext_encode_bound(C.byref(it))
    if n == 0:
        raise JpegGpuError(Status.INVALID_ARGUMENT, "jpeggpu_ext_encode_bound")
    return n


def _per_image(v, n, name):
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError("%s must be one value or one per image" % name)
        return list(v)
    return [v] * n


def _encode_items(images, quality, subsampling, restart_interval, layout, optimize=False, progressive=False):
    """The items of a call, without output slots: `images` a list of uint8 device tensors or one 4-D tensor."""
    import torch

    if layout not in IMAGE_LAYOUTS:
        raise ValueError("layout %r is not one of %s" % (layout, ", ".join(IMAGE_LAYOUTS)))
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError("a batch tensor must have 4 dimensions")
        images = list(images)
    images = list(images)
    n = len(images)
    qs, ss, rs = _per_image(quality, n, "quality"), _per_image(subsampling, n, "subsampling"), _per_image(restart_interval, n, "restart_interval")
    os_ = _per_image(optimize, n, "optimize")
    ps_ = _per_image(progressive, n, "progressive")
    items = (EncodeItem * max(n, 1))()
    for i, x in enumerate(images):
        if x.dtype != torch.uint8 or not x.is_cuda or x.dim() not in (2, 3):
            raise ValueError("image %d: a uint8 device tensor of 2 or 3 dimensions is expected" % i)
        if x.dim() == 2:
            h, w, ch, ps, cs = x.shape[0], x.shape[1], 1, x.stride(1), 0
            rp = x.stride(0)
        elif layout == "HWC":
            h, w, ch = x.shape
            rp, ps, cs = x.stride()
        else:
            ch, h, w = x.shape
            cs, rp, ps = x.stride()
        if ch not in (1, 3):
            raise ValueError("image %d: 1 or 3 channels are expected, not %d" % (i, ch))
        it = encode_item(w, h, ch, qs[i], ss[i], rs[i], os_[i], ps_[i])
        it.data, it.row_pitch, it.pixel_stride, it.channel_stride = x.data_ptr(), rp, ps, cs
        items[i] = it
    return images, items


def encode_into(images, outs, quality=75, subsampling="4:2:0", restart_interval=0, layout="HWC", optimize=False, progressive=False):
    """jpeggpu_ext_encode_batch on torch's current stream, without synchronising: image i into the slot outs[i] (a contiguous
    uint8 device tensor whose length is the capacity; None: capacity 0, only the size is reported). Returns the device
    tensors (sizes int64[n], status int32[n]); status 1 marks a slot that was too small, whose size is the capacity it
    needs and which was not written; status 2 (only with `optimize` or `progressive`) an image whose optimised code would be
    longer than 32 bits, which libjpeg refuses too: its size is 0. `optimize`, `progressive`: one value or one per image,
    like `quality`."""
    import torch

    images, items = _encode_items(images, quality, subsampling, restart_interval, layout, optimize, progressive)
    n = len(images)
    if len(outs) != n:
        raise ValueError("outs must have one entry per image")
    if n == 0:
        raise ValueError("no images")
    device = images[0].device
    for i, o in enumerate(outs):
        if o is not None and (o.dtype != torch.uint8 or not o.is_contiguous() or o.device != device):
            raise ValueError("outs[%d]: a contiguous uint8 tensor on the images' device is expected" % i)
        items[i].out = o.data_ptr() if o is not None and o.numel() else None
        items[i].capacity = o.numel() if o is not None else 0
    need = lib().jpeggpu_ext_encode_scratch_size(items, n)
    if need == 0:
        raise JpegGpuError(Status.NOT_SUPPORTED, "jpeggpu_ext_encode_scratch_size")
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    result = torch.empty(12 * n, dtype=torch.uint8, device=device)  # sizes, then status: one copy brings both to the host
    _check(lib().jpeggpu_ext_encode_batch(items, n, scratch.data_ptr(), need, result.data_ptr(), result.data_ptr() + 8 * n,
                                          torch.cuda.current_stream(device).cuda_stream), "jpeggpu_ext_encode_batch")
    # the scratch tensor is freed by torch's caching allocator in stream order: it is not reused before the launches ran
    return result[:8 * n].view(torch.int64), result[8 * n:].view(torch.int32)


def _encode_results(sizes, status):
    """encode_into's two tensors on the host, with one copy; this synchronises."""
    import torch

    n = sizes.numel()
    raw = torch.cat([sizes.view(torch.uint8), status.view(torch.uint8)]).cpu()
    return raw[:8 * n].view(torch.int64).tolist(), raw[8 * n:].view(torch.int32).tolist()


def encode_jpeg_to_device(images, quality=75, subsampling="4:2:0", restart_interval=0, layout="HWC", capacities=None, optimize=False, progressive=False):
    """Baseline JPEG files of `images`, left on the device: returns (buffer, offsets, sizes) -- file i is
    buffer[offsets[i]:offsets[i] + sizes[i]], a uint8 device tensor and two lists of ints. Arguments and the files are
    encode_jpeg's. `capacities`: the slot sizes to start with (default: each image's raw sample count plus its header);
    items whose file is larger are encoded once more into slots of the size they reported, behind the others. One
    jpeggpu_ext_encode_batch call (two after an overflow) and one synchronisation per call. `optimize` and `progressive` as
    in encode_jpeg; the default capacities are those of the same call without them (a baseline header and the raw samples)."""
    import torch

    images, items = _encode_items(images, quality, subsampling, restart_interval, layout, optimize, progressive)
    n = len(images)
    if n == 0:
        return None, [], []
    device = images[0].device
    if capacities is None:
        capacities = []
        for i in range(n):
            size = C.c_size_t(0)
            plain = EncodeItem.from_buffer_copy(items[i])
            plain.optimize = plain.progressive = 0
            _check(lib().jpeggpu_ext_encode_header(C.byref(plain), None, C.byref(size)), "jpeggpu_ext_encode_header")
            capacities.append(items[i].width * items[i].height * items[i].channels + size.value)
    capacities = _per_image(capacities, n, "capacities")

    def run(which, caps):
        offsets, total = [], 0
        for c in caps:
            offsets.append(total)
            total = (total + c + 15) // 16 * 16
        buf = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
        outs = [buf[o:o + c] for o, c in zip(offsets, caps)]
        pick = lambda v: [v[i] for i in which] if isinstance(v, (list, tuple)) else v  # noqa: E731
        sizes, status = _encode_results(*encode_into([images[i] for i in which], outs, pick(quality), pick(subsampling), pick(restart_interval), layout,
                                                     pick(optimize), pick(progressive)))
        for i, st in zip(which, status):
            if st == 2:
                raise JpegGpuError(Status.NOT_SUPPORTED, "jpeggpu_ext_encode_batch: image %d needs a Huffman code of more than 32 bits (libjpeg refuses it too)" % i)
        return buf, offsets, sizes, status

    buf, offsets, sizes, status = run(list(range(n)), [int(c) for c in capacities])
    again = [i for i in range(n) if status[i]]
    if again:
        buf2, offsets2, sizes2, status2 = run(again, [sizes[i] for i in again])
        if any(status2):
            raise JpegGpuError(Status.INTERNAL_ERROR, "jpeggpu_ext_encode_batch (retry)")
        base = buf.numel()
        buf = torch.cat([buf, buf2])
        for k, i in enumerate(again):
            offsets[i], sizes[i] = base + offsets2[k], sizes2[k]
    return buf, offsets, sizes


def encode_jpeg(images, quality=75, subsampling="4:2:0", restart_interval=0, layout="HWC", optimize=False, progressive=False):
    """Baseline JPEG files of uint8 device tensors, as a list of bytes: each file is, byte for byte, what Pillow on
    libjpeg-turbo writes with Image.fromarray(x).save(f, "JPEG", quality=quality, subsampling=subsampling,
    restart_marker_blocks=restart_interval) for the same pixels on the host.
    `images`: a list of tensors of any sizes, or one 4-D batch tensor; an item is H x W x 3 (RGB), H x W x 1 or H x W (grey),
    or with layout="CHW" 3 x H x W / 1 x H x W. Views (crops, row-padded, permuted) are read through their strides, without a
    copy. `quality` 1..100, `subsampling` "4:4:4" | "4:2:2" | "4:2:0" (grey has no chroma) and `restart_interval` (MCUs
    between restart markers, 0: none) are one value or one per image, and so is `optimize`: True writes the file of
    save(..., optimize=True), with Huffman tables made from the image's own symbol counts. `progressive` (one value or one
    per image): True writes the file of save(..., progressive=True), libjpeg's ten scans (six for grey), whatever `optimize`
    is. The whole list is ONE jpeggpu_ext_encode_batch call (a
    second one for the items whose file is larger than its raw pixels), one synchronisation and one copy to the host."""
    import torch

    buf, offsets, sizes = encode_jpeg_to_device(images, quality, subsampling, restart_interval, layout, optimize=optimize, progressive=progressive)
    if not sizes:
        return []
    host = torch.cat([buf[o:o + s] for o, s in zip(offsets, sizes)]).cpu().numpy().tobytes()  # only the files' bytes travel
    out, p = [], 0
    for s in sizes:
        out.append(host[p:p + s])
        p += s
    return out


def _fit_items(images, max_bytes, quality, min_quality, subsampling, restart_interval, layout, optimize):
    """The items of a budget call, without output slots: _encode_items' with each image's budget and range of qualities."""
    images, plain = _encode_items(images, 75, subsampling, restart_interval, layout, optimize)
    n = len(images)
    bs, his, los = _per_image(max_bytes, n, "max_bytes"), _per_image(quality, n, "quality"), _per_image(min_quality, n, "min_quality")
    items = (EncodeFitItem * max(n, 1))()
    for i in range(n):
        if int(bs[i]) < 0:
            raise ValueError("image %d: max_bytes must not be negative" % i)
        items[i].item = plain[i]
        items[i].max_bytes, items[i].quality_min, items[i].quality_max = int(bs[i]), int(los[i]), int(his[i])
    return images, items


def encode_fit_launches(width, height, channels=3, max_bytes=0, quality=75, min_quality=1, subsampling="4:2:0", restart_interval=0, optimize=False) -> int:
    """jpeggpu_ext_encode_fit_launches (host only) for one item of this geometry: the kernel launches a budget call over the
    range min_quality..quality enqueues -- 10 + 8 P, with optimize 12 + 10 P, P the evaluations the range needs. Raises
    JpegGpuError (INVALID_ARGUMENT) for an item the library refuses."""
    items = (EncodeFitItem * 1)()
    items[0].item = encode_item(width, height, channels, 75, subsampling, restart_interval, optimize)
    items[0].max_bytes, items[0].quality_min, items[0].quality_max = int(max_bytes), int(min_quality), int(quality)
    n = _newer_symbol("jpeggpu_ext_encode_fit_launches")(items, 1)
    if n == 0:
        raise JpegGpuError(Status.INVALID_ARGUMENT, "jpeggpu_ext_encode_fit_launches")
    return n


def encode_fit_into(images, outs, max_bytes, quality=75, min_quality=1, subsampling="4:2:0", restart_interval=0, layout="HWC", optimize=False):
    """jpeggpu_ext_encode_fit_batch on torch's current stream, without synchronising: for image i the best quality of
    min_quality..quality whose file is at most max_bytes long, and that file -- encode_into's at that quality, byte for byte
    -- in the slot outs[i] (None: only quality and size are reported). The search runs on the device: the pixel stage once,
    then one requantisation and the size stages per evaluation, with nothing on the host in between. `max_bytes`, `quality`,
    `min_quality` and the encoder's arguments are one value or one per image. Returns the device tensors (sizes int64[n],
    status int32[n], qualities int32[n]); status as encode_into, and EncodeStatus.OVER_BUDGET (5) for an image whose file
    exceeds max_bytes even at min_quality: its size is that file's, its quality min_quality, its slot untouched.
    The chosen quality is the answer of a bisection (include/jpeggpu/jpeggpu_ext.h states it exactly): the file always fits,
    and the quality is the largest that fits wherever the size grows with the quality, which on small images it sometimes
    does not."""
    import torch

    images, items = _fit_items(images, max_bytes, quality, min_quality, subsampling, restart_interval, layout, optimize)
    n = len(images)
    if len(outs) != n:
        raise ValueError("outs must have one entry per image")
    if n == 0:
        raise ValueError("no images")
    device = images[0].device
    for i, o in enumerate(outs):
        if o is not None and (o.dtype != torch.uint8 or not o.is_contiguous() or o.device != device):
            raise ValueError("outs[%d]: a contiguous uint8 tensor on the images' device is expected" % i)
        items[i].item.out = o.data_ptr() if o is not None and o.numel() else None
        items[i].item.capacity = o.numel() if o is not None else 0
    fit_batch = _newer_symbol("jpeggpu_ext_encode_fit_batch")
    need = lib().jpeggpu_ext_encode_fit_scratch_size(items, n)
    if need == 0:  # a range the library refuses, or (as in encode_into) a size beyond the kernels' limits
        bad_range = any(not 1 <= items[i].quality_min <= items[i].quality_max <= 100 for i in range(n))
        raise JpegGpuError(Status.INVALID_ARGUMENT if bad_range else Status.NOT_SUPPORTED, "jpeggpu_ext_encode_fit_scratch_size")
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    result = torch.empty(16 * n, dtype=torch.uint8, device=device)  # sizes, status, qualities: one copy brings all to the host
    _check(fit_batch(items, n, scratch.data_ptr(), need, result.data_ptr(), result.data_ptr() + 8 * n, result.data_ptr() + 12 * n,
                     torch.cuda.current_stream(device).cuda_stream), "jpeggpu_ext_encode_fit_batch")
    # the scratch tensor is freed by torch's caching allocator in stream order: it is not reused before the launches ran
    return result[:8 * n].view(torch.int64), result[8 * n:12 * n].view(torch.int32), result[12 * n:].view(torch.int32)


def encode_jpeg_fit(images, max_bytes, quality=75, min_quality=1, subsampling="4:2:0", restart_interval=0, layout="HWC", optimize=False, strict=True):
    """JPEG files of uint8 device tensors under a size limit: returns (files, qualities), file i the one encode_jpeg writes
    for image i at qualities[i], the best quality of min_quality..quality whose file is at most max_bytes long (encode_fit_into
    says which that is, exactly). `quality` is the upper end: the file of plain encode_jpeg if it fits, a lower quality only
    if it must be. `max_bytes`, `quality`, `min_quality` and the encoder's arguments are one value or one per image. An
    image that exceeds its limit even at min_quality raises a JpegGpuError naming it; with strict=False its file is None and
    its quality min_quality. One jpeggpu_ext_encode_fit_batch call, one synchronisation and one copy to the host."""
    import torch

    images, items = _fit_items(images, max_bytes, quality, min_quality, subsampling, restart_interval, layout, optimize)
    n = len(images)
    if n == 0:
        return [], []
    device = images[0].device
    # no file is longer than its budget, nor than the bound of its geometry
    caps = [min(int(items[i].max_bytes), lib().jpeggpu_ext_encode_bound(C.byref(items[i].item))) for i in range(n)]
    offsets, total = [], 0
    for c in caps:
        offsets.append(total)
        total = (total + c + 15) // 16 * 16
    buf = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    sizes, status, qualities = encode_fit_into(images, [buf[o:o + c] for o, c in zip(offsets, caps)], max_bytes, quality, min_quality, subsampling,
                                               restart_interval, layout, optimize)
    raw = torch.cat([sizes.view(torch.uint8), status.view(torch.uint8), qualities.view(torch.uint8)]).cpu()
    sizes, status = raw[:8 * n].view(torch.int64).tolist(), raw[8 * n:12 * n].view(torch.int32).tolist()
    qualities = raw[12 * n:].view(torch.int32).tolist()
    for i, st in enumerate(status):
        if st == EncodeStatus.OVER_BUDGET and strict:
            raise JpegGpuError(Status.INVALID_ARGUMENT, "jpeggpu_ext_encode_fit_batch: image %d takes %d bytes at quality %d, more than its max_bytes of %d"
                               % (i, sizes[i], qualities[i], int(items[i].max_bytes)))
        if st == EncodeStatus.TABLE_OVERFLOW:
            raise JpegGpuError(Status.NOT_SUPPORTED, "jpeggpu_ext_encode_fit_batch: image %d needs a Huffman code of more than 32 bits (libjpeg refuses it too)" % i)
        if st not in (EncodeStatus.OK, EncodeStatus.OVER_BUDGET):
            raise JpegGpuError(Status.INTERNAL_ERROR, "jpeggpu_ext_encode_fit_batch: image %d, status %d" % (i, st))
    keep = [i for i in range(n) if status[i] == EncodeStatus.OK]
    files = [None] * n
    if keep:
        host = torch.cat([buf[offsets[i]:offsets[i] + sizes[i]] for i in keep]).cpu().numpy().tobytes()  # only the files' bytes travel
        p = 0
        for i in keep:
            files[i] = host[p:p + sizes[i]]
            p += sizes[i]
    return files, qualities


def jpeg_roundtrip(images, quality=75, subsampling="4:2:0", layout="HWC", out=None):
    """JPEG compression as an augmentation: for each uint8 device tensor the pixels it has after it was saved as a baseline
    JPEG and opened again -- byte for byte np.asarray(Image.open(buf)) after Image.fromarray(x).save(buf, "JPEG",
    quality=quality, subsampling=subsampling) of Pillow on libjpeg-turbo --, without a file, an entropy coder or the host.
    `images`: a list of tensors of any sizes (or one 4-D batch tensor); an item is H x W (grey) or, by `layout`, H x W x 3 /
    3 x H x W. Any strided view is read through its strides, without a copy. `quality` 1..100 and `subsampling` "4:4:4" |
    "4:2:2" | "4:2:0" (not used for grey) are one value or one per image. Returns a list of new tensors of the inputs'
    shapes; with `out` (one tensor per image, of its shape, whose rows are dense: stride 1 along x, or 3 and 1 for HWC) the
    result is written there, and out[i] may be images[i] itself. ONE jpeggpu_ext_roundtrip_batch call on torch's current
    stream -- two launches, one with grey images only -- and no synchronisation."""
    import torch

    images, enc = _encode_items(images, quality, subsampling, 0, layout)
    n = len(images)
    if n == 0:
        return []
    device = images[0].device
    if out is None:
        out = [torch.empty(x.shape, dtype=torch.uint8, device=device) for x in images]
    out = list(out)
    if len(out) != n:
        raise ValueError("out must have one tensor per image")
    items = (RoundtripItem * n)()
    for i, (x, o, e) in enumerate(zip(images, out, enc)):
        if x.dim() != 2 and e.channels != 3:
            raise ValueError("image %d: H x W or three channels are expected" % i)
        if o.dtype != torch.uint8 or o.device != device or o.shape != x.shape:
            raise ValueError("out[%d]: a uint8 tensor of the image's shape on its device is expected" % i)
        if x.dim() == 2:
            pitch, plane, dense = o.stride(0), 0, o.stride(1) == 1
        elif layout == "HWC":
            pitch, plane, dense = o.stride(0), 0, o.stride(1) == 3 and o.stride(2) == 1
        else:
            pitch, plane, dense = o.stride(1), o.stride(0), o.stride(2) == 1
        if not dense:
            raise ValueError("out[%d]: rows of adjacent pixels are expected" % i)
        it = items[i]
        it.data, it.width, it.height, it.channels = e.data, e.width, e.height, e.channels
        it.row_pitch, it.pixel_stride, it.channel_stride = e.row_pitch, e.pixel_stride, e.channel_stride
        it.quality, it.subsampling = e.quality, e.subsampling
        it.dst, it.dst_pitch, it.plane_stride = o.data_ptr(), pitch, plane
    need = lib().jpeggpu_ext_roundtrip_scratch_size(items, n)
    if need == 0:
        raise JpegGpuError(Status.INVALID_ARGUMENT, "jpeggpu_ext_roundtrip_scratch_size")
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    _check(lib().jpeggpu_ext_roundtrip_batch(items, n, IMAGE_LAYOUTS[layout], scratch.data_ptr(), need, torch.cuda.current_stream(device).cuda_stream),
           "jpeggpu_ext_roundtrip_batch")
    # the scratch tensor is freed by torch's caching allocator in stream order: it is not reused before the launches ran
    return out


def _transcode_orientations(bd, orientation, exif_transpose, trim):
    """Per file of a BatchDecode: (orientation 1..8, trim) as jpeggpu_ext_set_transcode_orientation takes them."""
    n = len(bd.decoders)
    os_, es, ts = _per_image(orientation, n, "orientation"), _per_image(exif_transpose, n, "exif_transpose"), _per_image(trim, n, "trim")
    out = []
    for i in range(n):
        if es[i] and os_[i] is not None:
            raise ValueError("item %d: orientation and exif_transpose are both given" % i)
        o = bd.orientations[i] if es[i] else 1 if os_[i] is None else int(os_[i])
        if not 1 <= o <= 8:
            raise ValueError("item %d: orientation must be 1..8" % i)
        out.append((o, bool(ts[i])))
    return out


def _expanded(rect, ths, tvs):
    """jpegtran's rule for a crop that does not start on an iMCU boundary: the origin moves up and left to one and the size
    grows by what that adds."""
    x, y, w, h = rect
    return x - x % (8 * ths), y - y % (8 * tvs), w + x % (8 * ths), h + y % (8 * tvs)


def transcode_crop_rects(width, height, hs, vs, rect, orientation=1, trim=False, expand=False):
    """The arithmetic of a cropped transcode (host only, no library call): for a stored width x height source whose luma has
    the factors hs x vs (1, 1 for grey) and a rectangle (x, y, w, h) in pixels of the image the transcode would write without
    a crop -- the displayed image under `orientation`, cut by `trim` where the orientation's edge rules need it -- returns
    (target, source): `target` the rectangle the library gets (with `expand`, x and y rounded down to the target's iMCU and w
    and h grown by what was cut, jpegtran's rule), `source` the rectangle of stored source pixels it holds, what
    Decoder.set_crop takes to decode no more than that. ValueError: the orientation refuses the source, or the rectangle is
    empty or does not lie inside the uncropped target. The alignment of x and y is the library's to judge."""
    o = int(orientation)
    if not 1 <= o <= 8:
        raise ValueError("orientation must be 1..8")
    w, h = int(width), int(height)
    if o in (2, 3, 7, 8) and w % (8 * hs):  # the stored x is mirrored
        if not trim or w < 8 * hs:
            raise ValueError("a mirrored edge with a partial iMCU")
        w -= w % (8 * hs)
    if o in (3, 4, 6, 7) and h % (8 * vs):
        if not trim or h < 8 * vs:
            raise ValueError("a mirrored edge with a partial iMCU")
        h -= h % (8 * vs)
    tw, th, ths, tvs = (h, w, vs, hs) if o >= 5 else (w, h, hs, vs)
    x, y, cw, ch = (int(v) for v in rect)
    if expand:
        x, y, cw, ch = _expanded((x, y, cw, ch), ths, tvs)
    if x < 0 or y < 0 or cw < 1 or ch < 1 or x + cw > tw or y + ch > th:
        raise ValueError("the rectangle does not lie inside the %d x %d image" % (tw, th))
    x0 = tw - x - cw if o in (2, 3, 6, 7) else x  # the displayed axes' mirrors, then the exchange
    y0 = th - y - ch if o in (3, 4, 7, 8) else y
    return (x, y, cw, ch), ((y0, x0, ch, cw) if o >= 5 else (x0, y0, cw, ch))


def _luma_factors(info, frame="encoder"):
    """(hs, vs) as the transcode counts iMCUs: luma's factors of a colour file, (1, 1) for grey; with frame="source" the
    largest factors of the file's components."""
    n = info.num_components
    if n == 1:
        return (1, 1)
    if frame == "source":
        return (max(info.subsampling.x[:n]), max(info.subsampling.y[:n]))
    return (info.subsampling.x[0], info.subsampling.y[0])


TRANSCODE_FRAMES = {"encoder": 0, "source": 1}


def _transcode_frames(n, frame):
    frames = _per_image(frame, n, "frame")
    for f in frames:
        if f not in TRANSCODE_FRAMES:
            raise ValueError('frame must be "encoder" or "source"')
    return frames


def _transcode_crops(n, crops):
    """`crops` of the transcode calls as a list of n entries: None or (x, y, w, h)."""
    if crops is None:
        return [None] * n
    if len(crops) == 4 and not any(c is None or hasattr(c, "__len__") for c in crops):
        return [tuple(int(v) for v in crops)] * n
    crops = list(crops)
    if len(crops) != n:
        raise ValueError("crops must be one rectangle or one entry per file")
    for i, c in enumerate(crops):
        if c is not None and len(c) != 4:
            raise ValueError("crops[%d]: (x, y, w, h) is expected" % i)
    return [None if c is None else tuple(int(v) for v in c) for c in crops]


def _transcode_items(bd, optimize, progressive, restart_interval, orientation=None, exif_transpose=False, trim=False, crops=None, expand=False,
                     frame="encoder"):
    """The items of a transcode call for the decoded files of a BatchDecode, without output slots; a source the writer cannot
    take raises JpegGpuError naming the item. Sets each decoder's transcode orientation (Decoder.set_transcode_orientation)
    and crop (Decoder.set_transcode_crop), which the calls on the items read."""
    n = len(bd.decoders)
    os_, ps_, rs = _per_image(optimize, n, "optimize"), _per_image(progressive, n, "progressive"), _per_image(restart_interval, n, "restart_interval")
    crops, expands, frames = _transcode_crops(n, crops), _per_image(expand, n, "expand"), _transcode_frames(n, frame)
    for i, (dec, (o, t)) in enumerate(zip(bd.decoders, _transcode_orientations(bd, orientation, exif_transpose, trim))):
        if frames[i] != "encoder" or hasattr(lib(), "jpeggpu_ext_set_transcode_frame"):
            dec.set_transcode_frame(TRANSCODE_FRAMES[frames[i]])
        if o != 1 or t or hasattr(lib(), "jpeggpu_ext_set_transcode_orientation"):
            dec.set_transcode_orientation(o, t)
        rect = crops[i]
        if rect is not None and expands[i]:
            hs, vs = _luma_factors(bd.infos[i], frames[i])
            ths, tvs = (vs, hs) if o >= 5 else (hs, vs)
            rect = _expanded(rect, ths, tvs)
        if rect is not None or hasattr(lib(), "jpeggpu_ext_set_transcode_crop"):
            try:
                dec.set_transcode_crop(*(rect or (0, 0, 0, 0)))
            except JpegGpuError as e:
                raise JpegGpuError(e.status, "jpeggpu_ext_set_transcode_crop: item %d: crop %r" % (i, rect))
    items = (TranscodeItem * max(n, 1))()
    bound = _newer_symbol("jpeggpu_ext_transcode_bound")
    for i, (dec, _, _, base, _) in enumerate(bd._entries):
        it = items[i]
        it.decoder, it.d_tmp = dec._h, base
        it.optimize, it.progressive = int(os_[i]), int(ps_[i])
        it.restart_interval = -1 if rs[i] is None else int(rs[i])
        if bound(C.byref(it)) == 0:  # say why: the header call returns the status
            size = C.c_size_t(0)
            st = lib().jpeggpu_ext_transcode_header(C.byref(it), None, C.byref(size))
            raise JpegGpuError(st if st else Status.NOT_SUPPORTED, "jpeggpu_ext_transcode_batch: item %d cannot be transcoded" % i)
    return items


def transcode_into(bd, outs, optimize=False, progressive=False, restart_interval=None, items=None, orientation=None, exif_transpose=False, trim=False,
                   crops=None, expand=False, frame="encoder"):
    """jpeggpu_ext_transcode_batch on torch's current stream, without synchronising, for the files of `bd`, a BatchDecode whose
    decode() was enqueued on the same stream: file i into the slot outs[i], as encode_into. Returns the device tensors
    (sizes int64[n], status int32[n]); status 1: the slot was too small, 2: as encode_into, 4: the source holds a
    coefficient that no Huffman code of the target expresses, and its size is 0. `items`: what _transcode_items made of the
    same arguments, for a caller that has them already. `orientation`, `exif_transpose`, `trim`, `crops`, `expand`, `frame`: as
    transcode_jpeg's; `bd` decodes what its maker asked for -- whole files, or with BatchDecode(crops=) the source rectangles
    of transcode_crop_rects, which must hold what the items read."""
    import torch

    if items is None:
        items = _transcode_items(bd, optimize, progressive, restart_interval, orientation, exif_transpose, trim, crops, expand, frame)
    n = len(bd.decoders)
    if len(outs) != n:
        raise ValueError("outs must have one entry per file")
    if n == 0:
        raise ValueError("no files")
    device = bd.tmps[0].device
    for i, o in enumerate(outs):
        if o is not None and (o.dtype != torch.uint8 or not o.is_contiguous() or o.device != device):
            raise ValueError("outs[%d]: a contiguous uint8 tensor on the decode's device is expected" % i)
        items[i].out = o.data_ptr() if o is not None and o.numel() else None
        items[i].capacity = o.numel() if o is not None else 0
    need = lib().jpeggpu_ext_transcode_scratch_size(items, n)
    if need == 0:
        raise JpegGpuError(Status.NOT_SUPPORTED, "jpeggpu_ext_transcode_scratch_size")
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    result = torch.empty(12 * n, dtype=torch.uint8, device=device)
    _check(lib().jpeggpu_ext_transcode_batch(items, n, scratch.data_ptr(), need, result.data_ptr(), result.data_ptr() + 8 * n,
                                             torch.cuda.current_stream(device).cuda_stream), "jpeggpu_ext_transcode_batch")
    return result[:8 * n].view(torch.int64), result[8 * n:].view(torch.int32)


def _transcode_windows(n, orientation, exif_transpose, trim, crops, expand, frame="encoder"):
    """BatchDecode's crop_hooks for a cropped transcode: each cropped file decodes only the source rectangle of its crop
    (transcode_crop_rects). A rectangle the rules refuse sets no window: the item is then refused by the library, by name."""
    crops = _transcode_crops(n, crops)
    if not any(c is not None for c in crops):
        return None
    os_, es, ts, xs = _per_image(orientation, n, "orientation"), _per_image(exif_transpose, n, "exif_transpose"), _per_image(trim, n, "trim"), _per_image(expand, n, "expand")
    frames = _transcode_frames(n, frame)

    def hook(i, dec, w, h):
        o = dec.orientation() if es[i] else 1 if os_[i] is None else int(os_[i])
        try:
            return transcode_crop_rects(w, h, *_luma_factors(dec.info, frames[i]), crops[i], o, bool(ts[i]), bool(xs[i]))[1]
        except ValueError:
            return None

    return [None if c is None else hook for c in crops]


def transcode_jpeg_to_device(datas, optimize=False, progressive=False, restart_interval=None, device="cuda:0", capacities=None, orientation=None,
                             exif_transpose=False, trim=False, crops=None, expand=False, frame="encoder", truncated=False):
    """transcode_jpeg's files left on the device: (buffer, offsets, sizes) as encode_jpeg_to_device returns them.
    `capacities`: the slot sizes to start with (default: twice the source's length, a header and three bytes per block of the
    TARGET's MCUs for restart markers and their padding); if a file is larger, the call is repeated once with the sizes it
    reported."""
    import torch

    datas = list(datas)
    if not datas:
        return None, [], []
    _newer_symbol("jpeggpu_ext_transcode_batch")
    n = len(datas)
    with BatchDecode(datas, device, coefficients_only=True, truncated=truncated,
                     crop_hooks=_transcode_windows(n, orientation, exif_transpose, trim, crops, expand, frame)) as bd:
        # (host only: refuses before anything is enqueued or allocated)
        items = _transcode_items(bd, optimize, progressive, restart_interval, orientation, exif_transpose, trim, crops, expand, frame)
        bd.decode()
        if capacities is None:
            caps = [2 * len(d) + 1024 + 3 * _transcode_blocks(items[i]) for i, d in enumerate(datas)]
        else:
            caps = [int(c) for c in _per_image(capacities, n, "capacities")]
        for attempt in range(2):
            offsets, total = [], 0
            for c in caps:
                offsets.append(total)
                total = (total + c + 15) // 16 * 16
            buf = torch.empty(max(total, 1), dtype=torch.uint8, device=bd.tmps[0].device)
            sizes, status = _encode_results(*transcode_into(bd, [buf[o:o + c] for o, c in zip(offsets, caps)], items=items))
            if 1 not in status:
                break
            caps = [max(c, s) for c, s in zip(caps, sizes)]
    for i, st in enumerate(status):
        if st == 4:
            raise JpegGpuError(Status.NOT_SUPPORTED, "jpeggpu_ext_transcode_batch: item %d holds a coefficient that no Huffman code of the target expresses" % i)
        if st == 2:
            raise JpegGpuError(Status.NOT_SUPPORTED, "jpeggpu_ext_transcode_batch: item %d needs a Huffman code of more than 32 bits (libjpeg refuses it too)" % i)
        if st:
            raise JpegGpuError(Status.INVALID_ARGUMENT, "jpeggpu_ext_transcode_batch: item %d needs %d bytes" % (i, sizes[i]))
    return buf, offsets, sizes


def _transcode_blocks(item):
    """The blocks of the file an item writes, dummy ones included, read from the frame header the library gives it: per
    component its blocks of an MCU times the MCUs (an encoder layout's luma: about ceil(w / 8) * ceil(h / 8) as before)."""
    size = C.c_size_t(2048)  # (four DQTs of 16-bit entries and four DHTs: 1028 bytes)
    head = (C.c_uint8 * 2048)()
    one = TranscodeItem()
    C.pointer(one)[0] = item
    one.optimize = one.progressive = 0
    _check(lib().jpeggpu_ext_transcode_header(C.byref(one), head, C.byref(size)), "jpeggpu_ext_transcode_header")
    head = bytes(head[:size.value])
    at = 2  # SOI; then APP0 or APP14 and the DQTs, then SOF0 or SOF1: marker, length, precision, height, width, components
    while head[at + 1] not in (0xC0, 0xC1):
        at += 2 + (head[at + 2] << 8 | head[at + 3])
    at += 5
    height, width, ncomp = head[at] << 8 | head[at + 1], head[at + 2] << 8 | head[at + 3], head[at + 4]
    if ncomp == 1 or (ncomp == 3 and head[at + 6] in (0x11, 0x21, 0x22) and head[at + 9] == head[at + 12] == 0x11):
        return (height + 7) // 8 * ((width + 7) // 8)  # an encoder layout: luma's real blocks, as before
    fs = [(head[at + 6 + 3 * c] >> 4, head[at + 6 + 3 * c] & 15) for c in range(ncomp)]
    hmax, vmax = max(f[0] for f in fs), max(f[1] for f in fs)
    return -(-width // (8 * hmax)) * -(-height // (8 * vmax)) * sum(f[0] * f[1] for f in fs)


def transcode_jpeg(datas, optimize=False, progressive=False, restart_interval=None, device="cuda:0", orientation=None, exif_transpose=False, trim=False,
                   crops=None, expand=False, frame="encoder", truncated=False):
    """JPEG files from JPEG files without a pixel in between, as a list of bytes: what jpegtran -optimize, -progressive and
    -restart N do. Each file holds the source's quantised coefficients exactly, in the layout encode_jpeg writes (the
    source's quantisation tables; EXIF, ICC and comments are dropped). `optimize`, `progressive` as in encode_jpeg;
    `restart_interval` in MCUs, 0: none, None: the source's; each one value or one per file. For a source Pillow wrote, the
    result is the file Pillow writes for the same pixels and parameters with those options. Sources: baseline or progressive,
    grey or YCbCr 4:4:4, 4:2:2 or 4:2:0 with 8-bit quantisation tables; anything else raises JpegGpuError naming the item.
    `orientation` (1..8, one value or one per file, None: 1) turns, flips or transposes the image without loss, like jpegtran
    -rotate / -flip / -transpose: the new file's stored image is the displayed image of the source under that EXIF
    orientation number. `exif_transpose` (one value or one per file): each file's own Orientation tag is the number, which
    bakes the tag into the file (the result holds no Exif segment); naming both for a file is a ValueError. A mirrored edge
    must be a whole number of iMCUs of the source: otherwise the item raises JpegGpuError before anything is enqueued, or
    with `trim` the partial iMCUs at that edge are cut off first, like jpegtran -trim. 4:2:2 takes 1..4 only, unless
    frame="source".
    `frame` ("encoder" | "source", one value or one per file): "source" keeps each source's own frame layout, as jpegtran
    does, and so takes every file the decoder reads: any sampling factors (4:4:0, 4:1:1 ..), separate Cb and Cr tables, 16-bit
    tables, RGB-coded, CMYK, YCCK and two-component files. The file then has the source's colour model, sampling factors and
    table numbers; orientations 5..8 exchange the factors of every component (4:2:2 becomes 4:4:0), and the iMCU of the edge
    and crop rules is 8 h_max x 8 v_max. A file the default takes gives the same bytes. `progressive` writes libjpeg's ten
    scans for three-component YCbCr and its all-purpose script of 2 + 4 n scans for everything else (18 for CMYK).
    `crops`: one rectangle (x, y, w, h) or one per file (None: the whole image), cut out without loss like jpegtran -crop, in
    pixels of the image the call would write without it -- after `orientation` and `trim`, so in displayed pixels. x and y
    must be multiples of the target's iMCU (8 hs x 8 vs of luma's factors, exchanged for 5..8; 8 x 8 for grey), or with
    `expand` (one value or one per file) they are rounded down to one and w and h grow by what that adds, which is what
    jpegtran does; w and h may be anything. Where w and h are multiples of the iMCU too or reach the image's edge, the file is
    the one Pillow writes for the cropped pixels. Each cropped file is decoded only as far as its rectangle needs
    (transcode_crop_rects, Decoder.set_crop: the restart segments that hold it, where the file has restart markers).
    One batched decode that stops in front of the IDCT, one jpeggpu_ext_transcode_batch call, one synchronisation and one
    copy of the files' bytes to the host. `truncated`: a source that ends early is taken as libjpeg finishes it (BatchDecode):
    the new file is whole, its blocks behind the cut all zero."""
    import torch

    buf, offsets, sizes = transcode_jpeg_to_device(datas, optimize, progressive, restart_interval, device, None, orientation, exif_transpose, trim, crops,
                                                   expand, frame, truncated=truncated)
    if not sizes:
        return []
    host = torch.cat([buf[o:o + s] for o, s in zip(offsets, sizes)]).cpu().numpy().tobytes()
    out, p = [], 0
    for s in sizes:
        out.append(host[p:p + s])
        p += s
    return out


COEFFICIENT_TYPE_NAMES = {"int16": 0, "float32": 1, "float16": 2}  # enum jpeggpu_ext_coefficient_type, by torch dtype name


class Coefficients:
    """The DCT-domain form of one JPEG (read_coefficients returns these; write_coefficients takes these or any object with
    the same fields): `coefficients[c]` a tensor [blocks_y, blocks_x, 8, 8] over component c's real block grid, the DC
    absolute; `qtables[c]` a uint16 numpy array [8, 8]; `width`, `height`; `sampling` [(h, v), ...] as in the frame header;
    `color_space` (ColorSpace); `progressive`: whether the source was (read only)."""

    def __init__(self, coefficients, qtables, width, height, sampling, color_space, progressive=False):
        self.coefficients, self.qtables, self.width, self.height = list(coefficients), list(qtables), int(width), int(height)
        self.sampling, self.color_space, self.progressive = [tuple(f) for f in sampling], ColorSpace(color_space), bool(progressive)


def coefficient_grid(width, height, sampling):
    """[(blocks_y, blocks_x), ...]: each component's real block grid -- libjpeg's height_in_blocks x width_in_blocks."""
    if len(sampling) == 1:
        return [(-(-height // 8), -(-width // 8))]
    hmax, vmax = max(f[0] for f in sampling), max(f[1] for f in sampling)
    return [(-(-(-(-height * v // vmax)) // 8), -(-(-(-width * h // hmax)) // 8)) for h, v in sampling]


def read_coefficients_into(bd, dtype=None, dequantize=False):
    """jpeggpu_ext_read_coefficients_batch on torch's current stream, without synchronising, for the files of `bd`, a
    BatchDecode whose decode() was enqueued on the same stream (with coefficients_only or without): a list of Coefficients.
    All tensors of the call are views of ONE allocation, each aligned to 256 bytes."""
    import numpy as np
    import torch

    dtype = torch.int16 if dtype is None else dtype
    names = {getattr(torch, k): v for k, v in COEFFICIENT_TYPE_NAMES.items()}
    if dtype not in names:
        raise ValueError("dtype must be torch.int16, torch.float32 or torch.float16")
    call = _newer_symbol("jpeggpu_ext_read_coefficients_batch")
    n = len(bd.decoders)
    if n == 0:
        return []
    device = bd.tmps[0].device
    esize = torch.empty(0, dtype=dtype).element_size()
    infos, offsets, total = [dec.coefficient_info() for dec in bd.decoders], [], 0
    for ci in infos:
        for c in range(ci.num_components):
            offsets.append(total)
            total = _align256(total + ci.blocks_y[c] * ci.blocks_x[c] * 64 * esize)
    buf = torch.empty(total + 256, dtype=torch.uint8, device=device)
    pad = _align256(buf.data_ptr()) - buf.data_ptr()
    items, out, k = (CoefficientReadItem * n)(), [], 0
    for i, (ci, (dec, _, _, base, _)) in enumerate(zip(infos, bd._entries)):
        items[i].decoder, items[i].d_tmp = dec._h, base
        tensors = []
        for c in range(ci.num_components):
            by, bx = ci.blocks_y[c], ci.blocks_x[c]
            t = buf[pad + offsets[k]:pad + offsets[k] + by * bx * 64 * esize].view(dtype).view(by, bx, 8, 8)
            items[i].dst[c] = t.data_ptr()
            tensors.append(t)
            k += 1
        tables = [np.ctypeslib.as_array(ci.qtable[c]).reshape(8, 8).copy() for c in range(ci.num_components)]
        out.append(Coefficients(tensors, tables, ci.width, ci.height, [(ci.h[c], ci.v[c]) for c in range(ci.num_components)], ci.color_space,
                                ci.progressive))
    spec = CoefficientSpec(names[dtype], int(bool(dequantize)))
    need = lib().jpeggpu_ext_read_coefficients_scratch_size(n)
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    _check(call(items, n, C.byref(spec), scratch.data_ptr(), need, torch.cuda.current_stream(device).cuda_stream), "jpeggpu_ext_read_coefficients_batch")
    return out


def read_coefficients(datas, device="cuda:0", dtype=None, dequantize=False, truncated=False):
    """The quantised DCT coefficients of JPEG files, on the device: what jpeg_read_coefficients (jpegio.read,
    torchjpeg.codec.read_coefficients) gives on the CPU. Returns one Coefficients per file; `dtype` torch.int16 (default:
    the values exactly), or torch.float32 / torch.float16, which with `dequantize` hold value * table entry (one float32
    multiply; for float16 that product converted once). Dequantised int16 is refused. Every file the decoder reads:
    baseline and progressive, 1..4 components, any sampling, 16-bit tables. One batched decode that stops in front of the
    IDCT, ONE allocation for all tensors, one read call; nothing synchronises. `truncated`: files that end early are read as
    libjpeg finishes them (BatchDecode): the blocks behind the cut are all zero, DC included."""
    import torch

    datas = list(datas)
    if not datas:
        return []
    _newer_symbol("jpeggpu_ext_read_coefficients_batch")
    if dequantize and (dtype is None or dtype == torch.int16):
        raise JpegGpuError(Status.INVALID_ARGUMENT, "read_coefficients: dequantised int16 (a 16-bit table overflows it)")
    with BatchDecode(datas, device, coefficients_only=True, truncated=truncated) as bd:
        bd.decode()
        return read_coefficients_into(bd, dtype, dequantize)


def _coefficient_items(cs, optimize, progressive, restart_interval):
    """The items of a write call without output slots, and the tensors they point into (kept alive by the caller)."""
    import numpy as np
    import torch

    cs = list(cs)
    n = len(cs)
    os_, ps_, rs = _per_image(optimize, n, "optimize"), _per_image(progressive, n, "progressive"), _per_image(restart_interval, n, "restart_interval")
    items, keep = (CoefficientItem * max(n, 1))(), []
    for i, x in enumerate(cs):
        nc = len(x.coefficients)
        if not 1 <= nc <= MAX_COMP or len(x.qtables) != nc or len(x.sampling) != nc:
            raise ValueError("item %d: 1..4 components with one table and one (h, v) each are expected" % i)
        it = items[i]
        it.width, it.height, it.components, it.color_space = int(x.width), int(x.height), nc, int(x.color_space)
        it.optimize, it.progressive, it.restart_interval = int(os_[i]), int(ps_[i]), int(rs[i])
        grids = coefficient_grid(it.width, it.height, [tuple(f) for f in x.sampling]) if it.width > 0 and it.height > 0 else [None] * nc
        for c in range(nc):
            t = x.coefficients[c]
            if t.dtype != torch.int16 or not t.is_cuda or not t.is_contiguous() or t.data_ptr() % 16:
                raise JpegGpuError(Status.INVALID_ARGUMENT,
                                   "write_coefficients: item %d component %d: a contiguous int16 device tensor aligned to 16 bytes is expected" % (i, c))
            if grids[c] is not None and tuple(t.shape) not in (grids[c] + (8, 8), grids[c] + (64,)):
                raise JpegGpuError(Status.INVALID_ARGUMENT,
                                   "write_coefficients: item %d component %d: shape %r does not fit the frame's grid %r" % (i, c, tuple(t.shape), grids[c]))
            it.h[c], it.v[c] = int(x.sampling[c][0]), int(x.sampling[c][1])
            q = np.asarray(x.qtables[c]).reshape(64)
            if q.min() < 1 or q.max() > 65535:
                raise JpegGpuError(Status.INVALID_ARGUMENT, "write_coefficients: item %d component %d: table entries must be 1..65535" % (i, c))
            for k in range(64):
                it.qtable[c][k] = int(q[k])
            it.coef[c] = t.data_ptr()
            keep.append(t)
        if lib().jpeggpu_ext_write_coefficients_bound(C.byref(it)) == 0:  # say why: the header call returns the status
            size = C.c_size_t(0)
            st = lib().jpeggpu_ext_write_coefficients_header(C.byref(it), None, C.byref(size))
            raise JpegGpuError(st if st else Status.NOT_SUPPORTED, "jpeggpu_ext_write_coefficients_batch: item %d cannot be written" % i)
    return items, keep


def write_coefficients_into(cs, outs, optimize=False, progressive=False, restart_interval=0, items=None):
    """jpeggpu_ext_write_coefficients_batch on torch's current stream, without synchronising: item i into the slot outs[i], as
    encode_into. Returns the device tensors (sizes int64[n], status int32[n]) with transcode_into's statuses."""
    import torch

    _newer_symbol("jpeggpu_ext_write_coefficients_batch")
    cs = list(cs)
    if items is None:
        items, _ = _coefficient_items(cs, optimize, progressive, restart_interval)
    n = len(cs)
    if len(outs) != n:
        raise ValueError("outs must have one entry per item")
    if n == 0:
        raise ValueError("no items")
    device = cs[0].coefficients[0].device
    for i, o in enumerate(outs):
        if o is not None and (o.dtype != torch.uint8 or not o.is_contiguous() or o.device != device):
            raise ValueError("outs[%d]: a contiguous uint8 tensor on the coefficients' device is expected" % i)
        items[i].out = o.data_ptr() if o is not None and o.numel() else None
        items[i].capacity = o.numel() if o is not None else 0
    need = lib().jpeggpu_ext_write_coefficients_scratch_size(items, n)
    if need == 0:
        raise JpegGpuError(Status.NOT_SUPPORTED, "jpeggpu_ext_write_coefficients_scratch_size")
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    result = torch.empty(12 * n, dtype=torch.uint8, device=device)
    _check(lib().jpeggpu_ext_write_coefficients_batch(items, n, scratch.data_ptr(), need, result.data_ptr(), result.data_ptr() + 8 * n,
                                                      torch.cuda.current_stream(device).cuda_stream), "jpeggpu_ext_write_coefficients_batch")
    return result[:8 * n].view(torch.int64), result[8 * n:].view(torch.int32)


def write_coefficients_to_device(cs, optimize=False, progressive=False, restart_interval=0, capacities=None):
    """write_coefficients' files left on the device: (buffer, offsets, sizes) as encode_jpeg_to_device returns them.
    `capacities`: the slot sizes to start with (default: a header and four bytes per coefficient block, restart markers
    included); if a file is larger, the call is repeated once with the sizes it reported."""
    import torch

    cs = list(cs)
    if not cs:
        return None, [], []
    _newer_symbol("jpeggpu_ext_write_coefficients_batch")
    n = len(cs)
    items, _keep = _coefficient_items(cs, optimize, progressive, restart_interval)
    if capacities is None:
        caps = [2048 + sum(48 * t.numel() // 64 for t in x.coefficients) for x in cs]
    else:
        caps = [int(c) for c in _per_image(capacities, n, "capacities")]
    for attempt in range(2):
        offsets, total = [], 0
        for c in caps:
            offsets.append(total)
            total = (total + c + 15) // 16 * 16
        buf = torch.empty(max(total, 1), dtype=torch.uint8, device=cs[0].coefficients[0].device)
        sizes, status = _encode_results(*write_coefficients_into(cs, [buf[o:o + c] for o, c in zip(offsets, caps)], items=items))
        if 1 not in status:
            break
        caps = [max(c, s) for c, s in zip(caps, sizes)]
    for i, st in enumerate(status):
        if st == 4:
            raise JpegGpuError(Status.NOT_SUPPORTED, "jpeggpu_ext_write_coefficients_batch: item %d holds a coefficient that no Huffman code expresses" % i)
        if st == 2:
            raise JpegGpuError(Status.NOT_SUPPORTED, "jpeggpu_ext_write_coefficients_batch: item %d needs a Huffman code of more than 32 bits (libjpeg refuses it too)" % i)
        if st:
            raise JpegGpuError(Status.INVALID_ARGUMENT, "jpeggpu_ext_write_coefficients_batch: item %d needs %d bytes" % (i, sizes[i]))
    return buf, offsets, sizes


def write_coefficients(cs, optimize=False, progressive=False, restart_interval=0):
    """JPEG files that hold exactly the given quantised coefficients, as a list of bytes: what jpeg_write_coefficients
    (jpegio.write, torchjpeg.codec.write_coefficients) does on the CPU. `cs`: Coefficients, as read_coefficients returns
    them (changed on the device or not) or built from scratch -- any object with `coefficients` (int16 device tensors
    [blocks_y, blocks_x, 8, 8] over each component's real grid, coefficient_grid), `qtables`, `width`, `height`, `sampling`
    and `color_space`. `optimize`, `progressive`, `restart_interval` (MCUs, 0: none): one value or one per item. A layout
    encode_jpeg writes gets its header, and the file is transcode_jpeg's for a source with these coefficients; every other
    layout is written as transcode_jpeg(frame="source") writes it. An item with an AC coefficient of magnitude 1024 or
    more, or a DC step of 2048 or more, raises JpegGpuError (write_coefficients_into reports it per item instead).
    One jpeggpu_ext_write_coefficients_batch call (a second for files larger than the default slots), one synchronisation
    and one copy of the files' bytes to the host."""
    import torch

    buf, offsets, sizes = write_coefficients_to_device(cs, optimize, progressive, restart_interval)
    if not sizes:
        return []
    host = torch.cat([buf[o:o + s] for o, s in zip(offsets, sizes)]).cpu().numpy().tobytes()
    out, p = [], 0
    for s in sizes:
        out.append(host[p:p + s])
        p += s
    return out


def encode_tables_from_counts(counts):
    """jpeggpu_ext_encode_tables_from_counts on torch's current stream, without synchronising: jpeg_gen_optimal_table of
    each row of `counts`, an n x 256 int32 device tensor of symbol counts (a negative one reads as a count beyond the range).
    Returns the device tensors (bits_values uint8[n, 272]: 16 `bits` bytes, then 256 `values` bytes; status int32[n]: 0,
    2 for a code longer than 32 bits before limiting, 3 for an empty table or counts beyond libjpeg's range)."""
    import torch

    if not isinstance(counts, torch.Tensor) or not counts.is_cuda or counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != 256:
        raise ValueError("counts: an n x 256 int32 device tensor is expected")
    if counts.shape[0] == 0:
        raise ValueError("counts: at least one table is expected")
    counts = counts.contiguous()
    n = counts.shape[0]
    out = torch.empty((n, 272), dtype=torch.uint8, device=counts.device)
    status = torch.empty(n, dtype=torch.int32, device=counts.device)
    _check(lib().jpeggpu_ext_encode_tables_from_counts(counts.data_ptr(), n, out.data_ptr(), status.data_ptr(),
                                                       torch.cuda.current_stream(counts.device).cuda_stream), "jpeggpu_ext_encode_tables_from_counts")
    return out, status
